"""Pose information (goicp_pose_information): what a call costs next to one ICP pass, on the bunny (model_bunny target, data_bunny source).

  single    wall-clock microseconds of one goicp_pose_information call (zeroing, launch, read-back of the accumulators, fp64 finish)
  batch64   the same per pose for goicp_pose_information_batch with K = 64 poses (small rotations about the identity)
  icp_pass  goicp_time_icp_pass of the same build at the identity pose (device time of one correspondence pass, HIP events): the yardstick
per metric (0 point-to-point, 1 point-to-plane; the ICP pass is timed under the same metric).  Every figure is the median of --reps
(default 9) measurements after one warm-up call, all values kept.  The call is host-synchronous and includes its copies; the pass figure is
device time only -- the two are not the same kind of number and the JSON says so.  Writes one JSON object.

    python tools/pose_info_probe.py --out profiles/pose_info_probe.json [--reps 9]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    from conftest import cloud, load_pkg
    pkg = load_pkg()
    pkg.load_library()
    from cuda_go_icp_amd import synth
    tgt, src = cloud("model_bunny"), cloud("data_bunny")
    reg = pkg.Registration(tgt, src, 1e-3)
    I9, Z3 = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
    rng = np.random.default_rng(0)
    Rs = np.stack([synth._rodrigues(rng.uniform(-0.05, 0.05, 3) + 1e-4) for _ in range(64)]).astype(np.float32).reshape(64, 9)
    ts = rng.uniform(-0.01, 0.01, (64, 3)).astype(np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    out = {"workload": "bunny", "n_source": int(len(src)), "n_target": int(len(tgt)), "kernel_source_hash": pkg.load_library().goicp_kernel_source_hash().decode(),
           "note": "single / batch64 are host wall-clock per call (copies and the fp64 finish included); icp_pass is device time of one pass (HIP events)"}
    for metric in (0, 1):
        reg.set_icp_options(metric, 16)
        reg.pose_information(I9, Z3)
        reg.pose_information_batch(Rs, ts)
        single, batch, ps = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            info = reg.pose_information(I9, Z3)
            single.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            reg.pose_information_batch(Rs, ts)
            batch.append((time.perf_counter() - t0) * 1e6 / 64)
            ms = C.c_float()
            pkg.binding.check(reg._lib.goicp_time_icp_pass(reg.handle, fp(I9), fp(Z3), 20, C.byref(ms)))
            ps.append(ms.value * 1e3)
        out["metric%d" % metric] = {"single_us": statistics.median(single), "single_us_all": single,
                                    "batch64_us_per_pose": statistics.median(batch), "batch64_us_per_pose_all": batch,
                                    "icp_pass_us": statistics.median(ps), "icp_pass_us_all": ps,
                                    "rank": info["rank"], "sigma": float(np.sqrt(info["sigma2"])), "inliers": info["inliers"]}
    reg.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
