"""Batched multi-start ICP (goicp_icp_run_batch) against the same starts run one after another (goicp_icp_run).

Per workload and K: K seeded start poses (rotations up to 90 degrees about random axes, translations up to 0.05 per axis), one batch call
(wall ms, median of --reps), the passes it ran (counters.icp_iters; icp_step publishes the counters), pose-passes/s, then the same K starts
as K sequential goicp_icp_run calls (wall ms) and the speed-up.  Every pose of the batch is checked bit for bit against its sequential run.
Writes one JSON object (--out, default stdout).

    python tools/icp_batch_probe.py --out profiles/icp_batch_probe.json [--reps 3] [--only bunny] [--K 1,4,16,64,256]
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


def _pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()
    return m


def workloads():
    from conftest import cloud, skull_problem
    return {
        "bunny": lambda: (cloud("model_bunny"), cloud("data_bunny"), 10000),                  # N 30 379: strided pass
        "skull": lambda: skull_problem()[:2] + (10000,),                                     # N ~29.5 k, M 98 k
        "spanner": lambda: (cloud("spanner_target"), cloud("spanner_source"), 100),          # N 150 k: neighbour pass (max_iter 100)
    }


def starts(K, seed):
    rng = np.random.default_rng(seed)
    R = np.empty((K, 3, 3), np.float32)
    for k in range(K):
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * np.deg2rad(rng.uniform(0, 90))
        th = np.linalg.norm(v)
        W = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]) / max(th, 1e-30)
        R[k] = np.eye(3) + np.sin(th) * W + (1 - np.cos(th)) * W @ W
    return R, rng.uniform(-0.05, 0.05, (K, 3)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--K", default="1,4,16,64,256")
    ap.add_argument("--no-sequential", action="store_true", help="batch calls only (kernel traces)")
    a = ap.parse_args()
    pkg = _pkg()
    fp = C.POINTER(C.c_float)
    Ks = [int(x) for x in a.K.split(",")]
    out = {"reps": a.reps, "err_diff": 1e-7, "workloads": {}}
    for name, make in workloads().items():
        if a.only and name not in a.only.split(","):
            continue
        target, source, max_iter = make()
        reg = pkg.Registration(target, source, 1e-3)
        w = {"N": len(source), "M": len(target), "max_iter": max_iter, "rows": []}
        R0, t0 = starts(4, 99)
        reg.icp_run_batch(R0, t0, max_iter, 1e-7)                                 # warm-up: code objects, buffers
        for K in Ks:
            R0, t0 = starts(K, 1000 + K)
            times = []
            for _ in range(a.reps):
                p0 = reg.icp_step().counters.icp_iters
                t1 = time.perf_counter()
                R, t, err, it = reg.icp_run_batch(R0, t0, max_iter, 1e-7)
                times.append((time.perf_counter() - t1) * 1e3)
                passes = reg.icp_step().counters.icp_iters - p0 - 1
            row = {"K": K, "batch_ms": statistics.median(times), "batch_ms_all": times, "passes": int(passes), "iters": int(it.sum()),
                   "pose_passes_per_s": passes / (statistics.median(times) * 1e-3)}
            if not a.no_sequential:
                seq = []
                for _ in range(a.reps):
                    same = True
                    t1 = time.perf_counter()
                    for k in range(K):
                        Rk, tk = R0[k].reshape(9).copy(), t0[k].copy()
                        e, n = C.c_float(), C.c_int32()
                        pkg.binding.check(reg._lib.goicp_icp_run(reg.handle, Rk.ctypes.data_as(fp), tk.ctypes.data_as(fp), max_iter, 1e-7,
                                                                 C.byref(e), C.byref(n)))
                        same &= bool(np.array_equal(Rk, R[k].reshape(9)) and np.array_equal(tk, t[k]) and e.value == err[k] and n.value == it[k])
                    seq.append((time.perf_counter() - t1) * 1e3)
                row.update(sequential_ms=statistics.median(seq), sequential_ms_all=seq, speedup=statistics.median(seq) / statistics.median(times),
                           bit_identical=same)
            w["rows"].append(row)
            print(name, json.dumps(row), file=sys.stderr, flush=True)
        reg.close()
        out["workloads"][name] = w
    s = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")
    else:
        print(s)


if __name__ == "__main__":
    main()
