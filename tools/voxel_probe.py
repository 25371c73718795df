"""Voxel-grid downsampling: what the device reduction costs next to the host function and next to a raw-cloud swap, and what a registration
gains from a reduced source.

Per case -- bunny (30 k source points), spanner (150 k / 150 k), the synthetic 1 M / 1 M cloud of bench.py's s2 workload -- with the voxel
bisected (on the host function) so that about 1/8 of the source points remain:
  (a) device_reduction_ms   the device reduction alone (HIP events around launch_voxel_downsample: the "device voxel" figure of the
                            verbose line of goicp_set_source_voxel)
  (b) host_ms               goicp_voxel_downsample_host on the same cloud, wall time on the same machine
  (c) set_source_voxel_ms   goicp_set_source_voxel(S, voxel) wall time, next to set_source_raw_ms: goicp_set_source(S) of the raw cloud, both on
                            a handle created with (T, S0), S0 = every second point of S in reverse order, and swapped back to S0 in between
  (d) register_*_ms         goicp_register on the reduced source and on the raw source (the poll snapshot's register_ms), alternated, and the
                            distance between the two optima: the angle of R_reduced^T R_raw in degrees and |t_reduced - t_raw|
Every figure is the median of --reps runs and is kept per repetition.  No figure is a pass mark: the comparison points are the host function
and the raw-cloud swap of this same build.  Writes one JSON object stamped with the git head (GOICP_GIT_HEAD, else git) and
goicp_kernel_source_hash.

    python tools/voxel_probe.py --out profiles/voxel_probe.json [--reps 5] [--only bunny,spanner,s2] [--limit 120]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from set_source_probe import Stderr, _pkg, cases, med, register  # noqa: E402


def pick_voxel(pkg, S, keep=0.125):
    """the voxel at which the host function keeps about `keep` of the points (bisection on log v; m falls as v grows)"""
    ext = float(np.max(S.max(0) - S.min(0)))
    lo, hi = ext * 2.0 ** -18, ext
    for _ in range(24):
        v = (lo * hi) ** 0.5
        m = len(pkg.voxel_downsample(S, v)[0])
        if m > keep * len(S):
            lo = v
        else:
            hi = v
        if abs(m - keep * len(S)) <= 0.01 * keep * len(S):
            break
    return float(np.float32(v)), m


def pose_of(reg):
    r = reg.poll()
    return np.array(r.optR, np.float64).reshape(3, 3), np.array(r.optT, np.float64), float(r.best_sse)


def run_case(pkg, name, T, S, kw, reps, limit):
    mse = kw.pop("mse")
    T, S = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(S, np.float32)
    S0 = np.ascontiguousarray(S[::-2])
    fp = C.POINTER(C.c_float)
    voxel, m = pick_voxel(pkg, S)
    res = {"n_target": len(T), "n_source": len(S), "voxel": voxel, "n_kept": m, "kept_fraction": round(m / len(S), 4), "mse_threshold": mse, **kw}
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pkg.voxel_downsample(S, voxel)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_ms"] = {"all": [round(x, 3) for x in host], "median": med(host)}
    dev, vox, raw, down = [], [], [], []
    v = pkg.Registration(T, S0, mse, verbose=1, **kw)
    lib = v._lib
    for _ in range(reps + 1):                       # the first repetition warms the kernels up and is dropped
        kept = C.c_size_t(0)
        with Stderr() as err:
            t0 = time.perf_counter()
            assert lib.goicp_set_source_voxel(v.handle, S.ctypes.data_as(fp), len(S), voxel, C.byref(kept)) == 0, lib.goicp_last_error()
            vox.append((time.perf_counter() - t0) * 1e3)
        assert kept.value == m
        g = re.search(r"set_source_voxel: \d+ -> \d+ points, [0-9.]+ ms \(device voxel ([0-9.]+) ms", err.text)
        dev.append(float(g.group(1)))
        with Stderr():
            v.set_source(S0)
            t0 = time.perf_counter()
            assert lib.goicp_set_source(v.handle, S.ctypes.data_as(fp), len(S)) == 0, lib.goicp_last_error()
            raw.append((time.perf_counter() - t0) * 1e3)
            v.set_source(S0)
            t0 = time.perf_counter()
            v.voxel_downsample(S, voxel)
            down.append((time.perf_counter() - t0) * 1e3)
    v.close()
    dev, vox, raw, down = dev[1:], vox[1:], raw[1:], down[1:]
    res["device_reduction_ms"] = {"all": dev, "median": med(dev)}
    res["voxel_downsample_device_wall_ms"] = {"all": [round(x, 3) for x in down], "median": med(down)}
    res["set_source_voxel_ms"] = {"all": [round(x, 3) for x in vox], "median": med(vox)}
    res["set_source_raw_ms"] = {"all": [round(x, 3) for x in raw], "median": med(raw)}
    res["device_reduction_beats_host"] = bool(med(dev) < med(host))
    # (d): a registration on the reduced source next to one on the raw source
    a = pkg.Registration(T, S0, mse, **kw)
    a.set_source(S, voxel=voxel)
    b = pkg.Registration(T, S0, mse, **kw)
    b.set_source(S)
    ra, rb, done = [], [], True
    for _ in range(reps):
        ma, _, fa = register(a, limit)
        mb, _, fb = register(b, limit)
        ra.append(round(ma, 3)); rb.append(round(mb, 3))
        done = done and fa and fb
    Ra, ta, ea = pose_of(a)
    Rb, tb, eb = pose_of(b)
    a.close(); b.close()
    ang = float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))
    res["register_reduced_ms"] = {"all": ra, "median": med(ra)}
    res["register_raw_ms"] = {"all": rb, "median": med(rb)}
    res["register_finished_within_limit"] = done
    res["pose_distance"] = {"rotation_deg": round(ang, 5), "translation": round(float(np.linalg.norm(ta - tb)), 6)}
    res["mse_reduced"] = ea / m
    res["mse_raw"] = eb / len(S)
    print("%-8s voxel %.4g keeps %d of %d | reduction: device %.3f ms, host %.2f ms | swap: voxel %.2f ms, raw %.2f ms | register reduced %.1f raw %.1f ms, "
          "optima %.4f deg / %.5f apart" % (name, voxel, m, len(S), res["device_reduction_ms"]["median"], res["host_ms"]["median"],
                                             res["set_source_voxel_ms"]["median"], res["set_source_raw_ms"]["median"], res["register_reduced_ms"]["median"],
                                             res["register_raw_ms"]["median"], ang, res["pose_distance"]["translation"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="bunny,spanner,s2")
    ap.add_argument("--limit", type=float, default=120.0)
    args = ap.parse_args()
    pkg = _pkg()
    head = os.environ.get("GOICP_GIT_HEAD")
    if not head:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    out = {"git_head": head, "kernel_source_hash": pkg.load_library().goicp_kernel_source_hash().decode(),
           "kernel_source_hash_of_tree": pkg.kernel_source_hash(), "reps": args.reps, "cases": {}}
    for name, (T, S, kw) in cases(args.only.split(",")).items():
        out["cases"][name] = run_case(pkg, name, T, S, dict(kw), args.reps, args.limit)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
