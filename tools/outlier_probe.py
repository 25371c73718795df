"""Radius outlier removal: what the device filter costs next to the host function and next to a raw-cloud swap, and what a registration
gains from a source without its clutter.

Per case -- bunny (30 k source points), spanner (150 k / 150 k), the synthetic 1 M / 1 M cloud of bench.py's s2 workload -- the source gets
5 % uniform clutter in its bounding box (shuffled in), min_neighbors = 4, and the radius is bisected (on the host function) so that about
95 % of the clutter goes:
  (a) device_filter_ms      the device filter alone (HIP events around launch_radius_outlier_removal: the "device outlier" figure of the
                            verbose line of goicp_set_source_filtered)
  (b) host_ms               goicp_radius_outlier_removal_host on the same cloud, wall time on the same machine
  (c) device_wall_ms        goicp_radius_outlier_removal as a whole: upload, allocations, filter, read-back
  (d) set_source_filtered_ms  goicp_set_source_filtered(S, radius, 4) wall time, next to set_source_raw_ms: goicp_set_source(S) of the
                            cluttered cloud, both on a handle created with (T, S0), S0 = every second point of S in reverse order, and
                            swapped back to S0 in between
  (e) register_*_ms         goicp_register on the filtered source and on the cluttered source under the handle's default options (the poll
                            snapshot's register_ms), alternated, and the distance between the two optima
Every figure is the median of --reps runs after a dropped warm-up and is kept per repetition; a registration that does not finish inside
--limit seconds is cancelled, recorded as such and not repeated.  No figure is a pass mark.  Every case runs in a child process of its own
under `timeout -k 10`, one after the other; a child that fails or runs out of time ends the probe.  Writes one JSON object stamped with the
git head (GOICP_GIT_HEAD, else git) and goicp_kernel_source_hash.

    python tools/outlier_probe.py --out profiles/outlier_probe.json [--reps 5] [--only bunny,spanner,s2] [--limit 60] [--step-limit 420]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from set_source_probe import Stderr, _pkg, cases, med, register  # noqa: E402
from voxel_probe import pose_of  # noqa: E402

K = 4


def add_clutter(S, share=0.05, seed=1):
    rng = np.random.default_rng(seed)
    n = int(round(share * len(S)))
    clutter = np.float32(rng.uniform(S.min(0), S.max(0), (n, 3)))
    order = rng.permutation(len(S) + n)
    return np.ascontiguousarray(np.concatenate([S, clutter])[order], np.float32), order >= len(S)


def pick_radius(pkg, X, is_clutter, drop=0.95):
    """the radius at which the host function drops about `drop` of the clutter (bisection on log r; the share falls as r grows)"""
    ext = float(np.max(X.max(0) - X.min(0)))
    lo, hi = ext * 2.0 ** -12, ext * 0.25
    for _ in range(12):
        r = (lo * hi) ** 0.5
        idx = pkg.radius_outlier_removal(X, r, K)[1]
        keep = np.zeros(len(X), bool)
        keep[idx] = True
        gone = float((~keep[is_clutter]).mean())
        if gone > drop:
            lo = r
        else:
            hi = r
        if abs(gone - drop) <= 0.005:
            break
    return float(np.float32(r)), keep


def run_case(pkg, name, T, S, kw, reps, limit):
    mse = kw.pop("mse")
    T = np.ascontiguousarray(T, np.float32)
    X, is_clutter = add_clutter(np.ascontiguousarray(S, np.float32))
    S0 = np.ascontiguousarray(S[::-2], np.float32)
    fp = C.POINTER(C.c_float)
    radius, keep = pick_radius(pkg, X, is_clutter)
    m = int(keep.sum())
    res = {"n_target": len(T), "n_source": len(X), "n_clutter": int(is_clutter.sum()), "radius": radius, "min_neighbors": K, "n_kept": m,
           "clutter_dropped": round(float((~keep[is_clutter]).mean()), 4), "own_points_kept": round(float(keep[~is_clutter].mean()), 4),
           "mse_threshold": mse, **kw}
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pkg.radius_outlier_removal(X, radius, K)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_ms"] = {"all": [round(x, 3) for x in host], "median": med(host)}
    from cuda_go_icp_amd import binding
    f = binding.CSourceFilter(0.0, radius, K)
    dev, flt, raw, wall = [], [], [], []
    v = pkg.Registration(T, S0, mse, verbose=1, **kw)
    lib = v._lib
    for _ in range(reps + 1):                       # the first repetition warms the kernels up and is dropped
        kept = C.c_size_t(0)
        with Stderr() as err:
            t0 = time.perf_counter()
            assert lib.goicp_set_source_filtered(v.handle, X.ctypes.data_as(fp), len(X), C.byref(f), C.byref(kept)) == 0, lib.goicp_last_error()
            flt.append((time.perf_counter() - t0) * 1e3)
        assert kept.value == m
        g = re.search(r"set_source_filtered: .*device outlier ([0-9.]+) ms", err.text)
        dev.append(float(g.group(1)))
        with Stderr():
            v.set_source(S0)
            t0 = time.perf_counter()
            assert lib.goicp_set_source(v.handle, X.ctypes.data_as(fp), len(X)) == 0, lib.goicp_last_error()
            raw.append((time.perf_counter() - t0) * 1e3)
            v.set_source(S0)
            t0 = time.perf_counter()
            v.radius_outlier_removal(X, radius, K)
            wall.append((time.perf_counter() - t0) * 1e3)
    v.close()
    dev, flt, raw, wall = dev[1:], flt[1:], raw[1:], wall[1:]
    res["device_filter_ms"] = {"all": dev, "median": med(dev)}
    res["device_wall_ms"] = {"all": [round(x, 3) for x in wall], "median": med(wall)}
    res["set_source_filtered_ms"] = {"all": [round(x, 3) for x in flt], "median": med(flt)}
    res["set_source_raw_ms"] = {"all": [round(x, 3) for x in raw], "median": med(raw)}
    res["device_filter_beats_host"] = bool(med(dev) < med(host))
    res["device_call_beats_host"] = bool(med(wall) < med(host))
    # (e): a registration on the filtered source next to one on the cluttered source
    a = pkg.Registration(T, S0, mse, **kw)
    a.set_source(X, radius=radius, min_neighbors=K)
    b = pkg.Registration(T, S0, mse, **kw)
    b.set_source(X)
    ra, rb, done = [], [], True
    for _ in range(reps):
        ma, _, fa = register(a, limit)
        mb, _, fb = register(b, limit)
        ra.append(round(ma, 3)); rb.append(round(mb, 3))
        done = done and fa and fb
        if not done:
            break                                  # a cancelled search is not a timing
    Ra, ta, ea = pose_of(a)
    Rb, tb, eb = pose_of(b)
    a.close(); b.close()
    ang = float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))
    res["register_filtered_ms"] = {"all": ra, "median": med(ra)}
    res["register_raw_ms"] = {"all": rb, "median": med(rb)}
    res["register_finished_within_limit"] = done
    res["pose_distance"] = {"rotation_deg": round(ang, 5), "translation": round(float(np.linalg.norm(ta - tb)), 6)}
    res["mse_filtered"] = ea / m
    res["mse_raw"] = eb / len(X)
    print("%-8s r %.4g keeps %d of %d (clutter dropped %.3f, own kept %.3f) | filter: device %.3f ms, whole call %.2f ms, host %.2f ms | swap: filtered "
          "%.2f ms, raw %.2f ms | register filtered %.1f raw %.1f ms%s, optima %.4f deg / %.5f apart"
          % (name, radius, m, len(X), res["clutter_dropped"], res["own_points_kept"], res["device_filter_ms"]["median"], res["device_wall_ms"]["median"],
             res["host_ms"]["median"], res["set_source_filtered_ms"]["median"], res["set_source_raw_ms"]["median"], res["register_filtered_ms"]["median"],
             res["register_raw_ms"]["median"], "" if done else " (cancelled at the limit)", ang, res["pose_distance"]["translation"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="bunny,spanner,s2")
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--step-limit", type=int, default=420, help="seconds a case's child process may take (timeout -k 10)")
    ap.add_argument("--case", help="(internal) run this one case in this process and write its result to --out")
    args = ap.parse_args()
    if args.case:
        pkg = _pkg()
        (T, S, kw), = cases([args.case]).values()
        res = run_case(pkg, args.case, T, S, dict(kw), args.reps, args.limit)
        with open(args.out, "w") as f:
            json.dump({"kernel_source_hash": pkg.load_library().goicp_kernel_source_hash().decode(), "kernel_source_hash_of_tree": pkg.kernel_source_hash(),
                       "case": res}, f)
        return 0
    head = os.environ.get("GOICP_GIT_HEAD")
    if not head:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    out = {"git_head": head, "reps": args.reps, "cases": {}}
    for name in args.only.split(","):
        # this process never opens the GPU: every case is a child with a time limit of its own, and the first that fails ends the probe
        with tempfile.TemporaryDirectory() as d:
            part = os.path.join(d, "part.json")
            rc = subprocess.run(["timeout", "-k", "10", str(args.step_limit), sys.executable, os.path.abspath(__file__), "--case", name, "--out", part,
                                 "--reps", str(args.reps), "--limit", str(args.limit)]).returncode
            if rc != 0:
                print("case %s ended with status %d: the probe stops here" % (name, rc), flush=True)
                return rc
            p = json.load(open(part))
        out["kernel_source_hash"], out["kernel_source_hash_of_tree"] = p["kernel_source_hash"], p["kernel_source_hash_of_tree"]
        out["cases"][name] = p["case"]
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
