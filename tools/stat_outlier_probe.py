"""Statistical outlier removal: what the device filter costs next to the host function and next to the radius filter's swap, how many grid
levels it takes, and what a registration gains from a source without its clutter.

Per case -- bunny (30 k source points), spanner (150 k / 150 k), the synthetic 1 M / 1 M cloud of bench.py's s2 workload -- the source gets
5 % uniform clutter in its bounding box (shuffled in, tools/outlier_probe.py's cloud), k = 20, std_ratio = 2:
  (a) device_filter_ms      the device filter alone (HIP events around launch_stat_outlier_removal: the "device statistical" figure of the
                            verbose line of goicp_set_source_pipeline), with the levels that ran and the share of points each resolved
  (b) host_ms               goicp_statistical_outlier_removal_host on the same cloud, wall time on the same machine
  (c) device_wall_ms        goicp_statistical_outlier_removal as a whole: upload, allocations, filter, read-back
  (d) set_source_pipeline_ms  goicp_set_source_pipeline(S, k, std_ratio) wall time, next to set_source_filtered_ms:
                            goicp_set_source_filtered of the same cloud at the radius and min_neighbors recorded for the case in
                            profiles/outlier_probe.json, both on a handle created with (T, S0), S0 = every second point of S in reverse order
  (e) register_*_ms         goicp_register on the filtered source and on the cluttered source under the handle's default options (the poll
                            snapshot's register_ms), alternated
Every figure is the median of --reps runs after a dropped warm-up and is kept per repetition; a registration that does not finish inside
--limit seconds is cancelled, recorded as such and not repeated.  No figure is a pass mark: the yardsticks are the host function and the
radius filter on the same machine.  Every case runs in a child process of its own under `timeout -k 10`, one after the other; a child that
fails or runs out of time ends the probe.  Writes one JSON object stamped with the git head (GOICP_GIT_HEAD, else git) and
goicp_kernel_source_hash.

    python tools/stat_outlier_probe.py --out profiles/stat_outlier_probe.json [--reps 5] [--only bunny,spanner,s2] [--limit 60] [--step-limit 420]
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

from outlier_probe import add_clutter  # noqa: E402
from set_source_probe import Stderr, _pkg, cases, med, register  # noqa: E402

K, ALPHA = 20, 2.0


def radius_settings(name):
    """the radius and min_neighbors the radius filter's probe settled on for this case"""
    with open(os.path.join(ROOT, "profiles", "outlier_probe.json")) as f:
        c = json.load(f)["cases"][name]
    return float(c["radius"]), int(c["min_neighbors"])


def run_case(pkg, name, T, S, kw, reps, limit):
    mse = kw.pop("mse")
    T = np.ascontiguousarray(T, np.float32)
    X, is_clutter = add_clutter(np.ascontiguousarray(S, np.float32))
    S0 = np.ascontiguousarray(S[::-2], np.float32)
    fp = C.POINTER(C.c_float)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx = pkg.statistical_outlier_removal(X, K, ALPHA)[1]
        host.append((time.perf_counter() - t0) * 1e3)
    keep = np.zeros(len(X), bool)
    keep[idx] = True
    m = int(keep.sum())
    radius, min_neighbors = radius_settings(name)
    res = {"n_target": len(T), "n_source": len(X), "n_clutter": int(is_clutter.sum()), "neighbors": K, "std_ratio": ALPHA, "n_kept": m,
           "clutter_dropped": round(float((~keep[is_clutter]).mean()), 4), "own_points_kept": round(float(keep[~is_clutter].mean()), 4),
           "radius_filter": {"radius": radius, "min_neighbors": min_neighbors}, "mse_threshold": mse, **kw}
    res["host_ms"] = {"all": [round(x, 3) for x in host], "median": med(host)}
    from cuda_go_icp_amd import binding
    p = binding.CSourcePipeline(0.0, K, ALPHA, 0.0, 0)
    f = binding.CSourceFilter(0.0, radius, min_neighbors)
    dev, pipe, flt, wall, rad_dev, levels = [], [], [], [], [], None
    v = pkg.Registration(T, S0, mse, verbose=1, **kw)
    lib = v._lib
    for _ in range(reps + 1):                       # the first repetition warms the kernels up and is dropped
        kept = C.c_size_t(0)
        with Stderr() as err:
            t0 = time.perf_counter()
            assert lib.goicp_set_source_pipeline(v.handle, X.ctypes.data_as(fp), len(X), C.byref(p), C.byref(kept)) == 0, lib.goicp_last_error()
            pipe.append((time.perf_counter() - t0) * 1e3)
        assert kept.value == m
        dev.append(float(re.search(r"set_source_pipeline: .*device statistical ([0-9.]+) ms", err.text).group(1)))
        g = re.search(r"statistical stage: \d+ -> \d+ points, levels (\d+), resolved((?: \d+)*), top (\d+)", err.text)
        levels = {"levels": int(g.group(1)), "resolved_share": [round(int(x) / len(X), 6) for x in g.group(2).split()], "top_share": round(int(g.group(3)) / len(X), 6)}
        with Stderr() as err:
            v.set_source(S0)
            t0 = time.perf_counter()
            assert lib.goicp_set_source_filtered(v.handle, X.ctypes.data_as(fp), len(X), C.byref(f), None) == 0, lib.goicp_last_error()
            flt.append((time.perf_counter() - t0) * 1e3)
        rad_dev.append(float(re.search(r"set_source_filtered: .*device outlier ([0-9.]+) ms", err.text).group(1)))
        with Stderr():
            v.set_source(S0)
            t0 = time.perf_counter()
            v.statistical_outlier_removal(X, K, ALPHA)
            wall.append((time.perf_counter() - t0) * 1e3)
    v.close()
    dev, pipe, flt, wall, rad_dev = dev[1:], pipe[1:], flt[1:], wall[1:], rad_dev[1:]
    res["device_filter_ms"] = {"all": dev, "median": med(dev)}
    res["device_levels"] = levels
    res["device_wall_ms"] = {"all": [round(x, 3) for x in wall], "median": med(wall)}
    res["set_source_pipeline_ms"] = {"all": [round(x, 3) for x in pipe], "median": med(pipe)}
    res["set_source_filtered_ms"] = {"all": [round(x, 3) for x in flt], "median": med(flt)}
    res["radius_device_filter_ms"] = {"all": rad_dev, "median": med(rad_dev)}
    res["device_filter_beats_host"] = bool(med(dev) < med(host))
    res["device_call_beats_host"] = bool(med(wall) < med(host))
    res["pipeline_swap_beats_filtered_swap"] = bool(med(pipe) < med(flt))
    # (e): a registration on the filtered source next to one on the cluttered source
    a = pkg.Registration(T, S0, mse, **kw)
    a.set_source(X, stat_neighbors=K, std_ratio=ALPHA)
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
    a.close(); b.close()
    res["register_filtered_ms"] = {"all": ra, "median": med(ra)}
    res["register_raw_ms"] = {"all": rb, "median": med(rb)}
    res["register_finished_within_limit"] = done
    print("%-8s keeps %d of %d (clutter dropped %.3f, own kept %.3f) | filter: device %.3f ms (levels %d, resolved %s, top %g), whole call %.2f ms, host %.2f ms | "
          "swap: pipeline %.2f ms, radius-filtered %.2f ms (device radius filter %.3f ms) | register filtered %.1f raw %.1f ms%s"
          % (name, m, len(X), res["clutter_dropped"], res["own_points_kept"], res["device_filter_ms"]["median"], levels["levels"], levels["resolved_share"],
             levels["top_share"], res["device_wall_ms"]["median"], res["host_ms"]["median"], res["set_source_pipeline_ms"]["median"],
             res["set_source_filtered_ms"]["median"], res["radius_device_filter_ms"]["median"], res["register_filtered_ms"]["median"],
             res["register_raw_ms"]["median"], "" if done else " (cancelled at the limit)"), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stat_outlier_probe.json"))
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
