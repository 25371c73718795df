"""Euclidean / DBSCAN clustering: what the device path costs next to the host function, what the clustered swap costs next to the pipeline
swap, and what a registration gains when a second dense object is cut away before it.

Per case -- bunny (30 k source points), spanner (150 k / 150 k), the synthetic 1 M / 1 M cloud of bench.py's s2 workload -- the source gets
5 % uniform clutter in its bounding box (tools/outlier_probe.py's cloud) PLUS one dense foreign object: a ball of 10 % of the points, of a
diameter of 0.3 of the cloud's largest extent, centred one extent beside the box, all shuffled in.  The cluster radius and min_neighbors
are the radius filter's of profiles/outlier_probe.json for the case; the selection keeps the largest cluster.
  (a) device_kernels_ms     the device work of goicp_cluster_filter alone (HIP events around launch_cluster and launch_cluster_compact: the
                            figure of the verbose line), next to device_wall_ms, the whole call (upload, allocations, read-back), and
                            host_ms, goicp_cluster_filter_host on the same cloud, wall time on the same machine
  (b) set_source_clustered_ms  goicp_set_source_clustered (statistical filter k = 20, std_ratio = 2, then keep-largest-cluster) wall time,
                            next to set_source_pipeline_ms, the same swap without the cluster stage, both on a handle created with
                            (T, S0), S0 = every second point of S in reverse order; device_cluster_stage_ms is the stage's share
  (c) register_*_ms         goicp_register under the handle's default options (the poll snapshot's register_ms) on the source behind (i)
                            the statistical filter alone and (ii) statistical filter + keep-largest-cluster, alternated, and angle_*_deg,
                            the angle between each optimum's rotation and the optimum of the clean cloud S
  (d) twice_the_radius      the partition and one registration of (ii) at 2 r: a scan whose own surface has gaps wider than r falls apart
                            at r, and this shows how much of that a wider radius mends
Every figure is the median of --reps runs after a dropped warm-up and is kept per repetition; a registration that does not finish inside
--limit seconds is cancelled, recorded as such and not repeated.  No figure is a pass mark.  Every case runs in a child process of its own
under `timeout -k 10`, one after the other; a child that fails or runs out of time ends the probe.  Writes one JSON object stamped with
the git head (GOICP_GIT_HEAD, else git) and goicp_kernel_source_hash.

    python tools/cluster_probe.py --out profiles/cluster_probe.json [--reps 3] [--only bunny,spanner,s2] [--limit 20] [--step-limit 420]
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
from stat_outlier_probe import ALPHA, K, radius_settings  # noqa: E402


def add_object(X, kind, share=0.10, seed=2):
    """a ball of share * len(X) points, diameter 0.3 of the largest extent, centred one extent beside the box along x -> (cloud, kind),
    kind 0 own point, 1 clutter, 2 the object"""
    rng = np.random.default_rng(seed)
    n = int(round(share * len(X)))
    lo, hi = X.min(0), X.max(0)
    ext = float((hi - lo).max())
    v = rng.normal(size=(n, 3))
    ball = v / np.linalg.norm(v, axis=1)[:, None] * (0.15 * ext * rng.uniform(0, 1, (n, 1)) ** (1.0 / 3.0))
    ball += np.array([hi[0] + ext, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
    order = rng.permutation(len(X) + n)
    return (np.ascontiguousarray(np.concatenate([X, np.float32(ball)])[order], np.float32),
            np.concatenate([kind, np.full(n, 2, np.int8)])[order])


def angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).reshape(3, 3).T @ np.asarray(Rb, np.float64).reshape(3, 3)) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def run_case(pkg, name, T, S, kw, reps, limit):
    mse = kw.pop("mse")
    T = np.ascontiguousarray(T, np.float32)
    S = np.ascontiguousarray(S, np.float32)
    X, is_clutter = add_clutter(S)
    X, kind = add_object(X, is_clutter.astype(np.int8))
    S0 = np.ascontiguousarray(S[::-2], np.float32)
    radius, min_neighbors = radius_settings(name)
    sel = (radius, min_neighbors, 0, 1)
    fp = C.POINTER(C.c_float)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx = pkg.cluster_filter(X, *sel)[1]
        host.append((time.perf_counter() - t0) * 1e3)
    labels, sizes = pkg.cluster(X, radius, min_neighbors)
    keep = np.zeros(len(X), bool)
    keep[idx] = True
    res = {"n_target": len(T), "n_source": len(X), "n_clutter": int((kind == 1).sum()), "n_object": int((kind == 2).sum()), "radius": radius,
           "min_neighbors": min_neighbors, "clusters": len(sizes), "largest_sizes": sorted(sizes.tolist())[-3:][::-1], "noise": int((labels < 0).sum()),
           "n_kept": int(keep.sum()), "object_dropped": round(float((~keep[kind == 2]).mean()), 4), "clutter_dropped": round(float((~keep[kind == 1]).mean()), 4),
           "own_points_kept": round(float(keep[kind == 0].mean()), 4), "stat_neighbors": K, "std_ratio": ALPHA, "mse_threshold": mse, **kw}
    res["host_ms"] = {"all": [round(x, 3) for x in host], "median": med(host)}
    from cuda_go_icp_amd import binding
    p = binding.CSourcePipeline(0.0, K, ALPHA, 0.0, 0)
    cs = binding.CClusterSelect(*sel)
    dev, wall, clus, pipe, stage = [], [], [], [], []
    v = pkg.Registration(T, S0, mse, verbose=1, **kw)
    lib = v._lib
    for _ in range(reps + 1):                       # the first repetition warms the kernels up and is dropped
        with Stderr() as err:
            t0 = time.perf_counter()
            got = v.cluster_filter(X, *sel)[1]
            wall.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(got, idx)
        dev.append(float(re.search(r"cluster_filter: .*device ([0-9.]+) ms", err.text).group(1)))
        kept = C.c_size_t(0)
        with Stderr() as err:
            t0 = time.perf_counter()
            assert lib.goicp_set_source_clustered(v.handle, X.ctypes.data_as(fp), len(X), C.byref(p), C.byref(cs), C.byref(kept)) == 0, lib.goicp_last_error()
            clus.append((time.perf_counter() - t0) * 1e3)
        stage.append(float(re.search(r"set_source_clustered: .*device cluster ([0-9.]+) ms", err.text).group(1)))
        n_clustered = kept.value
        with Stderr():
            v.set_source(S0)
            t0 = time.perf_counter()
            assert lib.goicp_set_source_pipeline(v.handle, X.ctypes.data_as(fp), len(X), C.byref(p), C.byref(kept)) == 0, lib.goicp_last_error()
            pipe.append((time.perf_counter() - t0) * 1e3)
            v.set_source(S0)
        n_pipeline = kept.value
    v.close()
    dev, wall, clus, pipe, stage = dev[1:], wall[1:], clus[1:], pipe[1:], stage[1:]
    res["device_kernels_ms"] = {"all": dev, "median": med(dev)}
    res["device_wall_ms"] = {"all": [round(x, 3) for x in wall], "median": med(wall)}
    res["set_source_clustered_ms"] = {"all": [round(x, 3) for x in clus], "median": med(clus)}
    res["set_source_pipeline_ms"] = {"all": [round(x, 3) for x in pipe], "median": med(pipe)}
    res["device_cluster_stage_ms"] = {"all": stage, "median": med(stage)}
    res["n_after_pipeline"], res["n_after_clustered"] = int(n_pipeline), int(n_clustered)
    res["device_kernels_beat_host"] = bool(med(dev) < med(host))
    res["device_call_beats_host"] = bool(med(wall) < med(host))
    # (c): the clean cloud's optimum, then stat alone next to stat + keep-largest-cluster
    c = pkg.Registration(T, S, mse, **kw)
    mc, _, fc = register(c, limit)
    Rc = np.array(list(c.poll().optR), np.float64)
    c.close()
    res["register_clean_ms"], res["register_clean_finished"] = round(mc, 3), bool(fc)
    a = pkg.Registration(T, S0, mse, **kw)
    a.set_source(X, stat_neighbors=K, std_ratio=ALPHA)
    b = pkg.Registration(T, S0, mse, **kw)
    b.set_source(X, stat_neighbors=K, std_ratio=ALPHA, cluster_radius=radius, cluster_min_neighbors=min_neighbors, cluster_keep=1)
    ra, rb, fin_a, fin_b = [], [], True, True
    for _ in range(reps):
        if fin_a:                                  # a cancelled search is not a timing and is not repeated
            ma, _, fin_a = register(a, limit)
            ra.append(round(ma, 3))
            res["angle_stat_deg"] = round(angle_deg(a.poll().optR, Rc), 4)
        if fin_b:
            mb, _, fin_b = register(b, limit)
            rb.append(round(mb, 3))
            res["angle_stat_cluster_deg"] = round(angle_deg(b.poll().optR, Rc), 4)
    a.close(); b.close()
    # the same at twice the radius: a scan whose own surface has gaps wider than r falls apart at r (one registration, not a timing series)
    idx2 = pkg.cluster_filter(X, 2.0 * radius, min_neighbors, 0, 1)[1]
    keep2 = np.zeros(len(X), bool)
    keep2[idx2] = True
    w = pkg.Registration(T, S0, mse, **kw)
    w.set_source(X, stat_neighbors=K, std_ratio=ALPHA, cluster_radius=2.0 * radius, cluster_min_neighbors=min_neighbors, cluster_keep=1)
    mw, _, fw = register(w, limit)
    res["twice_the_radius"] = {"radius": 2.0 * radius, "n_kept": int(keep2.sum()), "object_dropped": round(float((~keep2[kind == 2]).mean()), 4),
                               "clutter_dropped": round(float((~keep2[kind == 1]).mean()), 4), "own_points_kept": round(float(keep2[kind == 0].mean()), 4),
                               "register_stat_cluster_ms": round(mw, 3), "finished_within_limit": bool(fw),
                               "angle_stat_cluster_deg": round(angle_deg(w.poll().optR, Rc), 4)}
    w.close()
    print("%-8s at 2 r: keeps %d (object dropped %.3f, own kept %.4f), register stat+cluster %.1f ms%s (%.3f deg)"
          % (name, keep2.sum(), res["twice_the_radius"]["object_dropped"], res["twice_the_radius"]["own_points_kept"], mw, "" if fw else " (cancelled)",
             res["twice_the_radius"]["angle_stat_cluster_deg"]), flush=True)
    res["register_stat_ms"] = {"all": ra, "median": med(ra), "finished_within_limit": bool(fin_a)}
    res["register_stat_cluster_ms"] = {"all": rb, "median": med(rb), "finished_within_limit": bool(fin_b)}
    print("%-8s %d clusters, keeps %d of %d (object dropped %.3f, clutter dropped %.3f, own kept %.4f) | filter: device %.3f ms, whole call %.2f ms, host %.2f ms | "
          "swap: clustered %.2f ms (cluster stage %.3f ms), pipeline %.2f ms | register clean %.1f ms, stat %.1f ms%s (%.3f deg), stat+cluster %.1f ms%s (%.3f deg)"
          % (name, len(sizes), res["n_kept"], len(X), res["object_dropped"], res["clutter_dropped"], res["own_points_kept"], med(dev), med(wall), med(host),
             med(clus), med(stage), med(pipe), mc, med(ra), "" if fin_a else " (cancelled)", res["angle_stat_deg"], med(rb), "" if fin_b else " (cancelled)",
             res["angle_stat_cluster_deg"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="bunny,spanner,s2")
    ap.add_argument("--limit", type=float, default=20.0)
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
