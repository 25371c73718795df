"""RANSAC plane segmentation: what the device path costs next to the host function, what the segmented swap costs next to the plain swap,
and what a registration gains when the floor under the object is cut away before it.

Per case -- the bunny scan and the spanner scan, each at 150 k and at 1 M points in all -- the object is 60 % of the points (the scan's own
points, every one once, as long as they last; the rest are copies with a jitter of sigma 0.002) and stands on a floor of the other 40 %: a
rectangle 10 % of the largest extent wider than the object's x-z box, at the object's min y, with noise sigma = distance / 3, all shuffled
in.  distance = 0.01, T = 1 000 hypotheses, one plane, refit on.  The cluster radius and min_neighbors are the radius filter's of
profiles/outlier_probe.json for the scan; the selection keeps the largest cluster.
  (a) device_kernels_ms     the device work of goicp_segment_plane alone (HIP events around launch_segment_plane, its read-backs of a key, a
                            plane and 16 words included: the figure of the verbose line), next to device_wall_ms, the whole call (upload,
                            allocations, labels back), and host_ms, goicp_segment_plane_host on the same cloud, wall time on the same machine
  (b) set_source_segmented_ms  goicp_set_source_segmented with the plane stage alone, wall time, next to set_source_plain_ms, goicp_set_source
                            of the same raw cloud, both on a handle created with (T, S0), S0 = every second point of the object in reverse
                            order; device_plane_stage_ms is the stage's share.  The two swaps end on different clouds (the segmented one
                            orders and mirrors 60 % of the points), so the difference is the stage's cost less what the smaller cloud saves
  (c) register_*_ms         goicp_register under the handle's default options (the poll snapshot's register_ms) on the source (i) as it is,
                            floor included, (ii) behind keep-largest-cluster alone and (iii) behind plane removal + keep-largest-cluster,
                            alternated, with the points each keeps, and angle_*_deg, the angle between each optimum's rotation and the
                            optimum of the object alone
Every figure is the median of --reps runs after a dropped warm-up and is kept per repetition; a registration that does not finish inside
--limit seconds is cancelled, recorded as such and not repeated.  No figure is a pass mark.  Every case runs in a child process of its own
under `timeout -k 10`, one after the other; a child that fails or runs out of time ends the probe.  Writes one JSON object stamped with
the git head (GOICP_GIT_HEAD, else git) and goicp_kernel_source_hash.

    python tools/plane_probe.py --out profiles/plane_probe.json [--reps 3] [--only bunny_150k,spanner_150k,bunny_1m,spanner_1m] [--limit 20]
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

from cluster_probe import angle_deg  # noqa: E402
from set_source_probe import Stderr, _pkg, cases, med, register  # noqa: E402
from stat_outlier_probe import radius_settings  # noqa: E402

DISTANCE, ITERATIONS, SEED = 0.01, 1000, 1
SIZES = {"150k": 150000, "1m": 1000000}


def on_a_floor(S, n, seed=3):
    """n points: 60 % the object (S's own points first, then jittered copies), 40 % the floor under it -> (cloud, is_floor, object)"""
    rng = np.random.default_rng(seed)
    n_obj = int(0.6 * n)
    S = np.asarray(S, np.float64)
    if n_obj <= len(S):
        obj = S[np.sort(rng.choice(len(S), n_obj, replace=False))]
    else:
        extra = n_obj - len(S)
        obj = np.concatenate([S, S[rng.integers(0, len(S), extra)] + rng.normal(0, 0.002, (extra, 3))])
    lo, hi = obj.min(0), obj.max(0)
    pad = 0.1 * float((hi - lo).max())
    nf = n - n_obj
    floor = np.c_[rng.uniform(lo[0] - pad, hi[0] + pad, nf), lo[1] + rng.normal(0, DISTANCE / 3, nf), rng.uniform(lo[2] - pad, hi[2] + pad, nf)]
    order = rng.permutation(n)
    return (np.ascontiguousarray(np.concatenate([obj, floor])[order], np.float32), (np.arange(n) >= n_obj)[order],
            np.ascontiguousarray(obj, np.float32))


def run_case(pkg, name, T, S, kw, n, reps, limit):
    mse = kw.pop("mse")
    T = np.ascontiguousarray(T, np.float32)
    X, is_floor, obj = on_a_floor(S, n)
    S0 = np.ascontiguousarray(obj[::-2], np.float32)
    radius, min_neighbors = radius_settings(name.split("_")[0])
    pk = dict(distance=DISTANCE, iterations=ITERATIONS, refine=1, max_planes=1, min_inliers=0, seed=SEED)
    fp = C.POINTER(C.c_float)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        want = pkg.segment_plane(X, **pk)
        host.append((time.perf_counter() - t0) * 1e3)
    res = {"n_target": len(T), "n_source": len(X), "n_floor": int(is_floor.sum()), "distance": DISTANCE, "iterations": ITERATIONS, "seed": SEED,
           "planes": int(len(want[1])), "plane_inliers": [int(p["inliers"]) for p in want[1]], "refined": [int(p["refined"]) for p in want[1]],
           "floor_share_taken": round(float(np.mean(want[0][is_floor] == 0)), 4), "object_share_taken": round(float(np.mean(want[0][~is_floor] == 0)), 4),
           "cluster_radius": radius, "cluster_min_neighbors": min_neighbors, "mse_threshold": mse, **kw}
    res["host_ms"] = {"all": [round(x, 3) for x in host], "median": med(host)}
    from cuda_go_icp_amd import binding
    pl = binding.CPlaneSelect(DISTANCE, ITERATIONS, 1, 1, 0, SEED)
    dev, wall, seg, plain, stage = [], [], [], [], []
    v = pkg.Registration(T, S0, mse, verbose=1, **kw)
    lib = v._lib
    same = True
    for _ in range(reps + 1):                       # the first repetition warms the kernels up and is dropped
        with Stderr() as err:
            t0 = time.perf_counter()
            got = v.segment_plane(X, **pk)
            wall.append((time.perf_counter() - t0) * 1e3)
        same = same and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        dev.append(float(re.search(r"segment_plane: .*device ([0-9.]+) ms", err.text).group(1)))
        kept = C.c_size_t(0)
        with Stderr() as err:
            t0 = time.perf_counter()
            assert lib.goicp_set_source_segmented(v.handle, X.ctypes.data_as(fp), len(X), None, C.byref(pl), None, C.byref(kept)) == 0, lib.goicp_last_error()
            seg.append((time.perf_counter() - t0) * 1e3)
        stage.append(float(re.search(r"device plane ([0-9.]+) ms", err.text).group(1)))
        n_segmented = kept.value
        with Stderr():
            v.set_source(S0)
            t0 = time.perf_counter()
            assert lib.goicp_set_source(v.handle, X.ctypes.data_as(fp), len(X)) == 0, lib.goicp_last_error()
            plain.append((time.perf_counter() - t0) * 1e3)
            v.set_source(S0)
    v.close()
    dev, wall, seg, plain, stage = dev[1:], wall[1:], seg[1:], plain[1:], stage[1:]
    res["same_bytes_as_host"] = bool(same)
    res["device_kernels_ms"] = {"all": dev, "median": med(dev)}
    res["device_wall_ms"] = {"all": [round(x, 3) for x in wall], "median": med(wall)}
    res["set_source_segmented_ms"] = {"all": [round(x, 3) for x in seg], "median": med(seg)}
    res["set_source_plain_ms"] = {"all": [round(x, 3) for x in plain], "median": med(plain)}
    res["device_plane_stage_ms"] = {"all": stage, "median": med(stage)}
    res["n_after_segmented"] = int(n_segmented)
    res["device_kernels_beat_host"] = bool(med(dev) < med(host))
    res["device_call_beats_host"] = bool(med(wall) < med(host))
    res["segmented_swap_beats_plain_swap"] = bool(med(seg) < med(plain))
    print("%-12s plane takes %.4f of the floor, %.4f of the object | segment: device %.3f ms, whole call %.2f ms, host %.2f ms, same bytes %s | "
          "swap: segmented %.2f ms (plane stage %.3f ms), plain %.2f ms" % (name, res["floor_share_taken"], res["object_share_taken"], med(dev), med(wall),
                                                                           med(host), same, med(seg), med(stage), med(plain)), flush=True)
    # (c): the object's own optimum, then the three settings
    c = pkg.Registration(T, obj, mse, **kw)
    mc, _, fc = register(c, limit)
    Rc = np.array(list(c.poll().optR), np.float64)
    c.close()
    res["register_object_alone_ms"], res["register_object_alone_finished"] = round(mc, 3), bool(fc)
    ckw = dict(cluster_radius=radius, cluster_min_neighbors=min_neighbors, cluster_keep=1)
    pkw = dict(plane_distance=DISTANCE, plane_iterations=ITERATIONS, plane_seed=SEED)
    settings = {"with_floor": {}, "cluster": ckw, "plane_cluster": dict(ckw, **pkw)}
    regs, ms, fin = {}, {k: [] for k in settings}, {k: True for k in settings}
    for k, skw in settings.items():
        regs[k] = pkg.Registration(T, S0, mse, **kw)
        regs[k].set_source(X, **skw)
        res["n_registered_" + k] = int(regs[k].ns)
    for _ in range(reps):
        for k in settings:
            if not fin[k]:                         # a cancelled search is not a timing and is not repeated
                continue
            m, _, fin[k] = register(regs[k], limit)
            ms[k].append(round(m, 3))
            res["angle_%s_deg" % k] = round(angle_deg(regs[k].poll().optR, Rc), 4)
            res["best_sse_" + k] = float(regs[k].poll().best_sse)
    for k in settings:
        regs[k].close()
        res["register_%s_ms" % k] = {"all": ms[k], "median": med(ms[k]), "finished_within_limit": bool(fin[k])}
    print("%-12s register: object alone %.1f ms%s | %s" % (name, mc, "" if fc else " (cancelled)", " | ".join(
        "%s %d points %.1f ms%s (%.3f deg)" % (k, res["n_registered_" + k], med(ms[k]), "" if fin[k] else " (cancelled)", res["angle_%s_deg" % k])
        for k in settings)), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="bunny_150k,spanner_150k,bunny_1m,spanner_1m")
    ap.add_argument("--limit", type=float, default=20.0)
    ap.add_argument("--step-limit", type=int, default=300, help="seconds a case's child process may take (timeout -k 10)")
    ap.add_argument("--case", help="(internal) run this one case in this process and write its result to --out")
    args = ap.parse_args()
    if args.case:
        pkg = _pkg()
        scan, size = args.case.split("_")
        (T, S, kw), = cases([scan]).values()
        res = run_case(pkg, args.case, T, S, dict(kw), SIZES[size], args.reps, args.limit)
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
