"""FPFH descriptors and descriptor matching: what the device path costs next to the host functions, and what the matches are worth
(DESIGN 25).

Timings, per case -- the source clouds of bunny (30 k points), spanner (150 k) and the synthetic 1 M cloud of bench.py's s2 workload --
in one process on one machine:
  (a) fpfh_device_ms   the self k-NN launch, spfh_kernel and fpfh_kernel (HIP events around launch_fpfh: the "device" figure of the
                       verbose line) at k = 16 over the device's own normals (k = 16, no viewpoint)
  (b) fpfh_wall_ms     goicp_fpfh as a whole: uploads, allocations, kernels, read-back
  (c) fpfh_host_ms     goicp_fpfh_host on the same cloud and normals, wall time
  (d) match_*          the same three figures for goicp_match_features (mutual flags included, i.e. both directions) between the
                       descriptors of the cloud and of a rigidly moved copy of it: bunny as it is, spanner voxel-reduced to about 20 k
                       points; s2 is not matched (10^12 pairs).  match_pair_rate is pairs of both directions per second of (a), and
                       match_flops_share that rate times 99 operations (33 subtractions, products and additions) over the vector fp32 peak
Quality, case "quality", at 6 000 points with k = 16 and at 2 000 points with k = 32: the bunny source reduced by a voxel grid against a
copy moved by a known rigid motion and reduced by a voxel grid of its own (another origin and other axes, so other points), normals
re-estimated towards the moved viewpoint:
  (e) mutual_matches, within_2_spacings   the mutual matches, and the share of them whose target point lies within twice the median
                       nearest-neighbour distance of the moved query point
  (f) triples_refined_to_optimum   of 64 poses, each the least-squares motion of a random triple of mutual matches, how many
                       goicp_icp_run_batch refines to within 1 degree and two spacings of the pose goicp_register finds (and of the true
                       motion: triples_refined_to_truth)
Every device figure is the median of --reps runs after a dropped warm-up and is kept per repetition; the host figures are single runs
for matching and the median of --host-reps runs for the descriptors.  No figure is a pass mark.  Every case runs in a child process of its
own under `timeout -k 10`, one after the other; a child that fails or runs out of time ends the probe.  Writes one JSON object stamped with
the git head (GOICP_GIT_HEAD, else git) and goicp_kernel_source_hash.

    python tools/fpfh_probe.py --out profiles/fpfh_probe.json [--reps 3] [--host-reps 2] [--only bunny,spanner,s2,quality] [--step-limit 420]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from set_source_probe import Stderr, _pkg, cases, med  # noqa: E402

K, NORMAL_K = 16, 16
QUALITY = ((6000, 16, 16), (2000, 32, 32))      # points after the voxel grid, k of the descriptors, k of the normals
PEAK_VECTOR_FP32 = 157.3e12


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def rodrigues(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K_ = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K_ + (1 - np.cos(th)) * K_ @ K_


def moved(X, R, t):
    return np.ascontiguousarray(X.astype(np.float64) @ R.T + t, np.float32)


def voxel_to(pkg, X, want):
    """the cloud reduced by the voxel grid that leaves about `want` points (bisection on the pitch, on the host)"""
    lo, hi = 0.0, float((X.max(0) - X.min(0)).max())
    for _ in range(18):
        mid = 0.5 * (lo + hi)
        m = len(pkg.voxel_downsample(X, mid)[0])
        if m > want:
            lo = mid
        else:
            hi = mid
        if abs(m - want) <= 0.02 * want:
            break
    return pkg.voxel_downsample(X, mid)[0], mid


def summary(vals):
    return {"all": [round(x, 3) for x in vals], "median": med(vals)}


def run_case(pkg, name, T, S, kw, reps, host_reps):
    mse = kw.pop("mse")
    X = np.ascontiguousarray(S, np.float32)
    n = len(X)
    res = {"n": n, "k": K, "normal_k": NORMAL_K}
    small_T = np.ascontiguousarray(T[:: max(1, len(T) // 4000)], np.float32)
    v = pkg.Registration(small_T, np.ascontiguousarray(X[::-2][:2000]), mse, verbose=1, **kw)
    with Stderr():
        nrm = v.estimate_normals(X, NORMAL_K)[0]
    host = []
    for _ in range(host_reps):
        ms, hf = timed(lambda: pkg.fpfh(X, K, nrm))
        host.append(ms)
    res["fpfh_host_ms"] = summary(host)
    dev, wall = [], []
    for _ in range(reps + 1):                       # the first repetition warms the kernels up and is dropped
        with Stderr() as err:
            ms, df = timed(lambda: v.fpfh(X, K, nrm))
        wall.append(ms)
        dev.append(float(re.search(r"fpfh: k \d+, device ([0-9.]+) ms", err.text).group(1)))
    assert df[0].tobytes() == hf[0].tobytes() and df[1].tobytes() == hf[1].tobytes(), "fpfh: the device and the host disagree"
    res["fpfh_device_ms"], res["fpfh_wall_ms"] = summary(dev[1:]), summary(wall[1:])
    line = "%-8s n %d k %d | fpfh: kernels %.3f ms, call %.2f ms, host %.1f ms" % (name, n, K, res["fpfh_device_ms"]["median"], res["fpfh_wall_ms"]["median"],
                                                                                   res["fpfh_host_ms"]["median"])
    if name in ("bunny", "spanner"):
        A = X
        if name == "spanner":
            A, pitch = voxel_to(pkg, X, 20000)
            res["match_voxel"] = pitch
        B = moved(A, rodrigues([0.3, -0.5, 0.8], 25.0), np.array([0.04, -0.03, 0.05]))
        with Stderr():
            fa = v.fpfh(A, K)[0]
            fb = v.fpfh(B, K)[0]
        ms, hm = timed(lambda: pkg.match_features(fa, fb))
        res["match_host_ms"] = summary([ms])
        dev, wall = [], []
        for _ in range(reps + 1):
            with Stderr() as err:
                ms, dm = timed(lambda: v.match_features(fa, fb))
            wall.append(ms)
            dev.append(float(re.search(r"match_features: \d+ x \d+, device ([0-9.]+) ms", err.text).group(1)))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dm, hm)), "match: the device and the host disagree"
        res["match_n"] = [len(fa), len(fb)]
        res["match_device_ms"], res["match_wall_ms"] = summary(dev[1:]), summary(wall[1:])
        rate = 2.0 * len(fa) * len(fb) / (res["match_device_ms"]["median"] * 1e-3)
        res["match_pair_rate"] = rate
        res["match_flops_share"] = round(rate * 99 / PEAK_VECTOR_FP32, 4)
        res["match_mutual"] = int(dm[3].sum())
        line += " | match %d x %d: kernels %.3f ms, call %.2f ms, host %.1f ms, %.3g pairs/s = %.1f %% of the vector fp32 peak" % (
            len(fa), len(fb), res["match_device_ms"]["median"], res["match_wall_ms"]["median"], res["match_host_ms"]["median"], rate,
            100 * res["match_flops_share"])
    v.close()
    print(line, flush=True)
    return res


def kabsch(a, b):
    """the least-squares rigid motion a -> b of two (m, 3) point sets"""
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cb - R @ ca


def angle_deg(Ra, Rb):
    return float(np.rad2deg(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def run_quality(pkg, limit, want, k, normal_k):
    from conftest import cloud
    X = np.ascontiguousarray(cloud("data_bunny"), np.float32)
    Rt, tt = rodrigues([0.3, -0.5, 0.8], 25.0), np.array([0.04, -0.03, 0.05])
    vp = (X.max(0) + np.float32(2.0)).astype(np.float32)
    A, pitch = voxel_to(pkg, X, want)
    B = pkg.voxel_downsample(moved(X, Rt, tt), pitch)[0]
    vpB = (Rt @ vp.astype(np.float64) + tt).astype(np.float32)
    res = {"n_query": len(A), "n_target": len(B), "voxel": pitch, "k": k, "normal_k": normal_k, "rotation_deg": 25.0, "translation": tt.tolist()}
    reg = pkg.Registration(B, A, 1e-3)
    fa = reg.fpfh(A, k, normal_k=normal_k, viewpoint=vp)[0]
    fb = reg.fpfh(B, k, normal_k=normal_k, viewpoint=vpB)[0]
    idx, d2, second, mutual = reg.match_features(fa, fb)
    spacing = float(np.median(np.sqrt(pkg.knn_self(B, 1)[1][:, 0])))
    keep = np.flatnonzero(mutual)
    err = np.linalg.norm(B[idx[keep]].astype(np.float64) - (A[keep].astype(np.float64) @ Rt.T + tt), axis=1)
    res.update(median_spacing=spacing, mutual_matches=int(len(keep)), within_2_spacings=round(float((err <= 2 * spacing).mean()), 4),
               all_matches_within_2_spacings=round(float((np.linalg.norm(B[idx].astype(np.float64) - (A.astype(np.float64) @ Rt.T + tt), axis=1)
                                                          <= 2 * spacing).mean()), 4))
    # the pose of the search, cancelled after `limit` seconds
    lib = reg._lib
    timer = threading.Timer(limit, lambda: lib.goicp_cancel(reg.handle))
    timer.start()
    t0 = time.perf_counter()
    assert lib.goicp_register(reg.handle) == 0, lib.goicp_last_error()
    wall = time.perf_counter() - t0
    timer.cancel()
    r = reg.poll()
    Ro, to = np.array(r.optR, np.float64).reshape(3, 3), np.array(r.optT, np.float64)
    res.update(register_s=round(wall, 3), register_finished=bool(wall < limit), register_off_truth_deg=round(angle_deg(Ro, Rt), 4),
               register_off_truth_translation=round(float(np.linalg.norm(to - tt)), 6))
    rng = np.random.default_rng(0)
    Rs, ts = [], []
    for _ in range(64):
        tri = rng.choice(keep, 3, replace=False)
        R, t = kabsch(A[tri].astype(np.float64), B[idx[tri]].astype(np.float64))
        Rs.append(R)
        ts.append(t)
    Rr, tr, e, it = reg.icp_run_batch(np.array(Rs), np.array(ts), 100, 1e-7)
    near = lambda R, t, R0, t0: angle_deg(R.astype(np.float64), R0) <= 1.0 and float(np.linalg.norm(t.astype(np.float64) - t0)) <= 2 * spacing
    res["triples"] = 64
    res["triples_start_within_10_deg_of_truth"] = int(sum(angle_deg(R, Rt) <= 10.0 for R in Rs))
    res["triples_refined_to_optimum"] = int(sum(near(Rr[k], tr[k], Ro, to) for k in range(64)))
    res["triples_refined_to_truth"] = int(sum(near(Rr[k], tr[k], Rt, tt) for k in range(64)))
    res["icp_iterations_median"] = float(np.median(it))
    reg.close()
    print("quality  %d x %d points, k %d, normal k %d, spacing %.4g | %d mutual matches, %.1f %% within two spacings (all matches: %.1f %%) | register %.2f s (%s), %.3f deg off "
          "the truth | of 64 triples %d start within 10 deg, %d refine to the optimum, %d to the truth"
          % (len(A), len(B), k, normal_k, spacing, len(keep), 100 * res["within_2_spacings"], 100 * res["all_matches_within_2_spacings"], wall,
             "finished" if res["register_finished"] else "cancelled", res["register_off_truth_deg"], res["triples_start_within_10_deg_of_truth"],
             res["triples_refined_to_optimum"], res["triples_refined_to_truth"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--only", default="bunny,spanner,s2,quality")
    ap.add_argument("--step-limit", type=int, default=420, help="seconds a case's child process may take (timeout -k 10)")
    ap.add_argument("--register-limit", type=float, default=15.0, help="seconds before the quality case cancels goicp_register")
    ap.add_argument("--case", help="(internal) run this one case in this process and write its result to --out")
    args = ap.parse_args()
    if args.case:
        pkg = _pkg()
        if args.case == "quality":
            res = [run_quality(pkg, args.register_limit, want, k, nk) for want, k, nk in QUALITY]
        else:
            (T, S, kw), = cases([args.case]).values()
            res = run_case(pkg, args.case, T, S, dict(kw), args.reps, args.host_reps)
        with open(args.out, "w") as f:
            json.dump({"kernel_source_hash": pkg.load_library().goicp_kernel_source_hash().decode(), "kernel_source_hash_of_tree": pkg.kernel_source_hash(),
                       "case": res}, f)
        return 0
    head = os.environ.get("GOICP_GIT_HEAD")
    if not head:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    out = {"git_head": head, "reps": args.reps, "host_reps": args.host_reps, "cases": {}}
    for name in args.only.split(","):
        # this process never opens the GPU: every case is a child with a time limit of its own, and the first that fails ends the probe
        with tempfile.TemporaryDirectory() as d:
            part = os.path.join(d, "part.json")
            rc = subprocess.run(["timeout", "-k", "10", str(args.step_limit), sys.executable, os.path.abspath(__file__), "--case", name, "--out", part,
                                 "--reps", str(args.reps), "--host-reps", str(args.host_reps), "--register-limit", str(args.register_limit)]).returncode
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
