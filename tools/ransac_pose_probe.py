"""RANSAC pose estimation from feature matches: what the device path costs next to the host function, and what the poses are worth
(DESIGN 26).

Timings, case "timing", T = 100 000 hypotheses, 8 poses, refit, edge similarity 0.9, in one process on one machine.  The correspondences
are the mutual FPFH matches of DESIGN 25's bunny pair (25 degrees) at 2 000 points / k = 32 and at 6 000 points / k = 16 (about 700 and
1 850 of them), and 20 000 synthetic ones (40 % true under a known pose, noise 0.005):
  (a) device_ms   the kernels, the sort and the read-backs (HIP events around launch_ransac_pose: the "device" figure of the verbose line)
  (b) wall_ms     goicp_ransac_pose as a whole: uploads, allocations, kernels, read-back
  (c) host_ms     goicp_ransac_pose_host on the same input, wall time (the yardstick), the median of --reps runs
Every device figure is the median of --reps runs after a dropped warm-up; every figure is kept per repetition.
Quality, case "quality": the bunny source reduced to about 2 000 points against a copy turned about (0.3, -0.5, 0.8) by each of --angles,
moved by (0.04, -0.03, 0.05) and reduced by a voxel grid of its own, k = 32 for descriptors and normals.  Per angle: does goicp_icp_run
from the identity end within 1 degree and two spacings of the truth; how many of the K = 64 RANSAC poses start within 10 degrees of the
truth without and with the ratio test (0.9); does register_features end at the truth and in what time; goicp_register's time and pose
(cancelled after --register-limit seconds).  ICP from the identity, register_features and goicp_register each run on a handle of their
own that has done nothing else, so none profits from another's state; their times do not include creating the handle.  first_angle_icp_fails is the smallest of --angles at which ICP from the identity fails.
No figure is a pass mark.  Every case runs in a child process of its own under `timeout -k 10`, one after the other; a child that fails
or runs out of time ends the probe.  Writes one JSON object stamped with the git head (GOICP_GIT_HEAD, else git) and
goicp_kernel_source_hash.

    python tools/ransac_pose_probe.py --out profiles/ransac_pose_probe.json [--reps 3] [--only timing,quality] [--step-limit 420]
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

from fpfh_probe import angle_deg, moved, rodrigues, timed, voxel_to  # noqa: E402
from set_source_probe import Stderr, _pkg, med  # noqa: E402

AXIS, SHIFT = [0.3, -0.5, 0.8], np.array([0.04, -0.03, 0.05])
T_TIMING = 100000


def summary(vals):
    return {"all": [round(x, 3) for x in vals], "median": med(vals)}


def feature_pair(pkg, reg, want, k, deg):
    """DESIGN 25's pair at `deg` degrees -> (A, B, match_features' output, the true motion, B's median spacing)"""
    from conftest import cloud
    X = np.ascontiguousarray(cloud("data_bunny"), np.float32)
    Rt = rodrigues(AXIS, deg)
    vp = (X.max(0) + np.float32(2.0)).astype(np.float32)
    A, pitch = voxel_to(pkg, X, want)
    B = pkg.voxel_downsample(moved(X, Rt, SHIFT), pitch)[0]
    vpB = (Rt @ vp.astype(np.float64) + SHIFT).astype(np.float32)
    fa = reg.fpfh(A, k, normal_k=k, viewpoint=vp)[0]
    fb = reg.fpfh(B, k, normal_k=k, viewpoint=vpB)[0]
    spacing = float(np.median(np.sqrt(pkg.knn_self(B, 1)[1][:, 0])))
    return A, B, reg.match_features(fa, fb), Rt, spacing, pitch, vp, vpB


def time_one(pkg, reg, name, src, tgt, corr, distance, reps):
    kw = dict(distance=distance, iterations=T_TIMING, refine=1, max_poses=8, edge_similarity=0.9, seed=0)
    host = []
    for _ in range(reps):
        ms, want = timed(lambda: pkg.ransac_pose(src, tgt, corr, **kw))
        host.append(ms)
    host_ms = med(host)
    dev, wall = [], []
    for _ in range(reps + 1):                       # the first repetition warms the kernels up and is dropped
        with Stderr() as err:
            ms, got = timed(lambda: reg.ransac_pose(src, tgt, corr, **kw))
        wall.append(ms)
        dev.append(float(re.search(r"ransac_pose: .* device ([0-9.]+) ms", err.text).group(1)))
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "ransac_pose: the device and the host disagree"
    res = {"M": int(len(corr)), "T": T_TIMING, "distance": distance, "poses": int(len(got[0])), "best_inliers": int(got[0][0]["inliers"]) if len(got[0]) else 0,
           "device_ms": summary(dev[1:]), "wall_ms": summary(wall[1:]), "host_ms": summary(host)}
    res["pairs_per_s_device"] = float(len(corr)) * T_TIMING / (res["device_ms"]["median"] * 1e-3)
    print("timing   %-10s M %5d T %d | kernels %.3f ms, call %.2f ms, host %.2f ms | %d poses, best %d inliers" % (
        name, len(corr), T_TIMING, res["device_ms"]["median"], res["wall_ms"]["median"], host_ms, res["poses"], res["best_inliers"]), flush=True)
    return res


def run_timing(pkg, reps):
    import ransac_twin as RT
    from conftest import cloud
    reg = pkg.Registration(np.ascontiguousarray(cloud("model_bunny")[::8]), np.ascontiguousarray(cloud("data_bunny")[::15]), 1e-3, verbose=1)
    out = {}
    with Stderr():
        pairs = [("bunny_2k", feature_pair(pkg, reg, 2000, 32, 25.0)), ("bunny_6k", feature_pair(pkg, reg, 6000, 16, 25.0))]
    for name, (A, B, m, _, spacing, _, _, _) in pairs:
        out[name] = time_one(pkg, reg, name, A, B, pkg.select_matches(*m), 3 * spacing, reps)
    src, tgt, corr, _ = RT.scene(20000, 0.4, 0.005, seed=3)
    out["synthetic_20k"] = time_one(pkg, reg, "synthetic", src, tgt, corr, 0.03, reps)
    reg.close()
    return out


def run_quality(pkg, angles, limit):
    from conftest import cloud
    out = {"angles": {}, "first_angle_icp_fails": None}
    lender = pkg.Registration(np.ascontiguousarray(cloud("model_bunny")[::8]), np.ascontiguousarray(cloud("data_bunny")[::15]), 1e-3)
    for deg in angles:
        A, B, m, Rt, spacing, pitch, vp, vpB = feature_pair(pkg, lender, 2000, 32, deg)
        reg = pkg.Registration(B, A, 1e-3)
        near = lambda R, t: angle_deg(np.asarray(R, np.float64), Rt) <= 1.0 and float(np.linalg.norm(np.asarray(t, np.float64) - SHIFT)) <= 2 * spacing
        res = {"n_query": len(A), "n_target": len(B), "voxel": pitch, "median_spacing": spacing, "mutual_matches": int(m[3].sum())}
        _, Ri, ti = pkg.IterativeClosestPoint3D(reg, 100, 1e-7).run()
        res["icp_from_identity_reaches_truth"] = bool(near(Ri, ti))
        res["icp_from_identity_off_truth_deg"] = round(angle_deg(Ri.astype(np.float64), Rt), 3)
        if not res["icp_from_identity_reaches_truth"] and out["first_angle_icp_fails"] is None:
            out["first_angle_icp_fails"] = deg
        for tag, ratio in (("no_ratio", 0.0), ("ratio_0.9", 0.9)):
            corr = pkg.select_matches(*m, ratio=ratio)
            true = np.linalg.norm(B[corr[:, 1]].astype(np.float64) - (A[corr[:, 0]].astype(np.float64) @ Rt.T + SHIFT), axis=1) <= 2 * spacing
            poses = reg.ransac_pose(A, B, corr, 3 * spacing, 100000, max_poses=64, seed=0)[0] if len(corr) >= 3 else []
            res[tag] = {"correspondences": int(len(corr)), "true_share": round(float(true.mean()), 4) if len(corr) else None, "poses": int(len(poses)),
                        "poses_within_10_deg": int(sum(angle_deg(p["R"].astype(np.float64), Rt) <= 10.0 for p in poses)),
                        "best_inliers": int(poses[0]["inliers"]) if len(poses) else 0,
                        "best_off_truth_deg": round(angle_deg(poses[0]["R"].astype(np.float64), Rt), 3) if len(poses) else None}
        reg.close()
        # register_features on a fresh handle's own clouds (they are A and B already: no voxel stage)
        reg = pkg.Registration(B, A, 1e-3)
        try:
            ms, (Rf, tf, ef, info) = timed(lambda: reg.register_features(0, 32, 3 * spacing, max_iter=100, normal_k=32, iterations=100000, max_poses=64,
                                                                         viewpoint_src=vp, viewpoint_tgt=vpB))
            res["register_features"] = {"ms": round(ms, 3), "reaches_truth": bool(near(Rf, tf)), "off_truth_deg": round(angle_deg(Rf.astype(np.float64), Rt), 3),
                                        "candidates": int(len(info["err"])), "err": float(ef)}
        except pkg.GoicpError as e:
            res["register_features"] = {"error": str(e)}
        reg.close()
        # goicp_register on another fresh handle
        reg = pkg.Registration(B, A, 1e-3)
        lib = reg._lib
        timer = threading.Timer(limit, lambda: lib.goicp_cancel(reg.handle))
        timer.start()
        t0 = time.perf_counter()
        assert lib.goicp_register(reg.handle) == 0, lib.goicp_last_error()
        wall = time.perf_counter() - t0
        timer.cancel()
        r = reg.poll()
        res["register"] = {"ms": round(wall * 1e3, 3), "finished": bool(wall < limit), "reaches_truth": bool(near(np.array(r.optR).reshape(3, 3), np.array(r.optT))),
                           "sse": float(r.best_sse), "rot_pops": int(r.counters.rot_pops), "trans_pops": int(r.counters.trans_pops)}
        reg.close()
        out["angles"][str(deg)] = res
        print("quality  %5.1f deg | ICP from identity %s (%.2f deg off) | poses within 10 deg: %d of %d (no ratio, %d pairs, %.0f %% true), %d of %d (ratio 0.9, %d pairs, "
              "%.0f %% true) | register_features %s | register %.3f ms %s, %s" % (
                  deg, "reaches the truth" if res["icp_from_identity_reaches_truth"] else "FAILS", res["icp_from_identity_off_truth_deg"],
                  res["no_ratio"]["poses_within_10_deg"], res["no_ratio"]["poses"], res["no_ratio"]["correspondences"], 100 * (res["no_ratio"]["true_share"] or 0),
                  res["ratio_0.9"]["poses_within_10_deg"], res["ratio_0.9"]["poses"], res["ratio_0.9"]["correspondences"], 100 * (res["ratio_0.9"]["true_share"] or 0),
                  res["register_features"], wall * 1e3, "finished" if res["register"]["finished"] else "cancelled",
                  "at the truth" if res["register"]["reaches_truth"] else "not at the truth"), flush=True)
    lender.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_pose_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="timing,quality")
    ap.add_argument("--angles", default="25,45,60,80,100,140")
    ap.add_argument("--step-limit", type=int, default=420, help="seconds a case's child process may take (timeout -k 10)")
    ap.add_argument("--register-limit", type=float, default=10.0, help="seconds before the quality case cancels goicp_register")
    ap.add_argument("--case", help="(internal) run this one case in this process and write its result to --out")
    args = ap.parse_args()
    if args.case:
        pkg = _pkg()
        res = run_timing(pkg, args.reps) if args.case == "timing" else run_quality(pkg, [float(a) for a in args.angles.split(",")], args.register_limit)
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
                                 "--reps", str(args.reps), "--angles", args.angles, "--register-limit", str(args.register_limit)]).returncode
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
