"""Exact self k-NN and normal estimation of any cloud: what the device path costs next to the host function, next to the statistical
filter's search (the yardstick for what the 64-bit keys and the row writes cost) and next to the hierarchy path of a handle's own target
(goicp_target_normals), and how many grid levels it takes.

Per case -- the source clouds of bunny (30 k points), spanner (150 k) and the synthetic 1 M cloud of bench.py's s2 workload -- at k = 16,
in one process on one machine:
  (a) knn_device_ms / normals_device_ms   the kernels and read-backs alone (HIP events around launch_self_knn / launch_estimate_normals: the
                            "device" figure of the verbose lines), with the levels that ran and the share of points each resolved
  (b) knn_wall_ms / normals_wall_ms       goicp_knn_self / goicp_estimate_normals as a whole: upload, allocations, kernels, read-back
  (c) knn_host_ms / normals_host_ms       goicp_knn_self_host / goicp_estimate_normals_host on the same cloud, wall time
  (d) stat_device_ms / stat_wall_ms       the statistical filter at k = 16, std_ratio = 2, unchanged: its kernels (the "device statistical"
                            figure of goicp_set_source_pipeline's verbose line, the same launcher) and goicp_statistical_outlier_removal as a
                            whole
  (e) target_create_ms / target_normals_ms   goicp_create of a handle whose target is the same cloud, and goicp_set_icp_options(point-to-plane,
                            normal_k = 16) + goicp_target_normals on it: the k-d hierarchy path
Every device figure is the median of --reps runs after a dropped warm-up and is kept per repetition; the host figures are the median of
--host-reps runs.  No figure is a pass mark.  Every case runs in a child process of its own under `timeout -k 10`, one after the other; a
child that fails or runs out of time ends the probe.  Writes one JSON object stamped with the git head (GOICP_GIT_HEAD, else git) and
goicp_kernel_source_hash.

    python tools/normals_probe.py --out profiles/normals_probe.json [--reps 3] [--host-reps 3] [--only bunny,spanner,s2] [--step-limit 420]
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

from set_source_probe import Stderr, _pkg, cases, med  # noqa: E402

K, ALPHA = 16, 2.0


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run_case(pkg, name, T, S, kw, reps, host_reps):
    mse = kw.pop("mse")
    X = np.ascontiguousarray(S, np.float32)
    S0 = np.ascontiguousarray(X[::-2][:2000])
    n = len(X)
    vp = (X.max(0) + np.float32(1.0)).astype(np.float32)
    res = {"n": n, "k": K, "mse_threshold": mse, **kw}
    knn_host, nor_host = [], []
    for _ in range(host_reps):
        ms, hk = timed(lambda: pkg.knn_self(X, K))
        knn_host.append(ms)
        ms, hn = timed(lambda: pkg.estimate_normals(X, K, vp))
        nor_host.append(ms)
    res["knn_host_ms"] = {"all": [round(x, 3) for x in knn_host], "median": med(knn_host)}
    res["normals_host_ms"] = {"all": [round(x, 3) for x in nor_host], "median": med(nor_host)}
    from cuda_go_icp_amd import binding
    p = binding.CSourcePipeline(0.0, K, ALPHA, 0.0, 0)
    fp = C.POINTER(C.c_float)
    small_T = np.ascontiguousarray(T[:: max(1, len(T) // 4000)], np.float32)
    v = pkg.Registration(small_T, S0, mse, verbose=1, **kw)
    lib = v._lib
    fig = {key: [] for key in ("knn_device_ms", "knn_wall_ms", "normals_device_ms", "normals_wall_ms", "stat_device_ms", "stat_wall_ms")}
    levels = {}
    line = r"%s: \d+ -> \d+ points, levels (\d+), resolved((?: \d+)*), top (\d+)"
    for _ in range(reps + 1):                       # the first repetition warms the kernels up and is dropped
        with Stderr() as err:
            ms, dk = timed(lambda: v.knn_self(X, K))
        fig["knn_wall_ms"].append(ms)
        fig["knn_device_ms"].append(float(re.search(r"knn_self: k \d+, device ([0-9.]+) ms", err.text).group(1)))
        g = re.search(line % "knn_self", err.text)
        levels["knn"] = {"levels": int(g.group(1)), "resolved_share": [round(int(x) / n, 6) for x in g.group(2).split()], "top_share": round(int(g.group(3)) / n, 6)}
        with Stderr() as err:
            ms, dn = timed(lambda: v.estimate_normals(X, K, vp))
        fig["normals_wall_ms"].append(ms)
        fig["normals_device_ms"].append(float(re.search(r"estimate_normals: k \d+, device ([0-9.]+) ms", err.text).group(1)))
        g = re.search(line % "estimate_normals", err.text)
        levels["normals"] = {"levels": int(g.group(1)), "resolved_share": [round(int(x) / n, 6) for x in g.group(2).split()], "top_share": round(int(g.group(3)) / n, 6)}
        with Stderr() as err:
            assert lib.goicp_set_source_pipeline(v.handle, X.ctypes.data_as(fp), n, C.byref(p), None) == 0, lib.goicp_last_error()
        fig["stat_device_ms"].append(float(re.search(r"set_source_pipeline: .*device statistical ([0-9.]+) ms", err.text).group(1)))
        with Stderr():
            v.set_source(S0)
            ms, _ = timed(lambda: v.statistical_outlier_removal(X, K, ALPHA))
        fig["stat_wall_ms"].append(ms)
    v.close()
    same = bool(np.array_equal(dk[0], hk[0]) and dk[1].tobytes() == hk[1].tobytes() and dn[0].tobytes() == hn[0].tobytes() and dn[1].tobytes() == hn[1].tobytes())
    assert same, "the device and the host disagree"
    res["device_equals_host"] = same
    for key, vals in fig.items():
        res[key] = {"all": [round(x, 3) for x in vals[1:]], "median": med(vals[1:])}
    res["device_levels"] = levels
    # (e): the hierarchy path of a handle whose target is this cloud
    create, tn = [], []
    for _ in range(reps + 1):
        ms, h = timed(lambda: pkg.Registration(X, S0, mse, **kw))
        create.append(ms)

        def build():
            h.set_icp_options(1, K)
            return h.target_normals()
        ms, _ = timed(build)
        tn.append(ms)
        h.close()
    res["target_create_ms"] = {"all": [round(x, 3) for x in create[1:]], "median": med(create[1:])}
    res["target_normals_ms"] = {"all": [round(x, 3) for x in tn[1:]], "median": med(tn[1:])}
    m = lambda key: res[key]["median"]
    res["normals_kernels_over_stat_kernels"] = round(m("normals_device_ms") / m("stat_device_ms"), 3)
    res["knn_kernels_over_stat_kernels"] = round(m("knn_device_ms") / m("stat_device_ms"), 3)
    res["normals_call_over_target_path"] = round(m("normals_wall_ms") / (m("target_create_ms") + m("target_normals_ms")), 3)
    res["normals_call_over_target_normals_alone"] = round(m("normals_wall_ms") / m("target_normals_ms"), 3)
    print("%-8s n %d k %d | knn: kernels %.3f ms, call %.2f ms, host %.1f ms | normals: kernels %.3f ms, call %.2f ms, host %.1f ms (levels %d, resolved %s, top %g) | "
          "stat filter: kernels %.3f ms, call %.2f ms | target path: create %.1f ms + normals %.2f ms"
          % (name, n, K, m("knn_device_ms"), m("knn_wall_ms"), m("knn_host_ms"), m("normals_device_ms"), m("normals_wall_ms"), m("normals_host_ms"),
             levels["normals"]["levels"], levels["normals"]["resolved_share"], levels["normals"]["top_share"], m("stat_device_ms"), m("stat_wall_ms"),
             m("target_create_ms"), m("target_normals_ms")), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only", default="bunny,spanner,s2")
    ap.add_argument("--step-limit", type=int, default=420, help="seconds a case's child process may take (timeout -k 10)")
    ap.add_argument("--case", help="(internal) run this one case in this process and write its result to --out")
    args = ap.parse_args()
    if args.case:
        pkg = _pkg()
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
                                 "--reps", str(args.reps), "--host-reps", str(args.host_reps)]).returncode
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
