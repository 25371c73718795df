"""Robust-kernel ICP (goicp_set_icp_robust): what the weights cost per pass, and what they buy on the clutter case.

  pass      per workload (bunny, skull, spanner) and metric: goicp_time_icp_pass at the identity pose of the plain pass, of the gated pass
            (full walk, a gate that holds every point) and of the robust pass per kernel (scale 0.05), each with its ratio to the plain pass
            of the same build
  clutter   the clutter case of tests/test_gpu_icp_gate.py from the identity, per kernel, scale and metric: rotation / translation error
            against the truth, iterations, W and C of the last pass, and the pass time; the plain and the gated (0.15, 0.05) runs beside them
Every time is the median of --reps (default 5) calls, all values kept (the run-to-run spread).  Writes one JSON object.

    python tools/icp_robust_probe.py --out profiles/icp_robust_probe.json [--reps 5] [--only pass,clutter]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
I9, Z3 = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
KERNELS = {1: "huber", 2: "cauchy", 3: "gm", 4: "tukey"}
TABLE = [(1, 0.05), (1, 0.01), (1, 0.002), (2, 0.05), (2, 0.01), (3, 0.05), (4, 0.15), (4, 0.05), (4, 0.02)]


def _pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()
    return m


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def pass_us(pkg, reg, reps, iters=20):
    v = []
    for _ in range(reps + 1):                                     # the first call warms up
        ms = C.c_float()
        pkg.binding.check(reg._lib.goicp_time_icp_pass(reg.handle, _fp(I9), _fp(Z3), iters, C.byref(ms)))
        v.append(ms.value * 1e3)
    v = v[1:]
    return {"us": statistics.median(v), "us_all": v}


def run(pkg, reg, Rt, tt):
    from conftest import rot_angle
    R, t = I9.copy(), Z3.copy()
    e, n = C.c_float(), C.c_int32()
    pkg.binding.check(reg._lib.goicp_icp_run(reg.handle, _fp(R), _fp(t), 10000, 1e-7, C.byref(e), C.byref(n)))
    c, w = reg.icp_robust_stats(1)
    return {"rot_err": float(rot_angle(R.reshape(3, 3), Rt)), "trans_err": float(np.linalg.norm(t - tt)), "iters": n.value, "err": e.value,
            "cost": float(c[0]), "weight_sum": float(w[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="pass,clutter")
    a = ap.parse_args()
    pkg = _pkg()
    from conftest import cloud, skull_problem
    from test_gpu_icp_gate import clutter_case
    out = {"reps": a.reps}
    if "pass" in a.only:
        loads = {"bunny": lambda: (cloud("model_bunny"), cloud("data_bunny")), "skull": lambda: skull_problem()[:2],
                 "spanner": lambda: (cloud("spanner_target"), cloud("spanner_source"))}
        out["pass"] = {}
        for name, make in loads.items():
            tgt, src = make()
            g = 10 * float(max((tgt.max(0) - tgt.min(0)).max(), (src.max(0) - src.min(0)).max()))
            reg = pkg.Registration(tgt, src, 1e-3)
            row = {"N": len(src), "M": len(tgt)}
            for metric in (0, 1):
                reg.set_icp_options(metric, 16)
                r = {"plain": pass_us(pkg, reg, a.reps)}
                reg.set_icp_gate(g, capped_walk=0)
                r["gated"] = pass_us(pkg, reg, a.reps)
                reg.set_icp_gate(0.0)
                for k, kn in KERNELS.items():
                    reg.set_icp_robust(k, 0.05)
                    r[kn] = pass_us(pkg, reg, a.reps)
                reg.set_icp_robust(0)
                for key in ("gated",) + tuple(KERNELS.values()):
                    r[key]["over_plain"] = r[key]["us"] / r["plain"]["us"]
                row["metric%d" % metric] = r
            reg.close()
            out["pass"][name] = row
            print(name, json.dumps(row), file=sys.stderr, flush=True)
    if "clutter" in a.only:
        tgt, src, Rt, tt = clutter_case()
        reg = pkg.Registration(tgt, src, 1e-3)
        res = {"N": len(src)}
        for metric in (0, 1):
            reg.set_icp_options(metric, 16)
            rows = {"plain": dict(run(pkg, reg, Rt, tt), pass_us=pass_us(pkg, reg, a.reps)["us"])}
            for g in (0.15, 0.05):
                reg.set_icp_gate(g)
                rows["gated_%g" % g] = dict(run(pkg, reg, Rt, tt), pass_us=pass_us(pkg, reg, a.reps)["us"])
            reg.set_icp_gate(0.0)
            for k, c in TABLE:
                reg.set_icp_robust(k, c)
                rows["%s_%g" % (KERNELS[k], c)] = dict(run(pkg, reg, Rt, tt), pass_us=pass_us(pkg, reg, a.reps)["us"])
            reg.set_icp_robust(0)
            res["metric%d" % metric] = rows
            print("clutter metric %d" % metric, json.dumps(rows), file=sys.stderr, flush=True)
        reg.close()
        out["clutter"] = res
    s = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")
    else:
        print(s)


if __name__ == "__main__":
    main()
