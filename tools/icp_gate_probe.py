"""Distance-gated ICP (goicp_set_icp_gate): what the gate costs, whether the capped walk pays, and the clutter case end to end.

  pass      per workload (bunny, skull, spanner, S2 1 M): goicp_time_icp_pass of the ungated pass, and of the gated pass with a gate that
            holds every point (10 x the clouds' extent), full and capped walk: the cost of the compare + count and of the 32-word stride
  cap       clutter case and bun000 -> bun045 at g = 2 / 5 / 15 x the bunny model's median point spacing (0.011), at the identity pose:
            gated pass with the capped and with the full walk, and the inlier share
  clutter   the clutter case end to end: iterations and wall ms, ungated / gated (per gate) / gated batch K = 64
Every figure is the median of --reps (default 5) calls, all values kept (the run-to-run spread).  Writes one JSON object.

    python tools/icp_gate_probe.py --out profiles/icp_gate_probe.json [--reps 5] [--only pass,cap,clutter] [--no-s2]
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
SPACING = 0.011
I9, Z3 = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)


def _pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()
    return m


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def pass_ms(pkg, reg, reps, iters=20):
    v = []
    for _ in range(reps):
        ms = C.c_float()
        pkg.binding.check(reg._lib.goicp_time_icp_pass(reg.handle, _fp(I9), _fp(Z3), iters, C.byref(ms)))
        v.append(ms.value * 1e3)
    return {"us": statistics.median(v), "us_all": v}


def run_ms(pkg, reg, reps, batch=None):
    v, it = [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        if batch is None:
            R, t = I9.copy(), Z3.copy()
            e, n = C.c_float(), C.c_int32()
            pkg.binding.check(reg._lib.goicp_icp_run(reg.handle, _fp(R), _fp(t), 10000, 1e-7, C.byref(e), C.byref(n)))
            it = n.value
        else:
            it = int(reg.icp_run_batch(batch[0], batch[1], 10000, 1e-7)[3].sum())
        v.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(v), "ms_all": v, "iters": it, "inliers": reg.icp_inliers(1 if batch is None else len(batch[0])).tolist()[:4]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="pass,cap,clutter")
    ap.add_argument("--no-s2", action="store_true")
    a = ap.parse_args()
    pkg = _pkg()
    from conftest import cloud, skull_problem
    from test_gpu_icp_gate import clutter_case
    out = {"reps": a.reps}
    if "pass" in a.only:
        loads = {"bunny": lambda: (cloud("model_bunny"), cloud("data_bunny"), {}), "skull": lambda: skull_problem()[:2] + ({},),
                 "spanner": lambda: (cloud("spanner_target"), cloud("spanner_source"), {})}
        if not a.no_s2:
            from cuda_go_icp_amd import synth
            loads["s2"] = lambda: synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"])[:2] + ({"dt_size": synth.S2["V"]},)
        out["pass"] = {}
        for name, make in loads.items():
            tgt, src, kw = make()
            g = 10 * float(max((tgt.max(0) - tgt.min(0)).max(), (src.max(0) - src.min(0)).max()))
            reg = pkg.Registration(tgt, src, 1e-3, **kw)
            row = {"N": len(src), "M": len(tgt)}
            for metric in (0, 1):
                reg.set_icp_options(metric, 16)
                reg.set_icp_gate(0.0)
                pass_ms(pkg, reg, 1)
                r = {"ungated": pass_ms(pkg, reg, a.reps)}
                for capped in (0, 1):
                    reg.set_icp_gate(g, capped_walk=capped)
                    pass_ms(pkg, reg, 1)
                    r["gated_capped" if capped else "gated_full"] = pass_ms(pkg, reg, a.reps)
                r["gated_full_over_ungated"] = r["gated_full"]["us"] / r["ungated"]["us"]
                row["metric%d" % metric] = r
            reg.close()
            out["pass"][name] = row
            print(name, json.dumps(row), file=sys.stderr, flush=True)
    if "cap" in a.only:
        out["cap"] = {}
        cases = {"clutter": lambda: clutter_case()[:2], "bun000_bun045": lambda: (cloud("bun000"), cloud("bun045"))}
        for name, make in cases.items():
            tgt, src = make()
            reg = pkg.Registration(tgt, src, 1e-3)
            rows = []
            for mult in (2, 5, 15):
                g = mult * SPACING
                row = {"g": g, "inlier_share": reg.eval_correspondences(I9, Z3, g)[2] / len(src)}
                for capped in (0, 1, 0, 1):                       # interleaved: drift shows up as a difference between the two rounds
                    reg.set_icp_gate(g, capped_walk=capped)
                    pass_ms(pkg, reg, 1)
                    row.setdefault("capped" if capped else "full", []).append(pass_ms(pkg, reg, a.reps))
                row["capped_over_full"] = min(x["us"] for x in row["capped"]) / min(x["us"] for x in row["full"])
                rows.append(row)
                print(name, json.dumps(row), file=sys.stderr, flush=True)
            reg.close()
            out["cap"][name] = {"N": len(src), "M": len(tgt), "rows": rows}
    if "clutter" in a.only:
        tgt, src, _, _ = clutter_case()
        reg = pkg.Registration(tgt, src, 1e-3)
        res = {"N": len(src), "ungated": run_ms(pkg, reg, a.reps)}
        rng = np.random.default_rng(64)
        Rb = np.tile(np.eye(3, dtype=np.float32), (64, 1, 1))
        tb = rng.uniform(-0.02, 0.02, (64, 3)).astype(np.float32)
        for g in (0.15, 0.05, 0.02):
            reg.set_icp_gate(g)
            res["gated_%g" % g] = run_ms(pkg, reg, a.reps)
            res["gated_%g_batch64" % g] = run_ms(pkg, reg, a.reps, batch=(Rb, tb))
        reg.close()
        out["clutter"] = res
        print("clutter", json.dumps(res), file=sys.stderr, flush=True)
    s = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")
    else:
        print(s)


if __name__ == "__main__":
    main()
