"""Point-to-point, point-to-plane, symmetric point-to-plane (goicp_set_icp_symmetric) and generalized plane-to-plane ICP
(goicp_set_icp_generalized, --epsilon, default 1e-3) on the project's workloads.

Per workload (those of tools/icp_metric_probe.py) and form: registration ms (median of --reps runs) and ICP iterations
(counters.icp_iters), the pass time at the found pose (goicp_time_icp_pass, 50 passes, --pass-reps repeats: median and spread), and the
source-normal build (wall time of set_icp_generalized(True, eps, 16) under metric 1: upload, self k-NN + PCA, the gather, one warm-up pass).
On the full bunny also ICP alone from perturbed starts: the eight of tests/test_gpu_point_to_plane.py::test_convergence_vs_point_to_point
(2-10 degrees, 0.01-0.05) and eight wider ones (20-45 degrees, 0.05-0.15) -- iterations and final pose per form.
Writes one JSON object (--out, default stdout).

    python tools/icp_generalized_probe.py --out profiles/icp_generalized_probe.json [--reps 5] [--only bunny,s2]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = {0: "point", 1: "plane", 2: "symmetric", 3: "generalized"}
FORMS = (0, 1, 2, 3)
EPSILON = 1e-3


def _set_metric(reg, metric):
    reg.set_icp_options(min(metric, 1), 16)
    reg.set_icp_symmetric(False, 16)                          # the two flags refuse each other: both off first
    reg.set_icp_generalized(False, EPSILON, 16)
    if metric == 2:
        reg.set_icp_symmetric(True, 16)
    if metric == 3:
        reg.set_icp_generalized(True, EPSILON, 16)


def _pass_us(pkg, reg, R, t, reps):
    out, us = C.c_float(), []
    for _ in range(reps):
        pkg.binding.check(reg._lib.goicp_time_icp_pass(reg.handle, R.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float)), 50,
                                                       C.byref(out)))
        us.append(out.value * 1e3)
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


def probe(pkg, name, make, reps, pass_reps):
    target, source, mse, kw = make()
    res = {"N": len(source), "M": len(target), "mse_threshold": float(mse)}
    eng = pkg.FastGoICP(target, source, mse, **kw)
    reg = eng.registration
    reg.set_icp_options(1, 16)
    t0 = time.perf_counter()
    reg.set_icp_generalized(True, EPSILON, 16)
    res["source_normal_build_ms"] = (time.perf_counter() - t0) * 1e3
    for metric in FORMS:
        _set_metric(reg, metric)
        ms, iters = [], []
        eng.run()                                                 # warm-up, dropped
        for _ in range(reps):
            eng.run()
            r = reg.poll()
            ms.append(r.register_ms)
            iters.append(int(r.counters.icp_iters))
        r = reg.poll()
        res[NAMES[metric]] = {"register_ms_median": statistics.median(ms), "register_ms": ms, "icp_iters": iters, "best_sse": float(r.best_sse),
                              "sse_threshold": float(eng.sse_threshold), "optR": list(r.optR), "optT": list(r.optT)}
    R, t = np.array(reg.poll().optR, np.float32), np.array(reg.poll().optT, np.float32)
    for metric in FORMS:
        _set_metric(reg, metric)
        res[NAMES[metric]]["pass_us"] = _pass_us(pkg, reg, R, t, pass_reps)
    res["pass_ratio_symmetric_over_plane"] = res["symmetric"]["pass_us"]["median"] / res["plane"]["pass_us"]["median"]
    res["pass_ratio_generalized_over_plane"] = res["generalized"]["pass_us"]["median"] / res["plane"]["pass_us"]["median"]
    reg.close()
    return res


def starts(pkg):
    """ICP alone on the full bunny from perturbations of the reference optimum: per start and metric the iterations and the final pose"""
    from conftest import cloud, golden, rot_angle
    from cuda_go_icp_amd import synth
    model, data = cloud("model_bunny"), cloud("data_bunny")
    g = golden("e2e_bunny_full")
    Rg, tg = np.array(g["R"]).reshape(3, 3), np.array(g["t"])
    reg = pkg.Registration(model, data, g["mse_threshold"])
    out = {}
    for label, seed, deg, tr in (("test_starts_2_10_deg", 2024, (2, 10), (0.01, 0.05)), ("wide_starts_20_45_deg", 2025, (20, 45), (0.05, 0.15))):
        rng = np.random.default_rng(seed)
        rows = []
        for _ in range(8):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            ang = np.deg2rad(rng.uniform(*deg))
            dt = rng.normal(size=3)
            dt *= rng.uniform(*tr) / np.linalg.norm(dt)
            R0 = (synth._rodrigues(axis * ang) @ Rg).astype(np.float32)
            t0 = (tg + dt).astype(np.float32)
            row = {"start_deg": float(np.rad2deg(ang)), "start_shift": float(np.linalg.norm(dt))}
            for metric in FORMS:
                _set_metric(reg, metric)
                icp = pkg.IterativeClosestPoint3D(reg, 10000, g["mse_threshold"] / 10000, R0, t0)
                err, R, t = icp.run()
                row[NAMES[metric]] = {"iters": int(icp.iters), "err": float(err), "R": [float(x) for x in np.ravel(R)], "t": [float(x) for x in t],
                                      "rad_from_optimum": float(rot_angle(R, Rg)), "shift_from_optimum": float(np.linalg.norm(t - tg))}
            rows.append(row)
        out[label] = rows
    reg.close()
    return out


def _write(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


def main():
    global EPSILON
    from icp_metric_probe import _pkg, workloads
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--only")
    ap.add_argument("--no-starts", action="store_true")
    ap.add_argument("--epsilon", type=float, default=EPSILON)
    a = ap.parse_args()
    EPSILON = a.epsilon
    pkg = _pkg()
    wl = workloads()
    names = a.only.split(",") if a.only else list(wl)
    out = {"reps": a.reps, "pass_reps": a.pass_reps, "epsilon": EPSILON, "workloads": {}}
    for n in names:
        w = out["workloads"][n] = probe(pkg, n, wl[n], a.reps, a.pass_reps)
        print("%-14s register %s ms  icp iters %s  pass %s us  source normals %.1f ms" % (
            n, " / ".join("%.2f" % w[NAMES[m]]["register_ms_median"] for m in FORMS),
            " / ".join("%d" % statistics.median(w[NAMES[m]]["icp_iters"]) for m in FORMS),
            " / ".join("%.1f" % w[NAMES[m]]["pass_us"]["median"] for m in FORMS), w["source_normal_build_ms"]), file=sys.stderr)
        if a.out:
            _write(a.out, out)                                      # after every workload: a long run leaves what it has
    if not a.no_starts:
        out["bunny_starts"] = starts(pkg)
        for label, rows in out["bunny_starts"].items():
            print("%s: iterations %s" % (label, " | ".join("/".join(str(r[NAMES[m]]["iters"]) for m in FORMS) for r in rows)), file=sys.stderr)
    if a.out:
        _write(a.out, out)
    else:
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
