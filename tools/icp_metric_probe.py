"""Point-to-point vs point-to-plane ICP (goicp_set_icp_options) on the project's workloads.

Per workload and metric: registration ms (median of --reps runs), ICP iterations (counters.icp_iters) and ICP ms (the verbose
"ICP + DT re-score" lap of the registration), the pass time of both metrics at the found pose (goicp_time_icp_pass), and the
normal build (wall time of set_icp_options(1, 16): target upload, k-NN + covariance + eigenvector kernel, one warm-up pass).
Writes one JSON object (--out, default stdout).

    python tools/icp_metric_probe.py --out profiles/icp_metric_probe.json [--reps 5] [--only bunny,s2]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()
    return m


def workloads():
    from conftest import cloud, skull_problem
    import importlib
    synth = importlib.import_module(_pkg().__name__ + ".synth")     # the package is registered under its import name by load_pkg
    out = {}
    out["bunny"] = lambda: (cloud("model_bunny"), cloud("data_bunny"), 1e-3, {})
    out["bunny_mse3e-5"] = lambda: (cloud("model_bunny"), cloud("data_bunny"), 3e-5, {})
    out["spanner"] = lambda: (cloud("spanner_target"), cloud("spanner_source"), 1e-4, {})
    out["skull"] = lambda: (lambda p: (p[0], p[1], 1e-3, {}))(skull_problem())
    out["s1"] = lambda: (lambda p: (p[0], p[1], 1e-3, {}))(synth.make_pair(**{k: synth.S1[k] for k in ("seed", "M", "N")}))

    def s2():
        t, s, Rgt, tgt = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"], amp=0.15)
        pkg = _pkg()
        r = pkg.Registration(t, s, 1e-3, dt_size=synth.S2["V"])
        floor = float(r.compute_sse_error(Rgt, tgt)) / len(s)
        r.close()
        return t, s, 1.2 * floor, {"dt_size": synth.S2["V"]}     # as tests/test_gpu_parity.py::test_s2_fullsize
    out["s2"] = s2
    out["rand100"] = lambda: (cloud("model_rand"), cloud("data_rand"), 1e-3, {})
    return out


def _run_verbose(eng):
    """eng.run() with the library's stderr captured: -> the 'ICP + DT re-score' ms of the verbose summary line"""
    sys.stderr.flush()
    fd = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            eng.run()
        finally:
            os.dup2(fd, 2)
            os.close(fd)
        tmp.seek(0)
        txt = tmp.read()
    m = re.search(r"ICP \+ DT re-score ([0-9.]+) ms", txt)
    return float(m.group(1)) if m else None


def probe(name, make, reps):
    pkg = _pkg()
    target, source, mse, kw = make()
    res = {"N": len(source), "M": len(target), "mse_threshold": float(mse)}
    eng = pkg.FastGoICP(target, source, mse, verbose=1, **kw)
    reg = eng.registration
    for metric in (0, 1):
        t0 = time.perf_counter()
        reg.set_icp_options(metric, 16)
        build_ms = (time.perf_counter() - t0) * 1e3
        if metric == 1:
            res["normal_build_ms"] = build_ms
        ms, icp_ms, iters = [], [], []
        for _ in range(reps):
            icp_ms.append(_run_verbose(eng))
            r = reg.poll()
            ms.append(r.register_ms)
            iters.append(int(r.counters.icp_iters))
        r = reg.poll()
        res["metric%d" % metric] = {"register_ms_median": statistics.median(ms), "register_ms": ms, "icp_iters": iters,
                                    "icp_ms_median": statistics.median([x for x in icp_ms if x is not None]) if any(x is not None for x in icp_ms) else None,
                                    "best_sse": float(r.best_sse), "sse_threshold": float(eng.sse_threshold),
                                    "optR": list(r.optR), "optT": list(r.optT)}
    R, t = np.array(reg.poll().optR, np.float32), np.array(reg.poll().optT, np.float32)
    for metric in (0, 1):
        reg.set_icp_options(metric, 16)
        out = C.c_float()
        pkg.binding.check(reg._lib.goicp_time_icp_pass(reg.handle, R.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float)),
                                                       50, C.byref(out)))
        res["metric%d" % metric]["pass_us"] = out.value * 1e3
    reg.close()
    m0, m1 = res["metric0"], res["metric1"]
    res["iters_ratio_plane_over_point"] = statistics.median(m1["icp_iters"]) / max(1, statistics.median(m0["icp_iters"]))
    res["pass_ratio_plane_over_point"] = m1["pass_us"] / m0["pass_us"]
    res["register_ratio_plane_over_point"] = m1["register_ms_median"] / m0["register_ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only")
    a = ap.parse_args()
    wl = workloads()
    names = a.only.split(",") if a.only else list(wl)
    out = {"reps": a.reps, "workloads": {}}
    for n in names:
        out["workloads"][n] = probe(n, wl[n], a.reps)
        w = out["workloads"][n]
        print("%-14s register %8.2f -> %8.2f ms  icp iters %6s -> %6s  pass %7.1f -> %7.1f us  normals %.1f ms" % (
            n, w["metric0"]["register_ms_median"], w["metric1"]["register_ms_median"], statistics.median(w["metric0"]["icp_iters"]),
            statistics.median(w["metric1"]["icp_iters"]), w["metric0"]["pass_us"], w["metric1"]["pass_us"], w["normal_build_ms"]), file=sys.stderr)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()
