"""Truncated-cost search (goicp_set_search_truncation): what the clamp costs in the bound kernels, and what the objective buys end to end.

  bounds    the headline sibling batch of bench.py (full bunny, 8 192 expansions x 8 children, 8 rotations) through goicp_time_bounds_device
            on ONE handle, truncation off / on (g = 0.05) / off / on ..., interleaved; per setting the median of --reps calls of 10 launches,
            all values kept, and the on / off ratio of the medians
  clutter   the clutter bunny of tests/test_gpu_search_trunc.py (30 % clutter, 75 degrees about a skew axis) registered three ways -- plain,
            trimmed (trim_fraction = the true clutter share) and truncated (g = 0.05 with the gate g on the same handle) -- each once with
            the default early exit (mse 1e-3) and once with a prove-the-optimum threshold (mse 1e-4), inside the test's rotation box: wall
            ms, cube bounds, ICP iterations, rotation / translation error against the known motion.  A run is cancelled after --limit
            seconds (recorded as unfinished, with the best pose it held then).
Writes one JSON object.

    python tools/search_trunc_probe.py --out profiles/search_trunc_probe.json [--reps 7] [--only bounds,clutter] [--limit 240]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
G = 0.05


def _pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()
    return m


def bounds_leg(pkg, reps):
    import torch
    import bench
    from conftest import cloud
    B = pkg.binding
    dev = torch.device("cuda", 0)
    reg = pkg.Registration(cloud("model_bunny"), cloud("data_bunny"), 1e-3)
    lib, h = reg._lib, reg.handle
    rots, recs, _ = bench.make_batch(pkg, reg, 8192, 8, seed=1234)
    Bc = len(recs)
    d_rots = torch.from_numpy(rots.reshape(-1)).to(dev)
    d_cubes = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev)
    d_ub = torch.empty(Bc, dtype=torch.float32, device=dev)
    d_lb = torch.empty(Bc, dtype=torch.float32, device=dev)
    ms = C.c_float()
    vals = {"off": [], "on": []}
    for g in (0.0, G):                                                    # first launches of both code objects, untimed
        reg.set_search_truncation(g)
        B.check(lib.goicp_time_bounds_device(h, d_rots.data_ptr(), d_cubes.data_ptr(), Bc, d_ub.data_ptr(), d_lb.data_ptr(), 3, C.byref(ms)))
    for _ in range(reps):
        for name, g in (("off", 0.0), ("on", G)):
            reg.set_search_truncation(g)
            B.check(lib.goicp_time_bounds_device(h, d_rots.data_ptr(), d_cubes.data_ptr(), Bc, d_ub.data_ptr(), d_lb.data_ptr(), 10, C.byref(ms)))
            vals[name].append(ms.value)
    reg.close()
    off, on = statistics.median(vals["off"]), statistics.median(vals["on"])
    return {"cubes": Bc, "points": int(len(cloud("data_bunny"))), "g": G, "ms_off": off, "ms_on": on, "ms_off_all": vals["off"], "ms_on_all": vals["on"],
            "cube_bounds_per_s_off": Bc / off * 1e3, "cube_bounds_per_s_on": Bc / on * 1e3, "on_over_off": on / off,
            "off_spread": (max(vals["off"]) - min(vals["off"])) / off}


def clutter_leg(pkg, limit):
    from conftest import rot_angle
    from test_gpu_search_trunc import clutter_bunny
    from test_gpu_search_trunc import BUNNY_BOX
    tgt, src, Rt, tt = clutter_bunny()
    share = 1.0 - len(tgt[::7]) / len(src)
    out = {"source_points": int(len(src)), "target_points": int(len(tgt)), "clutter_share": share, "g": G, "rotation_box_deg": [BUNNY_BOX["rot_min"], BUNNY_BOX["rot_max"]],
           "limit_s": limit, "runs": []}
    for mse, what in ((1e-3, "default early exit"), (1e-4, "prove the optimum")):
        for name, kw in (("plain", {}), ("trimmed", {"trim_fraction": share}), ("truncated", {"trunc_dist": G, "max_corr_dist": G})):
            eng = pkg.FastGoICP(tgt, src, mse, **BUNNY_BOX, **kw)
            timer = threading.Timer(limit, eng.cancel)
            timer.start()
            t0 = time.perf_counter()
            eng.run()
            wall = (time.perf_counter() - t0) * 1e3
            timer.cancel()
            c = eng.counters
            out["runs"].append({"objective": name, "mse_threshold": mse, "threshold_is": what, "sse_threshold": float(eng.sse_threshold), "finished": bool(eng.finished) and wall < limit * 1e3,
                                "wall_ms": wall, "best_sse": float(eng.get_best_error()), "cube_bounds": int(c.cubes), "rot_nodes": int(c.rot_pops), "icp_iters": int(c.icp_iters),
                                "rot_error_rad": float(rot_angle(eng.optR, Rt)), "trans_error": float(np.linalg.norm(eng.optT.astype(np.float64) - tt))})
            print(json.dumps(out["runs"][-1]), flush=True)
            eng.registration.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_trunc_probe.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="bounds,clutter")
    ap.add_argument("--limit", type=float, default=240.0)
    args = ap.parse_args()
    only = set(args.only.split(","))
    if "bounds" in only:
        import torch                                                      # before the library: torch brings its own HIP runtime, as in bench.py
        torch.cuda.init()
    pkg = _pkg()
    res = {"tool": "tools/search_trunc_probe.py", "kernel_source_hash": pkg.load_library().goicp_kernel_source_hash().decode()}
    if "bounds" in only:
        res["bounds"] = bounds_leg(pkg, args.reps)
        print(json.dumps({k: v for k, v in res["bounds"].items() if not k.endswith("_all")}), flush=True)
    if "clutter" in only:
        res["clutter"] = clutter_leg(pkg, args.limit)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
