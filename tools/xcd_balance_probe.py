#!/usr/bin/env python3
"""Do the eight XCDs finish the pair launch of the headline batch together?  (EXPERIMENTS R9.1)

Needs the diagnostic build (make -C cuda-go-icp_amd/csrc stamps -> libgoicp_mi355_stamps.so): its bounds_pair_kernel stamps every
workgroup's entry and exit on the 100 MHz clock per XCC (HW_REG_XCC_ID) and per block label (blockIdx & 7); the shipped library stamps
nothing.  The batch is bench.py's (make_batch, seed 1234, 8 192 expansions, 8 rotations) on the bunny, DT 300^3.

Per configuration (bounds_balance 0, then 1 at each weight of --a) and per launch: the span of every XCC (last exit - first entry), its
workgroups, the labels it served (with bounds_balance = 0 label x is chunk x), the mean workgroup time per label; medians over --reps
launches.  From the bounds_balance = 0 rows: 1 - mean span / max span, the ceiling of what any mapping can gain, and the least-squares fit
of the mean workgroup time of chunk k against alpha * waves_k + beta * lines_k (a = alpha / beta, goicp_params::bounds_balance_a).
Stamped launches are also timed (host clock around a device synchronise, 20 launches): the stamps cost 30 us a launch, so these times
compare the configurations with each other, not with bench.py.

  python3 tools/xcd_balance_probe.py [--a 4,8,16,32] [--reps 9] [--out profiles/r09_bounds_xcd_spans.json] [--workload bunny|s1|s2]

--time N: the configurations timed against each other on any build, without stamps (time_only below); with
GOICP_LIBRARY=.../libgoicp_mi355.so that is the shipped library.

  GOICP_LIBRARY=$PWD/cuda-go-icp_amd/libgoicp_mi355.so python3 tools/xcd_balance_probe.py --time 4 --a 4,8,21 --out sweep.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GOICP_LIBRARY", os.path.join(ROOT, "cuda-go-icp_amd", "libgoicp_mi355_stamps.so"))
from __graft_entry__ import _pkg  # noqa: E402
import bench  # noqa: E402

ROWS, COLS = 16, 6


def time_only(args, pkg, lib, B, torch, model, data, V, configs):
    """--time N: no stamps (any build).  One handle per configuration, all alive; N rounds, each timing 20 launches of every configuration in
    turn (host clock around a device synchronise, 30 launches of warm-up per handle first)."""
    dev = torch.device("cuda", 0)
    runs = []
    for name, kw in configs:
        reg = pkg.Registration(model, data, 1e-3, dt_size=V, **kw)
        rots, recs, _ = bench.make_batch(pkg, reg, args.expansions, 8, seed=1234)
        t = [torch.from_numpy(rots.reshape(-1)).to(dev), torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev),
             torch.empty(len(recs), dtype=torch.float32, device=dev), torch.empty(len(recs), dtype=torch.float32, device=dev)]
        runs.append((name, reg, t, len(recs), []))

    def steps(reg, t, Bc, n):
        for _ in range(n):
            B.check(lib.goicp_eval_bounds_device(reg.handle, t[0].data_ptr(), t[1].data_ptr(), Bc, t[2].data_ptr(), t[3].data_ptr(), None))
        torch.cuda.synchronize()

    for name, reg, t, Bc, ms in runs:
        steps(reg, t, Bc, 30)
    for _ in range(args.time):
        for name, reg, t, Bc, ms in runs:
            steps(reg, t, Bc, 5)
            t0 = time.perf_counter()
            steps(reg, t, Bc, 20)
            ms.append((time.perf_counter() - t0) * 1e3 / 20)
    ref = (runs[0][2][2].cpu().numpy().view(np.uint32), runs[0][2][3].cpu().numpy().view(np.uint32))
    out = {"workload": args.workload, "rounds": args.time, "configs": []}
    for name, reg, t, Bc, ms in runs:
        same = bool(np.array_equal(t[2].cpu().numpy().view(np.uint32), ref[0]) and np.array_equal(t[3].cpu().numpy().view(np.uint32), ref[1]))
        print("%-24s ms per launch %s  min %.4f max %.4f mean %.4f  bits equal to the first configuration: %s" % (name, " ".join("%.4f" % x for x in ms), min(ms), max(ms), sum(ms) / len(ms), same))
        out["configs"].append({"name": name, "ms_per_launch": ms, "same_bits": same})
        reg.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=0, help="N > 0: time the configurations against each other in N alternating rounds instead (no stamps, any build)")
    ap.add_argument("--a", default="4,8,16,32", help="weights of a wavefront (bounds_balance_a) to run the balanced mapping at")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--expansions", type=int, default=8192)
    ap.add_argument("--workload", default="bunny", choices=["bunny", "s1", "s2"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_bounds_xcd_spans.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("xcd_balance_probe.py needs a GPU")
    pkg = _pkg()
    lib = pkg.load_library()
    from cuda_go_icp_amd import binding as B
    from cuda_go_icp_amd import synth
    if args.workload == "bunny":
        g = os.path.join(ROOT, "tests", "golden")
        model = np.fromfile(os.path.join(g, "model_bunny.f32"), dtype="<f4").reshape(-1, 3)
        data = np.fromfile(os.path.join(g, "data_bunny.f32"), dtype="<f4").reshape(-1, 3)
        V = 300
    else:
        cfg = synth.S1 if args.workload == "s1" else synth.S2
        model, data, _, _ = synth.make_pair(seed=cfg["seed"], M=cfg["M"], N=cfg["N"])
        V = cfg["V"]
    configs = [("balance 0", {"bounds_balance": 0})] + [("balance 0", {"bounds_balance": 0}) if a == "off" else
                                                        ("balance 1, a = %g" % float(a), {"bounds_balance": 1, "bounds_balance_a": float(a)}) for a in args.a.split(",") if a]
    if args.time:
        return time_only(args, pkg, lib, B, torch, model, data, V, configs)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"workload": args.workload, "N": int(len(data)), "V": V, "expansions": args.expansions, "reps": args.reps, "clock_hz": 1e8, "configs": []}
    for name, kw in configs:
        reg = pkg.Registration(model, data, 1e-3, dt_size=V, **kw)
        h = reg.handle
        rots, recs, _ = bench.make_batch(pkg, reg, args.expansions, 8, seed=1234)
        Bc = len(recs)
        d_rots = torch.from_numpy(rots.reshape(-1)).to(dev)
        d_cubes = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev)
        d_ub = torch.empty(Bc, dtype=torch.float32, device=dev)
        d_lb = torch.empty(Bc, dtype=torch.float32, device=dev)

        def step():
            B.check(lib.goicp_eval_bounds_device(h, d_rots.data_ptr(), d_cubes.data_ptr(), Bc, d_ub.data_ptr(), d_lb.data_ptr(), stream))

        words = (C.c_uint64 * (ROWS * COLS))()

        def take():
            torch.cuda.synchronize()
            rc = lib.goicp_debug_bounds_xcd_spans(h, words)
            if rc != 0:
                raise SystemExit("goicp_debug_bounds_xcd_spans failed: load the diagnostic build (make -C cuda-go-icp_amd/csrc stamps; GOICP_LIBRARY)")
            return np.array(words[:], dtype=np.uint64).reshape(ROWS, COLS)

        for _ in range(30):
            step()
        take()
        info = (C.c_int32 * 26)()
        per = []
        for _ in range(args.reps):
            step()
            per.append(take())
        B.check(lib.goicp_debug_bounds_balance(h, info))
        cut, lines, waves, used = list(info[0:9]), list(info[9:17]), list(info[17:25]), int(info[25])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            step()
        torch.cuda.synchronize()                                       # the launches go to the engine's own stream: a host clock around a device synchronise
        ms = (time.perf_counter() - t0) * 1e3 / 20
        take()
        per = np.stack(per).astype(np.float64)                         # reps x rows x cols
        t_first = per[:, :8, 0].min(axis=1)[:, None]
        span = (per[:, :, 1] - per[:, :, 0]) * 1e-2                    # us; whole launch: last exit anywhere - first entry anywhere
        launch = (per[:, :8, 1].max(axis=1) - per[:, :8, 0].min(axis=1)) * 1e-2
        done_at = (per[:, :, 1] - t_first) * 1e-2                      # us after the launch's first entry
        mean_wg = per[:, :, 3] / np.maximum(per[:, :, 2], 1) * 1e-2
        med = lambda a: np.median(a, axis=0)
        c = {"name": name, "params": kw, "cut": cut, "lines": lines, "waves": waves, "balanced": used, "ms_per_launch_stamped": ms,
             "launch_span_us": float(np.median(launch)),
             "xcc": [{"xcc": x, "span_us": float(med(span)[x]), "done_at_us": float(med(done_at)[x]), "workgroups": int(med(per[:, :, 2])[x]),
                      "left_at_once": int(med(per[:, :, 5])[x]), "mean_wg_us": float(med(mean_wg)[x]),
                      "labels": [l for l in range(8) if int(per[-1, x, 4]) >> l & 1]} for x in range(8)],
             "label": [{"label": x, "span_us": float(med(span)[8 + x]), "done_at_us": float(med(done_at)[8 + x]), "workgroups": int(med(per[:, :, 2])[8 + x]),
                        "left_at_once": int(med(per[:, :, 5])[8 + x]), "mean_wg_us": float(med(mean_wg)[8 + x]), "busy_us": float(med(per[:, :, 3])[8 + x] * 1e-2)} for x in range(8)]}
        sp = np.array([r["span_us"] for r in c["xcc"]])
        c["span_mean_us"], c["span_max_us"] = float(sp.mean()), float(sp.max())
        c["max_minus_mean_us"] = float(sp.max() - sp.mean())
        c["ceiling_1_minus_mean_over_max"] = float(1 - sp.mean() / sp.max())
        print("\n== %s: %.4f ms per stamped launch, launch span %.1f us; cut %s; balanced %d" % (name, ms, c["launch_span_us"], cut, used))
        print("   lines %s\n   waves %s" % (lines, waves))
        print("   XCC  span us  done at us  workgroups  left at once  mean wg us  labels")
        for r in c["xcc"]:
            print("   %3d  %7.1f  %10.1f  %10d  %12d  %10.2f  %s" % (r["xcc"], r["span_us"], r["done_at_us"], r["workgroups"], r["left_at_once"], r["mean_wg_us"], r["labels"]))
        print("   label span us  done at us  workgroups  left at once  mean wg us   busy us")
        for r in c["label"]:
            print("   %5d %7.1f  %10.1f  %10d  %12d  %10.2f  %8.0f" % (r["label"], r["span_us"], r["done_at_us"], r["workgroups"], r["left_at_once"], r["mean_wg_us"], r["busy_us"]))
        print("   spans: mean %.1f max %.1f us, max - mean %.1f us, 1 - mean / max = %.4f" % (c["span_mean_us"], c["span_max_us"], c["max_minus_mean_us"], c["ceiling_1_minus_mean_over_max"]))
        if not used and sum(waves) > 0:
            # label x = chunk x: the mean workgroup time of a chunk against its waves and lines (per workgroup both scale alike, so the totals serve)
            T = np.array([r["mean_wg_us"] for r in c["label"]])
            A = np.stack([np.array(waves, float), np.array(lines, float)], 1)
            coef, *_ = np.linalg.lstsq(A, T, rcond=None)
            res = T - A @ coef
            c["fit"] = {"alpha_us_per_wave": float(coef[0]), "beta_us_per_line": float(coef[1]), "a": float(coef[0] / coef[1]) if coef[1] != 0 else None,
                        "residual_us": res.tolist(), "T_us": T.tolist()}
            print("   fit T_k = alpha waves_k + beta lines_k: alpha %.6g beta %.6g a = alpha / beta = %.3f; residuals us %s" % (coef[0], coef[1], coef[0] / coef[1], np.round(res, 3).tolist()))
            sT = np.array([r["span_us"] for r in c["label"]])
            coef2, *_ = np.linalg.lstsq(A, sT, rcond=None)
            c["fit_span"] = {"alpha": float(coef2[0]), "beta": float(coef2[1]), "a": float(coef2[0] / coef2[1]) if coef2[1] != 0 else None, "residual_us": (sT - A @ coef2).tolist(), "span_us": sT.tolist()}
            print("   fit of the label spans: a = %.3f; residuals us %s" % (coef2[0] / coef2[1], np.round(sT - A @ coef2, 2).tolist()))
        out["configs"].append(c)
        reg.close()
        sys.stdout.flush()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("\nwrote", args.out)


if __name__ == "__main__":
    main()
