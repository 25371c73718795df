#!/usr/bin/env python3
"""What the sharded ICP loop (goicp_icp_run_collective) costs per iteration, and what it would buy on G GPUs.

Runs 1 / 2 / 4 / 8 ranks as host threads over the library's in-process communicator on ONE GPU (N engines made from the same clouds,
the library's own collective loop -- the same code as over RCCL) from the identity pose, for the spanner (150 k points) and the
synthetic S2 (1 M points, DT 512^3), and reports per world:

  ms_per_iter        wall time of the collective run / its iterations (the thread ranks SHARE one GPU: no speed-up is expected here)
  round_trip_ms      host time per iteration of rank 0's round trip: slice pass + export + read-back, upload + finalize launch
  sum_wait_ms        host time per iteration rank 0 spent blocked in the integer sum (waiting for the slowest rank)
  bit_identical      every rank's (R, t, err, iters) equals goicp_icp_run at world 1, bit for bit
  pass_ms_world1     one full pass (goicp_time_icp_pass) and loop_ms_per_iter_world1 (goicp_icp_run) for the overhead comparison

and, labelled UNMEASURED (no multi-GPU node has been available), the projected ICP speed-up on G GPUs if a rank's slice costs
pass_ms / G and the per-iteration overhead stays what one GPU measured at world 1 of the collective loop:
  projected = loop_ms_per_iter_world1 / (pass_ms / G + collective_overhead_ms)

usage (needs a GPU): python tools/icp_shard_probe.py [--worlds 1,2,4,8] [--max-iter 400] > profiles/icp_shard_probe.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--max-iter", type=int, default=400)
    ap.add_argument("--workloads", default="spanner,s2")
    args = ap.parse_args()
    worlds = [int(w) for w in args.worlds.split(",")]
    from __graft_entry__ import _pkg
    pkg = _pkg()
    pkg.load_library()
    from cuda_go_icp_amd import binding as B, sharded, synth
    g = os.path.join(ROOT, "tests", "golden")
    ld = lambda n: np.fromfile(os.path.join(g, n + ".f32"), dtype="<f4").reshape(-1, 3)
    loads = {
        "spanner": lambda: ("spanner 150 k x 150 k", ld("spanner_target"), ld("spanner_source"), {}),
        "s2": lambda: ("S2 1 M x 1 M, DT 512^3", *synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"])[:2],
                       {"dt_size": synth.S2["V"]}),
    }
    R0, t0 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    out = {"tool": "tools/icp_shard_probe.py", "max_iter": args.max_iter, "err_diff": 1e-7, "workloads": []}
    for key in args.workloads.split(","):
        label, target, source, params = loads[key]()
        regs = [pkg.Registration(target, source, 1e-3, **params) for _ in range(max(worlds))]
        icp = pkg.IterativeClosestPoint3D(regs[0], args.max_iter, 1e-7, R0, t0)
        icp.run()                                                     # warm-up (first use of pinned blocks, code objects)
        t_a = time.perf_counter()
        icp = pkg.IterativeClosestPoint3D(regs[0], args.max_iter, 1e-7, R0, t0)
        err1, R1, T1 = icp.run()
        loop_ms = (time.perf_counter() - t_a) * 1e3
        it1 = icp.iters
        ref = (np.float32(err1).tobytes(), R1.astype(np.float32).tobytes(), T1.astype(np.float32).tobytes(), it1)
        ms, Rp, tp = C.c_float(), np.ascontiguousarray(R1, np.float32).reshape(-1), np.ascontiguousarray(T1, np.float32)
        B.check(regs[0]._lib.goicp_time_icp_pass(regs[0].handle, Rp.ctypes.data_as(C.POINTER(C.c_float)), tp.ctypes.data_as(C.POINTER(C.c_float)),
                                                 20, C.byref(ms)))
        pass_ms = ms.value
        w = {"workload": label, "N": len(source), "iters": it1, "pass_ms_world1": round(pass_ms, 4),
             "loop_ms_per_iter_world1": round(loop_ms / max(it1, 1), 4), "worlds": []}
        for world in worlds:
            sharded.icp_run_thread_ranks(regs[:world], R0, t0, 5, 1e-7)                   # warm-up of the slice path
            before = [r.icp_shard_stats() for r in regs[:world]]
            t_a = time.perf_counter()
            res = sharded.icp_run_thread_ranks(regs[:world], R0, t0, args.max_iter, 1e-7)
            wall = (time.perf_counter() - t_a) * 1e3
            after = [r.icp_shard_stats() for r in regs[:world]]
            ident = all((np.float32(e).tobytes(), R.astype(np.float32).tobytes(), t.astype(np.float32).tobytes(), it) == ref
                        for _, e, R, t, it in res)
            iters = max(res[0][4], 1)
            d = lambda k, r=0: after[r][k] - before[r][k]
            w["worlds"].append({"world": world, "ms_per_iter": round(wall / iters, 4),
                                "round_trip_ms": round(d("round_trip_ms") / iters, 4), "sum_wait_ms": round(d("sum_wait_ms") / iters, 4),
                                "collectives": d("collectives"), "bit_identical": bool(ident),
                                "blocks_rank0": [after[0]["block_begin"], after[0]["block_end"], after[0]["blocks"]]})
        c1 = w["worlds"][0]["ms_per_iter"] if worlds[0] == 1 else None
        if c1 is not None:
            overhead = max(c1 - pass_ms, 0.0)
            w["collective_overhead_ms_per_iter"] = round(overhead, 4)
            w["projected_speedup_unmeasured"] = {str(G): round(w["loop_ms_per_iter_world1"] / (pass_ms / G + overhead), 2) for G in (2, 4, 8)}
        out["workloads"].append(w)
        for r in regs:
            r.close()
        print(json.dumps(w), file=sys.stderr)
    out["note"] = ("thread ranks share ONE GPU: ms_per_iter does not fall with world; projected_speedup_unmeasured assumes a slice costs "
                   "pass_ms / G on G GPUs and the per-iteration overhead measured here (host round trip + in-process sum), not RCCL over xGMI")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
