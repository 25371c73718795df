#!/usr/bin/env python3
"""bench.py -- BnB cube bounds/sec (+ inner-ICP iterations/sec) of the MI355X Go-ICP engine.

Contract: `python bench.py --gpus N --steps K --warmup W`.  N > 1 runs one rank per GPU over RCCL, started either way:
  * by torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment), or
  * plainly, `python3 bench.py --gpus N ...` with no WORLD_SIZE in the environment: this process then starts the N ranks itself as
    FRESH child processes (it never touches a GPU, never re-executes itself), forwards rank 0's JSON line to its stdout and
    exits non-zero if any rank did.
Rank 0 prints ONE JSON line.

Workload (BASELINE.json configs[1], "bunny_goicp.toml Go-ICP on 1xMI355X, DT grid 300^3,
subsample=1.0"): the Stanford-bunny clouds the reference's config names (M = 35 947 target,
N = 30 379 source; committed data fixtures, tests/golden/*.f32), distance transform 300^3.
  step   = one pass of the hot path over one batch: ONE launch of the cube-bound evaluator over
           B = 65 536 translation sub-cubes (8 192 BnB expansions x 8 children, widths 1/2 .. 1/64,
           spread over 8 rotations, every second expansion a lower-bound pass with rotation radii),
           followed -- as in the sharded search -- by the min-reduction of the best upper bound
           (the library's own reduce kernel; all-reduced over RCCL when N > 1).  Inputs are resident in HBM.
  value  = cube bounds evaluated by all ranks / wall time of the K timed steps (max over ranks).
The headline batch is SIBLING-STRUCTURED (8 children per expansion, as the search produces them); SURVEY 8(d)'s literal
microbench -- 65 536 unrelated cubes -- is `generic_path` / `roofline.frac_generic`, about half that rate.

A plain run does only what the headline needs: set-up, the untimed prewarm + W warm-up steps, the K timed steps, and the line
(metric, value, unit, ms_per_step, ...).  `--dump-outputs DIR` then writes what the last timed step computed -- the upper and lower
bounds of the batch and its best upper bound, float32 -- as DIR/ub.npy, DIR/lb.npy, DIR/best_ub.npy (rank r > 0: *_rank<r>.npy);
the inputs are seeded, so two builds run with the same arguments can be compared output for output.
Only with `--full` does the line also report: `value_repeats` (four more timed regions of K steps),
`sustained` (the same step for >= 8 s: mean and slowest-window rate), `s2` (the HBM-bound configuration,
N = M = 1 M, DT 512^3: three launches and its HBM roofline from the committed PMC traffic), ICP iterations/s (NN + sums + SVD update, host round trip included), an end-to-end
registration of the same clouds (exact cube-bound count / wall time), the roofline of the dominant
kernel (HIP events on the launch stream) and the CPU baseline timed on the host cores: the reference's own
InnerBnB (oracle/_ref/ref_harness, compiled from the reference's sources in the build container) when that
binary travelled with the snapshot, and the oracle port (1 thread and all cores) either way.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable)


def _profile(suffix):
    """Newest committed PMC summary profiles/rNN_<suffix> (the counters cannot be read from inside this process; they are
    collected with `rocprofv3 --pmc` on this command, tools/pmc_collect.sh, and committed)."""
    d = os.path.join(ROOT, "profiles")
    for rnd in ("r04", "r03", "r02"):
        p = os.path.join(d, "%s_%s" % (rnd, suffix))
        if os.path.exists(p):
            return p
    return None


def _profile_traffic(path, key, lib_hash):
    """(traffic bytes or None, provenance dict) of a committed PMC summary: the counters are only quoted when they were collected on the
    kernels this library was built from (the summary's kernel_source_hash, stamped by tools/pmc_to_profile.py, equals the library's)."""
    with open(path) as f:
        j = json.load(f)
    prov = {"traffic_profile": "profiles/" + os.path.basename(path), "traffic_profile_head": j.get("git_head", "unstamped (collected before round 4)"),
            "traffic_profile_kernel_hash": j.get("kernel_source_hash"), "library_kernel_hash": lib_hash}
    if j.get("kernel_source_hash") != lib_hash:
        prov["traffic_null_because"] = "the committed counter profile was collected on other kernel sources than this library's: re-collect (tools/profile_round.sh)"
        return None, prov, j
    return j[key], prov, j


def make_batch(pkg, reg, n_expansions, n_rot, seed):
    """Cube records exactly as the engine's BnB driver generates them (engine.cpp run_inner)."""
    from cuda_go_icp_amd import binding as B
    rng = np.random.default_rng(seed)
    rots = np.stack([pkg.fgoicp.rodrigues(rng.uniform(-2.0, 2.0, 3)) for _ in range(n_rot)]).astype(np.float32)
    recs = np.zeros(n_expansions * 8, dtype=[("tx", "<f4"), ("ty", "<f4"), ("tz", "<f4"), ("delta", "<f4"),
                                              ("coeff", "<f4"), ("rot", "<i4")])
    lev = rng.integers(0, 6, n_expansions)                 # parent widths 1 .. 1/32 -> child widths 1/2 .. 1/64
    pw = (1.0 / (1 << lev)).astype(np.float32)
    corner = (rng.uniform(-0.5, 0.5, (n_expansions, 3)) * (1 - pw[:, None]) - pw[:, None] / 2).astype(np.float32)
    w = pw / np.float32(2)
    j = np.arange(8)
    off = np.stack([(j & 1), (j >> 1) & 1, (j >> 2) & 1], 1).astype(np.float32)         # (8,3)
    cx = corner[:, None, :] + off[None, :, :] * w[:, None, None] + (w / np.float32(2))[:, None, None]
    recs["tx"], recs["ty"], recs["tz"] = cx[..., 0].ravel(), cx[..., 1].ravel(), cx[..., 2].ravel()
    delta = np.array([reg._lib.goicp_trans_delta(float(x)) for x in np.unique(w)], np.float32)
    dmap = dict(zip(np.unique(w).tolist(), delta.tolist()))
    recs["delta"] = np.repeat(np.array([dmap[float(x)] for x in w], np.float32), 8)
    lb_pass = (np.arange(n_expansions) % 2) == 1
    rot_level = rng.integers(3, 9, n_expansions)
    coeff = np.array([float(reg.rot_coeff(int(l))) for l in range(20)], np.float32)
    recs["coeff"] = np.repeat(np.where(lb_pass, coeff[rot_level], np.float32(0)), 8)
    recs["rot"] = np.repeat((np.arange(n_expansions) * n_rot) // n_expansions, 8)       # grouped by rotation
    n_lb = int(lb_pass.sum()) * 8
    return rots, recs, n_lb


def make_generic_batch(pkg, reg, n_cubes, n_rot, seed):
    """SURVEY 8(d)'s microbench batch: independent translation cubes (centres U[-0.5,0.5]^3, half-width 1/64), rotations
    uniform in the pi-ball, every second cube a lower-bound pass.  No two cubes of a workgroup are siblings, so the
    kernel takes its generic path (24 voxel-index computations per point instead of 6)."""
    rng = np.random.default_rng(seed)
    rv = []
    while len(rv) < n_rot:
        v = rng.uniform(-np.pi, np.pi, 3)
        if np.linalg.norm(v) <= np.pi:
            rv.append(v)
    rots = np.stack([pkg.fgoicp.rodrigues(v) for v in rv]).astype(np.float32)
    recs = np.zeros(n_cubes, dtype=[("tx", "<f4"), ("ty", "<f4"), ("tz", "<f4"), ("delta", "<f4"), ("coeff", "<f4"), ("rot", "<i4")])
    c = rng.uniform(-0.5, 0.5, (n_cubes, 3)).astype(np.float32)
    recs["tx"], recs["ty"], recs["tz"] = c[:, 0], c[:, 1], c[:, 2]
    recs["delta"] = np.float32(reg._lib.goicp_trans_delta(1.0 / 32))          # child width 1/32 = half-width 1/64
    lb_pass = (np.arange(n_cubes) % 2) == 1
    coeff = np.array([float(reg.rot_coeff(int(l))) for l in range(20)], np.float32)
    recs["coeff"] = np.where(lb_pass, coeff[rng.integers(3, 9, n_cubes)], np.float32(0))
    recs["rot"] = rng.integers(0, n_rot, n_cubes)
    return rots, recs, int(lb_pass.sum())


def cpu_baseline(reg, model, data, seconds=6.0):
    """The CPU oracle (a port of the reference's InnerBnB body) on the same DT, 1 thread and all cores."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    V, scale, origin = reg.dt_info()
    dt = O.DistanceTransform.wrap(V, scale, origin[0], origin[1], origin[2], reg.dt_download())
    R = O.rodrigues([0.3, -0.2, 0.9])
    prot = O.rotate(R, data)
    _, rho = O.rot_radii(data)
    rng = np.random.default_rng(2)
    out = {}
    ncores = len(os.sched_getaffinity(0))
    for name, par, nb in (("1thread", False, 64), ("allcores", True, 64 * ncores)):
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            cubes = np.concatenate([rng.uniform(-0.4, 0.4, (nb, 3)), np.full((nb, 1), 0.0625)], 1).astype(np.float32)
            O.cube_bounds_batch(dt, prot, rho[5] if (n // nb) % 2 else None, cubes, parallel=par)
            n += nb
        out[name] = n / (time.perf_counter() - t0)
    out["ncores"] = ncores
    kd = O.KdTree(model)
    t0 = time.perf_counter()
    _, _, _, it = kd.icp_run(data, np.eye(3), np.zeros(3), 8, -1e30)
    out["icp_iters_per_s_1thread"] = it / (time.perf_counter() - t0)
    return out


REF_FLAGS = ("jly_goicp.cpp, matrix.cpp and DT3D::Distance (jly_3ddt.cpp): g++ -O3 -DNDEBUG = the reference's CMake Release default "
             "(CMakeLists.txt:20-23); DT3D::Build and the rest of jly_3ddt.cpp: -O0 (its Release build corrupts 2.7 % of the voxels, "
             "SURVEY A.3) -- the build is outside the timed region")


def reference_baseline(seconds=10.0):
    """oracle/_ref/ref_harness_bench (the REAL reference CPU Go-ICP at its Release flags, compiled from its sources by
    oracle/Makefile in the build container; it travels with the snapshot): the reference's own GoICP::InnerBnB on the
    fixture clouds, timed on this host.  The exact number of cube bounds of the seeded call sequence comes from
    tests/golden/ref_bench_counts.json (DT3D::Distance calls / Nd, counted once by oracle/_ref/ref_harness_count);
    it is used only when the reference's own tNodeCount of this run matches the table.  None when the binary is not there."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_harness_bench")
    g = os.path.join(ROOT, "tests", "golden")
    if not os.path.exists(exe):
        return None
    try:
        r = subprocess.run([exe, "bench", os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32"), str(seconds)],
                           capture_output=True, text=True, timeout=300)
        out = json.loads(r.stdout.strip().splitlines()[-1])
        out["cube_bounds"], out["count"] = out["cube_bounds_upper"], "8 x tNodeCount (upper bound: counts each call's final non-expanding pop)"
        tab_path = os.path.join(g, "ref_bench_counts.json")
        if os.path.exists(tab_path):
            with open(tab_path) as f:
                tab = json.load(f)
            k = out["inner_bnb_calls"]
            if k < len(tab["pops_prefix"]) and tab["pops_prefix"][k] == out["trans_pops"]:
                out["cube_bounds"], out["count"] = tab["cube_bounds_prefix"][k], "exact (DT3D::Distance calls / Nd, tests/golden/ref_bench_counts.json; tNodeCount of this run matches the table)"
        out["cube_bounds_per_s"] = out["cube_bounds"] / out["seconds"]
        return out
    except Exception as e:                      # a baseline leg must never take the GPU measurement down
        print("reference baseline unavailable: %r" % (e,), file=sys.stderr)
        return None


def s2_leg(pkg, B, lib, args, dev, torch):
    from cuda_go_icp_amd import synth
    t0 = time.perf_counter()
    model, data, _, _ = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"])
    t_synth = time.perf_counter() - t0
    t0 = time.perf_counter()
    reg = pkg.Registration(model, data, 1e-3, dt_size=synth.S2["V"], device=dev.index)
    t_create = time.perf_counter() - t0
    rots, recs, n_lb = make_batch(pkg, reg, args.expansions, 8, seed=1234)
    Bc, N = len(recs), len(data)
    d_rots = torch.from_numpy(rots.reshape(-1)).to(dev)
    d_cubes = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev)
    d_ub = torch.empty(Bc, dtype=torch.float32, device=dev)
    d_lb = torch.empty(Bc, dtype=torch.float32, device=dev)
    ms = C.c_float()
    B.check(lib.goicp_time_bounds_device(reg.handle, d_rots.data_ptr(), d_cubes.data_ptr(), Bc, d_ub.data_ptr(), d_lb.data_ptr(), args.s2_steps, C.byref(ms)))
    launch_s = ms.value * 1e-3
    res = {"workload": "synthetic S2 (SURVEY 8d; BASELINE configs[4] per GPU): N=%d source, M=%d target, DT %d^3 (%d MB)" % (N, len(model), synth.S2["V"], synth.S2["V"] ** 3 * 4 // 1000000),
           "synth_s": round(t_synth, 3), "engine_create_s": round(t_create, 3), "steps": args.s2_steps, "cubes_per_step": Bc,
           "launch_ms": round(ms.value, 3), "cube_bounds_per_s": round(Bc / launch_s, 1),
           "algorithmic_bytes_per_launch_survey": (Bc - n_lb) * 16.0 * N + n_lb * 20.0 * N, "algorithmic_bytes_per_launch_as_built": Bc * 6.0 * N}
    pmc = _profile("pmc_bounds_s2.json")
    if pmc and Bc == 65536:
        tr, prov, _ = _profile_traffic(pmc, "hbm_bytes_per_launch_corrected", lib.goicp_kernel_source_hash().decode())
        alg = res["algorithmic_bytes_per_launch_survey"]
        res["roofline"] = {"bound": "hbm", "kernel": "goicp::bounds_kernel", "achieved": None if tr is None else round(tr / launch_s / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": None if tr is None else round(tr / launch_s / 1e9 / HBM_PEAK_GBS, 4), "traffic": tr,
                           "traffic_source": "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE of this batch, separate passes, FETCH_SIZE x2 on gfx950; fabric side of L2)" % os.path.basename(pmc),
                           "launch_ms": round(ms.value, 3),
                           "frac_survey_model": round(alg / launch_s / 1e9 / HBM_PEAK_GBS, 4),
                           "frac_survey_model_is": "SURVEY 8(d)'s 16 N / 20 N bytes per cube bound over the launch time over 8 TB/s: above 1 -- void as a fraction, the model prices no sibling reuse (a point is loaded once per 8 cubes)",
                           "as_built_frac": round(Bc * 6.0 * N / launch_s / 1e9 / HBM_PEAK_GBS, 4)}
        res["roofline"].update(prov)
    reg.close()
    return res


def spawn_ranks(n, backend):
    """`python3 bench.py --gpus N` started plainly: run the N ranks as fresh child processes of THIS one (which has not touched and
    never touches the GPU -- no torch.cuda call, no HIP call), one per GPU, rendezvous on 127.0.0.1.  Rank 0's stdout (the ONE
    JSON line) is forwarded to ours as it comes, the other ranks' stdout goes to stderr.  Exit code: 0 only if every rank's was 0;
    when a rank fails the others get 30 s to notice (their collectives have deadlines) before they are ended -- by PID."""
    import socket
    import threading
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")            # dmabuf IPC: RCCL across processes needs it on this driver
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=subprocess.PIPE, text=True, bufsize=1))

    def pump(r, pipe):
        for line in pipe:
            # ONE JSON line on stdout: rank 0's; anything else a rank writes there (gloo prints its connection banner to stdout) goes to stderr
            to_out = r == 0 and line.lstrip().startswith("{")
            (sys.stdout if to_out else sys.stderr).write(line if to_out else "[rank %d] %s" % (r, line))
            (sys.stdout if to_out else sys.stderr).flush()
    pumps = [threading.Thread(target=pump, args=(r, p.stdout), daemon=True) for r, p in enumerate(procs)]
    for t in pumps:
        t.start()
    rc, failed_at = 0, None
    while any(p.poll() is None for p in procs):
        time.sleep(0.2)
        bad = [p.returncode for p in procs if p.poll() is not None and p.returncode != 0]
        if bad and failed_at is None:
            failed_at, rc = time.time(), bad[0]
            print("bench.py: a rank exited with code %d; waiting up to 30 s for the others" % rc, file=sys.stderr)
        if failed_at is not None and time.time() - failed_at > 30:
            for p in procs:
                if p.poll() is None:
                    p.terminate()                                   # this exact child, by PID
            time.sleep(2)
            for p in procs:
                if p.poll() is None:
                    p.kill()
    for t in pumps:
        t.join(5)
    for p in procs:
        if p.returncode != 0 and rc == 0:
            rc = p.returncode
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (>= 1); ms_per_step = their wall time / this")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also run every other leg (repeats, sustained, ICP, roofline and probes, host-pointer "
                                                           "path, end-to-end registrations, CPU baselines, S2, sharded legs); off: the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs (ub, lb, best_ub; float32 .npy) to DIR")
    ap.add_argument("--prewarm", type=int, default=30, help="untimed setup steps before the W warm-up steps (GPU clock ramp); reported as setup_prewarm_steps")
    ap.add_argument("--expansions", type=int, default=8192, help="BnB expansions (x8 cubes) per step per GPU")
    ap.add_argument("--sustain-s", type=float, default=8.0, help="length of the sustained leg, seconds (0 = skip); long enough for a 5-second SMI sampler to see the GPU busy")
    ap.add_argument("--s2-steps", type=int, default=3, help="launches of the S2 (1 M points, DT 512^3) leg in the default run (0 = skip)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-deep", action="store_true", help="skip the prove-the-optimum registration of the N = 1 line (~5 s)")
    ap.add_argument("--dt-layout", type=int, default=1)
    ap.add_argument("--dt-size", type=int, default=300, help="tuning only: the BASELINE workload is 300")
    ap.add_argument("--kd-gpu-build", type=int, default=-1, help="tuning only: target hierarchy built on the device 1 / host 0 / auto -1")
    ap.add_argument("--morton", type=int, default=2, help="tuning only: source order 0 input / 1 Morton / 2 k-d order")
    ap.add_argument("--no-icp", action="store_true")
    ap.add_argument("--bounds-fp16", type=int, default=0, help="opt-in half-precision DT copy for the BnB bounds (not the bit-parity path)")
    ap.add_argument("--icp-fused", type=int, default=-1, help="tuning only: ICP iteration as one fused launch 1 / pass + finalize 0 / engine default -1")
    ap.add_argument("--icp-nn-cache", type=int, default=0, help="tuning only: exact walk-skipping neighbour cache of the ICP pass 1 / off 0")
    ap.add_argument("--flow", type=int, default=0, help="tuning only: continuous flow of the outer search (low-water mark of running inner searches) / lock-step batches 0")
    ap.add_argument("--device-queues", type=int, default=1, help="tuning only: inner-BnB queues on the device 1 / host 0")
    ap.add_argument("--no-probe", action="store_true", help="profiling runs: skip the gather-ceiling probes and the generic-path leg")
    ap.add_argument("--workload", default="bunny", choices=["bunny", "s1", "s2"],
                    help="bunny = BASELINE configs[1] (default); s1 = synthetic 40k/40k V=300; s2 = synthetic 1M/1M V=512 (configs[4] per GPU)")
    ap.add_argument("--no-sharded", action="store_true", help="skip the sharded end-to-end registration when N > 1")
    ap.add_argument("--sharded-timeout", type=int, default=240, help="watchdog of the sharded leg, seconds")
    ap.add_argument("--no-s2-sharded", action="store_true", help="skip the sharded registration of the 1 M-point configuration (BASELINE configs[4]) when N > 1")
    ap.add_argument("--backend", default="nccl", help="nccl (RCCL; one GPU per rank) | gloo (rehearsal: all ranks on GPU 0)")
    ap.add_argument("--shard-ramp", type=int, default=32, help="sharded legs: a rank's step follows the single-GPU driver's ramp of rotation parents per batch, 8 -> this (0 = a fixed 8 per step)")
    ap.add_argument("--deep-mse", type=float, default=3e-5, help="mse threshold of the deep strong-scaling leg (bunny; below the optimum's error: the search has to PROVE the optimum, 6.7 s on one GPU); 0 = skip")
    ap.add_argument("--e2e-repeats", type=int, default=5, help="registrations of the end-to-end leg (min / median / spread reported)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0 or args.prewarm < 0:
        ap.error("--steps must be >= 1, --warmup and --prewarm >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started plainly: be the launcher.  Nothing above or in spawn_ranks initialises the GPU; the ranks are children, not re-executions
        sys.exit(spawn_ranks(args.gpus, args.backend))

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d, or plainly (no WORLD_SIZE) to let bench.py start the ranks" % (args.gpus, world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the engine has no CPU path")
    if args.backend == "gloo":
        local_rank = 0                       # rehearsal of the N>1 path on a single GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        tmo = datetime.timedelta(seconds=600)          # a failed rank must not hang the others for the default 10+ min (rank 0's single-rank legs -- probes, CPU baseline, S2 -- take ~1 min while the others wait)
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(backend="gloo", timeout=tmo)

    from __graft_entry__ import _pkg
    pkg = _pkg()
    pkg.load_library()
    from cuda_go_icp_amd import binding as B
    if args.workload == "bunny":
        g = os.path.join(ROOT, "tests", "golden")
        model = np.fromfile(os.path.join(g, "model_bunny.f32"), dtype="<f4").reshape(-1, 3)
        data = np.fromfile(os.path.join(g, "data_bunny.f32"), dtype="<f4").reshape(-1, 3)
        wname = "bunny_goicp.toml (BASELINE configs[1])"
    else:
        from cuda_go_icp_amd import synth
        cfg = synth.S1 if args.workload == "s1" else synth.S2
        model, data, _, _ = synth.make_pair(seed=cfg["seed"], M=cfg["M"], N=cfg["N"])
        if args.dt_size == 300:
            args.dt_size = cfg["V"]
        wname = "synthetic %s (SURVEY 8d)" % args.workload.upper()
    N, M, V = len(data), len(model), args.dt_size

    t_create = time.perf_counter()
    reg = pkg.Registration(model, data, 1e-3, dt_size=V, dt_layout=args.dt_layout, device=local_rank, morton_sort=args.morton, kd_gpu_build=args.kd_gpu_build,
                           bounds_fp16=args.bounds_fp16, icp_nn_cache=args.icp_nn_cache, **({"icp_fused": args.icp_fused} if args.icp_fused >= 0 else {}))
    t_create = time.perf_counter() - t_create
    lib, h = reg._lib, reg.handle
    rots, recs, n_lb = make_batch(pkg, reg, args.expansions, 8, seed=1234 + rank)
    Bc = len(recs)
    d_rots = torch.from_numpy(rots.reshape(-1)).to(dev)
    d_cubes = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev)
    d_ub = torch.empty(Bc, dtype=torch.float32, device=dev)
    d_lb = torch.empty(Bc, dtype=torch.float32, device=dev)
    best2 = [torch.empty(1, dtype=torch.float32, device=dev) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    pending = [None]
    nstep = [0]

    def step():
        # one batch of cube bounds, its best upper bound, and -- N > 1 -- the global min over the ranks.  The exchange of
        # step i runs on RCCL's stream beside the kernel of step i+1 (its result prunes from step i+2 on: a bound that is one
        # batch stale costs speculation, never validity -- the library's protocol exchanges once per several batches);
        # every exchange is complete before the timed region ends (drain()).
        best = best2[nstep[0] & 1]
        nstep[0] += 1
        B.check(lib.goicp_eval_bounds_device(h, d_rots.data_ptr(), d_cubes.data_ptr(), Bc, d_ub.data_ptr(), d_lb.data_ptr(), stream))
        B.check(lib.goicp_reduce_min_device(h, d_ub.data_ptr(), Bc, best.data_ptr(), None, stream))   # best upper bound of the batch (library kernel)
        if world > 1:
            if pending[0] is not None:
                pending[0].wait()                                # the exchange before last: long finished
            pending[0] = dist.all_reduce(best, op=dist.ReduceOp.MIN, async_op=True)   # RCCL: prune globally

    def drain():
        if pending[0] is not None:
            pending[0].wait()
            pending[0] = None

    # setup: bring the GPU to its steady clock before anything is measured (the first ~50 ms after an idle period run ~3 %
    # slower: `value_repeats`, taken after the timed region, showed 36.0 M against 34.8 M for a cold first region)
    for _ in range(args.prewarm):
        step()
    for _ in range(args.warmup):
        step()
    drain()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    drain()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    value = world * Bc * args.steps / elapsed
    if args.dump_outputs:
        # what the last timed step handed its caller: the batch's bounds and its best upper bound (all-reduced over the ranks when N > 1)
        os.makedirs(args.dump_outputs, exist_ok=True)
        sfx = "" if rank == 0 else "_rank%d" % rank
        keep = slice(None)
        if Bc > (1 << 22):           # 64 MB in all: a fixed, seeded sample of 4 M cubes of a larger batch
            keep = np.sort(np.random.default_rng(0).choice(Bc, 1 << 22, replace=False))
        for name, t, sel in (("ub", d_ub, keep), ("lb", d_lb, keep), ("best_ub", best2[(nstep[0] - 1) & 1], slice(None))):
            np.save(os.path.join(args.dump_outputs, name + sfx + ".npy"), t.cpu().numpy()[sel].astype(np.float32))
    out = None
    if rank == 0:
        out = {"metric": "bnb_cube_bounds_per_s", "value": round(value, 1), "unit": "cube-bounds/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "setup_prewarm_steps": args.prewarm, "ms_per_step": round(1e3 * elapsed / args.steps, 4),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
               "data": ("Stanford-bunny clouds named by the reference's bunny_goicp.toml (committed fixture)" if args.workload == "bunny" else "synthetic clouds (cuda-go-icp_amd/synth.py)") + " + synthetic cube batch",
               "config": {"workload": "%s: N=%d source, M=%d target, DT %d^3, subsample 1.0" % (wname, N, M, V),
                          "cubes_per_step_per_gpu": Bc, "lb_pass_fraction": n_lb / Bc, "rotations_per_step": 8,
                          "dt_layout": "bricked4x4x4" if args.dt_layout else "linear", "exchange": "all_reduce(MIN) of the batch's best ub per step, running beside the next step's kernel, all complete inside the timed region" if world > 1 else "local min"}}
    # ---- everything below is --full only ----
    # run-to-run spread: four more timed regions of the same K steps (reported beside `value`, never instead of it)
    repeats = []
    for _ in range(4 if args.full else 0):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        tr0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        drain()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        er = torch.tensor([time.perf_counter() - tr0], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(er, op=dist.ReduceOp.MAX)
        repeats.append(world * Bc * args.steps / float(er.item()))

    # ---- sustained: the same step for >= --sustain-s seconds, in windows of 100 steps (thermal / clock steady state; long enough
    # for an SMI sampler to see the GPU busy).  The window count comes from the MAX-reduced timing above, so every rank runs
    # the same number of steps (the step holds a collective when N > 1).
    sustained = None
    if args.full and args.sustain_s > 0:
        wsteps = 100
        nwin = max(3, int(np.ceil(args.sustain_s / (wsteps * elapsed / args.steps))))
        rates = []
        ts0 = time.perf_counter()
        for _ in range(nwin):
            tw = time.perf_counter()
            for _ in range(wsteps):
                step()
            drain()
            torch.cuda.synchronize()
            ew = torch.tensor([time.perf_counter() - tw], dtype=torch.float64, device=dev)
            if world > 1:
                dist.all_reduce(ew, op=dist.ReduceOp.MAX)
            rates.append(world * Bc * wsteps / float(ew.item()))
        sustained = {"seconds": round(time.perf_counter() - ts0, 3), "steps": nwin * wsteps, "window_steps": wsteps, "windows": nwin,
                     "value_mean": round(nwin / sum(1.0 / r for r in rates), 1), "value_min_window": round(min(rates), 1),
                     "value_max_window": round(max(rates), 1), "value_last_window": round(rates[-1], 1), "unit": "cube-bounds/s",
                     "is": "the timed step repeated back to back, one host sync per 100 steps; mean = total cube bounds / total time"}

    # ---- ICP iterations/s: the loop does not shard, so N GPUs run N replicas side by side ----
    icp = None
    if args.full and not args.no_icp:
        ms = C.c_float()
        Ri, ti = np.eye(3, dtype=np.float32).reshape(9).copy(), np.zeros(3, np.float32)
        err, it = C.c_float(), C.c_int32()
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        B.check(lib.goicp_icp_run(h, fp(Ri), fp(ti), 5, -1e30, C.byref(err), C.byref(it)))
        if world > 1:
            dist.barrier()
        t1 = time.perf_counter()
        B.check(lib.goicp_icp_run(h, fp(Ri), fp(ti), 200, -1e30, C.byref(err), C.byref(it)))
        rate = torch.tensor([it.value / (time.perf_counter() - t1)], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(rate, op=dist.ReduceOp.SUM)
        icp_rate = float(rate.item())
        B.check(lib.goicp_time_icp_pass(h, fp(Ri), fp(ti), 50, C.byref(ms)))          # every query walks the tree (neighbour cache bypassed)
        ms_hit = C.c_float(float("nan"))
        if args.icp_nn_cache != 0:
            B.check(lib.goicp_time_icp_pass_cached(h, fp(Ri), fp(ti), 50, C.byref(ms_hit)))   # repeated pose: every query hits the cache
        # an ICP iteration moves N x [12 B query + D x 16 B nodes + L x 12 B leaf points] + N x 12 B write-back with L = 10,
        # D = ceil(log2(M / L)) = N (24 + 16 D + 120) bytes; time = pass + finalize (HIP events around back-to-back iterations)
        D = int(np.ceil(np.log2(M / 10.0)))
        icp_bytes = N * (24.0 + 16.0 * D + 120.0)
        built_bytes_icp = N * (16.0 + 4.0 + int(np.ceil(np.log2(M / 16.0)) / 6 + 0.999) * 1536.0 / 4 + 16 * 16.0)   # as built: query, DT seed, a quarter of a 64-box group per level (per row of 16 lanes), one 256-B leaf
        nn_gbs = icp_bytes / (ms.value * 1e-3) / 1e9
        icp = {"icp_iters_per_s": round(icp_rate, 1), "icp_replicas": world, "icp_iteration_ms": round(ms.value, 4),
               "icp_iteration_ms_is": "pass + finalize, HIP events around 50 back-to-back iterations at a frozen pose",
               "icp_iters_per_s_is": "iterations 6..205 of ONE ICP trajectory from the identity pose (every iteration moves the cloud; host round trips included)",
               "icp_pass_all_hits_ms": round(ms_hit.value, 4),
               "icp_bytes_per_iter": icp_bytes, "icp_bytes_per_iter_as_built": built_bytes_icp,
               "roofline_nn": {"bound": "latency", "kernel": "goicp::icp_pass_kernel + icp_finalize_update_acc", "achieved": round(nn_gbs, 1),
                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(nn_gbs / HBM_PEAK_GBS, 4), "traffic": None,
                               "bytes_model": "SURVEY 8(d): N (24 + 16 ceil(log2(M/10)) + 120) bytes per iteration",
                               "limiter": "not bytes: the dependent seed -> group -> leaf round trips of the slowest walks and VALU issue (DESIGN 3.2); "
                                          "the HBM fraction is reported because SURVEY 8(d) asks for it, it is not this kernel's ceiling"},
               "pose": "ICP-only local minimum reached from identity (205 forced iterations)"}
        pmc_icp = _profile("pmc_icp.json")
        if args.workload == "bunny" and pmc_icp:
            tr, prov, pj = _profile_traffic(pmc_icp, "hbm_bytes_per_pass_corrected", lib.goicp_kernel_source_hash().decode())
            icp["roofline_nn"].update({"traffic": tr, "traffic_source": "profiles/%s (rocprofv3 --pmc, FETCH_SIZE x2 + WRITE_SIZE per pass, fabric side of L2)" % os.path.basename(pmc_icp),
                                       "hbm_frac": None if tr is None else round(tr / (ms.value * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "pmc_reading": pj.get("reading")})
            icp["roofline_nn"].update(prov)

    if rank == 0 and args.full:
        # ---- roofline of the dominant kernel: HIP events on the launch stream, live ----
        ms = C.c_float()
        B.check(lib.goicp_time_bounds_device(h, d_rots.data_ptr(), d_cubes.data_ptr(), Bc, d_ub.data_ptr(), d_lb.data_ptr(), 10, C.byref(ms)))
        launch_s = ms.value * 1e-3
        # The kernel is NOT HBM-bound at these sizes (cloud + DT are cache-resident, 95 % L2 hits): the PMC counters say
        # the vector-memory address / L1 path is busy for the whole kernel.  Its ceiling is therefore
        # measured, in this run, by a probe kernel that only issues independent 4-byte loads into the same resident DT
        # (goicp_probe_gather): coalesced / fully divergent, from an L1-sized, an L2-sized and the whole-grid window.
        probe = {}
        for name, mode, window in () if args.no_probe else (("coalesced_l1", 0, 16 << 10), ("coalesced_l2", 0, 2 << 20), ("coalesced_dt", 0, 1 << 40),
                                   ("divergent_l1", 1, 16 << 10), ("divergent_l2", 1, 2 << 20), ("divergent_dt", 1, 1 << 40),
                                   ("lines4_l2", 4, 2 << 20), ("lines8_l2", 8, 2 << 20), ("lines16_l2", 16, 2 << 20), ("lines32_l2", 32, 2 << 20),
                                   ("lines16_l1", 16, 64 << 10), ("lines32_l1", 32, 64 << 10), ("lds_tile_gather", 2, 64 << 10)):
            v = C.c_double()
            B.check(lib.goicp_probe_gather(h, mode, window, C.byref(v)))
            probe[name] = round(v.value / 1e9, 2)
        lookups = float(Bc) * N                                    # one DT lookup per (cube, point)
        glook = lookups / launch_s / 1e9
        peak = probe.get("coalesced_l1", float("nan"))
        # algorithmic bytes: SURVEY 8(d)'s no-reuse model (16 N ub pass / 20 N lb pass) and the kernel as built
        # (a point's 16 B are loaded once per 8 sibling cubes = 2 N per cube bound, + 4 N of DT voxels)
        alg_bytes = (Bc - n_lb) * 16.0 * N + n_lb * 20.0 * N
        built_bytes = Bc * (2.0 + 4.0) * N
        # HBM-side traffic of the same launch: PMC counters cannot be read from inside this process; they are
        # collected with `rocprofv3 --pmc` on this exact command (separate passes for FETCH_SIZE and WRITE_SIZE,
        # gfx950 x2 correction on FETCH_SIZE) and committed under profiles/
        traffic, traffic_src, limiter, traffic_prov = None, None, None, {}
        for pmc in (_profile("pmc_bounds_%s.json" % args.workload),):
            cand = os.path.basename(pmc) if pmc else ""
            if cand and Bc == 65536 and args.dt_size == (300 if args.workload != "s2" else 512):
                traffic, traffic_prov, j = _profile_traffic(pmc, "hbm_bytes_per_launch_corrected", lib.goicp_kernel_source_hash().decode())
                traffic_src = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, FETCH_SIZE x2 on gfx950; fabric side of L2, Infinity-Cache hits included: an upper bound on HBM bytes)" % cand
                limiter = j.get("limiter")
                break
        roofline = {"bound": "l1-gather", "kernel": "goicp::bounds_kernel", "achieved": round(glook, 2), "peak": peak, "unit": "Glookup/s",
                    "frac": round(glook / peak, 4),
                    "peak_source": "goicp_probe_gather in this run: independent coalesced 4-B loads from a 16 KiB window per workgroup of the resident DT",
                    "probe_Glookup_per_s": probe,
                    "frac_of_divergent_l2_probe": round(glook / probe.get("divergent_l2", float("nan")), 4),
                    "traffic": traffic, "traffic_source": traffic_src,
                    "hbm": {"peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "traffic_GBs": None if traffic is None else round(traffic / launch_s / 1e9, 1),
                            "frac": None if traffic is None else round(traffic / launch_s / 1e9 / HBM_PEAK_GBS, 4),
                            "algorithmic_GBs_survey_model": round(alg_bytes / launch_s / 1e9, 1),
                            "algorithmic_GBs_as_built": round(built_bytes / launch_s / 1e9, 1),
                            "note": "SURVEY 8(d) prices a cube bound at 16 N / 20 N bytes (no reuse); the kernel loads a point once per 8 sibling cubes "
                                    "(2 N + 4 N bytes per cube bound) and both operands are cache-resident, so bytes per second against the HBM peak is "
                                    "not a ceiling for this kernel -- informational only"},
                    "launch_ms": round(ms.value, 4), "lookups_per_launch": lookups,
                    "algorithmic_bytes_per_launch": alg_bytes, "algorithmic_bytes_per_launch_as_built": built_bytes,
                    "cube_bounds_per_s_kernel": round(Bc / launch_s, 1)}
        roofline["frac_of_lines16_l1_probe"] = round(glook / probe.get("lines16_l1", float("nan")), 4)
        roofline.update(traffic_prov)
        # SURVEY 8(d)'s own recipe, so that its answer is in the line and not only in prose: algorithmic bytes (16 N ub pass / 20 N lb pass, no
        # reuse) / launch time / 8 TB/s.  Above 1 at these sizes -- void as a fraction: both operands are cache-resident (L2 hit 95 %) and a
        # point is loaded once per 8 sibling cubes; `frac` (measured gather ceiling) and hbm.frac (counter traffic) are the ones that bind
        roofline["frac_survey_model"] = round(alg_bytes / launch_s / 1e9 / HBM_PEAK_GBS, 4)
        roofline["frac_survey_model_is"] = "SURVEY 8(d) bytes (16 N / 20 N per cube bound, no reuse) / launch time / 8 TB/s -- void when > 1: cache-resident operands + sibling reuse (a point's 16 B serve 8 cubes)"
        if limiter:
            roofline["limiter"] = limiter
        if args.workload == "s2" and traffic is not None:
            # BASELINE configs[4] is the HBM-roofline configuration: the 537 MB DT does not fit the Infinity Cache, half of the L2
            # lookups miss, and the bytes that cross the fabric per launch (PMC) over the launch time ARE the bound here
            roofline = dict(roofline, bound="hbm", achieved=round(traffic / launch_s / 1e9, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                            frac=round(traffic / launch_s / 1e9 / HBM_PEAK_GBS, 4),
                            peak_source="MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured achievable)",
                            l1_gather={"achieved_Glookup_per_s": round(glook, 2), "peak": peak, "frac": round(glook / peak, 4) if probe else None})
        # ---- the generic path: SURVEY 8(d)'s batch of unrelated cubes through the same entry point ----
        generic = None
        if not args.no_probe:
            g_rots, g_recs, g_nlb = make_generic_batch(pkg, reg, Bc, 8, seed=99)
            gd_rots = torch.from_numpy(g_rots.reshape(-1)).to(dev)
            gd_cubes = torch.from_numpy(g_recs.view(np.uint8).reshape(-1)).to(dev)
            gms = C.c_float()
            B.check(lib.goicp_time_bounds_device(h, gd_rots.data_ptr(), gd_cubes.data_ptr(), len(g_recs), d_ub.data_ptr(), d_lb.data_ptr(), 5, C.byref(gms)))
            generic = {"workload": "SURVEY 8(d) microbench batch: %d independent cubes (centres U[-0.5,0.5]^3, half-width 1/64), 8 rotations in the pi-ball, every second a lb pass" % Bc,
                       "launch_ms": round(gms.value, 4), "cube_bounds_per_s": round(Bc / (gms.value * 1e-3), 1),
                       "Glookup_per_s": round(lookups / (gms.value * 1e-3) / 1e9, 2), "frac_of_peak": round(lookups / (gms.value * 1e-3) / 1e9 / peak, 4)}
            # the same batch through goicp_eval_bounds_device_grouped: bucketed on the device by (rotation, pass, translation cell), evaluated,
            # written back in the caller's order -- bit-identical bounds; the grouping kernels are inside the timed region
            ref_ub = d_ub.clone()
            ggms = C.c_float()
            B.check(lib.goicp_time_bounds_device_grouped(h, gd_rots.data_ptr(), len(g_rots), gd_cubes.data_ptr(), len(g_recs), d_ub.data_ptr(), d_lb.data_ptr(), 5, C.byref(ggms)))
            assert torch.equal(ref_ub, d_ub), "grouped evaluation changed a bound"
            generic["grouped"] = {"call_ms": round(ggms.value, 4), "cube_bounds_per_s": round(Bc / (ggms.value * 1e-3), 1),
                                  "frac_of_peak": round(lookups / (ggms.value * 1e-3) / 1e9 / peak, 4),
                                  "is": "goicp_eval_bounds_device_grouped: device counting sort by (rotation, pass, 12-bit Morton cell of the translation) + evaluation + un-permute, all timed; same bits"}
            roofline["frac_generic_grouped"] = generic["grouped"]["frac_of_peak"]
            # `frac` is on the sibling-structured batch the search produces; SURVEY 8(d)'s literal microbench batch gives:
            roofline["frac_generic"] = generic["frac_of_peak"]
            roofline["achieved_generic"] = generic["Glookup_per_s"]
            roofline["frac_is"] = "sibling-structured batch (8 children per expansion: 6 voxel-index computations per point); frac_generic = SURVEY 8(d)'s batch of unrelated cubes (24 per point)"
            B.check(lib.goicp_eval_bounds_device(h, d_rots.data_ptr(), d_cubes.data_ptr(), Bc, d_ub.data_ptr(), d_lb.data_ptr(), stream))   # restore the headline batch's outputs
            torch.cuda.synchronize()
        # ---- what this GPU's HBM actually streams (device-to-device copy of 2 GiB, read + write counted) ----
        a_ = torch.empty(1 << 29, dtype=torch.float32, device=dev); b_ = torch.empty_like(a_)
        b_.copy_(a_); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            b_.copy_(a_)
        e1.record(); torch.cuda.synchronize()
        roofline["hbm_copy_probe_GBs"] = round(5 * 2 * a_.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
        del a_, b_
        # ---- the same batch through the host-pointer entry point (PCIe-inclusive; never `value`) ----
        h_ub, h_lb = np.empty(Bc, np.float32), np.empty(Bc, np.float32)
        cube_arr = (B.CCube * Bc).from_buffer_copy(recs.tobytes())
        fpp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        B.check(lib.goicp_eval_bounds_batch(h, fpp(rots.reshape(-1)), len(rots), cube_arr, Bc, fpp(h_ub), fpp(h_lb)))
        t1 = time.perf_counter()
        for _ in range(5):
            B.check(lib.goicp_eval_bounds_batch(h, fpp(rots.reshape(-1)), len(rots), cube_arr, Bc, fpp(h_ub), fpp(h_lb)))
        host_ms = (time.perf_counter() - t1) / 5 * 1e3
        roofline["host_pointer_call_ms"] = round(host_ms, 4)
        roofline["host_pointer_cube_bounds_per_s"] = round(Bc / (host_ms * 1e-3), 1)
        assert np.array_equal(h_ub, d_ub.cpu().numpy()), "host-pointer and device-pointer entry points disagree"
        # ---- end-to-end registration of the same clouds ----
        e2e = None
        if not args.no_e2e:
            eng = pkg.FastGoICP(model, data, 1e-3, dt_size=V, dt_layout=args.dt_layout, device=local_rank, kd_gpu_build=args.kd_gpu_build,
                                bounds_fp16=args.bounds_fp16, device_queues=args.device_queues, icp_nn_cache=args.icp_nn_cache, flow=args.flow,
                                **({"icp_fused": args.icp_fused} if args.icp_fused >= 0 else {}))
            walls = []
            for _ in range(max(1, args.e2e_repeats)):          # the same registration, repeated on the same engine (every run starts from scratch: register_begin)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng.run()
                walls.append(time.perf_counter() - t1)
            wall = float(np.median(walls))
            r = eng.registration.poll()
            e2e = {"register_s": round(wall, 4), "register_s_is": "median of %d runs" % len(walls), "register_s_min": round(min(walls), 4), "register_s_max": round(max(walls), 4),
                   "register_s_spread_pct": round(100 * (max(walls) - min(walls)) / wall, 2), "register_s_runs": [round(w, 4) for w in walls],
                   "sse": float(r.best_sse), "cube_bounds": int(r.counters.cubes),
                   "cube_bounds_per_s": round(r.counters.cubes / wall, 1), "rot_pops": int(r.counters.rot_pops),
                   "trans_pops": int(r.counters.trans_pops), "icp_iters": int(r.counters.icp_iters),
                   "dt_build_ms": round(r.dt_build_ms, 2), "engine_create_s": round(t_create, 3)}
            if args.workload == "bunny":
                with open(os.path.join(ROOT, "tests", "golden", "e2e_bunny_full.json")) as f:
                    gj = json.load(f)
                dR = np.linalg.norm(np.asarray(r.optR, np.float64).reshape(3, 3) - np.array(gj["R"]).reshape(3, 3))
                e2e.update({"reference_cpu_register_s": 502.7, "reference_sse": gj["sse"],
                            "rot_error_rad": round(float(2 * np.arcsin(min(1.0, dR / (2 * np.sqrt(2))))), 6),
                            "trans_error": round(float(np.linalg.norm(np.asarray(r.optT, np.float64) - np.array(gj["t"]))), 6),
                            "pose_error_vs": "the reference CPU Go-ICP's optimum (tests/golden/e2e_bunny_full.json); tolerance 2e-3 rad / 2e-3 (SURVEY 8c)"})
        # ---- the prove-the-optimum registration (bunny at --deep-mse, below the optimum's error: no early exit; the search expands every node whose
        # lower bound stays SSEThresh under the optimum -- 343 M cube bounds): what a registration costs when it has to certify global optimality.
        # At N > 1 the same run is the world-1 side of e2e_sharded.deep, so it is made here only at N = 1
        e2e_deep = None
        if not args.no_e2e and world == 1 and args.workload == "bunny" and args.deep_mse > 0 and not args.no_deep:
            engd = pkg.FastGoICP(model, data, args.deep_mse, dt_size=V, dt_layout=args.dt_layout, device=local_rank)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            engd.run()
            walld = time.perf_counter() - t1
            cd = engd.counters
            e2e_deep = {"workload": "bunny (N=%d, M=%d, DT %d^3) at mse %g: SSEThresh below the optimum's error, the search proves the optimum" % (N, M, V, args.deep_mse),
                        "register_s": round(walld, 4), "sse": float(engd.get_best_error()), "sse_threshold": float(engd.sse_threshold), "cube_bounds": int(cd.cubes),
                        "cube_bounds_per_s": round(cd.cubes / walld, 1), "from_lds_tiles_pct": round(800.0 * cd.tile_expansions / max(cd.cubes, 1), 1),
                        "rot_pops": int(cd.rot_pops), "icp_iters": int(cd.icp_iters), "batches_in_lanes": int(cd.lane_batches), "queue_fallbacks": int(cd.queue_fallbacks),
                        "vs_microbench_rate": round(cd.cubes / walld / value, 3)}
            engd.registration.close()
        cpu = None
        if not args.no_cpu:                      # rank 0's host cores, at every N (the other ranks wait at the next collective)
            c = cpu_baseline(reg, model, data)
            port = {"port_value": round(c["1thread"], 1), "port_allcores_value": round(c["allcores"], 1), "port_allcores": c["ncores"],
                    "port_sample": "oracle cube_bound (restated InnerBnB body) on the same DT/cloud, ~6 s per leg, alternating ub/lb batches of 64 cubes; all-core leg = OpenMP over cubes",
                    "icp_iters_per_s_1thread": round(c["icp_iters_per_s_1thread"], 2)}
            ref = reference_baseline() if args.workload == "bunny" else None
            if ref:
                cpu = {"value": round(ref["cube_bounds_per_s"], 1), "unit": "cube-bounds/s", "cores": 1, "kind": "reference",
                       "sample": "oracle/_ref/ref_harness_bench: the reference's own GoICP::InnerBnB on the same clouds, %d alternating ub/lb searches over "
                                 "seeded rotations in %.1f s = %d cube bounds [%s] (%d translation-node pops); its DT build (%.1f s) is outside the timed "
                                 "region.  Flags per TU: %s" % (ref["inner_bnb_calls"], ref["seconds"], ref["cube_bounds"], ref["count"], ref["trans_pops"],
                                                                ref["dt_build_s"], REF_FLAGS),
                       "reference_dt_build_s": ref["dt_build_s"]}
            else:
                cpu = {"value": port["port_value"], "unit": "cube-bounds/s", "cores": 1, "kind": "port", "sample": port["port_sample"]}
            cpu.update(port)
        out.update({"value_repeats": {"n": len(repeats), "min": round(min(repeats), 1), "max": round(max(repeats), 1),
                                      "spread_pct": round(100 * (max(repeats) - min(repeats)) / value, 2)},
                    "sustained": sustained,
                    "roofline": roofline, "generic_path": generic, "cpu_baseline": cpu, "icp": icp, "e2e": e2e, "e2e_deep": e2e_deep, "e2e_sharded": None})
    reg.close()
    del d_rots, d_cubes, d_ub, d_lb

    # ---- the HBM-bound configuration (BASELINE configs[4] per GPU: N = M = 1 M, DT 512^3 = 537 MB, beyond the Infinity Cache):
    # a few launches of the same 65 536-cube batch, and the HBM roofline of that launch = fabric-side bytes (PMC, committed
    # profile of this same batch) / the launch time measured HERE / 8 TB/s
    if rank == 0 and args.full and args.workload == "bunny" and args.s2_steps > 0:
        try:
            out["s2"] = s2_leg(pkg, B, lib, args, dev, torch)
        except Exception as e:      # reported, never fatal for the headline line
            out["s2"] = {"error": repr(e)}

    # ---- N > 1: the sharded search itself (rotation cubes dealt to the ranks, RCCL min-all-reduce of the best error + winner's pose
    # between steps, rebalancing; csrc/shard.cpp over csrc/rccl_comm.cpp), two workloads:
    #   spanner  BASELINE configs[3]: the reference's own scans (tests/golden/spanner_*.f32: noisy_flipped_model_spanner.ply /
    #            rotated_model_spanner.ply x 0.02, 150 000 points each, mse 1e-4) -- 64 rotation nodes, ~20 ms on ONE GPU: the
    #            latency-floor case (what an exchange costs), bulk-synchronous and with the one-step-stale exchange;
    #   deep     the bunny at --deep-mse (3e-5: below the optimum's error, so the search has to PROVE the optimum -- 6.7 s and 340 M
    #            cube bounds on one GPU): the strong-scaling case.  A world-1 run of the same problem is timed in this same invocation
    #            (rank 0 alone, the others wait), so `speedup_vs_world1` and `work_inflation` (cube bounds of all ranks / world-1's)
    #            are measured, not quoted.
    sharded_res = None
    sharded_failed = False
    if world > 1 and args.full and not args.no_sharded:
        box = {}

        def sharded_leg():
            try:
                torch.cuda.set_device(local_rank)
                from cuda_go_icp_amd import sharded
                g = os.path.join(ROOT, "tests", "golden")
                tgt = np.fromfile(os.path.join(g, "spanner_target.f32"), dtype="<f4").reshape(-1, 3)
                srcc = np.fromfile(os.path.join(g, "spanner_source.f32"), dtype="<f4").reshape(-1, 3)
                ms_, md_ = srcc.astype(np.float64).mean(0), tgt.astype(np.float64).mean(0)        # ground truth: the files correspond point by point
                U, _, Vt = np.linalg.svd((srcc - ms_).T @ (tgt - md_))
                Rgt = Vt.T @ np.diag([1, 1, np.linalg.det(Vt.T @ U.T)]) @ U.T
                tgt_t = md_ - Rgt @ ms_
                # the exchange runs inside the library (csrc/shard.cpp) over its own RCCL communicator (csrc/rccl_comm.cpp):
                # rank 0 makes the ncclUniqueId, torch.distributed only carries those 128 bytes to the other ranks
                if args.backend == "nccl":
                    ident = C.create_string_buffer(128)
                    if rank == 0:
                        B.check(lib.goicp_rccl_unique_id(ident))
                    idt = torch.tensor(list(ident.raw), dtype=torch.uint8, device=dev)
                    dist.broadcast(idt, src=0)
                    ident = C.create_string_buffer(bytes(idt.cpu().tolist()), 128)
                    comm = B.CCommOps()
                    B.check(lib.goicp_rccl_comm_create(ident, rank, world, local_rank, C.byref(comm)))
                    # every collective has a deadline inside the library: a lost rank is GOICP_ERR_TIMEOUT there, well before the watchdog below
                    B.check(lib.goicp_comm_set_timeout_ms(C.byref(comm), max(5, args.sharded_timeout // 3) * 1000))
                    exchange = "library protocol over RCCL (ncclAllReduce MIN of 6 packed u64 + ncclBroadcast of R|t on change + rebalancing; per-collective deadline)"
                else:
                    comm = sharded.torch_comm_ops(dist, torch.device("cpu"))
                    exchange = "library protocol over torch.distributed gloo (rehearsal: every rank on GPU 0)"
                ramp = max(0, args.shard_ramp)
                step_rule = "8 rotation parents in the first step, doubling per step up to %d (the single-GPU driver's ramp), one exchange per batch" % ramp if ramp > 8 else "8 rotation parents per step"

                def one(t_cloud, s_cloud, mse, stale, dt_size=300):
                    eng = pkg.FastGoICP(t_cloud, s_cloud, mse, dt_size=dt_size, device=local_rank)
                    dist.barrier()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    lstats = sharded.run_sharded_library(eng, comm, rot_pops_per_step=8, stale=stale, ramp_to=ramp)
                    wall = time.perf_counter() - t1
                    sse, Rr, tr = eng.pose()
                    c = eng.counters
                    tot = torch.tensor([float(c.cubes), float(c.rot_pops), float(lstats["steps_idle"]), float(c.icp_iters)], dtype=torch.float64, device=dev)
                    dist.all_reduce(tot, op=dist.ReduceOp.SUM)
                    mx = torch.tensor([wall, lstats["wait_ms"], lstats["step_ms"], float(c.cubes)], dtype=torch.float64, device=dev)
                    dist.all_reduce(mx, op=dist.ReduceOp.MAX)
                    out_ = {"wall_s": round(float(mx[0].item()), 4), "sse": float(sse), "sse_threshold": float(eng.sse_threshold),
                            "cube_bounds_all_ranks": int(tot[0].item()), "cube_bounds_busiest_rank": int(mx[3].item()), "rot_pops_all_ranks": int(tot[1].item()), "icp_iters_all_ranks": int(tot[3].item()),
                            "steps": lstats["steps"], "exchanges": lstats["exchanges"], "pose_broadcasts": lstats["broadcasts"], "donations": lstats["donations"],
                            "idle_steps_all_ranks": int(tot[2].item()), "max_rank_wait_ms": round(float(mx[1].item()), 3), "max_rank_step_ms": round(float(mx[2].item()), 3)}
                    eng.registration.close()
                    return out_, Rr.reshape(3, 3), tr

                res = {"exchange": exchange, "step": step_rule,
                       "spanner": {"workload": "BASELINE configs[3] spanner_goicp: N=M=150000 (the reference's noisy / rotated scans x 0.02), mse 1e-4, DT 300^3 -- 64 rotation nodes, ~20 ms on one GPU: the latency-floor case"}}
                for mode, stale in (("bulk_synchronous", False), ("stale_exchange", True)):
                    r_, Rr, tr = one(tgt, srcc, 1e-4, stale)
                    ang = float(2 * np.arcsin(min(1.0, np.linalg.norm(Rr.astype(np.float64) - Rgt) / (2 * np.sqrt(2)))))
                    r_.update({"rot_error_rad_vs_ground_truth": round(ang, 5), "trans_error_vs_ground_truth": round(float(np.linalg.norm(tr - tgt_t)), 5)})
                    res["spanner"][mode] = r_
                if args.deep_mse > 0:
                    bm = np.fromfile(os.path.join(g, "model_bunny.f32"), dtype="<f4").reshape(-1, 3)
                    bd = np.fromfile(os.path.join(g, "data_bunny.f32"), dtype="<f4").reshape(-1, 3)
                    w1 = torch.zeros(5, dtype=torch.float64, device=dev)
                    if rank == 0:
                        e1 = pkg.FastGoICP(bm, bd, args.deep_mse, dt_size=300, device=local_rank)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        e1.run()
                        w1[0] = time.perf_counter() - t1
                        c1 = e1.counters
                        w1[1], w1[2], w1[3], w1[4] = float(c1.cubes), float(c1.rot_pops), float(e1.get_best_error()), float(c1.icp_iters)
                        e1.registration.close()
                    dist.broadcast(w1, src=0)
                    wall1, cubes1, rot1, sse1 = float(w1[0].item()), float(w1[1].item()), float(w1[2].item()), float(w1[3].item())
                    d_, _, _ = one(bm, bd, args.deep_mse, False)
                    d_.update({"workload": "bunny (N=30379, M=35947, DT 300^3) at mse %g: SSEThresh below the optimum's error, so no early exit -- the search proves the optimum (strong scaling: the same problem at every N)" % args.deep_mse,
                               "world1": {"wall_s": round(wall1, 4), "cube_bounds": int(cubes1), "rot_pops": int(rot1), "sse": sse1, "is": "the same problem on rank 0 alone (goicp_register, no exchange), timed in this invocation"},
                               "speedup_vs_world1": round(wall1 / d_["wall_s"], 3), "work_inflation": round(d_["cube_bounds_all_ranks"] / max(cubes1, 1.0), 4),
                               "rot_nodes_inflation": round(d_["rot_pops_all_ranks"] / max(rot1, 1.0), 4),
                               "parallel_efficiency": round(wall1 / d_["wall_s"] / world, 3),
                               "same_optimum": bool(abs(d_["sse"] - sse1) <= 1e-3 * max(sse1, 1e-6) + d_["sse_threshold"])})
                    res["deep"] = d_
                if not args.no_s2_sharded:
                    # BASELINE configs[4]: the synthetic 1 M x 1 M cloud on a 512^3 DT (537 MB, HBM-resident), full SE(3) BnB, sharded.  The variant the
                    # parity test registers (tests/test_gpu_parity.py test_s2_fullsize): relief 0.15 and mse = 1.2 x the measured noise floor of the true
                    # pose, so that the outer BnB has to work (128 rotation nodes, ~1 400 ICP iterations of ~1 ms: an ICP-dominated registration --
                    # every rank refines its own candidates, the ICP loop does not shard -- hence a latency / replication case, not the scaling one)
                    from cuda_go_icp_amd import synth
                    s2t, s2s, s2R, s2tt = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"], amp=0.15)
                    w2 = torch.zeros(6, dtype=torch.float64, device=dev)
                    if rank == 0:
                        e2 = pkg.FastGoICP(s2t, s2s, 1e-3, dt_size=synth.S2["V"], device=local_rank)
                        floor = float(e2.registration.compute_sse_error(s2R, s2tt)) / len(s2s)
                        e2.registration.close()
                        e2 = pkg.FastGoICP(s2t, s2s, 1.2 * floor, dt_size=synth.S2["V"], device=local_rank)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        e2.run()
                        w2[0] = time.perf_counter() - t1
                        c2 = e2.counters
                        w2[1], w2[2], w2[3], w2[4], w2[5] = float(c2.cubes), float(c2.rot_pops), float(e2.get_best_error()), float(c2.icp_iters), floor
                        e2.registration.close()
                    dist.broadcast(w2, src=0)
                    floor = float(w2[5].item())
                    r2, R2, t2 = one(s2t, s2s, 1.2 * floor, False, dt_size=synth.S2["V"])
                    ang2 = float(2 * np.arcsin(min(1.0, np.linalg.norm(R2.astype(np.float64) - s2R) / (2 * np.sqrt(2)))))
                    r2.update({"workload": "BASELINE configs[4]: synthetic N=M=1000000, DT 512^3 (537 MB), relief 0.15, mse = 1.2 x the measured floor of the true pose (%.3g) -- the parity test's registration; ICP-dominated" % floor,
                               "rot_error_rad_vs_ground_truth": round(ang2, 5), "trans_error_vs_ground_truth": round(float(np.linalg.norm(t2 - s2tt)), 5),
                               "tolerance": "3e-2 rad / 1e-2 (tests/test_gpu_parity.py test_s2_fullsize: flat landscape at 1.2 x floor)",
                               "world1": {"wall_s": round(float(w2[0].item()), 4), "cube_bounds": int(w2[1].item()), "rot_pops": int(w2[2].item()), "sse": float(w2[3].item()), "icp_iters": int(w2[4].item())},
                               "speedup_vs_world1": round(float(w2[0].item()) / max(r2["wall_s"], 1e-9), 3)})
                    res["s2"] = r2
                if args.backend == "nccl":
                    B.check(lib.goicp_rccl_comm_destroy(C.byref(comm)))
                box['res'] = res
            except Exception as e:      # reported in the line; fatal for the exit code (below)
                import traceback
                traceback.print_exc()
                box['res'] = dict(box.get('res') or {}, error=repr(e))
                box['failed'] = True

        # the leg runs under a watchdog as a second line of defence behind the library's own per-collective deadlines
        import threading
        th = threading.Thread(target=sharded_leg, daemon=True)
        th.start()
        th.join(args.sharded_timeout)
        if th.is_alive():
            sharded_failed = True
            sharded_res = {"error": "no result within %d s (watchdog)" % args.sharded_timeout}
        else:
            sharded_res = box.get('res')
            sharded_failed = bool(box.get('failed'))

    if rank == 0:
        if args.full:
            out["e2e_sharded"] = sharded_res
        def _clean(o):                      # NaN (a leg that was switched off) is not JSON: null instead
            if isinstance(o, float) and o != o:
                return None
            if isinstance(o, dict):
                return {k: _clean(v) for k, v in o.items()}
            if isinstance(o, list):
                return [_clean(v) for v in o]
            return o
        print(json.dumps(_clean(out), allow_nan=False), flush=True)
    if sharded_failed:
        # ANY failure of the sharded leg on this rank (a lost rank / missed deadline / device error / exception) is fatal: the line
        # is out with its `error`, and the process reports FAILURE -- without the teardown (a collective may be stuck in it).  The
        # launcher ends the other ranks (spawn_ranks here, torchrun likewise) and starts fresh processes next time, never a re-exec
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
