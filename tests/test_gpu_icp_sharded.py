"""The sharded ICP loop on the GPU (goicp_icp_run_collective, goicp_register_sharded_collective_icp): N thread ranks on one
MI355X, each with its own engine made from the same clouds, over the library's in-process communicator (and two processes
over gloo).  Each rank evaluates a contiguous range of the world-1 pass's workgroups and the ranks add up the integer sums,
so every rank must end with the world-1 result BIT FOR BIT -- pose, error and iteration count."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, cloud, golden, load_pkg, rot_angle

pytestmark = pytest.mark.gpu

WORLDS = (1, 2, 3, 4, 8)
ERR_DIFF = 1e-7
TIMEOUT_MS = 120000


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _s2():
    from cuda_go_icp_amd import synth
    target, source, _, _ = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"])
    return target, source, {"dt_size": synth.S2["V"]}


# name -> (target, source, engine parameters)
CLOUDS = {
    "bunny": lambda: (cloud("model_bunny"), cloud("data_bunny"), {}),                 # 30 379 points: strided pass
    "bun000": lambda: (cloud("bun045"), cloud("bun000"), {}),                         # 40 256 points: neighbour pass, just above the threshold
    "spanner": lambda: (cloud("spanner_target"), cloud("spanner_source"), {}),        # 150 000
    "s2": _s2,                                                                        # 1 000 000, DT 512^3
    "bunny_cache": lambda: (cloud("model_bunny"), cloud("data_bunny"), {"icp_nn_cache": 1}),
    "spanner_cache": lambda: (cloud("spanner_target"), cloud("spanner_source"), {"icp_nn_cache": 1}),
    "rand": lambda: (cloud("model_rand"), cloud("data_rand"), {}),                    # 100 points = 7 workgroups: rank 0 of 8 is empty
}

# (R, t, max_iter): a full run from the identity, and a run capped at 7 iterations from a nearby pose
def _poses(pkg):
    return [(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 3000),
            (pkg.fgoicp.rodrigues([0.12, -0.07, 0.09]).astype(np.float32), np.array([0.02, -0.015, 0.03], np.float32), 7)]


def _bits(err, R, t, iters):
    return (np.float32(err).tobytes(), np.asarray(R, np.float32).tobytes(), np.asarray(t, np.float32).tobytes(), int(iters))


def _world1(pkg, reg, R, t, max_iter):
    icp = pkg.IterativeClosestPoint3D(reg, max_iter, ERR_DIFF, R, t)
    err, Rw, tw = icp.run()
    return _bits(err, Rw, tw, icp.iters)


def _regs(pkg, name, world):
    target, source, params = CLOUDS[name]()
    return [pkg.Registration(target, source, 1e-3, **params) for _ in range(world)], len(source)


def _check_partition(before, after, n, world):
    """the ranks' block ranges partition the world-1 grid, each query was evaluated once per pass, the pass was sliced"""
    st = sorted(after[:world], key=lambda s: s["rank"])
    assert [s["rank"] for s in st] == list(range(world)) and all(s["world"] == world for s in st)
    assert st[0]["block_begin"] == 0 and st[-1]["block_end"] == st[0]["blocks"]
    assert all(st[r]["block_end"] == st[r + 1]["block_begin"] for r in range(world - 1))
    assert all(s["sliced"] == 1 for s in st)
    passes = {after[r]["passes"] - before[r]["passes"] for r in range(world)}
    assert len(passes) == 1
    assert sum(after[r]["queries"] - before[r]["queries"] for r in range(world)) == n * passes.pop()
    assert len({after[r]["collectives"] - before[r]["collectives"] for r in range(world)}) == 1


@pytest.mark.parametrize("name", list(CLOUDS))
def test_collective_icp_bit_identical(pkg, name):
    from cuda_go_icp_amd import sharded
    regs, n = _regs(pkg, name, max(WORLDS))
    try:
        for R, t, max_iter in _poses(pkg):
            ref = _world1(pkg, regs[0], R, t, max_iter)
            for world in WORLDS:
                before = [r.icp_shard_stats() for r in regs[:world]]
                res = sharded.icp_run_thread_ranks(regs[:world], R, t, max_iter, ERR_DIFF, timeout_ms=TIMEOUT_MS)
                after = [r.icp_shard_stats() for r in regs[:world]]
                for rank, (rc, err, Rr, tr, it) in enumerate(res):
                    assert rc == 0
                    assert _bits(err, Rr, tr, it) == ref, (name, world, rank, max_iter, err, it, ref[3])
                _check_partition(before, after, n, world)
                if name == "rand" and world == 8:
                    assert after[0]["block_begin"] == after[0]["block_end"]      # the empty rank took part with zero totals
            print("%s: max_iter %d -> %d iterations, bit-identical at worlds %s" % (name, max_iter, ref[3], WORLDS))
    finally:
        for r in regs:
            r.close()


def test_collective_icp_trimmed_falls_back_to_replicas(pkg):
    """trim_fraction > 0 needs a global k-selection: every rank runs the full loop, still the world-1 result, sliced == 0"""
    from cuda_go_icp_amd import sharded
    target, source = cloud("model_bunny"), cloud("data_bunny", 3)
    regs = [pkg.Registration(target, source, 1e-3, trim_fraction=0.1) for _ in range(3)]
    try:
        for R, t, max_iter in _poses(pkg):
            ref = _world1(pkg, regs[0], R, t, max_iter)
            for world in (2, 3):
                res = sharded.icp_run_thread_ranks(regs[:world], R, t, max_iter, ERR_DIFF, timeout_ms=TIMEOUT_MS)
                assert all(rc == 0 and _bits(err, Rr, tr, it) == ref for rc, err, Rr, tr, it in res)
                assert all(r.icp_shard_stats()["sliced"] == 0 for r in regs[:world])
    finally:
        for r in regs:
            r.close()


def test_collective_icp_disagreement_is_invalid_everywhere(pkg):
    """ranks handed different start poses: all return GOICP_ERR_INVALID, none waits for the deadline"""
    from cuda_go_icp_amd import sharded
    regs = [pkg.Registration(cloud("model_bunny"), cloud("data_bunny"), 1e-3) for _ in range(3)]
    try:
        I, Z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        t1 = np.array([0.0, 0.0, 1e-3], np.float32)
        t0 = time.time()
        res = sharded.icp_run_thread_ranks(regs, [I, I, I], [Z, t1, Z], 50, ERR_DIFF, timeout_ms=20000, raise_on_error=False)
        assert [r[0] for r in res] == [-1, -1, -1]
        assert time.time() - t0 < 15
        # the engines are fine afterwards: agreeing ranks run
        res = sharded.icp_run_thread_ranks(regs[:2], I, Z, 50, ERR_DIFF, timeout_ms=20000, raise_on_error=False)
        assert [r[0] for r in res] == [0, 0]
    finally:
        for r in regs:
            r.close()


def _s2_registration_setup(pkg):
    from cuda_go_icp_amd import synth
    from test_gpu_parity import S2_AMP, S2_OVER_FLOOR
    target, source, Rgt, tgt = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"], amp=S2_AMP)
    V = synth.S2["V"]
    reg = pkg.Registration(target, source, 1e-3, dt_size=V)
    floor = float(reg.compute_sse_error(Rgt, tgt)) / len(source)
    reg.close()
    return target, source, Rgt, tgt, S2_OVER_FLOOR * floor, {"dt_size": V}


def _collective_registration(pkg, engines, world):
    from cuda_go_icp_amd import sharded
    before = [e.registration.icp_shard_stats() for e in engines[:world]]
    stats = sharded.run_thread_ranks(engines[:world], rot_pops_per_step=8, ramp_to=32, timeout_ms=TIMEOUT_MS, collective_icp=True)
    after = [e.registration.icp_shard_stats() for e in engines[:world]]
    assert all(s["status"] == 0 and s["failed_rank"] == -1 for s in stats)
    poses = [(e.optR.tobytes(), e.optT.tobytes(), e.get_best_error().tobytes()) for e in engines[:world]]
    assert len(set(poses)) == 1, "ranks ended with different poses"
    assert len({(s["exchanges"], s["broadcasts"], s["donations"]) for s in stats}) == 1
    coll = {a["collectives"] - b["collectives"] for a, b in zip(after, before)}
    assert len(coll) == 1 and coll.pop() > 0
    return stats, engines[0].counters


def test_register_sharded_collective_icp_s2(pkg):
    """BASELINE configs[4] (synthetic S2, 1 M x 1 M, DT 512^3) with test_s2_fullsize's setup (relief 0.15, mse 1.2 x the measured
    floor): the sharded registration with collective refinements at world 2 and 4 -- every rank ends with the same pose bits, near
    the ground truth, and the refinement passes stay within 1.5 x world 1's (replicated refinements: 1.9 x at world 2)."""
    target, source, Rgt, tgt, mse, params = _s2_registration_setup(pkg)
    w1 = pkg.FastGoICP(target, source, mse, **params)
    w1.run()
    base_iters = w1.counters.icp_iters
    assert w1.finished
    w1.registration.close()
    engines = [pkg.FastGoICP(target, source, mse, **params) for _ in range(4)]
    try:
        for world in (2, 4):
            stats, c = _collective_registration(pkg, engines, world)
            e = engines[0]
            assert e.get_best_error() < e.sse_threshold
            assert rot_angle(e.optR, Rgt) <= 3e-2 and np.linalg.norm(e.optT - tgt) <= 1e-2
            assert c.icp_iters <= 1.5 * base_iters, (world, c.icp_iters, base_iters)
            print("S2 world %d collective refinements: %d ICP passes (world 1: %d), %d exchanges" % (world, c.icp_iters, base_iters, stats[0]["exchanges"]))
    finally:
        for e in engines:
            e.registration.close()


def test_register_sharded_collective_icp_spanner(pkg):
    """BASELINE configs[3] (spanner, every 50th source point, tests/golden/e2e_spanner_sub.json) at world 2"""
    g = golden("e2e_spanner_sub")
    target, source = cloud("spanner_target"), cloud("spanner_source", 50)
    engines = [pkg.FastGoICP(target, source, g["mse_threshold"]) for _ in range(2)]
    try:
        _collective_registration(pkg, engines, 2)
        e = engines[0]
        assert e.get_best_error() < g["sse_threshold"]
        assert rot_angle(e.optR, np.array(g["R"])) <= 8e-2 and np.linalg.norm(e.optT - np.array(g["t"])) <= 2e-2
    finally:
        for e in engines:
            e.registration.close()


def test_register_collective_icp_rejects_stale_exchange(pkg):
    from cuda_go_icp_amd import sharded
    engines = [pkg.FastGoICP(cloud("model_rand"), cloud("data_rand"), 5e-3) for _ in range(2)]
    try:
        stats = sharded.run_thread_ranks(engines, stale=True, raise_on_error=False, collective_icp=True, timeout_ms=20000)
        assert [s["status"] for s in stats] == [-1, -1]
    finally:
        for e in engines:
            e.registration.close()


WORKER_GLOO = r"""
import json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import datetime
import numpy as np
import torch, torch.distributed as dist
from conftest import cloud, load_pkg
pkg = load_pkg(); pkg.load_library()
from cuda_go_icp_amd import sharded
dist.init_process_group(backend="gloo", timeout=datetime.timedelta(seconds=300))
rank = dist.get_rank()
reg = pkg.Registration(cloud("spanner_target"), cloud("spanner_source"), 1e-3)
comm = sharded.torch_comm_ops(dist, torch.device("cpu"))
out = []
for R, t, max_iter in {poses!r}:
    R, t = np.array(R, np.float32), np.array(t, np.float32)
    rc, err, Rr, tr, it = reg.icp_run_collective(comm, R, t, max_iter, {err_diff!r}, raise_on_error=False)
    icp = pkg.IterativeClosestPoint3D(reg, max_iter, {err_diff!r}, R, t)
    e1, R1, t1 = icp.run()
    out.append({{"rc": rc, "coll": [float(err), Rr.reshape(-1).tolist(), tr.tolist(), it],
                 "w1": [float(e1), R1.reshape(-1).tolist(), t1.tolist(), icp.iters]}})
st = reg.icp_shard_stats()
json.dump({{"runs": out, "stats": st}}, open(os.path.join({out!r}, "icp_rank%d.json" % rank), "w"))
reg.close()
dist.barrier()
dist.destroy_process_group()
"""


def test_collective_icp_gloo_two_processes(pkg, tmp_path):
    """two processes over gloo (torch_comm_ops: the broadcast fallback of the sum), one GPU: bit-identical collective ICP on the spanner"""
    poses = [(R.reshape(-1).tolist(), t.tolist(), min(m, 80)) for R, t, m in _poses(pkg)]
    script = tmp_path / "worker_icp.py"
    script.write_text(WORKER_GLOO.format(root=ROOT, out=str(tmp_path), poses=poses, err_diff=ERR_DIFF))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29563", str(script)]
    r = subprocess.run(cmd, env=env, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = [json.load(open(tmp_path / ("icp_rank%d.json" % k))) for k in range(2)]
    for a, b in zip(res[0]["runs"], res[1]["runs"]):
        assert a["rc"] == 0 and b["rc"] == 0
        assert a["coll"] == b["coll"] == a["w1"] == b["w1"]
    s0, s1 = res[0]["stats"], res[1]["stats"]
    assert s0["sliced"] == s1["sliced"] == 1 and s0["block_end"] == s1["block_begin"]
    assert s0["queries"] + s1["queries"] == 150000 * s0["passes"]
