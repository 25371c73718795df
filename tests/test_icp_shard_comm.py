"""The integer sum behind the sharded ICP loop, on CPU: goicp_comm_allreduce_sum_i64 over the library's in-process thread
communicator (its native sum) and over torch.distributed's gloo through sharded.torch_comm_ops (a caller's table: the
fallback of `world` broadcasts).  Every rank must get the exact sum mod 2^64 -- the collective ICP's bit-identity rests on it."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from conftest import ROOT, load_pkg

MASK = (1 << 64) - 1


def _words(rank, n=19):
    """mixed-sign words, some near +-2^63 so that the sum wraps, distinct per rank"""
    rng = np.random.default_rng(100 + rank)
    w = [(1 << 63) - 1 - rank, -(1 << 63) + rank, -1 - rank, 3 * rank]
    w += [int(x) for x in rng.integers(-(1 << 62), 1 << 62, max(n - 4, 0))]
    return w[:n]


def _i64(v):
    v &= MASK
    return v - (1 << 64) if v >= (1 << 63) else v


def _expected(world, n=19):
    tot = [0] * n
    for r in range(world):
        for i, v in enumerate(_words(r, n)):
            tot[i] += v
    return [_i64(v) for v in tot]


@pytest.fixture(scope="module")
def lib():
    return load_pkg().load_library()


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_sum_thread_comm(lib, world):
    from cuda_go_icp_amd import binding as B, sharded
    comms = sharded.thread_comms(world)
    out, rcs = [None] * world, [None] * world

    def worker(r):
        a = (C.c_int64 * 19)(*_words(r))
        rcs[r] = lib.goicp_comm_allreduce_sum_i64(C.byref(comms[r]), a, 19)
        out[r] = list(a)

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r in range(world):
        lib.goicp_thread_comm_destroy(comms[r])
    assert rcs == [B.OK] * world
    want = _expected(world)
    assert all(o == want for o in out)
    if world > 1:
        assert want != _words(0)


def test_sum_thread_comm_repeated_and_interleaved_with_min(lib):
    """sums and MIN all-reduces alternate on the same communicator (the collective ICP's check word, then its sums)"""
    from cuda_go_icp_amd import sharded
    world = 3
    comms = sharded.thread_comms(world)
    res = [[] for _ in range(world)]

    def worker(r):
        for k in range(20):
            m = (C.c_uint64 * 2)(10 + r + k, MASK - r)
            assert lib.goicp_comm_set_timeout_ms(C.byref(comms[r]), 20000) == 0
            assert comms[r].allreduce_min_u64(comms[r].ctx, m, 2) == 0
            a = (C.c_int64 * 3)(r + k, -r, (1 << 63) - 1)
            assert lib.goicp_comm_allreduce_sum_i64(C.byref(comms[r]), a, 3) == 0
            res[r].append((list(m), list(a)))

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r in range(world):
        lib.goicp_thread_comm_destroy(comms[r])
    for k in range(20):
        assert all(res[r][k] == res[0][k] for r in range(world))
        m, a = res[0][k]
        assert m == [10 + k, MASK - 2]
        assert a == [3 * k + 3, -3, _i64(3 * ((1 << 63) - 1))]


def test_sum_missing_rank_is_a_timeout(lib):
    """one of two ranks never joins: the other returns GOICP_ERR_TIMEOUT at the communicator's deadline, no hang"""
    from cuda_go_icp_amd import sharded
    comms = sharded.thread_comms(2)
    assert lib.goicp_comm_set_timeout_ms(C.byref(comms[0]), 300) == 0
    a = (C.c_int64 * 4)(1, 2, 3, 4)
    t0 = time.time()
    rc = lib.goicp_comm_allreduce_sum_i64(C.byref(comms[0]), a, 4)
    assert rc == -7 and 0.25 <= time.time() - t0 < 30
    for r in range(2):
        lib.goicp_thread_comm_destroy(comms[r])


def test_sum_rejects_a_null_table(lib):
    a = (C.c_int64 * 1)(1)
    assert lib.goicp_comm_allreduce_sum_i64(None, a, 1) == -1
    from cuda_go_icp_amd import binding as B
    assert lib.goicp_comm_allreduce_sum_i64(C.byref(B.CCommOps()), a, 1) == -1     # no functions in the table
    assert lib.goicp_abi_version() == 4


def test_collective_icp_needs_real_engines(lib):
    from cuda_go_icp_amd import binding as B, sharded
    with pytest.raises(TypeError):
        sharded.run_sharded_library(B.CShardEngineOps(), B.CCommOps(), collective_icp=True)


WORKER_SUM = r"""
import json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import ctypes as C, datetime
import torch, torch.distributed as dist
from conftest import load_pkg
lib = load_pkg().load_library()
from cuda_go_icp_amd import sharded
from test_icp_shard_comm import _words
dist.init_process_group(backend="gloo", timeout=datetime.timedelta(seconds=120))
comm = sharded.torch_comm_ops(dist, torch.device("cpu"))
r = dist.get_rank()
res = []
for n in (19, 1, 0):
    a = (C.c_int64 * max(n, 1))(*_words(r, max(n, 1)))
    rc = lib.goicp_comm_allreduce_sum_i64(C.byref(comm), a, n)
    res.append([rc, list(a)[:n]])
json.dump(res, open(os.path.join({out!r}, "sum_rank%d.json" % r), "w"))
dist.barrier()
dist.destroy_process_group()
"""


def test_sum_gloo_world2_broadcast_fallback(lib, tmp_path):
    """two processes over gloo: torch_comm_ops is a caller's table, so the sum is `world` broadcasts added up on every rank"""
    script = tmp_path / "worker_sum.py"
    script.write_text(WORKER_SUM.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29561", str(script)]
    r = subprocess.run(cmd, env=env, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = [json.load(open(tmp_path / ("sum_rank%d.json" % k))) for k in range(2)]
    assert res[0] == res[1]
    assert res[0][0] == [0, _expected(2, 19)]
    assert res[0][1] == [0, _expected(2, 1)]
    assert res[0][2] == [0, []]
