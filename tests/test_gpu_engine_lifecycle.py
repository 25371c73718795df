"""The engine's device memory, streams and events over a handle's life: buffers that grow on demand keep their results, every opt-in
family of buffers can be created and destroyed again and again with the same answers, a refused goicp_create leaves nothing behind,
and the device's free memory comes back after close().  Public Python API only.

Clouds: synth.make_pair, M = 300 target and N = 257 source points, dt_size 16 -- a registration takes milliseconds."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu
INVALID = -1
DT = 16
MSE = 1e-3
# test_memory_comes_back: twice the largest repetition-to-repetition change of the reading measured at the parent commit, which was 0
# (docstring there)
SLACK_BYTES = 0


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@functools.lru_cache(maxsize=None)
def clouds(N=257):
    from cuda_go_icp_amd import synth
    T, S = synth.make_pair(seed=11, M=300, N=N)[:2]
    T.setflags(write=False)
    S.setflags(write=False)
    return T, S


def _b(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _rots(pkg, K):
    rng = np.random.default_rng(3)
    return np.stack([pkg.fgoicp.rodrigues(v) for v in rng.uniform(-1.5, 1.5, (K, 3))]).astype(np.float32).reshape(K, 9)


def _cubes(B, K):
    rng = np.random.default_rng(4)
    c = np.zeros((B, 6), np.float32)
    c[:, :3] = rng.uniform(-0.3, 0.3, (B, 3))
    c[:, 3], c[:, 4] = 0.125, rng.uniform(0.0, 0.5, B)
    c[:, 5] = np.arange(B) % K
    return c


def _starts(pkg, K):
    t = np.random.default_rng(5).uniform(-0.05, 0.05, (K, 3)).astype(np.float32)
    return _rots(pkg, K), t


def _pose(fg):
    sse, R, t = fg.pose()
    return _b(np.float32(sse), R, t)


def _fresh(pkg, fn, S=None, **params):
    T, S0 = clouds()
    reg = pkg.Registration(T, S0 if S is None else S, MSE, dt_size=DT, **params)
    try:
        return fn(reg)
    finally:
        reg.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. growth keeps results
# ---------------------------------------------------------------------------------------------------------------------------------
def test_growth_keeps_results(pkg):
    T, S = clouds()
    bounds_small = lambda r: _b(*r.eval_bounds_batch(_rots(pkg, 1), _cubes(8, 1)))
    bounds_large = lambda r: _b(*r.eval_bounds_batch(_rots(pkg, 65), _cubes(4104, 65)))       # past ensure_batch(4096, 64) of creation
    q = np.random.default_rng(6).uniform(-0.6, 0.6, (10000, 3)).astype(np.float32)
    nn_small = lambda r: _b(*r.nn_query(q[:16]))
    nn_large = lambda r: _b(*r.nn_query(q))                                                    # past the 64 KiB scratch floor
    icp = lambda K: (lambda r: r.icp_run_batch(*_starts(pkg, K), max_iter=30))
    info = lambda K: (lambda r: [_b(*(np.float64(v) for v in d.values())) for d in r.pose_information_batch(*_starts(pkg, K))])
    reg = pkg.Registration(T, S, MSE, dt_size=DT)
    try:
        grown = [fn(reg) for fn in (bounds_small, bounds_large, bounds_small, nn_small, nn_large)]
        icp3, icp40 = icp(3)(reg), icp(40)(reg)                                                # past the batch capacity of 16
        info2, info9 = info(2)(reg), info(9)(reg)
    finally:
        reg.close()
    for got, fn in zip(grown, (bounds_small, bounds_large, bounds_small, nn_small, nn_large)):
        assert got == _fresh(pkg, fn)
    assert grown[0] == grown[2]
    assert _b(*icp3) == _b(*_fresh(pkg, icp(3))) and _b(*icp40) == _b(*_fresh(pkg, icp(40)))
    assert all(_b(a[0]) == _b(b[0]) for a, b in zip(icp3, icp40))                              # pose 0 of both calls: the same start
    assert info2 == _fresh(pkg, info(2)) and info9 == _fresh(pkg, info(9))


def _after_swap(pkg, fg):
    out = _b(*fg.registration.icp_run_batch(*_starts(pkg, 3), max_iter=30))
    fg.run()
    return out + _pose(fg)


def test_set_source_growth_keeps_results(pkg):
    T, S = clouds()
    big = clouds(4001)[1]
    fg = pkg.FastGoICP(T, S, MSE, dt_size=DT)
    try:
        got = [_after_swap(pkg, fg)]
        for s in (big, S):
            fg.set_source(s)
            got.append(_after_swap(pkg, fg))
    finally:
        fg.registration.close()
    want = {}
    for s in (S, big):
        f = pkg.FastGoICP(T, s, MSE, dt_size=DT)
        try:
            want[len(s)] = _after_swap(pkg, f)
        finally:
            f.registration.close()
    assert got == [want[257], want[4001], want[257]]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. every opt-in family, then destroy
# ---------------------------------------------------------------------------------------------------------------------------------
def family_body(pkg):
    """every lazily created family of buffers once, on four handles, all closed; -> the answers as bytes"""
    T, S = clouds()
    out = []

    def icp(reg):
        return _b(*pkg.IterativeClosestPoint3D(reg, 30, 1e-7).run())

    fg = pkg.FastGoICP(T, S, MSE, dt_size=DT, device_queues=1, lanes=2, lane_min_searches=2)
    try:
        reg = fg.registration
        reg.set_icp_options(metric=1, normal_k=8)
        out.append(icp(reg))
        reg.set_icp_gate(0.2)
        out.append(icp(reg))
        reg.set_icp_gate(0.0)
        reg.set_icp_robust(1, 0.05)
        out.append(icp(reg))
        reg.set_icp_robust(0, 0.0)
        reg.set_icp_options(metric=0)
        fg.run()
        out.append(_pose(fg))
    finally:
        fg.registration.close()
    for params in ({"trim_fraction": 0.1}, {"icp_nn_cache": 1}, {"bounds_fp16": 1}):
        fg = pkg.FastGoICP(T, S, MSE, dt_size=DT, **params)
        try:
            fg.run()
            out.append(_pose(fg))
        finally:
            fg.registration.close()
    return out


def test_every_family_then_destroy(pkg):
    first = family_body(pkg)
    assert len(first) == 7 and family_body(pkg) == first


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a refused create leaves nothing behind
# ---------------------------------------------------------------------------------------------------------------------------------
def _plain_run(pkg):
    T, S = clouds()
    fg = pkg.FastGoICP(T, S, MSE, dt_size=DT)
    try:
        fg.run()
        return _pose(fg)
    finally:
        fg.registration.close()


def test_refused_create_leaves_nothing(pkg):
    T, S = clouds()
    refusals = ({"trim_fraction": 1.0},                                                        # refused after the streams and events exist
                {"use_rot_range": 1, "rot_min": (10, 10, 10), "rot_max": (-10, -10, -10)})       # ... and a little later
    for i in range(50):
        with pytest.raises(pkg.GoicpError) as e:
            pkg.Registration(T, S, MSE, dt_size=DT, **refusals[i % 2])
        assert e.value.code == INVALID
    got = _plain_run(pkg)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert got.hex() == r.stdout.strip().splitlines()[-1]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. memory comes back
# ---------------------------------------------------------------------------------------------------------------------------------
def memory_series(pkg):
    """free device memory after the last close() of each of 8 repetitions of family_body, after one untimed repetition that loads the
    code objects and fills the runtime's pools"""
    import torch
    family_body(pkg)
    free = []
    for _ in range(8):
        family_body(pkg)
        free.append(torch.cuda.mem_get_info()[0])
    return free


def test_memory_comes_back():
    """Free device memory (torch.cuda.mem_get_info) after each of 8 repetitions of test 2's body: repetition 8 may not read lower
    than repetition 1 by more than SLACK_BYTES.  The readings are taken in a fresh process that initialises torch's device
    context BEFORE the library is loaded (the order bench.py uses): torch ships a HIP runtime of its own, and the second runtime
    to initialise in a process finds no device.

    A coarse guard: the reading is the whole device's, it moves by the runtime's allocation granules, and a leak smaller than a
    granule per handle does not show in 8 repetitions.  The precise checks are the construction (every resource of the engine is
    a member that releases itself) and the owner type's own test in csrc/host_selftest.cpp.

    Measured series, bytes relative to repetition 1:
      parent commit:  0, 0, 0, 0, 0, 0, 0, 0   (largest repetition-to-repetition change: 0)
      this commit:    0, 0, 0, 0, 0, 0, 0, 0
    SLACK_BYTES = 2 x the parent's largest repetition-to-repetition change."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "memory"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    free = [int(x) for x in r.stdout.strip().splitlines()[-1].split()]
    assert len(free) == 8
    print("free-memory series, bytes relative to repetition 1:", [f - free[0] for f in free])
    print("largest repetition-to-repetition change:", max(abs(b - a) for a, b in zip(free, free[1:])))
    assert free[-1] >= free[0] - SLACK_BYTES, (free, SLACK_BYTES)


if __name__ == "__main__":      # the fresh processes of test_refused_create_leaves_nothing and test_memory_comes_back
    if sys.argv[1:] == ["memory"]:
        import torch
        torch.cuda.init()
    p = load_pkg()
    p.load_library()
    print(" ".join(map(str, memory_series(p))) if sys.argv[1:] == ["memory"] else _plain_run(p).hex())
