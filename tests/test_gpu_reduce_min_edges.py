"""goicp_reduce_min_device at the seams of reduce_min_kernel: one workgroup of 1 024 threads, a thread reads quads (float4) 4 096 values
apart in sweeps of eight quads (32 768 values), then of two (8 192), then quad by quad, and the ragged end value by value; wavefronts
own 256 consecutive values of a quad row.  Against numpy's (min, first argmin) with NaNs never taken (they compare as +inf here, so an
input without a value below +inf gives (inf, 0)), with and without d_argmin.
"""
import numpy as np
import pytest

import test_gpu_bounds_order_pairs as P
from test_gpu_bounds_order_pairs import pkg, hip  # noqa: F401  (fixtures)


pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 65536, 65539)
LO = np.float32(0.25)


@pytest.fixture(scope="module")
def reg(pkg):
    t, s = P._clouds(257)
    r = pkg.Registration(t, s, 1e-3, dt_size=64)
    yield r
    r.close()


def _reduce(reg, hip, v, with_idx=True):
    d_v = hip.upload(np.ascontiguousarray(v, np.float32))
    d_min, d_idx = hip.upload(np.full(1, np.nan, np.float32)), hip.upload(np.full(1, -7, np.int32))
    rc = reg._lib.goicp_reduce_min_device(reg.handle, d_v, len(v), d_min, d_idx if with_idx else None, None)
    assert rc == 0, reg._lib.goicp_last_error()
    out = hip.download(d_min, 1, np.float32)[0], int(hip.download(d_idx, 1, np.int32)[0])
    hip.free_all()
    return out


def _want(v):
    w = np.where(np.isnan(v), np.float32(np.inf), v)
    return w.min(), int(np.argmin(w))


def _check(reg, hip, v, what):
    m, i = _want(v)
    gm, gi = _reduce(reg, hip, v)
    assert gm == m and gi == i, (what, len(v), float(gm), gi, float(m), i)
    gm, gi = _reduce(reg, hip, v, with_idx=False)
    assert gm == m and gi == -7, (what, len(v), "no d_argmin", float(gm), gi, float(m))


def _seams(n):
    """first indices of a quad, a wavefront's slice, a thread row, a two-quad sweep, an eight-quad sweep, the ragged end"""
    return sorted({p for p in (4, 256, 4092, 4096, 8192, 12288, 32768, 40960, 65536, n // 4 * 4) if 0 < p < n})


@pytest.mark.parametrize("n", SIZES)
def test_single_minimum_everywhere_it_can_hide(pkg, reg, hip, n):
    """the minimum alone at the first and last element and on both sides of every seam"""
    rng = np.random.default_rng(3000 + n)
    base = rng.uniform(1.0, 2.0, n).astype(np.float32)
    for p in sorted({0, n - 1} | {q for s in _seams(n) for q in (s - 1, s)}):
        v = base.copy()
        v[p] = LO
        _check(reg, hip, v, "minimum at %d" % p)


@pytest.mark.parametrize("n", SIZES)
def test_ties(pkg, reg, hip, n):
    """equal minima: the first and the last element, the two sides of every seam (the later one belongs to an earlier thread at a thread row's
    seam), and every element equal"""
    rng = np.random.default_rng(3100 + n)
    base = rng.uniform(1.0, 2.0, n).astype(np.float32)
    pairs = [(0, n - 1)] + [(s - 1, s) for s in _seams(n)] + [(s, n - 1) for s in _seams(n)]
    for a, b in pairs:
        v = base.copy()
        v[[a, b]] = LO
        _check(reg, hip, v, "tie at %d and %d" % (a, b))
    _check(reg, hip, np.full(n, LO, np.float32), "all equal")
    v = base.copy()
    v[n // 2:] = LO                                               # the first copy sits mid-way, copies in every later thread and sweep
    _check(reg, hip, v, "upper half equal")


@pytest.mark.parametrize("n", SIZES)
def test_inf_and_nan(pkg, reg, hip, n):
    rng = np.random.default_rng(3200 + n)
    base = rng.uniform(1.0, 2.0, n).astype(np.float32)
    _check(reg, hip, np.full(n, np.inf, np.float32), "all +inf")
    assert _reduce(reg, hip, np.full(n, np.inf, np.float32)) == (np.inf, 0)
    one = np.full(n, np.inf, np.float32)
    one[(2 * n) // 3] = LO
    _check(reg, hip, one, "+inf but one")
    scattered = base.copy()
    scattered[rng.random(n) < 0.3] = np.nan
    _check(reg, hip, scattered, "NaNs scattered")
    v = scattered.copy()
    v[0] = np.nan
    _check(reg, hip, v, "NaN at index 0")
    v[[min(1, n - 1), n - 1]] = LO                                # the minimum right behind the NaN, and tied at the end
    _check(reg, hip, v, "NaN at index 0, minimum behind it")
    v = base.copy()
    v[[0, n // 2]] = -np.nan, LO
    _check(reg, hip, v, "negative NaN at index 0")
    for s in _seams(n):
        v = base.copy()
        v[s - 1], v[s] = np.nan, LO
        if s + 1 < n:
            v[s + 1] = LO
        _check(reg, hip, v, "NaN before the minimum at seam %d" % s)
