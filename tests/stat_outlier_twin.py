"""The numpy twin of the statistical outlier removal operator (include/goicp_mi355.h), the clouds and the grid of cases that
tests/test_stat_outlier_host.py and tests/test_gpu_stat_outlier.py share.  The twin is brute force over all pairs, in row chunks, and
shares nothing with the library but the rule:
  pair     dx = x_i - x_j, dy, dz likewise; d2 = dx*dx + dy*dy + dz*dz in float32, left to right; a point is never its own neighbour;
  nearest  the k smallest d2 of a row, ascending; s_i = the float64 sum of float64(sqrt_float32(d2)) in that order; u_i = float32(s_i / k);
  image    U = max u; e = frexp(U).exponent; q_i = floor(ldexp(float64(u_i), 31 - e)) as integers; S1 = sum q, A = sum (q*q >> 32),
           B = sum (q*q & 0xffffffff) as Python integers;
  finish   Python floats (IEEE double, one rounding per operation): mean = S1 / n, S2 = ldexp(A, 32) + B,
           var = (S2 - S1 * mean) / (n - 1), 0 unless > 0, Tq = mean + alpha * sqrt(var);
  keep     q_i <= Tq; U == 0 keeps everything with threshold 0; the reported threshold is ldexp(Tq, e - 31).
It knows no grid."""
import functools
import math

import numpy as np

import outlier_twin as OT

SIZES = [2, 63, 64, 65, 255, 256, 257, 1000, 4097]
KINDS = OT.KINDS
ALPHAS = [0.0, 1.0, 2.5]
MAX_K = 64
TEXTBOOK_KINDS = ["uniform", "offset", "planar", "lattice", "shell", "edge"]

make_cloud = OT.make_cloud
same_bits = OT.same_bits


def ks_for(n):
    return sorted({k for k in (1, 5, 20, 64, n - 1) if 1 <= k <= min(MAX_K, n - 1)})


def nearest_d2(xyz, kmax, chunk=256):
    """the kmax smallest d2 of every point, ascending (n, kmax) float32: all pairs, the header's expression"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    assert 1 <= kmax <= n - 1
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty((n, kmax), np.float32)
    with np.errstate(under="ignore"):
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            dx, dy, dz = x[a:b, None] - x[None, :], y[a:b, None] - y[None, :], z[a:b, None] - z[None, :]
            d2 = dx * dx + dy * dy + dz * dz
            assert d2.dtype == np.float32
            d2[np.arange(b - a), np.arange(a, b)] = np.inf
            out[a:b] = np.sort(np.partition(d2, kmax - 1, axis=1)[:, :kmax], axis=1)
    assert np.all(np.isfinite(out))
    return out


@functools.lru_cache(maxsize=None)
def nearest_of(kind, n):
    """computed once per cloud of the grid, shared, never changed"""
    d = nearest_d2(make_cloud(kind, n), min(MAX_K, n - 1))
    d.setflags(write=False)
    return d


def mean_dist(nearest, k):
    """u of every point from its sorted nearest d2: cumsum adds in order, in float64"""
    root = np.sqrt(nearest[:, :k])
    assert root.dtype == np.float32
    s = np.cumsum(root.astype(np.float64), axis=1)[:, k - 1]
    return (s / np.float64(k)).astype(np.float32)


def decide(u, alpha):
    """-> (keep mask, threshold)"""
    n = len(u)
    U = np.float32(u.max())
    if U == 0:
        return np.ones(n, bool), 0.0
    e = int(np.frexp(U)[1])
    q = np.floor(np.ldexp(u.astype(np.float64), 31 - e)).astype(np.int64)
    assert q.min() >= 0 and q.max() < 2 ** 31
    qq = q * q
    S1, A, B = int(q.sum()), int((qq >> 32).sum()), int((qq & 0xFFFFFFFF).sum())
    assert max(S1, A, B) < 2 ** 60
    nd = float(n)
    mean = float(S1) / nd
    S2 = math.ldexp(float(A), 32) + float(B)
    prod = float(S1) * mean
    var = (S2 - prod) / (nd - 1.0)
    if not var > 0.0:
        var = 0.0
    dev = float(np.float32(alpha)) * math.sqrt(var)
    Tq = mean + dev
    return q.astype(np.float64) <= Tq, math.ldexp(Tq, e - 31)


def twin(xyz, k, alpha, nearest=None):
    """-> (cloud (m, 3) float32, indices (m,) int32, u (n,) float32, threshold); nearest: nearest_d2(xyz, >= k) computed before"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if nearest is None:
        nearest = nearest_d2(xyz, k)
    u = mean_dist(nearest, k)
    keep, thr = decide(u, alpha)
    idx = np.flatnonzero(keep).astype(np.int32)
    return xyz[idx], idx, u, thr


def textbook_nearest(xyz, kmax, chunk=256):
    """the kmax smallest float64 distances of every point, ascending (n, kmax)"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(p)
    out = np.empty((n, kmax))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        d2 = ((p[a:b, None, :] - p[None, :, :]) ** 2).sum(2)
        d2[np.arange(b - a), np.arange(a, b)] = np.inf
        out[a:b] = np.sqrt(np.sort(np.partition(d2, kmax - 1, axis=1)[:, :kmax], axis=1))
    return out


def textbook(nearest, k, alpha):
    """the textbook form in float64: m_i = the mean of the k smallest distances, T = mean(m) + alpha * std(m, ddof=1) -> (m, T)"""
    m = nearest[:, :k].mean(1)
    return m, float(m.mean() + alpha * m.std(ddof=1))
