"""The numpy twin of the radius outlier removal operator (include/goicp_mi355.h), the clouds and the grid of cases that
tests/test_outlier_removal_host.py and tests/test_gpu_outlier_removal.py share.  The twin is brute force over all pairs, in row chunks and
in float32, and shares nothing with the library but the rule:
  r2      = r * r;
  pair    dx = x_i - x_j, dy, dz likewise; d2 = dx*dx + dy*dy + dz*dz, left to right; j is a neighbour of i iff j != i and d2 <= r2;
  count   count_i = min(number of neighbours, min_neighbors); point i is kept iff count_i == min_neighbors;
  output  the kept points in input order, their indices, and count_i of all points.
It knows no grid.  valid() is the header's list of refusals that depend on the cloud and the radius."""
import numpy as np

import voxel_twin as VT

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097]
KINDS = VT.KINDS + ["shell", "edge"]
SHELL_R = np.float32(0.5)


def make_cloud(kind, n, seed=0):
    if kind in VT.KINDS:
        return VT.make_cloud(kind, n, seed)
    rng = np.random.default_rng(104729 * seed + 17 * n + KINDS.index(kind))
    if kind == "shell":
        # a tight cluster at the origin (half of it exactly there) and points at distance r-, r and r+ from the origin along the axes, r = SHELL_R:
        # for the points at the origin d2 == r2 exactly (kept), and the next float above r gives d2 > r2 (dropped)
        r = SHELL_R
        nc = n - n // 2
        c = rng.integers(-3, 4, (nc, 3)).astype(np.float32) * np.float32(2.0 ** -30)
        c[::2] = 0.0
        dist = np.array([np.nextafter(r, np.float32(0)), r, np.nextafter(r, np.float32(1))], np.float32)[rng.integers(0, 3, n // 2)]
        s = np.zeros((n // 2, 3), np.float32)
        s[np.arange(n // 2), rng.integers(0, 3, n // 2)] = dist * np.float32(1) * rng.choice(np.array([-1, 1], np.float32), n // 2)
        p = np.concatenate([c, s])[rng.permutation(n)]
    elif kind == "edge":
        # the unit cube with both faces of every axis occupied (E == 1), pairs half a smallest radius apart, two of them in cell 0 and in the
        # highest cell of every axis
        p = np.float32(rng.uniform(0, 1, (n, 3)))
        if n >= 2:
            p[0], p[1] = 0.0, 1.0
        h = np.float32(2.0 ** -17)
        for a in range(6, n - 1, 4):                     # every other pair of points is such a pair, the rest stay alone
            p[a + 1] = p[a] + h * rng.integers(-1, 2, 3).astype(np.float32)
        if n >= 6:
            p[2] = 1.0
            p[3] = np.float32(1.0) - h
            p[4] = 0.0
            p[5] = (h, 0, 0)
        p = np.clip(p, 0, 1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, np.float32)


def extent(xyz):
    xyz = np.asarray(xyz, np.float32)
    return np.float32((xyz - xyz.min(0)).max())


def valid(xyz, r):
    """what the header refuses of a finite cloud and a radius: r <= 0, NaN, infinite; r * r no normal float; E / r >= 2^16"""
    r = np.float32(r)
    if not (np.isfinite(r) and r > 0):
        return False
    with np.errstate(over="ignore", under="ignore"):
        r2 = r * r
        if not (np.isfinite(r2) and r2 >= np.finfo(np.float32).tiny):
            return False
        return bool(extent(xyz) / r < np.float32(65536.0))


def smallest_radius(xyz):
    """the smallest float32 r with E / r < 2^16 (E > 0)"""
    E = extent(xyz)
    r = np.float32(E / np.float32(65536.0))
    while not E / r < np.float32(65536.0):
        r = np.nextafter(r, np.float32(np.inf))
    return r


def radii_for(kind, xyz):
    """from "every point alone" (for clouds of distinct, spread points) to "everybody is everybody's neighbour"; radii the header refuses for
    the cloud are part of the list (the tests expect the refusal)"""
    ext = float(extent(xyz))
    if ext == 0.0:
        return [0.5, 1e-3, 1e18]
    r = [ext * 2.0 ** -15, ext / 37.0, ext / 3.0, ext * 4.0]
    if not any(valid(xyz, x) for x in r):
        r.append(2.0 ** -60)                             # a cloud so small that the radii above square to less than a normal float (the
                                                         # "denormal" kind, some "zeros"): they are refused, this one is taken
    if kind == "lattice":
        r += [0.25, float(np.nextafter(np.float32(0.25), np.float32(0)))]      # neighbours at exactly r, and just outside
    if kind == "shell":
        r.append(float(SHELL_R))
    if kind == "edge":
        r.append(float(smallest_radius(xyz)))
    return [float(np.float32(x)) for x in r]


def ks_for(n):
    return sorted({k for k in (1, 2, 5, n - 1, n) if k >= 1})


def neighbour_counts(xyz, r, chunk=256):
    """the unsaturated number of neighbours of every point: all pairs, float32, the header's expression"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    r = np.float32(r)
    r2 = r * r
    n = len(xyz)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.zeros(n, np.int64)
    with np.errstate(under="ignore"):
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            dx, dy, dz = x[a:b, None] - x[None, :], y[a:b, None] - y[None, :], z[a:b, None] - z[None, :]
            d2 = dx * dx + dy * dy + dz * dz
            assert d2.dtype == np.float32
            near = d2 <= r2
            near[np.arange(b - a), np.arange(a, b)] = False
            out[a:b] = near.sum(1)
    return out


def twin(xyz, r, k, counts=None):
    """-> (cloud (m, 3) float32, indices (m,) int32, count (n,) int32); counts: neighbour_counts(xyz, r) computed before"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if counts is None:
        counts = neighbour_counts(xyz, r)
    c = np.minimum(counts, k).astype(np.int32)
    idx = np.flatnonzero(c == k).astype(np.int32)
    return xyz[idx], idx, c


same_bits = VT.same_bits
