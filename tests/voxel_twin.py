"""The numpy twin of the voxel-grid operator (include/goicp_mi355.h), the clouds and the grid of cases that
tests/test_voxel_downsample_host.py and tests/test_gpu_voxel_downsample.py share.  The twin shares nothing with the library but the rule:
  frame   mn = per-axis minimum, d = x - mn (float32), E = max d;
  cell    c = int(floor(d / v)) in float32, key = cx | cy << 21 | cz << 42;
  sums    terms rint(ldexp(float64(d), s)) as int64, s = 62 - frexp(E).exponent - n.bit_length() (0 when E == 0), reduced per cell with
          np.add.reduceat over the stable argsort of the keys;
  output  cells in ascending key order; a cell of one point is that point, any other float32(float64(mn) + ldexp(S / count, -s))."""
import numpy as np

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 20000]
KINDS = ["uniform", "offset", "planar", "identical", "duplicates", "zeros", "lattice", "denormal"]


def make_cloud(kind, n, seed=0):
    rng = np.random.default_rng(7919 * seed + 31 * n + KINDS.index(kind))
    if kind == "uniform":
        p = rng.uniform(-1, 1, (n, 3))
    elif kind == "offset":
        p = np.float32(rng.uniform(-1, 1, (n, 3))) * np.float32(0.01) + np.float32(1000)
    elif kind == "planar":
        p = rng.uniform(-1, 1, (n, 3))
        p[:, 2] = 0.375                                  # one zero extent
    elif kind == "identical":
        p = np.tile(np.array([[0.3, -1.7, 2.5]]), (n, 1))    # E == 0
    elif kind == "duplicates":
        base = rng.uniform(-1, 1, (max(1, n // 7), 3))
        p = base[rng.integers(0, len(base), n)]
    elif kind == "zeros":
        vals = np.array([-0.0, 0.0, -0.0, 0.0, -0.25, 0.25, -1e-30, 1e-30])
        p = vals[rng.integers(0, len(vals), (n, 3))]
    elif kind == "lattice":
        p = rng.integers(-8, 9, (n, 3)) * 0.25           # with v = 0.25 every point sits on a cell face
    elif kind == "denormal":
        # every coordinate, every offset d and the extent (below 1.5e-39) are float32 denormals: a path that flushed them to zero would put
        # all points into one cell
        p = np.ldexp(rng.integers(-2000, 2001, (n, 3)).astype(np.float64), -140)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, np.float32)


def voxels_for(kind, xyz):
    """from "every point alone" (for clouds of distinct points) to "one cell"; the lattice adds its own pitch"""
    ext = float(np.max(xyz.max(0) - xyz.min(0)))
    if ext == 0.0:
        return [0.5, 1e-3, 1e30]
    if kind == "denormal":
        return [2.0 ** -140, ext / 37.0, ext / 3.0, ext * 4.0]     # the lattice's own pitch: ext * 2^-20 is not a float32
    v = [ext * 2.0 ** -20, ext / 37.0, ext / 3.0, ext * 4.0]
    if kind == "lattice":
        v.append(0.25)
    return v


def frame(xyz, voxel):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    v = np.float32(voxel)
    mn = xyz.min(0)
    d = xyz - mn
    assert d.dtype == np.float32
    E = np.float32(d.max())
    with np.errstate(over="ignore"):
        assert E / v < np.float32(2097152.0), "21-bit rule"
    s = 0
    if E > 0:
        s = 62 - int(np.frexp(E)[1]) - int(len(xyz)).bit_length()
    return xyz, v, mn, d, E, s


def keys_of(d, v):
    c = np.floor(d / v).astype(np.int64)
    assert c.min() >= 0 and c.max() < 2 ** 21
    c = c.astype(np.uint64)
    return c[:, 0] | (c[:, 1] << np.uint64(21)) | (c[:, 2] << np.uint64(42))


def twin(xyz, voxel):
    """-> (cloud (m, 3) float32, counts (m,) int32, keys (m,) uint64, the cell of every input point (n,))"""
    xyz, v, mn, d, E, s = frame(xyz, voxel)
    key = keys_of(d, v)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    counts = np.diff(np.concatenate([head, [len(ks)]]))
    T = np.rint(np.ldexp(d.astype(np.float64), s)).astype(np.int64)
    S = np.add.reduceat(T[order], head, axis=0)
    assert S.max() < 2 ** 62
    out = (mn.astype(np.float64) + np.ldexp(S.astype(np.float64) / counts[:, None].astype(np.float64), -s)).astype(np.float32)
    single = counts == 1
    out[single] = xyz[order[head[single]]]
    cell = np.empty(len(xyz), np.int64)
    cell[order] = np.cumsum(np.concatenate([[0], (ks[1:] != ks[:-1]).astype(np.int64)]))
    return out, counts.astype(np.int32), ks[head], cell


def bound(xyz, denormal=False):
    """|c - c64| <= 2^-23 (E + max|x|): d rounds once (2^-24 E), the fixed-point quantum is below 2^-32 E, the final cast rounds once.
    The derivation takes every rounding as relative.  In the "denormal" cloud each of the two roundings is absolute instead, at most half
    the float32 subnormal spacing 2^-149 each, so that kind alone adds 2^-149."""
    xyz = np.asarray(xyz, np.float32)
    return 2.0 ** -23 * (float(np.max(xyz - xyz.min(0))) + float(np.abs(xyz).max())) + (2.0 ** -149 if denormal else 0.0)


def centroids64(xyz, cell, m):
    xyz = np.asarray(xyz, np.float64)
    out = np.zeros((m, 3))
    np.add.at(out, cell, xyz)
    return out / np.bincount(cell, minlength=m)[:, None]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
