"""The numpy twin of goicp_cluster / goicp_cluster_filter (include/goicp_mi355.h) and the clouds both cluster test files share.

The twin knows no grid: all pairs in float32, the header's pair expression evaluated left to right, the saturating neighbour count for the
core flag, a min-label iterated over the core adjacency to a fixed point (with label jumping, lab <- lab[lab], between the sweeps: a label
is always the index of a core point of the same component, so jumping only speeds the iteration up), the border points by the smallest key
(bits of d2) << 32 | index over their core neighbours, labels in ascending order of the smallest core index.  Everything is cached per
case and never changed."""
import functools

import numpy as np

NOISE = -1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def pair_d2(xyz):
    """(n, n) float32: dx*dx + dy*dy + dz*dz left to right, every operation rounded to float32 once"""
    x = np.ascontiguousarray(xyz, np.float32)
    dx, dy, dz = (x[:, None, k] - x[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def twin(xyz, radius, min_neighbors):
    """-> (labels (n,) int32, sizes (c,) int32)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = len(xyz)
    r2 = np.float32(radius) * np.float32(radius)
    d2 = pair_d2(xyz)
    adj = d2 <= r2
    adj[np.arange(n), np.arange(n)] = False
    core = np.minimum(adj.sum(1), min_neighbors) == min_neighbors
    lab = np.where(core, np.arange(n), n).astype(np.int64)
    ei, ej = np.nonzero(adj & core[:, None] & core[None, :])
    while True:
        new = lab.copy()
        np.minimum.at(new, ei, lab[ej])
        while True:                                            # label jumping
            jumped = np.where(core, new[np.minimum(new, n - 1)], n)
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            break
        lab = new
    root = np.where(core, lab, -1)
    keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    keys = np.where(adj & core[None, :], keys, np.uint64(2 ** 64 - 1))
    for i in np.nonzero(~core)[0]:
        best = keys[i].min()
        if best != np.uint64(2 ** 64 - 1):
            root[i] = lab[int(best & np.uint64(0xffffffff))]
    roots = np.unique(root[core])
    labels = np.where(root < 0, NOISE, np.searchsorted(roots, np.maximum(root, 0))).astype(np.int32)
    sizes = np.bincount(labels[labels >= 0], minlength=len(roots)).astype(np.int32)
    return labels, sizes


def select(xyz, labels, sizes, min_size, keep):
    """the filter on top of twin(): -> (cloud (m, 3), indices (m,), labels (m,))"""
    order = sorted(range(len(sizes)), key=lambda l: (-int(sizes[l]), l))
    order = [l for l in order if sizes[l] >= max(min_size, 1)]
    if keep:
        order = order[:keep]
    idx = np.nonzero(np.isin(labels, np.array(order, np.int32)))[0].astype(np.int32)
    return np.ascontiguousarray(xyz[idx]), idx, labels[idx]


# ----------------------------------------------------------------------------------------------
# the clouds: name -> (xyz float32, radius, tuple of min_neighbors)
# ----------------------------------------------------------------------------------------------
def _f32(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


def bridge(px):
    """Two blobs of 9 core points (min_neighbors 4, r = 0.5) whose tips a = (0, 0, 0) and b = (1, 0, 0) are 1 apart, and the point
    P = (px, 0, 0), which has at most the two tips within r and so is no core point.  Order: B's others, b (index 8), A's others, a
    (index 17), P (index 18).  At px = 0.5 both d2 are exactly 0.25 = r2: the key's index decides, b.  One ulp below, b is still at
    d2 = 0.25 (0.5 + 2^-25 rounds to 0.5) and a is closer: a.  One ulp above, a is beyond r: b."""
    rng = np.random.default_rng(3)
    oth = rng.uniform(-0.04, 0.04, (8, 3))
    A = oth + np.array([-0.2, 0.0, 0.0])
    Bb = oth + np.array([1.2, 0.0, 0.0])
    return _f32(np.concatenate([Bb, [[1.0, 0.0, 0.0]], A, [[0.0, 0.0, 0.0]], [[px, 0.0, 0.0]]]))


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(21)
    out = {}
    out["n1"] = (_f32([[0.25, -1.0, 3.0]]), 0.5, (0, 1))
    out["n2_at_r2"] = (_f32([[0, 0, 0], [0.5, 0, 0]]), 0.5, (0, 1, 2))
    out["n2_one_ulp_beyond"] = (_f32([[0, 0, 0], [np.nextafter(np.float32(0.5), np.float32(1)), 0, 0]]), 0.5, (0, 1))
    out["n2_duplicates"] = (_f32([[0.3, 0.3, 0.3], [0.3, 0.3, 0.3]]), 0.5, (0, 1, 2))
    for n in (255, 256, 257, 1023, 1025):
        pts = _f32(rng.uniform(0, 1, (n, 3)))
        out["uniform%d_sparse" % n] = (pts, 0.7 * n ** (-1.0 / 3.0), (0, 1, 3))
        out["uniform%d_dense" % n] = (pts, 1.2 * n ** (-1.0 / 3.0), (0, 4))
    out["one_cell"] = (_f32(rng.uniform(0, 0.1, (1000, 3))), 1.0, (0, 5, 999, 1000))
    out["one_cell_parts"] = (_f32(rng.uniform(0, 0.1, (1000, 3))), 0.008, (0, 2))          # the same box in some 1 700 cells
    out["offset"] = (_f32(1000.0 + rng.uniform(-0.01, 0.01, (600, 3))), 0.002, (0, 2))
    out["negative"] = (_f32(rng.uniform(-1.0, -0.5, (500, 3))), 0.05, (0, 2))
    half = np.float32(0.5)
    out["bridge_at"] = (bridge(half), 0.5, (4,))
    out["bridge_below"] = (bridge(np.nextafter(half, np.float32(0))), 0.5, (4,))
    out["bridge_above"] = (bridge(np.nextafter(half, np.float32(1))), 0.5, (4,))
    blob = rng.uniform(-0.05, 0.05, (50, 3))
    out["equal_sizes"] = (_f32(np.concatenate([blob + [2, 0, 0], blob])[rng.permutation(100)]), 0.2, (0, 3))
    t = np.arange(600)[:, None]
    lines = np.concatenate([t * [0.05, 0.0, 0.0], t * [0.05, 0.0, 0.0] + [0.0, 0.3, 0.0]])
    out["straddle"] = (_f32(lines[rng.permutation(1200)]), 0.1, (0, 2, 4))                # 2 lines over 28 cells and 5 tiles each
    out["chain"] = (_f32((np.arange(4096, dtype=np.float32) * np.float32(0.9))[rng.permutation(4096)][:, None] * [1.0, 0.0, 0.0]), 1.0, (0, 2))
    return out


SELECTIONS = ((0, 0), (3, 0), (0, 2), (5, 1), (1, 1), (10 ** 6, 0))       # (min_size, keep)
SELECT_CASES = ("uniform1025_sparse", "uniform257_dense", "equal_sizes", "one_cell", "bridge_at")


@functools.lru_cache(maxsize=None)
def twin_of(name, min_neighbors):
    xyz, r, _ = cases()[name]
    labels, sizes = twin(xyz, r, min_neighbors)
    labels.setflags(write=False)
    sizes.setflags(write=False)
    return labels, sizes
