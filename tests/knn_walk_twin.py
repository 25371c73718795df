"""A plain numpy model of the k-NN walk's control flow (rows_knn, csrc/device.hip) over the box hierarchy as the device build lays it out
(launch_kd_build, csrc/kdbuild.hip).  It restates what decides whether a walk ends and what it returns -- nothing about lanes, shuffles or
memory -- so that the "group exhausted" test can be exchanged and the walk stepped under a cap, on a CPU:

  hierarchy   30-bit Morton keys of the points quantised to 1024 cells per axis of the cloud's cube (float32, the kernel's expression), a
              stable sort, leaf f = the sorted points [f M / L, (f + 1) M / L) of L = 64^K leaves with 16 slots each (unused slots: index
              INT_MAX), an empty leaf's box inverted and infinite, every upper box the union of its 64 children;
  keys        a child is the bits of its float32 box distance with the two low bits replaced by its place j = c & 3 in its owner's quad;
              0xffffffff once taken;
  take        the smallest key of the group; among equal keys the first owner (quad) wins, and the child taken is that quad's place
              (key & 3) -- so a group with nothing left "takes" child 3 and returns 0xffffffff;
  list        at most k keys (distance bits << 32 | index), ascending; candidates at or above the k-th key are dropped, the bound of the
              pruning is the k-th key's distance bits, 0xffffffff while the list is short;
  seed        optionally one leaf slot whose point enters the list first and is skipped by the scans.

exhausted(m, bound) is a parameter: EXHAUSTED_BOUND_ONLY is the test the kernel had, EXHAUSTED_ALL_TAKEN the one it has now.
The clouds of tests/test_gpu_kd_device_build.py are made here too (target_cloud), so that the host test looks at the very hierarchies the
device will build.  Nothing here touches a device."""
import bisect

import numpy as np

INT_MAX = 2 ** 31 - 1
TAKEN = 0xFFFFFFFF
LEAF_SLOTS = 16
NO_KEY = (1 << 64) - 1


def EXHAUSTED_BOUND_ONLY(m, bound):
    return (m & ~3 & TAKEN) > bound


def EXHAUSTED_ALL_TAKEN(m, bound):
    return m == TAKEN or (m & ~3 & TAKEN) > bound


def depth_of(M):
    """the device build's K: the smallest number of box levels whose 64^K leaves of 16 slots hold M points"""
    K = 1
    while LEAF_SLOTS * 64 ** K < M:
        K += 1
    return K


def _spread10(x):
    x = x & np.uint32(0x3FF)
    x = (x ^ (x << np.uint32(16))) & np.uint32(0xFF0000FF)
    x = (x ^ (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x ^ (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x ^ (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def morton_keys(xyz):
    xyz = np.asarray(xyz, np.float32)
    mn, mx = xyz.min(0), xyz.max(0)
    ext = np.float32((mx - mn).max())
    inv = np.float32(1.0) / ext if ext > 0 else np.float32(0.0)
    key = np.zeros(len(xyz), np.uint32)
    for a in range(3):
        f = (xyz[:, a] - mn[a]) * inv
        q = np.minimum(np.float32(1023.0), np.maximum(np.float32(0.0), f * np.float32(1024.0))).astype(np.uint32)
        key |= _spread10(q) << np.uint32(a)
    return key


class Hierarchy:
    """pts (L * 16, 3) float32 and ids (L * 16,) int64 by leaf slot; lo[l], hi[l]: (64^l, 64, 3) float32, the child boxes of every group of
    level l; count (L,): points per leaf"""

    def __init__(self, xyz, K=None):
        xyz = np.ascontiguousarray(xyz, np.float32)
        M = len(xyz)
        self.M, self.K = M, depth_of(M) if K is None else K
        L = self.L = 64 ** self.K
        order = np.argsort(morton_keys(xyz), kind="stable")
        f = np.arange(L + 1, dtype=np.int64)
        start = f * M // L
        self.count = np.diff(start)
        assert self.count.max() <= LEAF_SLOTS
        self.pts = np.full((L * LEAF_SLOTS, 3), np.inf, np.float32)
        self.ids = np.full(L * LEAF_SLOTS, INT_MAX, np.int64)
        leaf_of = np.searchsorted(start, np.arange(M), side="right") - 1           # the leaf of every sorted position
        slot = leaf_of * LEAF_SLOTS + (np.arange(M) - start[leaf_of])
        self.pts[slot] = xyz[order]
        self.ids[slot] = order
        self.slot_of = np.empty(M, np.int64)                                       # leaf slot of every original index
        self.slot_of[order] = slot
        p = self.pts.reshape(L, LEAF_SLOTS, 3)
        lo = np.where(np.isinf(p), np.float32(np.inf), p).min(1)
        hi = np.where(np.isinf(p), np.float32(-np.inf), p).max(1)
        self.lo, self.hi = [None] * self.K, [None] * self.K
        for l in range(self.K - 1, -1, -1):
            self.lo[l], self.hi[l] = lo.reshape(-1, 64, 3), hi.reshape(-1, 64, 3)
            lo, hi = self.lo[l].min(1), self.hi[l].max(1)

    def group_count(self):
        """points per bottom-level group"""
        return self.count.reshape(-1, 64).sum(1)

    def trigger_groups(self, k):
        """the bottom-level groups with fewer than k points whose child 3 is an empty leaf: a walk that exhausts one with a short list
        rescans that leaf for ever under EXHAUSTED_BOUND_ONLY"""
        c = self.count.reshape(-1, 64)
        return np.nonzero((c.sum(1) < k) & (c[:, 3] == 0))[0]

    def keys(self, level, group, q):
        lo, hi = self.lo[level][group], self.hi[level][group]
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.maximum(np.maximum(lo - q, q - hi), np.float32(0.0))
            d = e[:, 0] * e[:, 0]
            d = d + e[:, 1] * e[:, 1]
            d = d + e[:, 2] * e[:, 2]
        return [(int(b) & ~3 & TAKEN) | (c & 3) for c, b in enumerate(d.astype(np.float32).view(np.uint32))]


def take(key):
    """-> (the smallest key, the child taken); marks it taken"""
    m = min(key)
    owner = next(l for l in range(16) if min(key[4 * l:4 * l + 4]) == m)
    child = 4 * owner + (m & 3)
    key[child] = TAKEN
    return m, child


def d2_bits(q, p):
    """the leaf scan's float32 expression, as bits"""
    d = (q - p).astype(np.float32)
    e = d[..., 0] * d[..., 0]
    e = e + d[..., 1] * d[..., 1]
    e = e + d[..., 2] * d[..., 2]
    return e.astype(np.float32).view(np.uint32)


def walk(h, q, k, exhausted=EXHAUSTED_ALL_TAKEN, seed_slot=None, cap=100000):
    """-> dict: ended (False: the cap was hit), steps, keys (the list, ascending, k entries once full), short_exhausts: the (group, child 3
    empty) of every bottom-level group left -- or not left -- with nothing to take while the list was short"""
    K = h.K
    q = np.asarray(q, np.float32)
    key = [[TAKEN] * 64 for _ in range(K)]
    node = [0] * K
    key[0] = h.keys(0, 0, q)
    d = 0
    if K > 1:
        _, node[1] = take(key[0])
        key[1] = h.keys(1, node[1], q)
        d = 1
    lst = []
    if seed_slot is not None and h.ids[seed_slot] != INT_MAX:
        lst.append((int(d2_bits(q, h.pts[seed_slot])) << 32) | int(h.ids[seed_slot]))
    else:
        seed_slot = -1 if seed_slot is None else seed_slot
    steps, short = 0, []
    while True:
        if steps == cap:
            return dict(ended=False, steps=steps, keys=lst, short_exhausts=short)
        steps += 1
        bound = lst[k - 1] >> 32 if len(lst) >= k else TAKEN
        cand, acted = [], False
        for L in range(K - 1, -1, -1):
            if acted or d != L:
                continue
            m, c = take(key[L])
            if m == TAKEN and L == K - 1 and len(lst) < k:
                short.append((node[L], bool(h.count[node[L] * 64 + 3] == 0)))
            if exhausted(m, bound):
                if L == 0:
                    return dict(ended=True, steps=steps, keys=lst, short_exhausts=short)
                d = L - 1
            elif L == K - 1:
                s0 = (node[L] * 64 + c) * LEAF_SLOTS
                bits = d2_bits(q, h.pts[s0:s0 + LEAF_SLOTS])
                for l in range(LEAF_SLOTS):
                    if s0 + l != seed_slot and h.ids[s0 + l] != INT_MAX:
                        cand.append((int(bits[l]) << 32) | int(h.ids[s0 + l]))
                acted = True
            else:
                node[L + 1] = node[L] * 64 + c
                key[L + 1] = h.keys(L + 1, node[L + 1], q)
                d = L + 1
                acted = True
        for c in cand:                                     # lane order; each against the k-th key of that moment
            if c < (lst[k - 1] if len(lst) >= k else NO_KEY):
                bisect.insort(lst, c)
                del lst[k:]


def brute_keys(target, q, k):
    """the k smallest (distance bits << 32 | index) of one query, ascending: the list an exact walk returns"""
    bits = d2_bits(np.asarray(q, np.float32), np.asarray(target, np.float32))
    keys = (bits.astype(np.uint64) << np.uint64(32)) | np.arange(len(target), dtype=np.uint64)
    return [int(v) for v in np.sort(keys)[:k]]


# ----------------------------------------------------------------------------------------------
# the target clouds of the device-build tests
# ----------------------------------------------------------------------------------------------
KINDS = ("uniform", "synth", "cluster", "duplicates", "coincident", "axis")     # "identical" is a cloud too, but one goicp_create refuses
M_K1 = (2, 17, 63, 64, 65, 1024)                       # one box level; up to 65 points some of the root's 64 leaves are empty
M_K2 = (1025, 1500, 2047, 2048, 2049)                  # two: 16.02, 23.4, 31.98, 32 and 32.02 points per bottom-level group
M_K3 = (65537, 100000, 131071, 131073)                 # three: 16.0002, 24.4, 31.9998 and 32.0002
KNN_K = (1, 16, 17, 31, 32)
N_QUERIES = 256
# (kind, M) of every cloud the device-build tests walk: every size on the synth surface, every kind at M = 1 500, the first three at 100 000
CELLS = tuple(("synth", M) for M in M_K1 + M_K2 + M_K3) + tuple((kind, 1500) for kind in KINDS if kind != "synth") + (("uniform", 100000), ("cluster", 100000))
# the cells inside the bands where a bottom-level group holds fewer than 32 points, with the k that makes a walk outlast such a group
BAND_CELLS = tuple((kind, M, 32) for kind, M in CELLS if M in (1025, 1500, 2047, 65537, 100000, 131071)) + (("synth", 1025, 17), ("synth", 65537, 17))


def query_seed(M):
    return 17 + M


def ks_of(M):
    """KNN_K clipped to M, ascending, each once"""
    return tuple(sorted({min(k, M) for k in KNN_K}))


def target_cloud(kind, M, seed=20261021):
    """(M, 3) float32 inside [-0.95, 0.95]^3.  uniform: a cube; cluster: M - 1 points within a few 1e-4 of one place and one far point, so
    nearly all Morton keys are equal and leaves are index runs with coinciding boxes; duplicates: a quarter of the cube's points overwritten
    by copies of other points (ties go to the lower index); identical: one place M times (extent 0: the engine refuses it, its distance
    transform needs a box); coincident: the same with one point elsewhere -- M - 1 equal keys, equal boxes and equal distances; axis: y = z = 0"""
    rng = np.random.default_rng(seed + M)
    if kind == "uniform":
        p = rng.uniform(-0.9, 0.9, (M, 3))
    elif kind == "cluster":
        p = np.array([0.3, 0.2, -0.1]) + rng.normal(scale=1e-4, size=(M, 3))
        p[M // 2] = [-0.9, -0.9, -0.9]
    elif kind == "duplicates":
        p = rng.uniform(-0.9, 0.9, (M, 3))
        dst = rng.choice(M, M // 4, replace=False)
        p[dst] = p[rng.integers(0, M, len(dst))]
    elif kind in ("identical", "coincident"):
        p = np.tile(np.array([0.25, -0.5, 0.125]), (M, 1))
        if kind == "coincident":
            p[M // 3] = [-0.5, 0.25, 0.75]
    elif kind == "axis":
        p = np.zeros((M, 3))
        p[:, 0] = rng.uniform(-0.9, 0.9, M)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, np.float32)


def device_build_case(synth, kind, M):
    """twins.make_case(SEED, M, N = 257): the synth surface as target, a source of 225 surface points and 32 far ones, the start pose; any other
    kind replaces the target.  Built once per cell by its callers; read-only"""
    import twins
    c = twins.make_case(synth, 20261017, M, 257)
    if kind != "synth":
        c["target"] = target_cloud(kind, M)
        c["extent"] = float(max((c["target"].max(0) - c["target"].min(0)).max(), (c["source"].max(0) - c["source"].min(0)).max()))
    c["kind"] = kind
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def walk_queries(target, n, seed):
    """a quarter each on target points, near them, around the cloud and far outside it"""
    rng = np.random.default_rng(seed)
    lo, hi = target.min(0), target.max(0)
    ext = float((hi - lo).max())
    m = n // 4
    on = target[rng.integers(0, len(target), m)]
    near = target[rng.integers(0, len(target), m)] + rng.normal(scale=2e-2 * ext, size=(m, 3))
    around = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (m, 3))
    out = rng.uniform(-1, 1, (n - 3 * m, 3)) * 4 * ext + (lo + hi) / 2 + 3 * ext
    return np.concatenate([on, near, around, out]).astype(np.float32)
