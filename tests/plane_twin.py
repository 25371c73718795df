"""The numpy twin of the RANSAC plane segmentation (include/goicp_mi355.h) and the cases that tests/test_plane_host.py and
tests/test_gpu_plane.py share.  The twin shares nothing with the library but the rule, which it follows line by line:
  draw     Python integers: h(c) = the splitmix64 finaliser of seed + (c + 1) * 0x9E3779B97F4A7C15 at the counters 3 (p T + t) + {0, 1, 2};
           a = h0 mod n, b = h1 mod (n - 1) (+1 when >= a), c = h2 mod (n - 2) (+1 when >= min(a, b), again when >= max(a, b));
  plane    float64, element-wise: u = pb - pa, v = pc - pa, n = u x v with both products rounded, l2 = (n0 n0 + n1 n1) + n2 n2; degenerate when
           not l2 > 0 or the float32 normal n / sqrt(l2) is not finite; sign: the first non-zero component positive, zeros +0;
  pair     float32, left to right: e = ((x0 - a0) n0 + (x1 - a1) n1) + (x2 - a2) n2; inlier iff |e| <= distance;
  score    integer counts, the largest, ties to the smallest t; below max(min_inliers, 3) the search ends;
  refit    q = rint(ldexp(float64(x - mn), 31 - e)) as Python integers, the moments m, S, P summed exactly; C = ldexp(float(m P - S S),
           -2 (31 - e)) / (float(m) float(m)) (float(int) rounds correctly); the Jacobi of tests/normals_twin.py; the smallest eigenvalue's
           column; the centroid anchor; adopted iff its count >= the hypothesis' count."""
import functools
import math
import os

import numpy as np

import normals_twin as NT

same_bits = NT.same_bits
PLANE_DTYPE = np.dtype([("normal", "<f4", (3,)), ("point", "<f4", (3,)), ("d", "<f4"), ("inliers", "<i4"), ("hypothesis", "<i4"), ("refined", "<i4")])
M64 = (1 << 64) - 1
SIZES = (3, 4, 63, 64, 65, 257, 1025)
ITERATIONS = (1, 63, 64, 65, 257, 1000)
SEEDS = (0, 12345)


def h(seed, c):
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, g, n):
    a = h(seed, 3 * g) % n
    b = h(seed, 3 * g + 1) % (n - 1)
    if b >= a:
        b += 1
    c = h(seed, 3 * g + 2) % (n - 2)
    if c >= min(a, b):
        c += 1
    if c >= max(a, b):
        c += 1
    return a, b, c


def signed(nf):
    """the sign rule on float32 normals (k, 3)"""
    lead = np.where(nf[:, 0] != 0, nf[:, 0], np.where(nf[:, 1] != 0, nf[:, 1], nf[:, 2]))
    out = np.where((lead < 0)[:, None], -nf, nf)
    return np.where(nf == 0, np.float32(0), out).astype(np.float32)


def planes_of(cur, abc):
    """-> (normals (T, 3) float32, ok (T,) bool) of the triples abc (T, 3) of the cloud"""
    X = cur.astype(np.float64)
    pa, pb, pc = X[abc[:, 0]], X[abc[:, 1]], X[abc[:, 2]]
    with np.errstate(all="ignore"):
        u, v = pb - pa, pc - pa
        n0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        n1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        n2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        l2 = (n0 * n0 + n1 * n1) + n2 * n2
        ln = np.sqrt(l2)
        nf = np.stack([(n0 / ln).astype(np.float32), (n1 / ln).astype(np.float32), (n2 / ln).astype(np.float32)], 1)
    ok = (l2 > 0) & np.all(np.isfinite(nf), axis=1)
    return signed(nf), ok


def inliers(cur, anchor, normal, distance):
    """the pair of every point against the planes (k, 3) / (k, 3) -> (k, n) bool"""
    x, a, n = cur.astype(np.float32), anchor.astype(np.float32), normal.astype(np.float32)
    with np.errstate(all="ignore"):
        e = ((x[None, :, 0] - a[:, None, 0]) * n[:, None, 0] + (x[None, :, 1] - a[:, None, 1]) * n[:, None, 1]) + (x[None, :, 2] - a[:, None, 2]) * n[:, None, 2]
        assert e.dtype == np.float32
        return np.abs(e) <= np.float32(distance)


def refit(cur, sel):
    """the least-squares plane over the points sel of the round's cloud -> (normal (3,) float32, anchor (3,) float32) or None"""
    mn = cur.min(0)
    E = float((cur - mn).max())
    e = math.frexp(E)[1]
    d = (cur[sel] - mn).astype(np.float64)
    q = [[int(v) for v in np.rint(np.ldexp(d[:, k], 31 - e))] for k in range(3)]
    m = len(q[0])
    S = [sum(q[k]) for k in range(3)]
    P = {(a, b): sum(x * y for x, y in zip(q[a], q[b])) for a in range(3) for b in range(a, 3)}
    Cm = {ab: np.array([math.ldexp(float(m * P[ab] - S[ab[0]] * S[ab[1]]), -2 * (31 - e)) / (float(m) * float(m))]) for ab in P}
    A = [[Cm[(min(a, b), max(a, b))].copy() for b in range(3)] for a in range(3)]
    V = [[np.full(1, 1.0 if a == b else 0.0) for b in range(3)] for a in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(NT.MAX_SWEEPS):
            r01 = NT._rotate(A, V, 0, 1)
            r02 = NT._rotate(A, V, 0, 2)
            r12 = NT._rotate(A, V, 1, 2)
            if not np.any(r01 | r02 | r12):
                break
        lam = [A[c][c][0] for c in range(3)]
        col, lmin = 0, lam[0]
        for c in (1, 2):
            if lam[c] < lmin:
                col, lmin = c, lam[c]
        v = [V[r][col][0] for r in range(3)]
        length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        nf = np.array([[np.float32(v[r] / length) for r in range(3)]], np.float32)
    if not np.all(np.isfinite(nf)) or not np.any(nf != 0):
        return None
    anchor = np.array([np.float32(np.float64(mn[k]) + math.ldexp(float(S[k]) / float(m), -(31 - e))) for k in range(3)], np.float32)
    return signed(nf)[0], anchor


def segment_plane(xyz, distance, iterations=1000, refine=1, max_planes=1, min_inliers=0, seed=0):
    """-> (labels (n,) int32, planes (c,) PLANE_DTYPE, kept cloud (m, 3) float32, kept indices (m,) int32)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    T, P = iterations or 1000, max_planes or 1
    n = len(xyz)
    label = np.full(n, -1, np.int32)
    cur, cmap = xyz, np.arange(n, dtype=np.int32)
    planes = []
    for p in range(P):
        np_ = len(cur)
        if np_ < 3:
            break
        abc = np.array([draw(seed, p * T + t, np_) for t in range(T)], np.int64)
        normal, ok = planes_of(cur, abc)
        counts = np.zeros(T, np.int64)
        for t0 in range(0, T, 64):
            counts[t0:t0 + 64] = inliers(cur, cur[abc[t0:t0 + 64, 0]], normal[t0:t0 + 64], distance).sum(1)
        counts[~ok] = 0
        best = int(np.argmax(counts))                           # the first of the largest
        if counts[best] < max(min_inliers, 3):
            break
        nr, an, cnt, refined = normal[best], cur[abc[best, 0]], int(counts[best]), 0
        if refine:
            r = refit(cur, inliers(cur, an[None], nr[None], distance)[0])
            if r is not None:
                c2 = int(inliers(cur, r[1][None], r[0][None], distance)[0].sum())
                if c2 >= cnt:
                    nr, an, cnt, refined = r[0], r[1], c2, 1
        rec = np.zeros(1, PLANE_DTYPE)[0]
        n64, p64 = nr.astype(np.float64), an.astype(np.float64)
        rec["normal"], rec["point"], rec["d"] = nr, an, np.float32(-((n64[0] * p64[0] + n64[1] * p64[1]) + n64[2] * p64[2]))
        rec["inliers"], rec["hypothesis"], rec["refined"] = cnt, best, refined
        took = inliers(cur, an[None], nr[None], distance)[0]
        label[cmap[took]] = len(planes)
        planes.append(rec)
        cur, cmap = cur[~took], cmap[~took]
    return label, np.array(planes, PLANE_DTYPE), np.ascontiguousarray(cur), np.ascontiguousarray(cmap)


def first_valid_hypothesis(xyz, iterations, seed):
    """the smallest non-degenerate t of round 0"""
    abc = np.array([draw(seed, t, len(xyz)) for t in range(iterations)], np.int64)
    return int(np.flatnonzero(planes_of(np.asarray(xyz, np.float32), abc)[1])[0])


# ---- the clouds ----
def _ro(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


def slab(n, seed=1):
    """four fifths of the points within 0.01 of a tilted plane, the rest anywhere in the unit cube"""
    rng = np.random.default_rng(100 + n + seed)
    p = rng.uniform(-1, 1, (n, 3))
    on = rng.uniform(size=n) < 0.8
    p[on, 2] = 0.3 * p[on, 0] - 0.2 * p[on, 1] + rng.normal(0, 0.004, on.sum())
    return _ro(p)


def exact_plane(n=257):
    rng = np.random.default_rng(7)
    p = rng.uniform(-1, 1, (n, 3))
    p[:, 2] = 0
    return _ro(p)


BOUNDARY_DISTANCE = np.float32(0.0625)


def boundary_plane():
    """200 points at z = 0, then 5 at z = distance (inliers) and 5 at nextafter(distance) (not)"""
    rng = np.random.default_rng(8)
    p = rng.uniform(-1, 1, (210, 3)).astype(np.float32)
    p[:200, 2] = 0
    p[200:205, 2] = BOUNDARY_DISTANCE
    p[205:, 2] = np.nextafter(BOUNDARY_DISTANCE, np.float32(1))
    return _ro(p)


def floor_wall_object():
    """a floor z ~ 0 (500 points), a wall x ~ 1 (300) and a ball of 200 above the floor, shuffled"""
    rng = np.random.default_rng(9)
    floor = np.c_[rng.uniform(-1, 1, (500, 2)), rng.normal(0, 0.002, 500)]
    wall = np.c_[1 + rng.normal(0, 0.002, 300), rng.uniform(-1, 1, 300), rng.uniform(0.05, 1, 300)]
    v = rng.normal(size=(200, 3))
    ball = v / np.linalg.norm(v, axis=1)[:, None] * 0.2 + np.array([0.0, 0.0, 0.4])
    return _ro(np.concatenate([floor, wall, ball])[rng.permutation(1000)])


@functools.lru_cache(maxsize=None)
def object_on_floor():
    """every 15th point of the bunny scan on a floor of 60 % as many points at the cloud's min y with noise sigma 0.002, the whole tilted
    0.3 rad about z and shuffled -> (cloud, is_floor)"""
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_bunny.f32")
    obj = np.fromfile(g, dtype="<f4").reshape(-1, 3)[::15].astype(np.float64)
    rng = np.random.default_rng(11)
    nf = int(0.6 * len(obj))
    lo, hi = obj.min(0), obj.max(0)
    floor = np.c_[rng.uniform(lo[0] - 0.2, hi[0] + 0.2, nf), lo[1] + rng.normal(0, 0.002, nf), rng.uniform(lo[2] - 0.2, hi[2] + 0.2, nf)]
    c, s = math.cos(0.3), math.sin(0.3)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    perm = rng.permutation(len(obj) + nf)
    is_floor = (np.arange(len(obj) + nf) >= len(obj))[perm]
    return _ro((np.concatenate([obj, floor]) @ R.T)[perm]), is_floor


OBJECT_ON_FLOOR = dict(distance=0.008, iterations=256)
OBJECT_SEEDS = (0, 1, 2, 12345)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (cloud, keyword arguments of segment_plane)"""
    out = {}
    i = 0
    for n in SIZES:
        for T in ITERATIONS:
            out["slab%d_T%d" % (n, T)] = (slab(n), dict(distance=0.012, iterations=T, refine=i % 2, max_planes=1 + (i // 2) % 2, seed=SEEDS[(i // 4) % 2]))
            i += 1
    for refine in (0, 1):
        for seed in SEEDS:
            out["slab257_r%d_s%d" % (refine, seed)] = (slab(257), dict(distance=0.012, iterations=257, refine=refine, max_planes=2, seed=seed))
        out["exact_plane_r%d" % refine] = (exact_plane(), dict(distance=0.01, iterations=64, refine=refine))
        out["boundary_r%d" % refine] = (boundary_plane(), dict(distance=float(BOUNDARY_DISTANCE), iterations=64, refine=refine))
    out["duplicates"] = (_ro(np.tile(np.array([[0.25, -0.5, 0.75]], np.float32), (65, 1))), dict(distance=0.01, iterations=65))
    out["collinear"] = (_ro(np.arange(65, dtype=np.float32)[:, None] * np.array([[1, 2, 3]], np.float32)), dict(distance=0.01, iterations=65))
    for P in (1, 2):
        out["floor_wall_object_P%d" % P] = (floor_wall_object(), dict(distance=0.01, iterations=128, max_planes=P, seed=3))
    out["floor_wall_object_min_inliers"] = (floor_wall_object(), dict(distance=0.01, iterations=128, max_planes=2, min_inliers=400, seed=3))
    for seed in OBJECT_SEEDS[:2]:
        out["object_on_floor_s%d" % seed] = (object_on_floor()[0], dict(seed=seed, **OBJECT_ON_FLOOR))
    return out


@functools.lru_cache(maxsize=None)
def twin_of(name):
    """computed once per case, shared, never changed"""
    xyz, kw = cases()[name]
    out = segment_plane(xyz, **kw)
    for a in out:
        a.setflags(write=False)
    return out
