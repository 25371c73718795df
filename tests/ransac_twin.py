"""The numpy twin of the RANSAC pose estimation from correspondences (include/goicp_mi355.h) and the cases that
tests/test_ransac_host.py and tests/test_gpu_ransac.py share.  The twin shares nothing with the library but the rule, which it follows line
by line, vectorised over the hypotheses:
  draw     tests/plane_twin.py's (Python integers) at the counters 3 t + {0, 1, 2} over the M correspondences;
  reject   float64: ls2, lt2 = dot3(d, d) of the three edges on either side; kept iff min >= (sigma sigma) max on every edge;
  pose     float64, element-wise: the centroids ((a + b) + c) / 3, H_ab summed in the order a, b, c, K = H^T H by dot3, the Jacobi of
           tests/normals_twin.py, the stable descending order by three exchanges, degenerate when not l_1 > 0, u_k = H v_k normalised,
           Gram-Schmidt on u_1, the two cross products, R and t cast to float32, degenerate when one is not finite;
  pair     float32, left to right: y_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a, e = y - m, d2 = (e0 e0 + e1 e1) + e2 e2 <= distance * distance;
  score    integer counts; the max_poses largest (count, smallest t first) with a count of at least max(min_inliers, 3);
  refit    q = rint(ldexp(float64(x - mn), 31 - e)) as Python integers on both sides, the moments summed exactly;
           H = ldexp(float(m P - St Ss), -(31 - es) - (31 - et)) / (float(m) float(m)) (float(int) rounds correctly), the centroids
           float64(mn) + ldexp(float(S) / float(m), -(31 - e)); the same pose text; adopted iff not degenerate and its count >= the hypothesis'."""
import functools
import math

import numpy as np

import normals_twin as NT
import plane_twin as PT

same_bits = NT.same_bits
POSE_DTYPE = np.dtype([("R", "<f4", (3, 3)), ("t", "<f4", (3,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("refined", "<i4")])
TILE, BLOCK = 256, 1024                                          # goicp_ransac_pose_tile() / goicp_ransac_pose_block(); the host test checks them
SIZES = (3, 4, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1)
ITERATIONS = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
SEEDS = (0, 12345)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def from_cross_covariance(H, cs, ct):
    """H[a][b], cs[k], ct[k]: float64 arrays (n,) -> (R (n, 3, 3) float32, t (n, 3) float32, ok (n,) bool)"""
    n = len(cs[0])
    with np.errstate(all="ignore"):
        A = [[dot3([H[0][a], H[1][a], H[2][a]], [H[0][b], H[1][b], H[2][b]]) for b in range(3)] for a in range(3)]
        V = [[np.full(n, 1.0 if a == b else 0.0) for b in range(3)] for a in range(3)]
        for _ in range(NT.MAX_SWEEPS):
            r01 = NT._rotate(A, V, 0, 1)
            r02 = NT._rotate(A, V, 0, 2)
            r12 = NT._rotate(A, V, 1, 2)
            if not np.any(r01 | r02 | r12):
                break
        lam = [A[c][c].copy() for c in range(3)]
        col = [[V[r][c].copy() for r in range(3)] for c in range(3)]
        for i, j in ((0, 1), (1, 2), (0, 1)):
            sw = lam[j] > lam[i]
            lam[i], lam[j] = np.where(sw, lam[j], lam[i]), np.where(sw, lam[i], lam[j])
            for r in range(3):
                col[i][r], col[j][r] = np.where(sw, col[j][r], col[i][r]), np.where(sw, col[i][r], col[j][r])
        ok = lam[1] > 0.0
        v0, v1 = col[0], col[1]
        u0 = [dot3(H[a], v0) for a in range(3)]
        u1 = [dot3(H[a], v1) for a in range(3)]
        n0, n1 = np.sqrt(dot3(u0, u0)), np.sqrt(dot3(u1, u1))
        u0, u1 = [u / n0 for u in u0], [u / n1 for u in u1]
        d = dot3(u0, u1)
        u1 = [u1[a] - d * u0[a] for a in range(3)]
        n2 = np.sqrt(dot3(u1, u1))
        u1 = [u / n2 for u in u1]
        u2, v2 = cross(u0, u1), cross(v0, v1)
        R = np.empty((n, 3, 3), np.float32)
        t = np.empty((n, 3), np.float32)
        for a in range(3):
            for b in range(3):
                R[:, a, b] = ((u0[a] * v0[b] + u1[a] * v1[b]) + u2[a] * v2[b]).astype(np.float32)
            t[:, a] = (ct[a] - dot3([R[:, a, b].astype(np.float64) for b in range(3)], cs)).astype(np.float32)
    ok = ok & np.all(np.isfinite(R.reshape(n, 9)), axis=1) & np.all(np.isfinite(t), axis=1)
    return R, t, ok


def poses_of(S, Mt, abc, sigma):
    """S, Mt: the source / target point of every correspondence (M, 3) float32; abc (T, 3) -> (R, t, ok) of the hypotheses"""
    s = [S[abc[:, i]].astype(np.float64) for i in range(3)]
    m = [Mt[abc[:, i]].astype(np.float64) for i in range(3)]
    keep = np.ones(len(abc), bool)
    with np.errstate(all="ignore"):
        if sigma > 0:
            ss = np.float64(np.float32(sigma)) * np.float64(np.float32(sigma))
            for i, j in ((0, 1), (1, 2), (2, 0)):
                ds, dt = s[j] - s[i], m[j] - m[i]
                ls2, lt2 = dot3(ds.T, ds.T), dot3(dt.T, dt.T)
                keep &= np.minimum(ls2, lt2) >= ss * np.maximum(ls2, lt2)
        cs = [((s[0][:, k] + s[1][:, k]) + s[2][:, k]) / 3.0 for k in range(3)]
        ct = [((m[0][:, k] + m[1][:, k]) + m[2][:, k]) / 3.0 for k in range(3)]
        H = [[((m[0][:, a] - ct[a]) * (s[0][:, b] - cs[b]) + (m[1][:, a] - ct[a]) * (s[1][:, b] - cs[b])) + (m[2][:, a] - ct[a]) * (s[2][:, b] - cs[b])
              for b in range(3)] for a in range(3)]
    R, t, ok = from_cross_covariance(H, cs, ct)
    return R, t, ok & keep


def inliers(S, Mt, R, t, distance):
    """the pair of every correspondence against the poses (k, 3, 3) / (k, 3) -> (k, M) bool"""
    d = np.float32(distance)
    with np.errstate(all="ignore"):
        e = [(((R[:, a, 0, None] * S[None, :, 0] + R[:, a, 1, None] * S[None, :, 1]) + R[:, a, 2, None] * S[None, :, 2]) + t[:, a, None]) - Mt[None, :, a]
             for a in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        assert d2.dtype == np.float32
        return d2 <= d * d


def frame(P):
    mn = P.min(0)
    return mn, math.frexp(float((P - mn).max()))[1]


def refit(S, Mt, sel):
    """the least-squares pose over the correspondences sel -> (R (3, 3), t (3,)) float32 or None"""
    (mns, es), (mnt, et) = frame(S), frame(Mt)
    qs = [[int(v) for v in np.rint(np.ldexp((S[sel, k] - mns[k]).astype(np.float64), 31 - es))] for k in range(3)]
    qt = [[int(v) for v in np.rint(np.ldexp((Mt[sel, k] - mnt[k]).astype(np.float64), 31 - et))] for k in range(3)]
    m = len(qs[0])
    if m == 0:
        return None
    Ss, St = [sum(q) for q in qs], [sum(q) for q in qt]
    P = [[sum(x * y for x, y in zip(qt[a], qs[b])) for b in range(3)] for a in range(3)]
    H = [[np.array([math.ldexp(float(m * P[a][b] - St[a] * Ss[b]), -(31 - es) - (31 - et)) / (float(m) * float(m))]) for b in range(3)] for a in range(3)]
    cs = [np.array([np.float64(mns[k]) + math.ldexp(float(Ss[k]) / float(m), -(31 - es))]) for k in range(3)]
    ct = [np.array([np.float64(mnt[k]) + math.ldexp(float(St[k]) / float(m), -(31 - et))]) for k in range(3)]
    R, t, ok = from_cross_covariance(H, cs, ct)
    return (R[0], t[0]) if ok[0] else None


def hypothesis_counts(src, tgt, corr, distance, iterations, edge_similarity=0.9, seed=0):
    """-> (R (T, 3, 3), t (T, 3), counts (T,) int64; 0 for a rejected or degenerate hypothesis), and the gathered S, Mt"""
    src, tgt = np.ascontiguousarray(src, np.float32).reshape(-1, 3), np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    S, Mt = src[corr[:, 0]], tgt[corr[:, 1]]
    T = iterations or 100000
    abc = np.array([PT.draw(seed, t, len(corr)) for t in range(T)], np.int64)
    R, t, ok = poses_of(S, Mt, abc, edge_similarity)
    counts = np.zeros(T, np.int64)
    for t0 in range(0, T, 64):
        counts[t0:t0 + 64] = inliers(S, Mt, R[t0:t0 + 64], t[t0:t0 + 64], distance).sum(1)
    counts[~ok] = 0
    return R, t, counts, S, Mt


def ransac_pose(src, tgt, corr, distance, iterations=100000, refine=1, max_poses=1, min_inliers=0, edge_similarity=0.9, seed=0):
    """-> (poses (c,) POSE_DTYPE, inlier mask (M,) uint8 of pose 0)"""
    R, t, counts, S, Mt = hypothesis_counts(src, tgt, corr, distance, iterations, edge_similarity, seed)
    poses = []
    for h in np.argsort(-counts, kind="stable")[:max_poses or 1]:    # descending count, the smaller t first among equals
        cnt = int(counts[h])
        if cnt < max(min_inliers, 3):
            break
        Rh, th, refined = R[h], t[h], 0
        if refine:
            r = refit(S, Mt, inliers(S, Mt, Rh[None], th[None], distance)[0])
            if r is not None:
                c2 = int(inliers(S, Mt, r[0][None], r[1][None], distance)[0].sum())
                if c2 >= cnt:
                    Rh, th, cnt, refined = r[0], r[1], c2, 1
        rec = np.zeros(1, POSE_DTYPE)[0]
        rec["R"], rec["t"], rec["inliers"], rec["hypothesis"], rec["refined"] = Rh, th, cnt, int(h), refined
        poses.append(rec)
    poses = np.array(poses, POSE_DTYPE)
    mask = inliers(S, Mt, poses["R"][:1], poses["t"][:1], distance)[0].astype(np.uint8) if len(poses) else np.zeros(len(S), np.uint8)
    return poses, mask


def select_matches(index, d2, d2_second, mutual=None, ratio=0.0, require_mutual=True):
    d2, d2_second, r = np.asarray(d2, np.float32), np.asarray(d2_second, np.float32), np.float32(ratio)
    keep = np.ones(len(index), bool) if (mutual is None or not require_mutual) else np.asarray(mutual) != 0
    if ratio != 0:
        keep = keep & (d2 <= (r * r) * d2_second)
    q = np.flatnonzero(keep)
    return np.stack([q, np.asarray(index)[q]], 1).astype(np.int32)


# ---- the inputs ----
def _ro(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(degrees)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


TRUE_R, TRUE_T = rotation([1.0, -2.0, 0.5], 100.0), np.array([0.3, -0.2, 0.5])


def scene(M, true_share=0.5, noise=0.005, seed=1, offset=0.0):
    """M correspondences between two clouds of max(M, 8) points each: the first true_share of them (shuffled afterwards) pair a source
    point with its image under (TRUE_R, TRUE_T) plus noise, the others pair random points -> (src, tgt, corr, is_true)"""
    rng = np.random.default_rng(1000 * seed + M)
    n = max(M, 8)
    src = rng.uniform(-1, 1, (n, 3)) + offset
    tgt = src @ TRUE_R.T + TRUE_T + rng.normal(0, noise, (n, 3))
    n_true = max(3, int(round(true_share * M))) if M > 3 else 3
    perm = rng.permutation(n)[:M]
    corr = np.stack([perm, perm], 1)
    wrong = np.arange(M) >= n_true
    corr[wrong, 1] = rng.integers(0, n, wrong.sum())
    wrong &= corr[:, 0] != corr[:, 1]
    order = rng.permutation(M)
    return _ro(src), _ro(tgt), _ro(corr[order], np.int32), ~wrong[order]


def exact_copy(M=65):
    """grid points and their exact images under a quarter turn about z: (x, y, z) -> (-y, x, z)"""
    rng = np.random.default_rng(5)
    src = rng.integers(-32, 33, (M, 3)) / 64.0
    tgt = np.stack([-src[:, 1], src[:, 0], src[:, 2]], 1)
    return _ro(src), _ro(tgt), _ro(np.stack([np.arange(M), np.arange(M)], 1), np.int32)


def recovery():
    """M = 400, 30 % true under (TRUE_R, TRUE_T) with noise sigma = distance / 3, the rest random pairs; T = 2 000, refit"""
    distance = 0.03
    src, tgt, corr, is_true = scene(400, 0.3, distance / 3, seed=7)
    return src, tgt, corr, is_true, dict(distance=distance, iterations=2000, refine=1, max_poses=1, edge_similarity=0.9, seed=0)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (src, tgt, corr, keyword arguments of ransac_pose)"""
    out = {}
    i = 0
    for M in SIZES:
        for T in ITERATIONS:
            src, tgt, corr, _ = scene(M)
            out["scene%d_T%d" % (M, T)] = (src, tgt, corr, dict(distance=0.03, iterations=T, refine=i % 2, max_poses=(1, 2, 64)[(i // 2) % 3],
                                                                edge_similarity=(0.0, 0.9, 1.0)[(i // 3) % 3] if M > 4 else 0.0, seed=SEEDS[(i // 4) % 2]))
            i += 1
    src, tgt, corr, _ = scene(257)
    for refine in (0, 1):
        for K in (1, 2, 64):
            for sigma in (0.0, 0.9, 1.0):
                out["scene257_r%d_K%d_e%g" % (refine, K, sigma)] = (src, tgt, corr, dict(distance=0.03, iterations=257, refine=refine, max_poses=K,
                                                                                       edge_similarity=sigma, seed=3))
    out["min_inliers_above_M"] = (src, tgt, corr, dict(distance=0.03, iterations=65, min_inliers=258))
    out["min_inliers_cuts"] = (src, tgt, corr, dict(distance=0.03, iterations=257, max_poses=64, min_inliers=100, edge_similarity=0.0))
    # lines along an axis: H has one non-zero entry, so l_1 is exactly 0 (on a skew line rounding may leave l_1 a few ulps above 0, and the
    # hypothesis then gets one of the poses that fit the line)
    line = np.arange(65, dtype=np.float32)[:, None] / 16 * np.array([[1, 0, 0]], np.float32)
    ident = _ro(np.stack([np.arange(65), np.arange(65)], 1), np.int32)
    out["collinear"] = (_ro(line), _ro(line[:, ::-1]), ident, dict(distance=0.01, iterations=65, edge_similarity=0.0))
    out["coincident_source"] = (_ro(np.tile(np.array([[0.25, -0.5, 0.75]], np.float32), (65, 1))), scene(65)[1][:65], ident,
                                dict(distance=0.01, iterations=65, edge_similarity=0.0))
    for refine in (0, 1):
        out["exact_copy_r%d" % refine] = exact_copy() + (dict(distance=1e-3, iterations=64, refine=refine, edge_similarity=0.9),)
        src, tgt, corr, _ = scene(257, offset=1000.0)
        out["offset1000_r%d" % refine] = (src, tgt, corr, dict(distance=0.03, iterations=257, refine=refine, max_poses=2, seed=1))
    src, tgt, corr, _ = scene(129)
    dup = np.array(corr)
    dup[::3, 0] = dup[0, 0]                                      # a third of the correspondences name one source point
    dup[1::5, 1] = dup[1, 1]                                     # and a fifth one target point
    out["duplicate_indices"] = (src, tgt, _ro(dup, np.int32), dict(distance=0.03, iterations=129, max_poses=2))
    return out


@functools.lru_cache(maxsize=None)
def twin_of(name):
    """computed once per case, shared, never changed"""
    src, tgt, corr, kw = cases()[name]
    out = ransac_pose(src, tgt, corr, **kw)
    for a in out:
        a.setflags(write=False)
    return out
