"""Plain float64 helpers shared by the small-shape GPU tests (tests/test_gpu_small_shapes.py): the seeded clouds with appended far points,
the gate picked from the data, one weighted Kabsch step, the conditioning of the pose systems and the cube-bound reference sums.
Nothing here touches a device; the twins of whole ICP loops stay in the test modules that own them."""
import numpy as np

START_ROT = np.array([0.02, -0.03, 0.01])          # the start pose of every ICP case: this turn and this shift on top of the ground truth
START_SHIFT = np.array([0.01, -0.02, 0.015])


def rodrigues64(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def default_outliers(N):
    """how many far points a source of N points ends with: none at N = 1, one up to N = 15, N // 8 above"""
    return 0 if N < 2 else max(1, N // 8)


def make_case(synth, seed, M, N, out_idx=None, noise=0.002):
    """-> dict: target (M, 3), source (N, 3) float32, the start pose R0 (3, 3), t0 (3,) float32, out_idx (the far points' places), extent.
    The source is synth.make_pair(seed, M, N - n_out)'s with n_out deterministic far points added (at the end unless out_idx names
    their places): points that the start pose carries to radius 1.3 .. 1.5 around the origin, the surface staying inside radius 0.95."""
    out_idx = np.arange(N - default_outliers(N), N) if out_idx is None else np.asarray(sorted(out_idx), np.int64)
    n_out = len(out_idx)
    target, inl, Rgt, tgt = synth.make_pair(seed=seed, M=M, N=N - n_out, noise=noise)
    R0 = (rodrigues64(START_ROT) @ Rgt).astype(np.float32)
    t0 = (tgt + START_SHIFT).astype(np.float32)
    k = np.arange(n_out, dtype=np.float64)
    # a golden-angle spiral: directions all over the sphere, no two alike
    z = 1 - 2 * (k + 0.5) / max(n_out, 1)
    phi = k * np.pi * (3 - np.sqrt(5))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    far = dirs * (1.3 + 0.2 * (k[:, None] + 0.5) / max(n_out, 1))
    far_src = (far - t0.astype(np.float64)) @ R0.astype(np.float64)          # R0 s + t0 = far
    source = np.empty((N, 3), np.float32)
    keep = np.ones(N, bool)
    keep[out_idx] = False
    source[keep] = inl
    source[out_idx] = far_src.astype(np.float32)
    extent = float(max((target.max(0) - target.min(0)).max(), (source.max(0) - source.min(0)).max()))
    return dict(target=target, source=np.ascontiguousarray(source), R0=R0, t0=t0, out_idx=out_idx, extent=extent, M=M, N=N)


def pick_gate(d, far=None):
    """A gate from the distances d.  With far points (their places in `far`): halfway between the largest distance of the others and the
    smallest of theirs.  Without: the middle of the widest gap inside the central half of the sorted distances (twice the distance for a
    single point).  -> (gate as the float the engine holds, the distance of the nearest d from it)"""
    d = np.asarray(d, np.float64)
    if far is not None and len(far):
        mask = np.zeros(len(d), bool)
        mask[far] = True
        g = 0.5 * ((d[~mask].max() if (~mask).any() else 0.0) + d[mask].min())
    elif len(d) == 1:
        g = 2.0 * d[0]
    else:
        s = np.sort(d)
        a, b = len(s) // 4, max(len(s) // 4 + 2, 3 * len(s) // 4)
        j = a + int(np.argmax(np.diff(s[a:b])))
        g = 0.5 * (s[j] + s[j + 1])
    g = float(np.float32(g))
    return g, float(np.abs(d - g).min())


def kabsch_weighted_f64(target, q, idx, w, R0, t0):
    """One weighted Kabsch step in float64 from correspondences (q = the moved source, target[idx] its neighbours, w the weights): the
    weighted means, H = sum w (q - mu_q)(m - mu_m)^T, R = V diag(1, 1, det) U^T, composed with the start pose.
    -> (R, t, singular values of H, descending)"""
    q, m, w = q.astype(np.float64), target[idx].astype(np.float64), np.asarray(w, np.float64)
    W = w.sum()
    mu_q, mu_m = (w[:, None] * q).sum(0) / W, (w[:, None] * m).sum(0) / W
    H = (w[:, None] * (q - mu_q)).T @ (m - mu_m)
    U, S, Vt = np.linalg.svd(H)
    Rs = Vt.T @ np.diag([1.0, 1.0, np.linalg.det(Vt.T @ U.T)]) @ U.T
    ts = mu_m - Rs @ mu_q
    return Rs @ np.asarray(R0, np.float64), Rs @ np.asarray(t0, np.float64) + ts, S


def kabsch_condition(target, q, idx, w=None):
    """sigma_3 / sigma_1 of the (weighted) covariance the Kabsch step decomposes"""
    w = np.ones(len(q)) if w is None else w
    S = kabsch_weighted_f64(target, q, idx, w, np.eye(3), np.zeros(3))[2]
    return float(S[2] / S[0]) if S[0] > 0 else 0.0


def plane_condition(q, m_normals, pivot):
    """lambda_min / lambda_max of the point-to-plane step's 6x6 normal matrix J^T J, J = [(q - pivot) x n, n]"""
    a = q.astype(np.float64) - pivot
    n = m_normals.astype(np.float64)
    J = np.concatenate([np.cross(a, n), n], 1)
    lam = np.linalg.eigvalsh(J.T @ J)
    return float(lam[0] / lam[-1]) if lam[-1] > 0 else 0.0


def trans_radius(w_child):
    """maxTransDis of a child cube of width w, the oracle's and the engine's float constant"""
    return float(np.float32(1.732050808 / 2.0 * float(np.float32(w_child))))


def bound_ref(m, w_child, trunc=0.0, inliers=None):
    """(ub, lb) in float64 from the per-point residuals m = max(DT - rho, 0) (float32, oracle.cube_terms) of one cube:
    ub = sum m^2, lb = sum max(m - delta, 0)^2; inliers: over the `inliers` smallest m only; trunc = g > 0: every term clamped at g after
    its subtractions, min(m, g)^2 and min(max(m - delta, 0), g)^2."""
    m = np.asarray(m, np.float32).astype(np.float64)
    if inliers is not None and inliers < len(m):
        m = np.partition(m, inliers - 1)[:inliers]
    dis = np.maximum(m - trans_radius(w_child), 0.0)
    if trunc > 0:
        g = float(np.float32(trunc))
        m, dis = np.minimum(m, g), np.minimum(dis, g)
    return float(np.sum(m * m)), float(np.sum(dis * dis))
