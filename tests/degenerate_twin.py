"""fp64 references and inputs for the ICP pose solvers on planar, linear and singular correspondences
(tests/test_icp_degenerate_host.py, tests/test_gpu_icp_degenerate.py).

kabsch64 / kabsch_objective: the 3x3 SVD step in the convention of device.hip's kabsch_rows, H = U S V^T -> R = V diag(1, 1, d) U^T with
d = sign det(V U^T); tr(R H) = s1 + s2 + d s3 is what that R attains and no rotation exceeds.  R is unique iff the gap (s2 + d s3) / s1 > 0.

min_norm_step: x = -A^+ b over the eigenvalues > rank_tol * lambda_max, the rank rule of information_decompose and pose_information
(default 1e-6) -- the step a 6x6 solve has to return where the Gauss-Newton matrix is rank deficient: no motion along directions the
correspondences say nothing about.

system: (A, b) of one iteration linearised about the pivot cq, fp64 on the float32 q: the expressions of test_gpu_point_to_plane._twin_step
(metric 1), test_gpu_icp_symmetric._twin_step (metric 2) and generalized_twin.system64 (metric 3), WITHOUT their 1e-12 trace shift.
compose: the pose update those functions apply to a step x.

Clouds (float32; every coordinate a multiple of 1/16 before the tilt, the source's in-plane offsets of 1/64):
  plane(tilt)       target: the 17 x 17 lattice of test_plane_point_to_plane_has_rank_three, centred, turned by rodrigues(tilt) in fp64, rounded;
                    source: its points (7 i) mod 289, i < 101, each moved in the plane by (+-1/64, +-1/64) -- the nearest lattice point is
                    3/64 closer along either axis than the next one
  line(tilt)        target: k / 16 along x, k = 0 .. 16; source: points 0, 3, 7, 12, 16
  one_target_point  17 target points, the first at the origin, the rest at distance >= 1 with a centroid away from the origin; five source
                    points within 0.09 of the origin: every correspondence is target point 0 and the covariance H vanishes
  start(tilt)       0.01 along the tilted z axis (the plane's normal; a perpendicular of the line) and a turn of (0.01, -0.02) rad about the tilted
                    x and y axes
"""
import numpy as np

import generalized_twin as T
from generalized_twin import q32, rodrigues64

f32 = np.float32
TILTS = [(0.0, 0.0, 0.0), (0.0, np.pi / 4, 0.0), (0.3, 0.5, 0.1), (0.7, -0.2, 0.4), (1.0, 1.0, 1.0)]
TILT_IDS = ["axis", "y45", "t1", "t2", "t3"]
RANK_TOL = 1e-6          # Engine::kPoseInfoRankTol
GICP_EPS = 1e-3          # EPS of tests/test_gpu_icp_generalized.py
# the rank of the plane's matrix under RANK_TOL, established by tests/test_icp_degenerate_host.py for every tilt and every pose of the twin loop.
# Metric 3: W = 2 eps Sigma^-1 has the eigenvalue 1 along the common normal and eps across it, so the plane's three free directions carry
# eps times an ordinary eigenvalue -- 1.6e-4 of the largest at eps = 1e-3, above the rule: generalized ICP on a plane is full rank
PLANE_RANK = {1: 3, 2: 3, 3: 6}


# ----------------------------------------------------------------------------------------------
# the 3x3 step
# ----------------------------------------------------------------------------------------------
def kabsch64(H):
    """-> (R, s, d) of the float H widened to double"""
    H = np.asarray(H, f32).astype(np.float64).reshape(3, 3)
    U, s, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    return V @ np.diag([1.0, 1.0, d]) @ U.T, s, d


def kabsch_objective(R, H):
    return float(np.trace(np.asarray(R, np.float64).reshape(3, 3) @ np.asarray(H, f32).astype(np.float64).reshape(3, 3)))


def kabsch_optimum(H):
    _, s, d = kabsch64(H)
    return float(s[0] + s[1] + d * s[2])


def kabsch_gap(H):
    """(s2 + d s3) / s1: 0 where the optimal rotation is not unique (H = 0: 0)"""
    _, s, d = kabsch64(H)
    return float((s[1] + d * s[2]) / s[0]) if s[0] > 0 else 0.0


# ----------------------------------------------------------------------------------------------
# the 6x6 step
# ----------------------------------------------------------------------------------------------
def spectrum(A):
    """eigenvalues of the symmetric A over the largest, ascending"""
    w = np.linalg.eigvalsh(0.5 * (A + A.T))
    return w / w[-1]


def min_norm_step(A, b, rank_tol=RANK_TOL):
    """-> (x = -A^+ b over the eigenvalues > rank_tol * lambda_max, rank)"""
    w, V = np.linalg.eigh(0.5 * (A + A.T))
    keep = w > rank_tol * w[-1]
    return -(V[:, keep] / w[keep]) @ (V[:, keep].T @ b), int(keep.sum())


def pivot(source, R, t):
    return np.asarray(R, np.float64) @ source.astype(np.float64).mean(0) + np.asarray(t, np.float64)


def system(metric, source, target, R, t, idx, nm, ns=None, weight=None, eps=GICP_EPS):
    """(A, b) of one iteration at the pose (R, t), correspondences idx into target.  nm: the target normals, ns: the source normals (float32, in
    their clouds' order).  weight: None or a function |r| -> w (metric 1: the robust weight is of the plane residual)"""
    R32, t32 = np.asarray(R, f32), np.asarray(t, f32)
    q = q32(R32, t32, source)
    cq = pivot(source, R, t)
    q64, m = q.astype(np.float64), target[idx].astype(np.float64)
    e, a = q64 - m, q64 - cq
    if metric == 3:
        H, g = T.system64(T.weight32(R32, ns, nm[idx], eps), a, e)
        return H.sum(0), g.sum(0)
    if metric == 2:
        from test_gpu_icp_symmetric import _sym32, _sym64
        _, dot, s0, _ = _sym32(R32, ns, nm[idx])
        n, h = _sym64(R32, ns, nm[idx], dot < 0, s0)
        a = a - h[:, None] * e
    else:
        n = nm[idx].astype(np.float64)
    r = np.sum(e * n, 1)
    J = np.concatenate([np.cross(a, n), n], 1)
    w = np.ones(len(q)) if weight is None else weight(np.abs(r))
    return (w[:, None] * J).T @ J, (w[:, None] * J).T @ r


def compose(source, R, t, x):
    """the pose after the step x = (omega, tau) about the pivot: R <- dR R, t <- dR (t - cq) + cq + tau"""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    cq = pivot(source, R, t)
    dR = rodrigues64(x[:3])
    return dR @ R, dR @ (t - cq) + cq + x[3:]


def finalize_solve(A, b):
    """the present solve of icp_plane_finalize_body, transcribed: mu = 1e-12 trace on the diagonal, Cholesky in place, ok = every pivot > 0,
    the step zero where it is not -> (x, ok, pivots over the trace)"""
    A = np.array(A, np.float64)
    tr = np.trace(A)
    A += 1e-12 * tr * np.eye(6)
    ok = bool(tr > 0.0)
    L, piv = np.zeros((6, 6)), np.zeros(6)
    for j in range(6):
        dj = A[j, j] - np.sum(L[j, :j] ** 2)
        piv[j] = dj
        ok = ok and bool(dj > 0.0)
        L[j, j] = np.sqrt(dj) if ok else 1.0
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    y, x = np.zeros(6), np.zeros(6)
    for i in range(6):
        y[i] = (-b[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(5, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return (x if ok else np.zeros(6)), ok, piv / tr if tr > 0 else piv


def system_f32_terms(source, target, R, t, idx, nm):
    """the metric-1 system as the pass forms it: float32 J about the float32 pivot, float32 products, summed in fp64 (the fixed-point
    rounding of the sums and the workgroup order are left out)"""
    R32, t32 = np.asarray(R, f32), np.asarray(t, f32)
    q = q32(R32, t32, source)
    cq = pivot(source, R, t).astype(f32)
    a, n = (q - cq).astype(f32), nm[idx].astype(f32)
    e = (q - target[idx]).astype(f32)
    r = ((e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]).astype(f32)
    J = np.stack([(a[:, 1] * n[:, 2] - a[:, 2] * n[:, 1]), (a[:, 2] * n[:, 0] - a[:, 0] * n[:, 2]), (a[:, 0] * n[:, 1] - a[:, 1] * n[:, 0]),
                  n[:, 0], n[:, 1], n[:, 2]], 1).astype(f32)
    A = np.array([[np.sum((J[:, i] * J[:, j]).astype(f32).astype(np.float64)) for j in range(6)] for i in range(6)])
    b = np.array([np.sum((J[:, i] * r).astype(f32).astype(np.float64)) for i in range(6)])
    return A, b


# ----------------------------------------------------------------------------------------------
# poses
# ----------------------------------------------------------------------------------------------
def rotvec(R):
    """the rotation vector of a rotation near the identity"""
    R = np.asarray(R, np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    return v if s == 0 else v * (np.arcsin(min(1.0, s)) / s)


def null_motion(R, t, R0, t0, normal):
    """of the motion (R, t) o (R0, t0)^-1: the rotation about `normal` and the translation across it -- what a plane leaves undetermined"""
    R, t, R0, t0 = (np.asarray(x, np.float64) for x in (R, t, R0, t0))
    D = R @ R0.T
    d = t - D @ t0
    return float(rotvec(D) @ normal), d - (d @ normal) * normal


# ----------------------------------------------------------------------------------------------
# clouds
# ----------------------------------------------------------------------------------------------
def frame(tilt):
    return rodrigues64(np.asarray(tilt, np.float64))


def start(tilt):
    """-> (R0, t0) float32"""
    F = frame(tilt)
    return rodrigues64(F @ np.array([0.01, -0.02, 0.0])).astype(f32), (0.01 * F[:, 2]).astype(f32)


def plane(tilt):
    """-> (target (289, 3), source (101, 3), index of each source point's lattice point)"""
    g = np.arange(17, dtype=np.float64) / 16 - 0.5
    P = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    P = np.concatenate([P, np.zeros((len(P), 1))], 1)
    F = frame(tilt)
    i = np.arange(101)
    sel = (7 * i) % len(P)
    off = np.stack([np.where(i % 2 == 0, 1.0, -1.0), np.where((i // 2) % 2 == 0, 1.0, -1.0), np.zeros(len(i))], 1) / 64
    return np.ascontiguousarray((P @ F.T).astype(f32)), np.ascontiguousarray(((P[sel] + off) @ F.T).astype(f32)), sel


def line(tilt):
    """-> (target (17, 3), source (5, 3))"""
    P = np.zeros((17, 3))
    P[:, 0] = np.arange(17) / 16
    tgt = np.ascontiguousarray((P @ frame(tilt).T).astype(f32))
    return tgt, np.ascontiguousarray(tgt[[0, 3, 7, 12, 16]])


def one_target_point():
    """-> (target (17, 3), source (5, 3)): every source point's nearest target point is point 0, at any pose near the identity"""
    far = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
    far += [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (-1, 0, 0), (0, -1, 0)]
    tgt = np.array([(0, 0, 0)] + far, f32)
    src = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)], f32) / f32(16)
    return tgt, src


def covariance(source, target, R, t, idx):
    """the point-to-point covariance H = sum (q - mean q)(m - mean m)^T of the correspondences, fp64 on the float32 q"""
    q = q32(R, t, source).astype(np.float64)
    m = target[idx].astype(np.float64)
    return (q - q.mean(0)).T @ (m - m.mean(0))


# ----------------------------------------------------------------------------------------------
# the 3x3 cases: name -> H (float32, 9)
# ----------------------------------------------------------------------------------------------
KABSCH_U = rodrigues64([0.4, -0.7, 0.2])
KABSCH_V = rodrigues64([-0.3, 0.5, 0.9])
KABSCH_S = {
    "rank2": (1, .5, 0), "s3=+1e-8": (1, .5, 1e-8), "s3=-1e-8": (1, .5, -1e-8), "reflect": (1, .5, -.4),
    "tie12+": (1, 1, .5), "tie12-": (1, 1, -.5), "tie23+": (1, .5, .5), "tie23-": (1, .5, -.5),
    "tie123+": (1, 1, 1), "tie123-": (1, 1, -1), "near-tie12": (1, 1 - 1e-6, .5), "rank1": (1, 0, 0), "near-rank1": (1, 1e-8, 1e-9),
}
KABSCH_SCALED = ["rank2", "s3=+1e-8", "s3=-1e-8", "reflect"]


def kabsch_cases():
    """-> {name: H}: U diag(s) V^T from fixed rotations, built in fp64 and rounded; the first four also at scale 1e-30 and 1e+30; the exact forms"""
    out = {}
    for name, s in KABSCH_S.items():
        out[name] = (KABSCH_U @ np.diag(np.array(s, np.float64)) @ KABSCH_V.T).astype(f32).reshape(9)
    for name in KABSCH_SCALED:
        for tag, scale in (("e-30", 1e-30), ("e+30", 1e+30)):
            out[name + "@1" + tag] = ((KABSCH_U @ np.diag(np.array(KABSCH_S[name], np.float64)) @ KABSCH_V.T) * scale).astype(f32).reshape(9)
    for z in range(3):                                             # diag(1, .5, 0), the zero column in each position
        d = [1.0, 0.5]
        d.insert(z, 0.0)
        out["diag-zero%d" % z] = np.diag(d).astype(f32).reshape(9)
        H = np.diag(d)
        nz = [k for k in range(3) if k != z]
        H[nz[1], nz[1]] = -H[nz[1], nz[1]]                          # a sign flip in the 2 x 2 block
        out["diag-zero%d-flip" % z] = H.astype(f32).reshape(9)
    for i in range(3):
        for j in range(3):
            H = np.zeros((3, 3), f32)
            H[i, j] = 1
            out["e%d e%d^T" % (i, j)] = H.reshape(9)
    return out
