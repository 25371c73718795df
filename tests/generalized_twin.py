"""Twin of generalized (plane-to-plane) ICP (goicp_set_icp_generalized; include/goicp_mi355.h).

weight32: s, Sigma, the six cofactors, the determinant and W = 2 eps Sigma^-1 in numpy float32, operation by operation in the header's
order -- the bits the device must hold.  system64: everything after W (g, b, [a]x W, H) in fp64 on those float inputs.  step64: one damped
Gauss-Newton iteration about the pivot, the solve of tests/test_gpu_icp_symmetric.py's _twin_step."""
import numpy as np

f32 = np.float32


def rodrigues64(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * (W @ W)


def q32(R, t, p):
    """the engine's float expression of q = R p + t, left to right"""
    R, t, p = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32), np.asarray(p, f32)
    return np.stack([((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a] for a in range(3)], 1).astype(f32)


def rotate32(R, ns):
    """s = R ns by the row expression of q without t"""
    R, ns = np.asarray(R, f32).reshape(3, 3), np.asarray(ns, f32)
    return np.stack([(R[a, 0] * ns[:, 0] + R[a, 1] * ns[:, 1]) + R[a, 2] * ns[:, 2] for a in range(3)], 1).astype(f32)


def sigma32(s, u, eps):
    """the six unique entries of Sigma = 2 I - (1 - eps) (u u^T + s s^T): (Sxx, Sxy, Sxz, Syy, Syz, Szz), float32"""
    s, u = np.asarray(s, f32), np.asarray(u, f32)
    k = f32(1) - f32(eps)
    two = f32(2)
    diag = lambda i: (two - k * (u[:, i] * u[:, i] + s[:, i] * s[:, i])).astype(f32)
    off = lambda i, j: (-(k * (u[:, i] * u[:, j] + s[:, i] * s[:, j]))).astype(f32)
    return diag(0), off(0, 1), off(0, 2), diag(1), off(1, 2), diag(2)


def weight32(R, ns, u, eps, s=None):
    """W = 2 eps Sigma^-1 from the cofactors and one determinant -> (N, 6) float32: W00, W01, W02, W11, W12, W22.
    s: the rotated source normals where the caller has them already (else R ns)"""
    s = rotate32(R, ns) if s is None else np.asarray(s, f32)
    Sxx, Sxy, Sxz, Syy, Syz, Szz = sigma32(s, u, eps)
    h = f32(2) * f32(eps)
    C00 = (Syy * Szz - Syz * Syz).astype(f32)
    C01 = (Sxz * Syz - Sxy * Szz).astype(f32)
    C02 = (Sxy * Syz - Sxz * Syy).astype(f32)
    C11 = (Sxx * Szz - Sxz * Sxz).astype(f32)
    C12 = (Sxy * Sxz - Sxx * Syz).astype(f32)
    C22 = (Sxx * Syy - Sxy * Sxy).astype(f32)
    det = ((Sxx * C00 + Sxy * C01) + Sxz * C02).astype(f32)
    return np.stack([((h * c) / det).astype(f32) for c in (C00, C01, C02, C11, C12, C22)], 1)


def full(W6):
    """(N, 6) -> (N, 3, 3) symmetric, fp64"""
    W6 = np.asarray(W6, np.float64)
    W = np.empty((len(W6), 3, 3))
    for k, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        W[:, i, j] = W[:, j, i] = W6[:, k]
    return W


def skew(a):
    a = np.asarray(a, np.float64)
    z = np.zeros(len(a))
    return np.stack([np.stack([z, -a[:, 2], a[:, 1]], 1), np.stack([a[:, 2], z, -a[:, 0]], 1), np.stack([-a[:, 1], a[:, 0], z], 1)], 1)


def system64(W6, a, e):
    """per correspondence, fp64: H (N, 6, 6) = [[ [a]x W [a]x^T, [a]x W ], [., W]] and b (N, 6) = (a x g, g), g = W e; e' = e + omega x a + tau"""
    W, A = full(W6), skew(a)
    e = np.asarray(e, np.float64)
    M = A @ W
    H = np.zeros((len(W), 6, 6))
    H[:, :3, :3] = M @ np.transpose(A, (0, 2, 1))
    H[:, :3, 3:] = M
    H[:, 3:, :3] = np.transpose(M, (0, 2, 1))
    H[:, 3:, 3:] = W
    g = np.einsum("nij,nj->ni", W, e)
    return H, np.concatenate([np.cross(np.asarray(a, np.float64), g), g], 1)


def step64(reg, source, target, R, t, eps, weight=None, ns=None, nm=None, W6=None):
    """one generalized iteration: float32 q and W, the rest fp64; the damped solve about the pivot cq (mu = 1e-12 trace).
    weight: None, or a function (d2 float32) -> w per correspondence (the robust weight is of the distance).  ns / nm: source normals and the
    whole target's normals in the place of the handle's; W6: the weights themselves -> (R, t, sum d^2)"""
    R32, t32 = np.asarray(R, f32), np.asarray(t, f32)
    q = q32(R32, t32, source)
    idx, d2 = reg.nn_query(q)
    nm = (reg.target_normals() if nm is None else nm)[idx]
    ns = reg.source_normals() if ns is None else ns
    if W6 is None:
        W6 = weight32(R32, ns, nm, eps)
    R64, t64 = np.asarray(R, np.float64), np.asarray(t, np.float64)
    cq = R64 @ source.astype(np.float64).mean(0) + t64
    e = q.astype(np.float64) - target[idx].astype(np.float64)
    H, b = system64(W6, q.astype(np.float64) - cq, e)
    w = np.ones(len(q)) if weight is None else weight(d2)
    A, g = np.einsum("n,nij->ij", w, H), np.einsum("n,ni->i", w, b)
    A = A + 1e-12 * np.trace(A) * np.eye(6)
    x = np.linalg.solve(A, -g)
    dR = rodrigues64(x[:3])
    return dR @ R64, dR @ (t64 - cq) + cq + x[3:], float(np.sum(d2.astype(np.float64)))
