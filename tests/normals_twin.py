"""The numpy twin of the exact self k-NN and of the normal estimation (include/goicp_mi355.h), the clouds and the grid of cases
that tests/test_normals_host.py and tests/test_gpu_normals.py share.  The twin is brute force over all pairs, in row chunks, vectorised
over the points with element-wise float64 operations (IEEE; np.sqrt and the division are correctly rounded), and shares nothing with the
library but the rule, which it follows line by line:
  pair     dx = x_i - x_j, dy, dz likewise; d2 = dx*dx + dy*dy + dz*dz in float32, left to right; a point is never its own neighbour;
  order    key = bits(d2) << 32 | j as uint64, ascending; row i = the k smallest keys;
  offsets  e_j = float64(x_j) - float64(x_i), the point itself first; m = (sum e_j) / k, added in order from 0;
  cov      d_j = e_j - m; six sums of rounded products, added in order from 0;
  eigen    cyclic Jacobi over (0,1), (0,2), (1,2) on the full matrix, the header's skip rule, rotation and stop test, at most 32 sweeps;
  normal   the column of V of the smallest diagonal entry (lowest index on ties), divided by sqrt((v0*v0 + v1*v1) + v2*v2), cast to float32;
  flat     largest entry <= 0: normal 0, variation 0;   variation  float32(max(a, 0) / ((a + b) + c)), a <= b <= c;
  sign     d = the float64 dot of the float32 normal with (vp - x_i), left to right; d < 0 flips; no viewpoint or d == 0: the first
           non-zero component is made positive; zero components are +0.
It knows no grid."""
import functools

import numpy as np

import stat_outlier_twin as ST

SIZES = ST.SIZES
KINDS = ST.KINDS
MAX_K = 32
MAX_SWEEPS = 32
KNN_KS = (1, 5, 16, 32)
NORMAL_KS = (3, 4, 16, 32)

make_cloud = ST.make_cloud
same_bits = ST.same_bits


def knn_ks_for(n):
    return sorted({k for k in KNN_KS + (n - 1,) if 1 <= k <= min(MAX_K, n - 1)})


def normal_ks_for(n):
    return [k for k in NORMAL_KS if k - 1 <= n - 1]


def knn_keys(xyz, kmax, chunk=256):
    """the kmax smallest keys of every point, ascending (n, kmax) uint64: all pairs, the header's expression"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    assert 1 <= kmax <= n - 1
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    col = np.arange(n, dtype=np.uint64)[None, :]
    out = np.empty((n, kmax), np.uint64)
    with np.errstate(under="ignore"):
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            dx, dy, dz = x[a:b, None] - x[None, :], y[a:b, None] - y[None, :], z[a:b, None] - z[None, :]
            d2 = dx * dx + dy * dy + dz * dz
            assert d2.dtype == np.float32 and np.all(np.isfinite(d2))
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | col
            key[np.arange(b - a), np.arange(a, b)] = np.uint64(2 ** 64 - 1)
            out[a:b] = np.sort(np.partition(key, kmax - 1, axis=1)[:, :kmax], axis=1)
    assert out.max() < np.uint64(2 ** 64 - 1)
    return out


@functools.lru_cache(maxsize=None)
def keys_of(kind, n):
    """computed once per cloud of the grid, shared, never changed"""
    k = knn_keys(make_cloud(kind, n), min(MAX_K, n - 1))
    k.setflags(write=False)
    return k


def split(keys, k):
    """-> (indices (n, k) int32, d2 (n, k) float32) of the first k keys of every row"""
    keys = np.ascontiguousarray(keys[:, :k])
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.int32), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)


def knn_twin(xyz, k, keys=None):
    if keys is None:
        keys = knn_keys(xyz, k)
    return split(keys, k)


def _rotate(A, V, p, q):
    """one Jacobi rotation of the pair (p, q) on every point's matrix; -> the mask of the points that rotated"""
    app, aqq, apq = A[p][p], A[q][q], A[p][q]
    skip = (apq == 0.0) | (apq * apq <= np.float64(1e-24) * np.abs(app * aqq))
    da = aqq - app
    db = apq + apq
    tn = np.where(da >= 0.0, db, -db) / (np.abs(da) + np.sqrt(da * da + db * db))
    cs = np.float64(1.0) / np.sqrt(np.float64(1.0) + tn * tn)
    sn = cs * tn
    keep = lambda new, old: np.where(skip, old, new)
    for r in range(3):
        arp, arq = A[r][p], A[r][q]
        A[r][p], A[r][q] = keep(cs * arp - sn * arq, arp), keep(sn * arp + cs * arq, arq)
    for r in range(3):
        apr, aqr = A[p][r], A[q][r]
        A[p][r], A[q][r] = keep(cs * apr - sn * aqr, apr), keep(sn * apr + cs * aqr, aqr)
    for r in range(3):
        vrp, vrq = V[r][p], V[r][q]
        V[r][p], V[r][q] = keep(cs * vrp - sn * vrq, vrp), keep(sn * vrp + cs * vrq, vrq)
    return ~skip


def pca(xyz, idx, viewpoint=None):
    """normals (n, 3) float32 and variation (n,) float32 of the neighbourhoods {i} + idx[i] (n, k - 1), in that order"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n, kk = idx.shape
    X = xyz.astype(np.float64)
    zero = np.zeros(n)
    with np.errstate(all="ignore"):
        # the offsets, the point itself first
        e = [[zero, zero, zero]] + [[X[idx[:, j], c] - X[:, c] for c in range(3)] for j in range(kk)]
        s = [zero, zero, zero]
        for ej in e:
            s = [s[c] + ej[c] for c in range(3)]
        kd = np.float64(kk + 1)
        m = [s[c] / kd for c in range(3)]
        C = {(a, b): zero for a in range(3) for b in range(a, 3)}
        for ej in e:
            d = [ej[c] - m[c] for c in range(3)]
            for (a, b) in C:
                C[(a, b)] = C[(a, b)] + d[a] * d[b]
        A = [[C[(min(a, b), max(a, b))] for b in range(3)] for a in range(3)]
        V = [[np.full(n, 1.0 if a == b else 0.0) for b in range(3)] for a in range(3)]
        for _ in range(MAX_SWEEPS):
            r01 = _rotate(A, V, 0, 1)
            r02 = _rotate(A, V, 0, 2)
            r12 = _rotate(A, V, 1, 2)
            if not np.any(r01 | r02 | r12):
                break
        lam = np.stack([A[0][0], A[1][1], A[2][2]], 1)
        ks = np.zeros(n, np.int64)
        lmin = lam[:, 0].copy()
        for c in (1, 2):
            lower = lam[:, c] < lmin
            ks[lower] = c
            lmin = np.where(lower, lam[:, c], lmin)
        rows = np.arange(n)
        v = [np.stack([V[r][0], V[r][1], V[r][2]], 1)[rows, ks] for r in range(3)]
        srt = np.sort(lam, axis=1)
        a, b, c = srt[:, 0], srt[:, 1], srt[:, 2]
        flat = ~(c > 0.0)
        var = (np.where(a > 0.0, a, 0.0) / ((a + b) + c)).astype(np.float32)
        length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        nf = np.stack([(v[r] / length).astype(np.float32) for r in range(3)], 1)
        d = np.zeros(n)
        if viewpoint is not None:
            vp = np.asarray(viewpoint, np.float32).astype(np.float64)
            n64 = nf.astype(np.float64)
            d = (n64[:, 0] * (vp[0] - X[:, 0]) + n64[:, 1] * (vp[1] - X[:, 1])) + n64[:, 2] * (vp[2] - X[:, 2])
        lead = np.where(nf[:, 0] != 0, nf[:, 0], np.where(nf[:, 1] != 0, nf[:, 1], nf[:, 2]))
        flip = np.where(d != 0.0, d < 0.0, lead < 0)
        out = np.where(flip[:, None], -nf, nf)
        out = np.where(nf == 0, np.float32(0), out).astype(np.float32)
        out[flat] = 0
        var[flat] = 0
    return out, var


def normals_twin(xyz, k, viewpoint=None, keys=None):
    """-> (normals (n, 3) float32, variation (n,) float32, the neighbours used (n, k - 1) int32)"""
    idx = knn_twin(xyz, k - 1, keys)[0]
    nrm, var = pca(xyz, idx, viewpoint)
    return nrm, var, idx


def viewpoint_of(xyz):
    """a viewpoint of a grid cloud: outside its box, off every axis"""
    xyz = np.asarray(xyz, np.float32)
    ext = np.float32(max(float((xyz.max(0) - xyz.min(0)).max()), 1.0))
    return (xyz.max(0) + ext * np.array([0.5, 1.25, 2.0], np.float32)).astype(np.float32)
