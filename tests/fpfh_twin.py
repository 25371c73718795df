"""The numpy twin of the FPFH descriptors and of the descriptor matching (include/goicp_mi355.h), the clouds and the grid of
cases that tests/test_fpfh_host.py and tests/test_gpu_fpfh.py share.  The twin is vectorised over all (point, neighbour) pairs with
element-wise float64 operations (IEEE; np.sqrt and the division are correctly rounded; numpy fuses nothing) and shares nothing with the
library but the rule and the header's table of (C_k, S_k), which it parses from the header's hex-float literals:
  rows     the self k-NN of normals_twin (brute force over all pairs), key order, with its float32 d2;
  pair     d = p_j - p_i; l2 = (d0*d0 + d1*d1) + d2*d2; skipped unless l2 > 0 and both normals have a non-zero component;
           a1 = (n_i . d) / sqrt(l2), a2 = (n_j . d) / sqrt(l2); |a1| < |a2| exchanges the normals, negates d and takes f3 = -a2, else
           f3 = a1; v = d x ns; skipped unless vl2 > 0; v / sqrt(vl2); w = ns x v; f2 = v . nt; x = ns . nt; y = w . nt;
  bins     clip(floor(11 * ((f + 1) * 0.5)), 0, 10) for f2 and f3; theta by the table rule: (a, b) = (-x, -y), cross_k = C_k*b - S_k*a,
           the count of k <= 5 with b < 0 or cross_k >= 0 plus the count of k >= 6 with b < 0 and cross_k >= 0; 5 when x == y == 0;
  SPFH     integer counts per point in the layout theta 0..10, f2 11..21, f3 22..32;
  FPFH     inc = 100 / k; a_b = the sum over the row from 0 of ((c_jb * inc) * (1 / d2_j)), neighbours at d2 == 0 left out; each group of 11
           scaled by 100 / (its sum, added ascending from 0) when that is > 0; float32(a_b + c_ib * inc);
  match    d2 = the float32 sum over b = 0..32 of (q_b - t_b)^2 from 0, left to right; key = bits(d2) << 32 | t; the smallest key, the d2 of
           the second smallest (+inf with one target), and mutual = the same rule backwards returns the query."""
import os
import re

import numpy as np

import normals_twin as NT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 33
BINS = 11
SIZES = [2, 3, 33, 64, 65, 257, 1000]
KS = (1, 2, 16, 17, 32)
MATCH_SIZES = [1, 2, 63, 64, 65, 255, 256, 257]
KINDS = NT.KINDS

make_cloud = NT.make_cloud
same_bits = NT.same_bits


def header_table():
    """(C, S): the header's twenty hex-float literals, k = 1..10"""
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    out = []
    for name in ("GOICP_FPFH_COS", "GOICP_FPFH_SIN"):
        m = re.search(r"#define %s \{([^}]*)\}" % name, hdr)
        vals = [float.fromhex(v.strip()) for v in m.group(1).replace("\\", " ").split(",")]
        assert len(vals) == 10
        out.append(np.array(vals, np.float64))
    return out[0], out[1]


COS, SIN = header_table()


def ks_for(n):
    return sorted({k for k in KS + (n - 1,) if 1 <= k <= min(NT.MAX_K, n - 1)})


def unit_normals(n, seed):
    """n float32 normals of length 1 up to the rounding, none along an axis"""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1)[:, None], np.float32)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def theta_bin(x, y):
    a, b = -x, -y
    count = np.zeros(x.shape, np.int64)
    for k in range(1, 11):
        turn = (COS[k - 1] * b - SIN[k - 1] * a) >= 0.0
        count += ((b < 0.0) | turn) if k <= 5 else ((b < 0.0) & turn)
    return np.where((x == 0.0) & (y == 0.0), 5, count)


def bin11(f):
    t = np.floor(np.float64(11.0) * ((f + np.float64(1.0)) * np.float64(0.5)))
    return np.clip(np.where(np.isnan(t), 0.0, t), 0.0, 10.0).astype(np.int64)


def pair_features(xyz, nrm, idx):
    """every pair (i, idx[i, j]) -> dict of (n, k) arrays: skip, b1, b2, b3 and the f2, f3, x, y they came from"""
    xyz, nrm = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
    P, N = xyz.astype(np.float64), nrm.astype(np.float64)
    shape = idx.shape
    pi, pj = [np.broadcast_to(P[:, c, None], shape) for c in range(3)], [P[idx, c] for c in range(3)]
    ni, nj = [np.broadcast_to(N[:, c, None], shape) for c in range(3)], [N[idx, c] for c in range(3)]
    d = [pj[c] - pi[c] for c in range(3)]
    l2 = _dot(d, d)
    zero = ~(nrm != 0).any(1)
    skip = ~(l2 > 0.0) | zero[:, None] | zero[idx]
    with np.errstate(all="ignore"):
        l = np.sqrt(l2)
        a1, a2 = _dot(ni, d) / l, _dot(nj, d) / l
        swap = np.abs(a1) < np.abs(a2)
        ns, nt = [np.where(swap, nj[c], ni[c]) for c in range(3)], [np.where(swap, ni[c], nj[c]) for c in range(3)]
        d = [np.where(swap, -d[c], d[c]) for c in range(3)]
        f3 = np.where(swap, -a2, a1)
        v = [d[1] * ns[2] - d[2] * ns[1], d[2] * ns[0] - d[0] * ns[2], d[0] * ns[1] - d[1] * ns[0]]
        vl2 = _dot(v, v)
        skip = skip | ~(vl2 > 0.0)
        vl = np.sqrt(vl2)
        v = [v[c] / vl for c in range(3)]
        w = [ns[1] * v[2] - ns[2] * v[1], ns[2] * v[0] - ns[0] * v[2], ns[0] * v[1] - ns[1] * v[0]]
        f2, x, y = _dot(v, nt), _dot(ns, nt), _dot(w, nt)
        b1, b2, b3 = theta_bin(x, y), bin11(f2), bin11(f3)
    return {"skip": skip, "b1": b1, "b2": b2, "b3": b3, "f2": f2, "f3": f3, "x": x, "y": y}


def spfh_counts(xyz, nrm, idx):
    n, k = idx.shape
    f = pair_features(xyz, nrm, idx)
    counts = np.zeros((n, DIM), np.int64)
    rows = np.broadcast_to(np.arange(n)[:, None], (n, k))
    ok = ~f["skip"]
    for base, name in ((0, "b1"), (BINS, "b2"), (2 * BINS, "b3")):
        np.add.at(counts, (rows[ok], base + f[name][ok]), 1)
    return counts


def fpfh_twin(xyz, nrm, k, keys=None):
    """-> (descriptors (n, 33) float32, SPFH counts (n, 33) uint8)"""
    idx, d2 = NT.knn_twin(xyz, k, keys)
    counts = spfh_counts(xyz, nrm, idx)
    n = len(idx)
    inc = np.float64(100.0) / np.float64(k)
    a = np.zeros((n, DIM), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):      # a neighbour at d2 == 0: its term is formed and left out
        for j in range(k):
            w = np.float64(1.0) / d2[:, j].astype(np.float64)
            term = (counts[idx[:, j]].astype(np.float64) * inc) * w[:, None]
            a = np.where((d2[:, j] == 0)[:, None], a, a + term)
    for g in range(3):
        s = np.zeros(n, np.float64)
        for b in range(BINS):
            s = s + a[:, g * BINS + b]
        with np.errstate(all="ignore"):
            scale = np.float64(100.0) / s
            for b in range(BINS):
                a[:, g * BINS + b] = np.where(s > 0.0, a[:, g * BINS + b] * scale, a[:, g * BINS + b])
    out = (a + counts.astype(np.float64) * inc).astype(np.float32)
    return out, counts.astype(np.uint8)


def match_keys(fq, ft):
    """(n_q, n_t) uint64 keys of all pairs"""
    fq, ft = np.ascontiguousarray(fq, np.float32).reshape(-1, DIM), np.ascontiguousarray(ft, np.float32).reshape(-1, DIM)
    acc = np.zeros((len(fq), len(ft)), np.float32)
    with np.errstate(over="ignore"):
        for b in range(DIM):
            d = fq[:, b, None] - ft[None, :, b]
            acc = acc + d * d
    assert acc.dtype == np.float32
    return (acc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(ft), dtype=np.uint64)[None, :]


def match_twin(fq, ft):
    """-> (index (n_q,) int32, d2 (n_q,) float32, d2 of the second (n_q,) float32, mutual (n_q,) uint8)"""
    keys = np.sort(match_keys(fq, ft), axis=1)
    split = lambda col: ((col & np.uint64(0xFFFFFFFF)).astype(np.int32), (col >> np.uint64(32)).astype(np.uint32).view(np.float32))
    idx, d2 = split(keys[:, 0])
    second = split(keys[:, 1])[1] if keys.shape[1] > 1 else np.full(len(keys), np.inf, np.float32)
    back = split(match_keys(ft, fq).min(axis=1))[0]
    return idx, d2, second, (back[idx] == np.arange(len(idx))).astype(np.uint8)


# ----------------------------------------------------------------------------------------------
# constructed clouds: name -> (xyz, normals, k)
# ----------------------------------------------------------------------------------------------
def constructed():
    rng = np.random.default_rng(25)
    out = {}
    base = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    dup = np.ascontiguousarray(np.concatenate([base, base, base[:20]]))
    out["duplicates"] = (dup, np.ascontiguousarray(np.concatenate([unit_normals(50, 1), unit_normals(50, 2), unit_normals(20, 3)])), 8)
    g = np.arange(6, dtype=np.float32)
    lat = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    axis = (lat[:, 0] + 2 * lat[:, 1] + 3 * lat[:, 2]).astype(np.int64) % 3
    sign = np.where(lat.sum(1).astype(np.int64) % 2 == 1, -1.0, 1.0)
    ln = np.zeros((216, 3), np.float32)
    ln[np.arange(216), axis] = sign
    out["lattice"] = (lat, ln, 6)
    out["lattice 26"] = (lat, ln, 26)
    plane = np.ascontiguousarray(np.concatenate([rng.uniform(-1, 1, (300, 2)), np.full((300, 1), 0.375)], 1), np.float32)
    up = np.tile(np.float32([0, 0, 1]), (300, 1))
    out["plane"] = (plane, up, 10)
    anti = up.copy()
    anti[::2] = -anti[::2]
    out["anti-parallel"] = (plane, anti, 10)
    cloud = rng.uniform(-1, 1, (257, 3)).astype(np.float32)
    some = unit_normals(257, 4)
    some[::5] = 0
    some[3] = np.float32([0, -0.0, 0])
    out["zero normals"] = (cloud, some, 16)
    # points on a line along x with normals along x too (every pair of the line has vl2 == 0), among others off it
    line = np.zeros((40, 3), np.float32)
    line[:, 0] = np.arange(40, dtype=np.float32) * np.float32(0.25)
    along = np.tile(np.float32([1, 0, 0]), (40, 1))
    off = rng.uniform(-1, 1, (60, 3)).astype(np.float32) + np.float32([5, 3, 0])
    out["normal along d"] = (np.ascontiguousarray(np.concatenate([line, off])), np.ascontiguousarray(np.concatenate([along, unit_normals(60, 5)])), 4)
    return out


def descriptors(n, seed):
    """n random float32 descriptors in [0, 100)"""
    return np.random.default_rng(seed).uniform(0, 100, (n, DIM)).astype(np.float32)
