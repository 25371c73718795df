"""The LDS-tile bound kernel (bounds_tile_kernel, csrc/device.hip) in its stand-alone launch (goicp_debug_bounds_tile) at edge shapes: source
sizes on and around the 64-point sub-patch and the 4 wavefronts x L lane-group deal, every lane split P = 1 .. 64 with and without dead lanes,
1 to 3 (and 129) point chunks, chunks without a patch, thin and long boxes, coincident nodes, two depths in a segment, the grid's edge and beyond.
EVERY child of every expansion of every segment, in both passes (level -1: the no-subtract loop; level 5), is held to the float64 sum of the
oracle's per-point terms (oracle.cube_terms, twins.bound_ref) -- the tile kernel's sums and the direct kernel's of the same call -- and every
case asserts which path its sub-patches took: the kernel's counters (stats: staged in LDS / fallen back to the gathers) are held EXACTLY to
predict_paths -- the kernel's float32 box rule on the oracle's grid geometry and the engine's point order (goicp_source_order_host), per
sub-patch: staged, inside the grid but too large for the tile, or over the grid's edge -- and each test asserts on top what its cases are there
for (all staged, none staged, both; at the grid's faces: sub-patches inside AND sub-patches over the edge in the same segment).

Reference and data are test_gpu_small_shapes': the 2 000-point target, synth.make_pair(SEED, 2000, N, noise = 0.002) sources, ROTS, LEVEL 5.
Two grids, because the staged path depends on the DT box of a sub-patch fitting 8 192 floats (checked with the oracle's geometry on the CPU):
  dt_size 32  a 4x4x4 block of width-1/64 nodes with its corner in [-0.15, 0.15 - 4/64]^3: the box of the WHOLE rotated cloud is at most 7 752
              voxels and inside the grid for every N here and all three rotations, so every sub-patch is staged: stats[0] > 0, stats[1] == 0
  dt_size 64  the whole-cloud box of that block is ~40 000 voxels, but a sub-patch of one to three points still fits (128 voxels), and so may
              any 64 points out of 65 .. 257.  For N <= 257 the nodes are therefore spread ("wide": the first two are opposite corners of
              [-0.45, 0.45]^3, the rest a lattice of pitch 0.3 between them): the box of a SINGLE point is then at least 11 616 voxels, so no
              sub-patch of any point order can be staged: stats[0] == 0, stats[1] > 0, all inside the grid for two of the rotations.  One node
              alone (n = 1) cannot be spread; there the node lies at x = 2.6, every point beyond the grid's end (1.59): the fallback with the
              out-of-grid extension.  At N = 8 193 the engine stages every 64-point sub-patch of the tight block (387 of 387: consecutive
              points of its order lie close together), so the block is pushed to the grid's high x face instead (nodes_block_at_edge): the
              sub-patches that reach over the edge fall back whole, the others are staged: stats[0] > 0 and stats[1] > 0 (328 .. 342 | 45 .. 59).

The bar of tile against oracle is min(TOL_TILE, ceiling): the ceiling is the worst case of the case's own summation, (r + log2 L + 3 + 4) x 2^-24
relative with floor max(ref, 1e-3): r = ceil(chunk points / (4 L)) sequential additions per lane, the lane-group shuffles, the three
wavefront additions and four roundings for forming a term.  TOL_TILE is TOL (2e-6) when the worst deviation measured on MI355X over this file
is <= 1e-6, else twice that worst rounded up to one digit (never above 1e-5).  Measured: 9.0e-7 (dt_size 32, N 8 193, n 64, 129 chunks), so
TOL_TILE = TOL; the ceiling is the smaller of the two for every case of r + log2 L <= 26.  N = 8 193 runs in 16 and 129 chunks: at most 132
sequential additions per lane.  (In 4 chunks a lane adds 528 terms one after the other and the same case measures 1.78e-6, inside its own
ceiling of 3.2e-5; by the rule above that one case would put the bar of every case of the file at 4e-6, so the long run is left out.)
Direct against oracle: TOL = 2e-6.  Measured worst deviations on MI355X (tile | direct):
  dt_size 32 block      9.0e-7 | 2.8e-7        dt_size 64 wide / edge block   7.8e-7 | 2.7e-7
  rows, same node, two depths  8.2e-7 | 2.7e-7  grid edge and beyond           2.1e-7 | 2.1e-7      truncated   6.0e-7 | 2.2e-7
Every test prints its worst deviation.

No defect was found: every case passed as first measured.

Teeth (done once on scratch copies of device.hip / bnbqueue.hip, on MI355X, the whole GPU suite per mutant; every mutant reads valid memory only):
  A  the tile loops' `j < np` -> `j < np - 1` when np < 64, the last point of a ragged sub-patch dropped:  6 of the 998 earlier tests fail, 148 of
     the 154 here and 69 of the 70 of test_gpu_bounds_tile_queue
  B  the lane-group reduction starts at off = 2 P, one lane group's sums lost for n <= 32:                 20 of the 998 earlier tests fail, 78 of
     the 154 here and 30 of the 70 of test_gpu_bounds_tile_queue
  C, D: queued form and digest, see test_gpu_bounds_tile_queue.
Wall time on MI355X: this file and test_gpu_bounds_tile_queue together 6.4 s (224 tests, the slowest 0.3 s); the GPU suite without them 291 s.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import twins
from conftest import load_pkg
from test_gpu_scale_parity import TOL
from test_gpu_search_trunc import _children
from test_gpu_small_shapes import LEVEL, M_ICP, ROTS, SEED, _bounds_target

pytestmark = pytest.mark.gpu
INVALID = -1
TOL_TILE = TOL      # the worst deviation measured over this file is <= 1e-6 (see above): the direct kernel's bar
TRUNC_G = 0.05
W64 = np.float32(1.0 / 64)
N_ALL = [1, 2, 3, 5, 63, 64, 65, 127, 129, 255, 257, 8193]
N_FEW = [5, 65, 257]
n_ALL = [1, 2, 3, 16, 17, 31, 32, 33, 63, 64]
n_FEW = [1, 17, 64]
NN = sorted({(N, n) for N in N_ALL for n in n_FEW} | {(N, n) for N in N_FEW for n in n_ALL})


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@functools.lru_cache(maxsize=None)
def _dt(V):
    import oracle
    target, dt64 = _bounds_target()
    return dt64 if V == 64 else oracle.DistanceTransform(target, V, 2.0)


@functools.lru_cache(maxsize=None)
def _source(N):
    """the source of N points, its rotation radii and its three rotated copies (oracle arithmetic): read-only"""
    import oracle as O
    pkg = load_pkg()
    from cuda_go_icp_amd import synth
    source = synth.make_pair(seed=SEED, M=M_ICP, N=N, noise=0.002)[1]
    _, rho = O.rot_radii(source)
    rots = np.stack([pkg.fgoicp.rodrigues(v) for v in ROTS]).astype(np.float32)
    prots = [O.rotate(R, source) for R in rots]
    for a in [source, rho, rots] + prots:
        a.setflags(write=False)
    return source, rho, rots, prots


@functools.lru_cache(maxsize=None)
def _ref_node(N, V, ri, level, node):
    """float64 (ub, lb) of the 8 children of one translation node (corner xyz, width) under rotation ROTS[ri]: [truncated 0 / 1][ub / lb][child]"""
    import oracle as O
    _, rho, _, prots = _source(N)
    out = np.empty((2, 2, 8))
    for c, kid in enumerate(_children(node)):
        m = O.cube_terms(_dt(V), prots[ri], rho[level] if level >= 0 else None, kid[:3], kid[3])
        out[0, :, c] = twins.bound_ref(m, kid[3])
        out[1, :, c] = twins.bound_ref(m, kid[3], TRUNC_G)
    out.setflags(write=False)
    return out


def ref_bounds(N, V, ri, level, nodes, trunc=False):
    """-> (ub, lb) float64 of 8 len(nodes) children, in the order of the nodes"""
    r = np.stack([_ref_node(N, V, ri, level, tuple(float(x) for x in nd))[1 if trunc else 0] for nd in nodes])     # (n, 2, 8)
    return r[:, 0, :].reshape(-1), r[:, 1, :].reshape(-1)


class Regs:
    """the handles of this module, one per (N, dt_size), made on first use and closed with the module"""

    def __init__(self, pkg):
        self.pkg, self.regs = pkg, {}

    def get(self, N, V, **kw):
        key = (N, V) + tuple(sorted(kw.items()))
        if key not in self.regs:
            self.regs[key] = self.pkg.Registration(_bounds_target()[0], _source(N)[0], 1e-3, dt_size=V, **kw)
        return self.regs[key]

    def close(self):
        for r in self.regs.values():
            r.close()
        self.regs.clear()


@pytest.fixture(scope="module")
def regs(pkg):
    r = Regs(pkg)
    yield r
    r.close()


# ----------------------------------------------------------------------------------------------
# node layouts: (nseg, n, 4) corners + widths, float32; segment i is evaluated under rotation i
# ----------------------------------------------------------------------------------------------
def nodes_block(seed, n, nseg=3, w=W64):
    """the first n nodes of a 4x4x4 block per segment, its corner a multiple of w in [-0.15, 0.15 - 4 w]"""
    rng = np.random.default_rng(seed)
    w = np.float32(w)
    par = np.zeros((nseg, n, 4), np.float32)
    for i in range(nseg):
        c0 = (np.floor(rng.uniform(-0.15, 0.15 - 4 * float(w), 3) / w) * w).astype(np.float32)
        for k in range(n):
            par[i, k] = (c0[0] + np.float32(k & 3) * w, c0[1] + np.float32((k >> 2) & 3) * w, c0[2] + np.float32((k >> 4) & 3) * w, w)
    return par


def nodes_block_at_edge(N, V, n, nseg=3, w=W64):
    """the same block pushed towards the grid's high x face, per segment so far that the points of the upper 40 % of the rotated cloud's positive x
    extent reach the last two voxels or leave the grid (their sub-patches fall back whole) and the points on its low side stay well inside"""
    par = nodes_block(N, n, nseg, w)
    dt = _dt(V)
    x_end = dt.origin[0] + dt.V / dt.scale
    for i in range(nseg):
        x_max = float(_source(N)[3][i][:, 0].max())
        c0 = x_end - 2.0 / dt.scale - 0.6 * x_max - 3.75 * float(w)
        par[i, :, 0] += np.float32(np.floor(c0 / float(w)) * float(w)) - par[i, 0, 0]
    return par


def nodes_wide(n, nseg=3):
    """two opposite corners of [-0.45, 0.45]^3 first, then the lattice of pitch 0.3 between them; n = 1: one node at x = 2.6, beyond the grid"""
    if n == 1:
        return np.tile(np.array([2.6, 0.0, 0.0, W64], np.float32), (nseg, 1, 1))
    lat = [(-0.45 + 0.3 * (k & 3), -0.45 + 0.3 * ((k >> 2) & 3), -0.45 + 0.3 * ((k >> 4) & 3)) for k in range(64)]
    order = [0, 63] + [k for k in range(1, 63)]
    one = np.array([lat[k] + (float(W64),) for k in order[:n]], np.float32)
    return np.tile(one, (nseg, 1, 1))


def nodes_row(axis, n=64, nseg=3):
    """n width-1/64 nodes in a row along one axis, from -0.5: thin and long boxes"""
    par = np.zeros((nseg, n, 4), np.float32)
    for i in range(nseg):
        par[i, :, :3] = np.float32(0.01 * (i + 1))
        par[i, :, axis] = np.float32(-0.5) + np.arange(n, dtype=np.float32) * W64
        par[i, :, 3] = W64
    return par


def nodes_same(n=64, nseg=3):
    par = np.zeros((nseg, n, 4), np.float32)
    for i in range(nseg):
        par[i, :] = np.array([0.03125 * i, -0.046875, 0.015625, W64], np.float32)
    return par


def nodes_two_depths(n=64, nseg=3):
    """w = 1/8 and w = 1/512 alternating, corners on each width's own lattice near the origin"""
    par = np.zeros((nseg, n, 4), np.float32)
    for i in range(nseg):
        for k in range(n):
            w = np.float32(1 / 8) if k % 2 == 0 else np.float32(1 / 512)
            q = k // 2
            par[i, k] = (np.float32(-0.25) + np.float32(q & 3) * w, np.float32(-0.125) + np.float32((q >> 2) & 3) * w, np.float32(0.0625 * i) + np.float32((q >> 4) & 1) * w, w)
    return par


def nodes_edge(n=16):
    """three segments: around (1, 0, 0) with w = 1/16 (the grid ends at x ~ 1.59, the rotated cloud reaches x ~ 1.98: sub-patches inside,
    straddling and outside), the mirror image on the low side, and around test_single_point_far_outside_the_grid's cube (50, -40, 30)"""
    w = np.float32(1 / 16)
    par = np.zeros((3, n, 4), np.float32)
    for k in range(n):
        dx, dy = np.float32((k & 3) - 2) * w, np.float32(((k >> 2) & 3) - 2) * w
        par[0, k] = (np.float32(1.0) + dx, dy, np.float32(0.0), w)
        par[1, k] = (np.float32(-1.0) - dx - w, -dy - w, np.float32(-0.0625), w)
        par[2, k] = (np.float32(50.0) + dx, np.float32(-40.0) + dy, np.float32(30.0), np.float32(0.125))
    return par


# ----------------------------------------------------------------------------------------------
# one launch against the oracle
# ----------------------------------------------------------------------------------------------
def ceiling(chunk_pts, n):
    """the worst case of the tile kernel's own summation, relative: r sequential additions per lane, log2 L shuffles, 3 wavefront additions,
    4 roundings per term"""
    P = 1
    while P < n:
        P <<= 1
    L = 64 // P
    r = -(-chunk_pts // (4 * L))
    return (r + math.log2(L) + 3 + 4) * 2.0 ** -24


def standalone_chunk_pts(N, chunks):
    cp = -(-N // chunks)
    return min(N, -(-cp // 64) * 64)


@functools.lru_cache(maxsize=None)
def _engine_order(N):
    """the source as the engine holds it (k-d order, goicp_source_order_host: the default morton_sort = 2), rotated three ways"""
    pkg = load_pkg()
    source, _, rots, _ = _source(N)
    src = source[pkg.fgoicp.source_order(source, 2)]
    out = []
    for R in rots:
        r = R.reshape(9)
        out.append(np.stack([(r[3 * k] * src[:, 0] + r[3 * k + 1] * src[:, 1]) + r[3 * k + 2] * src[:, 2] for k in range(3)], 1).astype(np.float32))
    return out


def predict_paths(N, V, par, chunks, rot_of=None):
    """The path of every sub-patch of a stand-alone launch, from the oracle's grid geometry and the kernel's own float32 box rule (device.hip:
    voxel index floor(((R p + t) - min) * scale + 0.5) of the segment's lowest and highest child translation, a voxel of margin each way, x
    aligned to bricks); segment i under rotation i, or rot_of[i]: -> per segment [staged, inside the grid but larger than 8 192 floats, reaching over the grid's edge]"""
    dt = _dt(V)
    f = np.float32
    org, scale = np.array(dt.origin, np.float64).astype(f), f(dt.scale)
    cp = -(-(-(-N // chunks)) // 64) * 64
    out = []
    for i, seg in enumerate(par):
        w = seg[:, 3] / f(2)
        tlo = (seg[:, :3] + (w / f(2))[:, None]).min(0)
        thi = (seg[:, :3] + w[:, None] + (w / f(2))[:, None]).max(0)
        rp = _engine_order(N)[i if rot_of is None else rot_of[i]]
        cnt = [0, 0, 0]
        for c in range(chunks):
            for s0 in range(c * cp, min(N, (c + 1) * cp), 64):
                q = rp[s0:min(s0 + 64, N, (c + 1) * cp)]
                lo = (np.floor(((q + tlo) - org) * scale + f(0.5)).astype(np.int64) - 1).min(0)
                hi = (np.floor(((q + thi) - org) * scale + f(0.5)).astype(np.int64) + 1).max(0)
                if not ((lo >= 0).all() and (hi <= dt.V - 1).all()):
                    cnt[2] += 1
                    continue
                x0 = int(lo[0]) & ~3
                vol = (((int(hi[0]) | 3) + 1) - x0) * int(hi[1] - lo[1] + 1) * int(hi[2] - lo[2] + 1)
                cnt[0 if vol <= 8192 else 1] += 1
        out.append(cnt)
    return out


def run_tile(pkg, reg, N, V, par, chunks, trunc=False):
    """goicp_debug_bounds_tile at level -1 and LEVEL; every child of both passes against the oracle, and the launch's path counters against
    predict_paths exactly.  -> (worst tile deviation, worst direct deviation, (staged, not staged), the prediction per segment)"""
    nseg, n = par.shape[:2]
    _, _, rots, _ = _source(N)
    assert nseg <= len(rots)
    paths = predict_paths(N, V, par, chunks)
    want = (sum(p[0] for p in paths), sum(p[1] + p[2] for p in paths))
    bar = min(TOL_TILE, ceiling(standalone_chunk_pts(N, chunks), n))
    worst_t = worst_d = 0.0
    for level in (-1, LEVEL):
        out = [np.full(nseg * n * 8, np.nan, np.float32) for _ in range(4)]
        ms = (C.c_float * 2)(); st = (C.c_uint32 * 2)()
        pkg.binding.check(reg._lib.goicp_debug_bounds_tile(reg.handle, _fp(np.ascontiguousarray(rots[:nseg].reshape(-1))), _fp(np.ascontiguousarray(par.reshape(-1))),
                                                            nseg, n, level, chunks, _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), ms, st))
        assert all(np.isfinite(o).all() for o in out), (N, V, n, chunks, level)
        for i in range(nseg):
            fu, fl = ref_bounds(N, V, i, level, par[i], trunc)
            sl = slice(i * n * 8, (i + 1) * n * 8)
            for got, ref, name in ((out[0][sl], fu, "tile ub"), (out[1][sl], fl, "tile lb"), (out[2][sl], fu, "direct ub"), (out[3][sl], fl, "direct lb")):
                dev = np.abs(got.astype(np.float64) - ref) / np.maximum(ref, 1e-3)
                k = int(np.argmax(dev))
                if name.startswith("tile"):
                    worst_t = max(worst_t, float(dev[k]))
                    assert dev[k] <= bar, (name, N, V, n, chunks, level, i, k, float(got[k]), float(ref[k]), float(dev[k]), bar)
                else:
                    worst_d = max(worst_d, float(dev[k]))
                    assert dev[k] <= TOL, (name, N, V, n, chunks, level, i, k, float(got[k]), float(ref[k]), float(dev[k]))
            assert np.all(out[1][sl] <= out[0][sl]) and np.all(out[3][sl] <= out[2][sl]), (N, V, n, chunks, level, i)
        # which path every sub-patch took: the kernel's counters against the prediction, exactly
        assert (int(st[0]), int(st[1])) == want, (N, V, n, chunks, level, list(st), want, paths)
    return worst_t, worst_d, want, paths


def chunk_list(N):
    """1, and 2 and 3 where there are that many 64-point patches -- and 3 at N = 1 and N = 65, where there are not; 8 193: a lane's run stays short"""
    if N == 8193:
        return [16, 129]
    if N == 1:
        return [1, 3]
    return [1, 2, 3] if N == 65 or N >= 129 else ([1, 2] if N > 64 else [1])


@pytest.mark.parametrize("N,n", NN)
def test_staged_grid32(pkg, regs, N, n):
    """dt_size 32, the tight block: every sub-patch is staged.  chunks 1, 2, 3 (N = 1 and N = 65 with 3: more chunks than 64-point patches,
    the surplus items leave zero rows); N = 8 193: 16 and 129 chunks"""
    reg = regs.get(N, 32)
    for chunks in chunk_list(N):
        t, d, st, paths = run_tile(pkg, reg, N, 32, nodes_block(N, n), chunks)
        assert st[0] > 0 and st[1] == 0, (N, n, chunks, st)
        print("grid 32 N %d n %d chunks %d: worst rel deviation tile %.2e direct %.2e, sub-patches staged %d, not %d" % (N, n, chunks, t, d, st[0], st[1]))


@pytest.mark.parametrize("N,n", NN)
def test_fallback_and_mixed_grid64(pkg, regs, N, n):
    """dt_size 64: N <= 257 with the wide nodes, nothing can be staged; N = 8 193 with the block at the grid's edge, some sub-patches are and some are not"""
    reg = regs.get(N, 64)
    for chunks in chunk_list(N):
        par = nodes_block_at_edge(N, 64, n) if N == 8193 else nodes_wide(n)
        t, d, st, paths = run_tile(pkg, reg, N, 64, par, chunks)
        if N == 8193:
            assert st[0] > 0 and st[1] > 0, (N, n, chunks, st)
        else:
            assert st[0] == 0 and st[1] > 0, (N, n, chunks, st)
        print("grid 64 N %d n %d chunks %d: worst rel deviation tile %.2e direct %.2e, sub-patches staged %d, not %d" % (N, n, chunks, t, d, st[0], st[1]))


GEOMETRY = {"row_x": lambda: nodes_row(0), "row_z": lambda: nodes_row(2), "same_node": nodes_same, "two_depths": nodes_two_depths}


@pytest.mark.parametrize("V", [32, 64])
@pytest.mark.parametrize("N", [1, 3, 8193])
@pytest.mark.parametrize("shape", sorted(GEOMETRY))
def test_segment_geometry(pkg, regs, shape, N, V):
    """segments other than the block: 64 nodes in a row along x and along z (thin and long boxes: the brick counts per axis far apart), 64
    copies of one node (spread 0), two depths in one segment (w = 1/8 and 1/512).  run_tile holds the counters to predict_paths exactly; what
    each case is there for is asserted on top.  N = 1: a single point's box under a row is 1 x 1 x ~11 (dt_size 32) or ~22 (64) voxels plus
    the margins and lies inside the grid: every segment staged.  N = 3: 64 copies of a node are as narrow as one node: staged; the rows and the
    two depths at dt_size 64 are too large for the tile under all three rotations: the fallback, inside the grid.  N = 8 193 in 129 chunks:
    the sub-patches are 64 neighbours of the k-d order, nearly all of them staged under every rotation -- the long thin boxes of the brick
    decode -- and under the x row a few reach over the grid's low x face (the row starts at -0.5)"""
    reg = regs.get(N, V)
    par = GEOMETRY[shape]()
    for chunks in ([129] if N == 8193 else [1]):
        t, d, st, paths = run_tile(pkg, reg, N, V, par, chunks)
        if N == 1 or shape == "same_node":
            assert st[0] > 0 and st[1] == 0, (shape, N, V, paths)
        elif N == 3 and V == 64:
            assert st[0] == 0 and all(p[1] == 1 and p[2] == 0 for p in paths), (shape, N, V, paths)
        elif N == 3:
            assert st[0] > 0, (shape, N, V, paths)
        else:
            assert all(p[0] >= 100 for p in paths) and st[1] <= 20 and (st[1] > 0) == (shape == "row_x"), (shape, N, V, paths)
        print("%s grid %d N %d chunks %d: worst rel deviation tile %.2e direct %.2e, sub-patches staged %d, not %d; per segment [staged, too large, over the edge] %s"
              % (shape, V, N, chunks, t, d, st[0], st[1], paths))


@pytest.mark.parametrize("V", [32, 64])
@pytest.mark.parametrize("N", [5, 257])
def test_grid_edge_and_beyond(pkg, regs, N, V):
    """three segments in one call: around (+1, 0, 0), around (-1, 0, 0), around (50, -40, 30).  A sub-patch whose box reaches over the grid's
    edge takes the fallback whole; its out-of-grid lookups are the oracle's extension.  The far segment cannot be staged at all.  At N = 257
    (five sub-patches) the two segments at the faces show the mix: some sub-patches inside the grid (staged at dt_size 32), some over the
    edge.  The five points of N = 5 are one sub-patch: over the edge or not as a whole."""
    reg = regs.get(N, V)
    par = nodes_edge()
    for chunks, trunc in ((1, False), (2, False), (1, True)):
        reg.set_search_truncation(TRUNC_G if trunc else 0.0)
        try:
            t, d, st, paths = run_tile(pkg, reg, N, V, par, chunks, trunc)
        finally:
            reg.set_search_truncation(0.0)
        patches = -(-N // 64)
        assert paths[2] == [0, 0, patches], (N, V, chunks, paths)        # the far segment: every sub-patch outside
        if N == 5:
            assert all(p[2] == 0 and p[0] == (1 if V == 32 else 0) for p in paths[:2]), (N, V, chunks, paths)   # wholly inside; too large for the tile at dt_size 64
        if N == 257:
            both = [p for p in paths[:2] if p[2] > 0 and p[0] + p[1] > 0]
            assert both and sum(p[2] for p in paths[:2]) > 0 and sum(p[0] + p[1] for p in paths[:2]) > 0, (N, V, chunks, paths)
            if V == 32:
                assert sum(p[0] for p in paths[:2]) > 0, (N, V, chunks, paths)
        print("edge grid %d N %d chunks %d%s: worst rel deviation tile %.2e direct %.2e, sub-patches staged %d, not %d; per segment [staged, too large, over the edge] %s"
              % (V, N, chunks, " truncated" if trunc else "", t, d, st[0], st[1], paths))


@pytest.mark.parametrize("V", [32, 64])
@pytest.mark.parametrize("N", [5, 257])
@pytest.mark.parametrize("n", [3, 64])
def test_truncated(pkg, regs, N, n, V):
    """g = 0.05 on the handle, trunc = 0.05 in the reference"""
    reg = regs.get(N, V)
    reg.set_search_truncation(TRUNC_G)
    try:
        for chunks in (1, 2):
            par = nodes_block(N, n) if V == 32 else nodes_wide(n)
            t, d, st, paths = run_tile(pkg, reg, N, V, par, chunks, trunc=True)
            assert (st[0] > 0 and st[1] == 0) if V == 32 else (st[0] == 0 and st[1] > 0), (N, n, V, chunks, st)
            print("truncated grid %d N %d n %d chunks %d: worst rel deviation tile %.2e direct %.2e" % (V, N, n, chunks, t, d))
    finally:
        reg.set_search_truncation(0.0)


@pytest.mark.parametrize("nseg,n,chunks", [(1, 0, 1), (1, 65, 1), (0, 8, 1), (1, 8, 0)])
def test_refusals(pkg, regs, nseg, n, chunks):
    reg = regs.get(65, 32)
    _, _, rots, _ = _source(65)
    par = nodes_block(1, 64, 1)
    out = [np.zeros(8 * 65, np.float32) for _ in range(4)]
    ms = (C.c_float * 2)(); st = (C.c_uint32 * 2)()
    rc = reg._lib.goicp_debug_bounds_tile(reg.handle, _fp(np.ascontiguousarray(rots[:1].reshape(-1))), _fp(np.ascontiguousarray(par.reshape(-1))), nseg, n, LEVEL, chunks,
                                          _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), ms, st)
    assert rc == INVALID
    with pytest.raises(pkg.GoicpError) as e:
        pkg.binding.check(rc)
    assert e.value.code == INVALID
    # the handle still works
    t, d, st2, _ = run_tile(pkg, reg, 65, 32, nodes_block(2, 8, 1), 1)
    assert st2[0] > 0 and st2[1] == 0
