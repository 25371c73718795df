"""The QUEUED form of the LDS-tile bound kernel (bounds_tile_kernel<true> through launch_bounds_tile_queue) and the digest of its chunk
partials by the next round's queue kernel, through goicp_debug_queue_expand_tiles: one round of two searches (upper-bound pass with n_ub nodes,
lower-bound pass with n) that lists everything in the TILE list -- the segment count is known to the device only, tile_shape() picks the
chunks there, block 0 writes ctl->tile_chunks, searches of more than 64 expansions are cut into segments, and with segments x chunks above the
grid the items walk the grid-stride loop a second time, reusing the LDS tile as accumulator.

Every child of both passes is held to the float64 oracle sums of test_gpu_bounds_tile_shapes (same reference, same bar min(TOL_TILE, ceiling)
with the chunk size the device chose) AND to goicp_debug_queue_expand -- the direct list -- on the same handle at TOL.  Every case asserts
the shape the device reported (info: chunks, segments, grid) against the transcription of tile_shape below.

Digest (digest = 1): the queue kernel is launched once more with K = 1; with the incumbent at 1e30 and n <= 128 it is one pass of <= 1 024
children.  Model on the oracle's bounds: best = the smallest ub (first index on ties), pushed = the children with lb < best in child order.
The pushed nodes' (ub, lb) -- added from the chunk partials in the digest's own P-strided order --, best, min_ub and the best child's corner
are held at the same bar.  A child whose oracle lb lies within twice the bar of best may fall on either side of `lb < best` and is exempt
from the membership test (its values are still held when it is there); the node the K = 1 selection took out of the queue must be one of the
pushed set, the others keep child order but for the one the removal moved into the hole.

The entry fills tile.ub, tile.lb and tile.scratch with NaN before the round, so an item that never stored its sums cannot pass for one that
did on the strength of what the buffer held before (that is how mutant C below first slipped through: the missing case the teeth found).

With more than one point chunk the entry adds the chunk partials on the host in double and rounds once: what comes back is the evaluation's
error, not that of a float sum of up to 342 partials, which the ceiling does not count.

Measured worst deviations on MI355X (bar: min(TOL_TILE = 2e-6, ceiling); TOL = 2e-6 against the direct list):
  queued rounds       from the oracle 2.9e-7, from the direct list 2.8e-7     truncated and edge node groups   1.5e-7
  grid-stride case    from the oracle 1.1e-7 (its ceiling: 1.37e-6 -- 16 sequential additions per lane), from the direct list 2.4e-7
  digest              pushed nodes, best, min_ub 3.3e-7; no child fell within the border zone of `lb < best`
No defect was found in the kernels.

Teeth (done once on scratch copies of device.hip / bnbqueue.hip, on MI355X, the whole GPU suite per mutant; every mutant reads valid memory only;
998 earlier tests, 154 in test_gpu_bounds_tile_shapes, 70 here):
  A  the tile loops' `j < np` -> `j < np - 1` when np < 64:               6 earlier tests fail, 148 of the stand-alone file, 69 here
  B  the lane-group reduction starts at off = 2 P:                        20 earlier, 78 of the stand-alone file, 30 here
  C  the issue's mutant (no __syncthreads() at the top of an item) cannot be shown: that barrier is redundant -- nothing writes the tile, rp, box
     or tr between an item's read-out and the two barriers that precede the next staging.  Instead: a workgroup's second and later items of the
     grid-stride loop do not store their sums.  46 earlier tests fail (whole registrations), none of the stand-alone file (one item per
     workgroup there) and at first none here -- the rows were never written, and what the buffer happened to hold passed; with the NaN fill
     test_grid_stride_second_pass fails
  D  the digest of a tile search ignores the chunk partials (chunks = 1 when S->tile):   31 earlier tests fail, the four digest cases with
     tile_chunks > 1 here
Wall time on MI355X: the two files together 6.4 s (224 tests, the slowest 0.3 s); the GPU suite without them 291 s.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_pkg
from test_gpu_scale_parity import TOL
from test_gpu_small_shapes import LEVEL
from test_gpu_bounds_tile_shapes import INVALID, TOL_TILE, TRUNC_G, W64, Regs, _fp, _source, ceiling, nodes_edge, nodes_wide, predict_paths, ref_bounds

pytestmark = pytest.mark.gpu
PATCH = 64


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def regs(pkg):
    r = Regs(pkg)
    yield r
    r.close()


def tile_shape(nseg, N, grid):
    """device.hip tile_shape: as many chunks (multiples of the 64-point sub-patch) as give every workgroup an item, at most one sub-patch each"""
    patches = -(-N // PATCH)
    c = max(1, -(-grid // nseg))
    c = min(c, patches)
    cp = -(-patches // c) * PATCH
    return -(-N // cp), cp


def nodes_blocks(seed, n):
    """n <= 128 nodes: the 4x4x4 block of width-1/64 nodes of the stand-alone tests and a second one beside it (+4 w in x): a segment each"""
    rng = np.random.default_rng(seed)
    c0 = (np.floor(rng.uniform(-0.15, 0.15 - 8 * float(W64), 3) / W64) * W64).astype(np.float32)
    par = np.zeros((n, 4), np.float32)
    for k in range(n):
        par[k] = (c0[0] + np.float32((k & 3) + 4 * (k >> 6)) * W64, c0[1] + np.float32((k >> 2) & 3) * W64, c0[2] + np.float32((k >> 4) & 3) * W64, W64)
    return par


def nodes_wide128(n):
    """nodes_wide's lattice, and the same lattice moved by 1/16 in y for the nodes from 64 on"""
    a = nodes_wide(64, 1)[0]
    b = a.copy()
    b[:, 1] += np.float32(1 / 16)
    return np.ascontiguousarray(np.concatenate([a, b])[:n])


def run_round(pkg, reg, N, V, ri, par, n_ub, trunc=False, digest=False, direct=True):
    """one tile round (and its digest) -> dict: the four bound arrays, info, the references, the per-child bars, worst deviations"""
    n = len(par)
    _, _, rots, _ = _source(N)
    R = np.ascontiguousarray(rots[ri].reshape(-1))
    flat = np.ascontiguousarray(par.reshape(-1))
    out = [np.full(8 * (n_ub if k < 2 else n), np.nan, np.float32) for k in range(4)]
    info = (C.c_int32 * 4)()
    qn = np.full((2, 8 * n, 6), np.nan, np.float32); qc = (C.c_int32 * 4)(); li = np.full((2, 4), np.nan, np.float32); se = np.full((2, 8), np.nan, np.float32)
    pkg.binding.check(reg._lib.goicp_debug_queue_expand_tiles(reg.handle, _fp(R), LEVEL, _fp(flat), n, n_ub, _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), info,
                                                               1 if digest else 0, _fp(qn), qc, _fp(li), _fp(se)))
    chunks, nsegs, grid, twins_on = (int(x) for x in info)
    # the shape the device chose
    want_segs = -(-n_ub // 64) + -(-n // 64)
    want_chunks, cp = tile_shape(want_segs, N, grid)
    assert grid > 0 and nsegs == want_segs and chunks == want_chunks, (N, n, n_ub, list(info), want_segs, want_chunks)
    assert all(np.isfinite(o).all() for o in out)
    refs = [ref_bounds(N, V, ri, -1, par[:n_ub], trunc), ref_bounds(N, V, ri, LEVEL, par, trunc)]
    bars = []
    for cnt in (n_ub, n):
        seg_n = np.array([min(64, cnt - 64 * (e // 64)) for e in range(cnt)])
        bars.append(np.repeat([min(TOL_TILE, ceiling(min(cp, N), int(m))) for m in seg_n], 8))
    worst = 0.0
    for ps in range(2):
        for got, ref, name in ((out[2 * ps], refs[ps][0], "ub"), (out[2 * ps + 1], refs[ps][1], "lb")):
            dev = np.abs(got.astype(np.float64) - ref) / np.maximum(ref, 1e-3)
            k = int(np.argmax(dev / bars[ps]))
            worst = max(worst, float(dev.max()))
            assert dev[k] <= bars[ps][k], ("tile queue vs oracle", name, ps, N, V, n, n_ub, k, float(got[k]), float(ref[k]), float(dev[k]), float(bars[ps][k]), list(info))
        assert np.all(out[2 * ps + 1] <= out[2 * ps])
    worst_direct = 0.0
    if direct:
        dout = [np.full(8 * n, np.nan, np.float32) for _ in range(4)]
        dinfo = (C.c_int32 * 2)()
        pkg.binding.check(reg._lib.goicp_debug_queue_expand(reg.handle, _fp(R), LEVEL, _fp(flat), n, _fp(dout[0]), _fp(dout[1]), _fp(dout[2]), _fp(dout[3]), dinfo))
        for k in range(4):
            m = 8 * (n_ub if k < 2 else n)
            d = dout[k][:m].astype(np.float64)
            dev = np.abs(out[k].astype(np.float64) - d) / np.maximum(np.abs(d), 1e-3)
            worst_direct = max(worst_direct, float(dev.max()))
            assert dev.max() <= TOL, ("tile queue vs direct list", k, N, V, n, n_ub, float(dev.max()))
            ref = refs[k // 2][k % 2]
            assert np.all(np.abs(d - ref) <= TOL * np.maximum(ref, 1e-3)), ("direct list vs oracle", k, N, V, n)
    return dict(out=out, info=(chunks, nsegs, grid, twins_on), refs=refs, bars=bars, worst=worst, worst_direct=worst_direct, cp=cp,
                queue=qn, counts=[int(x) for x in qc], listed=li, search=se)


EXPECT_CHUNKS_1024 = {1: 1, 63: 1, 65: 2, 257: 5, 8193: 129}       # tile_shape on a grid of 1 024 workgroups, 2 .. 4 segments


@pytest.mark.parametrize("V", [32, 64])
@pytest.mark.parametrize("n", [1, 17, 64, 65, 100, 128])
@pytest.mark.parametrize("N", [1, 63, 65, 257, 8193])
def test_queued_round(pkg, regs, N, n, V):
    """segments of 1, 17, 64, 64 + 1, 64 + 36 and 64 + 64 expansions per search; dt_size 32 (the tight blocks: staged) and 64 (N <= 257 the
    spread nodes: the fallback; 8 193: both)"""
    reg = regs.get(N, V)
    par = nodes_blocks(N, n) if (V == 32 or N == 8193) else nodes_wide128(n)
    r = run_round(pkg, reg, N, V, N % 3, par, n)
    chunks, nsegs, grid, _ = r["info"]
    if grid == 1024:
        assert chunks == EXPECT_CHUNKS_1024[N], (N, n, r["info"])
    print("queued grid %d N %d n %d: chunks %d x %d points, %d segments on %d workgroups; worst rel deviation from the oracle %.2e, from the direct list %.2e"
          % (V, N, n, chunks, r["cp"], nsegs, grid, r["worst"], r["worst_direct"]))


def test_grid_stride_second_pass(pkg, regs):
    """n = 128, n_ub = 64: three segments.  The source size follows from the grid the device reports: ceil(grid / 3) + 1 sub-patches of 64 points
    (21 850 points on 1 024 workgroups: 342 chunks, 1 026 items), so that segments x chunks exceeds the grid and some workgroups take a second item"""
    probe = regs.get(63, 32)
    grid = run_round(pkg, probe, 63, 32, 0, nodes_blocks(7, 2), 1, direct=False)["info"][2]
    N = -(-grid // 3) * 64 - 38
    if grid == 1024:
        assert N == 21850
    reg = regs.get(N, 32)
    r = run_round(pkg, reg, N, 32, 1, nodes_blocks(99, 128), 64)
    chunks, nsegs, grid2, _ = r["info"]
    assert grid2 == grid and nsegs == 3 and r["cp"] == 64
    assert nsegs * chunks > grid2, r["info"]
    print("grid-stride: N %d, %d segments x %d chunks = %d items on %d workgroups; worst rel deviation from the oracle %.2e, from the direct list %.2e"
          % (N, nsegs, chunks, nsegs * chunks, grid2, r["worst"], r["worst_direct"]))


@pytest.mark.parametrize("V", [32, 64])
def test_queued_truncated_and_edges(pkg, regs, V):
    """g = 0.05 on the tight blocks, and the edge / outside-the-grid node groups of the stand-alone tests -- around (+1, 0, 0), around (-1, 0, 0)
    and around (50, -40, 30) -- each as a round of its own (one search is one segment with one translation range: together they would all fall
    back), under the rotation the stand-alone test gives that group, plain and truncated.  The queued kernel has no path counters; which path
    the sub-patches take follows from the same box rule (predict_paths, held to the stand-alone kernel's counters exactly there) with the
    chunks the device chose: the two groups at the faces have sub-patches inside the grid and sub-patches over its edge, the far group
    only the latter."""
    N = 257
    reg = regs.get(N, V)
    edge = nodes_edge()
    for trunc in (False, True):
        reg.set_search_truncation(TRUNC_G if trunc else 0.0)
        try:
            a = run_round(pkg, reg, N, V, 2, nodes_blocks(5, 100), 37, trunc) if trunc else None
            worst = 0.0
            for i in range(3):
                b = run_round(pkg, reg, N, V, i, np.ascontiguousarray(edge[i]), len(edge[i]), trunc)
                worst = max(worst, b["worst"])
                staged, large, over = predict_paths(N, V, edge[i:i + 1], b["info"][0], rot_of=[i])[0]
                assert staged + large + over == b["info"][0] == 5
                assert (over == 5) if i == 2 else (over > 0 and staged + large > 0 and (staged > 0 or V == 64)), (V, i, staged, large, over)
        finally:
            reg.set_search_truncation(0.0)
        print("queued grid %d%s: edges worst rel deviation %.2e%s" % (V, " truncated" if trunc else "", worst, (", blocks %.2e" % a["worst"]) if a else ""))


def _call(pkg, reg, n, n_ub, R, par):
    out = [np.zeros(8 * 128, np.float32) for _ in range(4)]
    info = (C.c_int32 * 4)()
    return reg._lib.goicp_debug_queue_expand_tiles(reg.handle, _fp(R), LEVEL, _fp(par), n, n_ub, _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), info, 0, None, None, None, None)


def test_refusals(pkg, regs):
    _, _, rots, _ = _source(65)
    R = np.ascontiguousarray(rots[0].reshape(-1))
    par = np.ascontiguousarray(np.concatenate([nodes_blocks(3, 128), nodes_blocks(4, 8)]).reshape(-1))
    reg = regs.get(65, 32)
    for n, n_ub in ((0, 0), (129, 1), (8, 0), (8, 9), (8, -1)):
        rc = _call(pkg, reg, n, n_ub, R, par)
        assert rc == INVALID, (n, n_ub, rc)
        with pytest.raises(pkg.GoicpError) as e:
            pkg.binding.check(rc)
        assert e.value.code == INVALID
    # a digest without its output arrays
    out = [np.zeros(64, np.float32) for _ in range(4)]
    info = (C.c_int32 * 4)()
    assert reg._lib.goicp_debug_queue_expand_tiles(reg.handle, _fp(R), LEVEL, _fp(par), 8, 8, _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), info, 1, None, None, None, None) == INVALID
    # handles without the tile list
    for kw in ({"lds_tiles": 0}, {"dt_layout": 0}, {"bounds_fp16": 1}, {"trim_fraction": 0.1}):
        other = regs.get(65, 32, **kw)
        rc = _call(pkg, other, 8, 8, R, par)
        assert rc == INVALID, (kw, rc)
        with pytest.raises(pkg.GoicpError) as e:
            pkg.binding.check(rc)
        assert e.value.code == INVALID
    assert _call(pkg, reg, 8, 8, R, par) == 0                              # the good handle still works


# ----------------------------------------------------------------------------------------------
# the digest of the tile partials
# ----------------------------------------------------------------------------------------------
def _child_corners(par):
    """corner + width of the 8 children of every node, in child order, float32 as the digest forms them (corner + bit * w / 2)"""
    out = []
    for p in par:
        px, py, pz, pw = (np.float32(x) for x in p)
        cw = pw / np.float32(2)
        for c in range(8):
            out.append((float(px + np.float32(c & 1) * cw), float(py + np.float32((c >> 1) & 1) * cw), float(pz + np.float32((c >> 2) & 1) * cw), float(cw)))
    return out


@pytest.mark.parametrize("n", [17, 128])
@pytest.mark.parametrize("N", [63, 257, 8193])
def test_digest_of_tile_partials(pkg, regs, N, n):
    """tile_chunks 1 (N = 63), 5 (257) and 129 (8 193): the digest reads tile.ub / tile.lb, or tile.scratch with ctl->tile_chunks, through the
    S->tile switch, for both searches"""
    reg = regs.get(N, 32)
    par = nodes_blocks(N, n)
    r = run_round(pkg, reg, N, 32, N % 3, par, n, digest=True, direct=False)
    chunks = r["info"][0]
    if r["info"][2] == 1024:
        assert chunks == {63: 1, 257: 5, 8193: 129}[N]
    corners = _child_corners(par)
    index = {c: i for i, c in enumerate(corners)}
    assert len(index) == 8 * n
    worst = 0.0
    for s in range(2):
        ub, lb = r["refs"][s]
        bar = r["bars"][s]
        best_i = int(np.argmin(ub))
        best = float(ub[best_i])
        tol_best = float(bar[best_i]) * max(best, 1e-3)
        se = r["search"][s]
        # incumbent, min_ub, the best child
        assert se[2] == 1.0 and se[0] == se[1], (s, se)
        worst = max(worst, abs(float(se[0]) - best) / max(best, 1e-3))
        assert abs(float(se[0]) - best) <= tol_best, (s, N, n, float(se[0]), best)
        got_i = index[tuple(float(x) for x in se[3:7])]
        assert got_i == best_i or ub[got_i] - best <= 2 * tol_best, (s, N, n, got_i, best_i)
        # the queue after the digest and the K = 1 selection
        cnt, nl = r["counts"][2 * s], r["counts"][2 * s + 1]
        assert nl == (0 if se[7] else 1), (s, N, n, nl, se[7])            # nothing is listed only when the stop rule ended the search (best - min lb < SSEThresh)
        q = r["queue"][s][:cnt]
        ids = [index[tuple(float(x) for x in nd[:4])] for nd in q]
        assert len(set(ids)) == cnt
        if cnt > 1:
            rest = list(ids)
            rest.remove(max(ids))
            assert rest == sorted(rest), (s, N, n, "the queue is not in child order")
        for i, nd in zip(ids, q):
            du, dl = abs(float(nd[4]) - ub[i]) / max(ub[i], 1e-3), abs(float(nd[5]) - lb[i]) / max(lb[i], 1e-3)
            worst = max(worst, du, dl)
            assert du <= bar[i] and dl <= bar[i], ("pushed node", s, N, n, i, float(nd[4]), ub[i], float(nd[5]), lb[i], float(bar[i]))
        pushed = set(ids)
        if nl:
            li = index[tuple(float(x) for x in r["listed"][s])]
            assert li not in pushed
            pushed.add(li)
        margin = 2 * bar * np.maximum(np.maximum(lb, best), 1e-3)
        must = set(np.nonzero(lb < best - margin)[0].tolist())
        may = set(np.nonzero(lb < best + margin)[0].tolist())
        assert must <= pushed <= may, (s, N, n, sorted(must - pushed), sorted(pushed - may))
        assert best_i in must                                             # never vacuous: the best child's own lb lies a whole delta below its ub
        print("digest N %d n %d search %d: tile chunks %d, %d of %d children pushed (%d border cases), one listed next: %d" % (N, n, s, chunks, len(pushed), 8 * n, len(may - must), nl))
    print("digest N %d n %d: worst rel deviation %.2e" % (N, n, worst))
