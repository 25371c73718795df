"""GPU tests of the truncated-cost search (goicp_set_search_truncation): with g > 0 every term of every cube bound and pose score of the
handle is clamped at g AFTER its subtractions,
    E_g(R, t) = sum min(DT(R p + t), g)^2,   ub term min(m, g)^2,   lb term min(max(m - delta, 0), g)^2,   m = max(DT - coeff |p|, 0).
What is held here:
  1. the bounds against the fp64 twin built on oracle.cube_terms (test_search_trunc_host.trunc_bound_f64) -- generic, lean sibling,
     grouped, tile and device-queue paths, layouts 1 and 0;
  2. g = 1e30 reproduces the plain handle's bits (operators and a whole registration);
  3. validity as a property: the score of any pose inside a (rotation cube, translation cube) pair is >= the pair's lower bound;
  4. small clouds with 30 % outliers: the search proves the optimum of E_g;
  5. the clutter bunny under a motion ICP alone cannot undo, with gated ICP inside the truncated search;
  6. the refusals on a live handle, and g = 0 bringing the plain bits back."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from conftest import cloud, load_pkg, rot_angle
from test_search_trunc_host import trunc_bound_f64

pytestmark = pytest.mark.gpu
INVALID = -1
GS = (0.02, 0.05, 0.15)
HUGE = 1e30
ROTS = ([1.5707963, -1.5707963, 1.5707963], [0.3, -0.2, 0.9], [-2.1, 0.4, 1.1])


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def rho10(oracle_mod, bunny_data10):
    _, rho = oracle_mod.rot_radii(bunny_data10)
    return rho


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _cubes(rng, n):
    lev = rng.integers(0, 7, n)
    w = (1.0 / (1 << lev)).astype(np.float32)
    c = (rng.uniform(-0.5, 0.5, (n, 3)) * (1 - w[:, None])).astype(np.float32)
    return np.concatenate([c, w[:, None]], 1).astype(np.float32)


def _children(parent):
    px, py, pz, pw = map(np.float32, parent)
    w = pw / np.float32(2)
    kids = []
    for j in range(8):
        cx = px + np.float32(j & 1) * w; cy = py + np.float32(j >> 1 & 1) * w; cz = pz + np.float32(j >> 2 & 1) * w
        kids.append([cx + w / np.float32(2), cy + w / np.float32(2), cz + w / np.float32(2), w])
    return np.array(kids, np.float32)


def _parents(rng, n_per_depth, depths):
    """translation nodes (corner xyz + width) as the BnB makes them: corner = -0.5 + k w; no node twice"""
    out = []
    for d in depths:
        w = np.float32(1.0) / np.float32(1 << d)
        seen = set()
        for kk in rng.integers(0, 1 << d, (4 * n_per_depth, 3)):
            if tuple(kk) in seen or len(seen) >= min(n_per_depth, 8 ** d):
                continue
            seen.add(tuple(kk))
            out.append([np.float32(-0.5) + np.float32(kk[0]) * w, np.float32(-0.5) + np.float32(kk[1]) * w, np.float32(-0.5) + np.float32(kk[2]) * w, w])
    return np.array(out, np.float32)


def _close(x, want):
    """test_eval_bounds_vs_oracle's tolerance: only the summation order differs"""
    return abs(float(x) - want) <= 1e-4 * max(want, 1e-3)


def score_f64(oracle_mod, dt, src, R, t, g):
    """E_g(R, t) of the twin: cube_terms at w = 0 without a rotation radius"""
    prot = oracle_mod.rotate(np.asarray(R, np.float32), src)
    return trunc_bound_f64(oracle_mod.cube_terms(dt, prot, None, np.asarray(t, np.float32), 0.0), 0.0, g)[0]


# ----------------------------------------------------------------------------------------------
# 1. bounds against the oracle's terms
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terms10(pkg, oracle_mod, oracle_dt_bunny, bunny_data10, rho10):
    """the per-point residuals of test_eval_bounds_vs_oracle's setup (three rotations x 64 cubes x levels -1, 3, 5, 7): they depend neither
    on the layout nor on g"""
    rng = np.random.default_rng(7)
    out = []
    for v in ROTS:
        R = pkg.fgoicp.rodrigues(v)
        prot = oracle_mod.rotate(R, bunny_data10)
        cubes = _cubes(rng, 64)
        per_level = {}
        for level in (-1, 3, 5, 7):
            rho = rho10[level] if level >= 0 else None
            per_level[level] = [oracle_mod.cube_terms(oracle_dt_bunny, prot, rho, c[:3], c[3]) for c in cubes]
        out.append((R, cubes, per_level))
    return out


@pytest.mark.parametrize("layout", [1, 0])
def test_truncated_bounds_vs_oracle_terms(pkg, bunny_model, bunny_data10, terms10, layout):
    reg = pkg.Registration(bunny_model, bunny_data10, 1e-3, dt_layout=layout)
    N = len(bunny_data10)
    worst = 0.0
    try:
        for g in GS:
            reg.set_search_truncation(g)
            assert reg.search_truncation() == np.float32(g)
            cap = N * float(np.float32(g)) ** 2
            for R, cubes, per_level in terms10:
                for level, terms in per_level.items():
                    ub, lb = reg.eval_bounds(R, cubes, level)
                    for i, c in enumerate(cubes):
                        oub, olb = trunc_bound_f64(terms[i], c[3], g)
                        worst = max(worst, abs(ub[i] - oub) / max(oub, 1e-3), abs(lb[i] - olb) / max(olb, 1e-3))
                        assert _close(ub[i], oub) and _close(lb[i], olb), (layout, g, level, i, ub[i], oub, lb[i], olb)
                        assert lb[i] <= ub[i] <= cap * (1 + 1e-5), (layout, g, level, i, lb[i], ub[i], cap)
        print("truncated bounds vs fp64 twin, layout %d: worst relative deviation %.2e" % (layout, worst))
    finally:
        reg.close()


def test_truncated_sibling_grouped_tile_and_queue_paths(pkg, oracle_mod, oracle_dt_bunny, bunny_model, bunny_data10, rho10):
    """the lean sibling path (eight children per group), an unrelated batch (grouped on the device, generic per-cube path), the LDS-tile
    kernel against the direct one and a twin-fused round of the device queues against per-cube evaluation -- all on a truncated handle"""
    B = pkg.binding
    reg = pkg.Registration(bunny_model, bunny_data10, 1e-3)
    lib, h = reg._lib, reg.handle
    rng = np.random.default_rng(23)
    level = 5
    g = 0.05
    reg.set_search_truncation(g)
    try:
        R = pkg.fgoicp.rodrigues(ROTS[1])
        prot = oracle_mod.rotate(R, bunny_data10)
        parents = _parents(rng, 6, range(0, 7))
        far = np.array([[0.75, -0.25, 0.0, 0.5], [-1.5, 0.5, 0.25, 0.5], [2.0, 2.0, -2.0, 1.0]], np.float32)     # children straddle / leave the grid
        parents = np.concatenate([parents, far])
        n = len(parents)
        kids = np.concatenate([_children(p) for p in parents])
        want = {}
        for ps, (lv, rho) in enumerate(((-1, None), (level, rho10[level]))):
            for i, k in enumerate(kids):
                want[(ps, i)] = trunc_bound_f64(oracle_mod.cube_terms(oracle_dt_bunny, prot, rho, k[:3], k[3]), k[3], g)
        # (i) siblings through the operator API: the lean path
        per_cube = {}
        for ps, lv in ((0, -1), (1, level)):
            ub, lb = reg.eval_bounds(R, kids, lv)
            per_cube[ps] = (ub, lb)
            for i in range(len(kids)):
                assert _close(ub[i], want[(ps, i)][0]) and _close(lb[i], want[(ps, i)][1]), ("siblings", ps, i)
        # (ii) an unrelated batch of four rotations: grouped on the device, generic path
        rots = np.stack([pkg.fgoicp.rodrigues(v) for v in ROTS] + [pkg.fgoicp.rodrigues([0.1, 0.2, -0.3])])
        cubes = _cubes(rng, 512)
        rot_of = rng.integers(0, 4, 512)
        coeff = reg.rot_coeff(level)
        recs = [(c[0], c[1], c[2], lib.goicp_trans_delta(float(c[3])), coeff if i % 2 else 0.0, int(rot_of[i])) for i, c in enumerate(cubes)]
        ub, lb = reg.eval_bounds_batch(rots, recs)
        prots = [oracle_mod.rotate(r, bunny_data10) for r in rots]
        for i in range(0, 512, 3):
            c = cubes[i]
            oub, olb = trunc_bound_f64(oracle_mod.cube_terms(oracle_dt_bunny, prots[rot_of[i]], rho10[level] if i % 2 else None, c[:3], c[3]), c[3], g)
            assert _close(ub[i], oub) and _close(lb[i], olb), ("grouped", i, ub[i], oub, lb[i], olb)
        # (iii) the tile kernel against the direct kernel (test_lds_tile_kernel_matches_direct_kernel's equality), and the direct one against the twin
        for depth, m, chunks in ((8, 64, 2), (3, 64, 1), (7, 17, 2)):
            nseg = 3
            w = np.float32(1.0 / (1 << depth))
            rr = np.stack([pkg.fgoicp.rodrigues(rng.uniform(-2.0, 2.0, 3)) for _ in range(nseg)]).astype(np.float32)
            par = np.zeros((nseg, m, 4), np.float32)
            for i in range(nseg):
                c0 = (np.floor(rng.uniform(-0.3, 0.3, 3) / w) * w).astype(np.float32)
                for k in range(m):
                    par[i, k] = (c0[0] + (k & 3) * w, c0[1] + ((k >> 2) & 3) * w, c0[2] + ((k >> 4) & 3) * w, w)
            out = [np.zeros(nseg * m * 8, np.float32) for _ in range(4)]
            ms = (C.c_float * 2)(); st = (C.c_uint32 * 2)()
            B.check(lib.goicp_debug_bounds_tile(h, _fp(np.ascontiguousarray(rr.reshape(-1))), _fp(par.reshape(-1)), nseg, m, level, chunks,
                                                _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), ms, st))
            # tile against direct: the same per-point terms, another summation order.  A tile lane adds the terms of its wavefront's share of a
            # chunk one after the other -- ceil(N / (4 chunks)) sequential float additions -- and under truncation most of them are the SAME
            # value g^2, so the roundings of a running sum line up instead of cancelling (the plain test's 3e-6 counts on cancellation):
            # the bar is the sequential sum's worst case, one half-ulp (2^-24 relative) per addition, plus 64 for the direct kernel's own tree
            bar = (-(-len(bunny_data10) // (4 * chunks)) + 64) * 2.0 ** -24
            for t, d in ((out[0], out[2]), (out[1], out[3])):
                assert np.all(np.abs(t - d) <= bar * np.maximum(np.abs(d), 1e-3)), ("tile", depth, m, float(np.max(np.abs(t - d) / np.maximum(np.abs(d), 1e-3))), bar)
            assert np.all(out[2] <= len(bunny_data10) * np.float32(g) ** 2 * (1 + 1e-5)) and np.all(out[3] <= out[2])
            p0 = oracle_mod.rotate(rr[0], bunny_data10)
            for c, kid in enumerate(_children(par[0, 0])):
                oub, olb = trunc_bound_f64(oracle_mod.cube_terms(oracle_dt_bunny, p0, rho10[level], kid[:3], kid[3]), kid[3], g)
                assert _close(out[0][c], oub) and _close(out[1][c], olb) and _close(out[2][c], oub) and _close(out[3][c], olb), ("tile vs twin", depth, c)
            if depth >= 8:
                assert st[0] > 0                                         # staged boxes: the LDS lookup path ran
        # (iv) one twin-fused round of the device queues against the per-cube evaluation and the twin
        out = [np.zeros(8 * n, np.float32) for _ in range(4)]
        info = (C.c_int32 * 2)()
        B.check(lib.goicp_debug_queue_expand(h, _fp(np.ascontiguousarray(R.reshape(-1).astype(np.float32))), level, _fp(np.ascontiguousarray(parents.reshape(-1))), n,
                                             _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), info))
        assert info[1] == 1                                              # the twin lists were in use
        for ps, (qu, ql) in enumerate(((out[0], out[1]), (out[2], out[3]))):
            for i in range(8 * n):
                assert _close(qu[i], want[(ps, i)][0]) and _close(ql[i], want[(ps, i)][1]), ("queue", ps, i)
                assert _close(qu[i], float(per_cube[ps][0][i])) and _close(ql[i], float(per_cube[ps][1][i])) and ql[i] <= qu[i]
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 2. identity
# ----------------------------------------------------------------------------------------------
def test_huge_truncation_is_the_plain_handle_bit_for_bit(pkg, bunny_model, bunny_data10):
    plain = pkg.Registration(bunny_model, bunny_data10, 1e-3)
    trunc = pkg.Registration(bunny_model, bunny_data10, 1e-3, trunc_dist=HUGE)
    assert trunc.search_truncation() == np.float32(HUGE) and plain.search_truncation() == 0.0
    rng = np.random.default_rng(31)
    try:
        for v in ROTS:
            R = pkg.fgoicp.rodrigues(v)
            cubes = _cubes(rng, 77)
            kids = np.concatenate([_children(p) for p in _parents(rng, 4, range(0, 6))])
            for level in (-1, 4):
                for batch in (cubes, kids):
                    a, b = plain.eval_bounds(R, batch, level), trunc.eval_bounds(R, batch, level)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            t = rng.uniform(-0.2, 0.2, 3).astype(np.float32)
            assert np.array_equal(plain.compute_sse_error(R, t), trunc.compute_sse_error(R, t))
            for level in (-1, 3):
                va, na, ca = plain.inner_bnb(R, level, 1e10)
                vb, nb, cb = trunc.inner_bnb(R, level, 1e10)
                assert np.array_equal(va, vb) and np.array_equal(na, nb) and (ca.trans_pops, ca.cubes) == (cb.trans_pops, cb.cubes)
        rots = np.stack([pkg.fgoicp.rodrigues(v) for v in ROTS])
        cubes = _cubes(rng, 512)
        recs = [(c[0], c[1], c[2], plain._lib.goicp_trans_delta(float(c[3])), plain.rot_coeff(5) if i % 2 else 0.0, int(i % 3)) for i, c in enumerate(cubes)]
        a, b = plain.eval_bounds_batch(rots, recs), trunc.eval_bounds_batch(rots, recs)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        plain.close(); trunc.close()
    res = []
    for kw in ({}, {"trunc_dist": HUGE}):
        eng = pkg.FastGoICP(bunny_model, bunny_data10, 1e-3, **kw)
        eng.run()
        c = eng.counters
        res.append((eng.optR.tobytes(), eng.optT.tobytes(), float(eng.get_best_error()), int(c.rot_pops), int(c.trans_pops), int(c.cubes), int(c.icp_runs), int(c.icp_iters)))
        eng.registration.close()
    assert res[0] == res[1], (res[0][2:], res[1][2:])


# ----------------------------------------------------------------------------------------------
# 3. validity as a property
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0.05, 0.15])
def test_lower_bound_holds_for_poses_inside_the_cubes(pkg, bunny_model, bunny_data10, g):
    """random rotation cubes (level l: width 2 pi / 2^l, radius goicp_rot_coeff(l), as the search uses them) x random translation cubes of
    levels 1..6, 32 poses sampled inside each pair: E_g(pose) >= lb(pair).  Both are float sums of at most N non-negative terms added as
    a tree over 256 lanes (about N / 256 + 10 sequential additions each): relative error below 30 x 2^-24 ~ 2e-6 each; the bar is 1e-5."""
    reg = pkg.Registration(bunny_model, bunny_data10, 1e-3, trunc_dist=g)
    rng = np.random.default_rng(41)
    pairs = positive = 0
    worst = np.inf
    try:
        for _ in range(48):
            lr = int(rng.integers(3, 9))
            wr = 2 * np.pi / (1 << lr)
            while True:
                r0 = rng.uniform(-np.pi, np.pi, 3)
                if np.linalg.norm(r0) <= np.pi:
                    break
            lt = int(rng.integers(1, 7))
            wt = np.float32(1.0 / (1 << lt))
            tc = (rng.uniform(-0.5, 0.5, 3) * (1 - wt)).astype(np.float32)
            R0 = pkg.fgoicp.rodrigues(r0.astype(np.float32))
            _, lb = reg.eval_bounds(R0, np.array([[tc[0], tc[1], tc[2], wt]], np.float32), lr)
            ub0, lb0 = reg.eval_bounds(R0, np.array([[tc[0], tc[1], tc[2], wt]], np.float32), -1)
            assert lb[0] <= lb0[0] <= ub0[0]
            pairs += 1
            positive += lb[0] > 0
            for _ in range(32):
                r = np.float32(r0) + rng.uniform(-0.5, 0.5, 3).astype(np.float32) * np.float32(wr)
                t = tc + rng.uniform(-0.5, 0.5, 3).astype(np.float32) * wt
                sse = float(reg.compute_sse_error(pkg.fgoicp.rodrigues(r), t))
                worst = min(worst, sse - float(lb[0]))
                assert sse >= float(lb[0]) * (1 - 1e-5), (g, lr, lt, sse, float(lb[0]))
        print("validity g = %g: %d pairs, %d with lb > 0, smallest E_g(pose) - lb %.3e" % (g, pairs, positive, worst))
        assert positive >= pairs // 4                                     # not vacuous
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 4. proven optimum on small clouds with outliers
# ----------------------------------------------------------------------------------------------
TINY_G = 0.15
TINY_MSE = 1e-3
TINY_SEEDS = (1, 2, 3, 6)


def tiny_outlier_problem(seed):
    """conftest.tiny_problem's construction (200 target / 60 source points of a seeded star-shaped surface under a seeded rigid motion) with
    the truth kept, plus 30 % outliers uniform in the moved source's bounding box.  -> (target, source, R_true, t_true)"""
    load_pkg()
    from cuda_go_icp_amd import synth
    amp = (0.35, 0.25, 0.30, 0.20)[seed % 4]
    tgt, src, R0, t0 = synth.make_pair(seed=7100 + seed, M=200, N=60, noise=0.004, amp=amp)
    rng = np.random.default_rng(9100 + seed)
    while True:
        v = rng.uniform(-np.pi, np.pi, 3)
        if np.linalg.norm(v) <= np.pi:
            break
    Rx = synth._rodrigues(v)
    tx = rng.uniform(-0.25, 0.25, 3)
    s2 = (src.astype(np.float64) - tx) @ Rx
    orng = np.random.default_rng(9300 + seed)
    out = orng.uniform(s2.min(0), s2.max(0), (int(0.3 * len(s2)), 3))
    return tgt, np.concatenate([s2, out]).astype(np.float32), R0 @ Rx, R0 @ tx + t0


def _run_with_limit(eng, seconds):
    """eng.run() with a time limit: past it the search is cancelled and the test fails"""
    timer = threading.Timer(seconds, eng.cancel)
    timer.start()
    t0 = time.perf_counter()
    try:
        eng.run()
    finally:
        timer.cancel()
    wall = time.perf_counter() - t0
    assert eng.finished and wall < seconds, "the registration did not finish inside %g s" % seconds
    return wall


@pytest.mark.parametrize("seed", TINY_SEEDS)
def test_tiny_with_outliers_proven_optimum(pkg, oracle_mod, seed):
    """SSEThresh = 1e-3 x 78 = 0.078 lies far below the optimum's cost (the 200-point target alone leaves the 60 true points 0.3-0.5 of
    squared distance), so there is no early exit: the search ends when every cube whose lower bound is SSEThresh under the incumbent has been
    refuted, i.e. best_sse <= min E_g + SSEThresh <= E_g(truth) + SSEThresh.  E_g(truth) < E_g(identity) on every seed (checked with the
    oracle alone on the CPU: the assertion is not met by the start pose)."""
    tgt, src, Rt, tt = tiny_outlier_problem(seed)
    dt = oracle_mod.DistanceTransform(tgt, 300, 2.0)
    e_truth = score_f64(oracle_mod, dt, src, Rt, tt, TINY_G)
    e_ident = score_f64(oracle_mod, dt, src, np.eye(3), np.zeros(3), TINY_G)
    assert e_truth < e_ident
    eng = pkg.FastGoICP(tgt, src, TINY_MSE, trunc_dist=TINY_G)
    try:
        thr = float(eng.sse_threshold)
        assert thr < 0.5 * e_truth
        wall = _run_with_limit(eng, 300.0)
        sse, c = float(eng.get_best_error()), eng.counters
        own = score_f64(oracle_mod, dt, src, eng.optR, eng.optT, TINY_G)
        print("tiny%d + outliers: %.2f s, best_sse %.6g, E_g(truth) %.6g, E_g(identity) %.6g, SSEThresh %.3g, rotation nodes %d, cube bounds %d, rot_error %.3e"
              % (seed, wall, sse, e_truth, e_ident, thr, c.rot_pops, c.cubes, rot_angle(eng.optR, Rt)))
        assert abs(sse - own) <= 1e-4 * max(own, 1e-3)                    # best_sse is E_g of the pose returned
        assert sse <= e_truth + thr, (sse, e_truth, thr)
    finally:
        eng.registration.close()


# ----------------------------------------------------------------------------------------------
# 5. clutter bunny, end to end
# ----------------------------------------------------------------------------------------------
BUNNY_G = 0.05
BUNNY_MSE = 1e-4
BUNNY_DEG = 75.0
BUNNY_T = np.array([0.08, -0.06, 0.05])
# [params.rotation] box, degrees per axis of the rotation vector.  The truth is (27.8, -55.7, 41.8), the start (0, 0, 0): both lie at least 20
# degrees inside every face.  The whole pi-ball is too slow to prove at this size inside a test's time limit (the plain search of it did not
# end in 420 s); the box is 1 / 36 of it
BUNNY_BOX = {"use_rot_range": 1, "rot_min": [-20.0, -90.0, -20.0], "rot_max": [60.0, 20.0, 75.0]}
BUNNY_LIMIT = 300.0            # seconds, truncated run
BUNNY_PLAIN_LIMIT = 60.0       # seconds, plain run (see the test)
# pose-error bar: the fp64 twin of gated ICP (tests/test_gpu_icp_gate.twin_icp, g = 0.05) started AT the truth ends 6.67e-5 rad / 1.48e-5
# from it (one iteration, 5 337 inliers) -- the nearest local optimum of the same objective on the exact distances -- plus two DT voxel
# widths (1 / scale = 1.168e-2 at dt_size 300 on this target) for the voxelised score that picks among refined poses; as an angle, two voxels
# over the largest radius of the target (the tightest conversion).  The same twin started at the identity ends 1.26 rad from the truth, the
# ungated one 0.118 rad: ICP alone does not undo this motion
BUNNY_TWIN_ROT, BUNNY_TWIN_TRANS = 6.67e-5, 1.48e-5


def _rodrigues64(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def clutter_bunny(deg=BUNNY_DEG, seed=20261016):
    """tests/test_gpu_icp_gate.clutter_case's generator under a larger motion: the bunny model as target; every 7th model point + N(0, 5e-4)
    moved by `deg` degrees about the skew axis (1, -2, 1.5) and BUNNY_T, plus 30 % clutter uniform in the bounding box grown by 0.1.
    -> (target, source, R_true, t_true): target ~= R_true s + t_true for the non-clutter points s"""
    tgt = cloud("model_bunny")
    rng = np.random.default_rng(seed)
    pts = tgt[::7].astype(np.float64) + rng.normal(scale=5e-4, size=(len(tgt[::7]), 3))
    R = _rodrigues64(np.array([1.0, -2.0, 1.5]) / np.linalg.norm([1.0, -2.0, 1.5]) * np.deg2rad(deg))
    t = BUNNY_T
    moved = (pts - t) @ R
    lo, hi = tgt.min(0).astype(np.float64) - 0.1, tgt.max(0).astype(np.float64) + 0.1
    clutter = rng.uniform(lo, hi, (int(0.3 * len(pts)), 3))
    src = np.concatenate([moved, clutter])
    return tgt, np.ascontiguousarray(src[rng.permutation(len(src))], np.float32), R, t


def test_clutter_bunny_truncated_search_with_gated_icp(pkg, oracle_mod, oracle_dt_bunny):
    """The truncated search with the gate g on the same handle proves its optimum (mse 1e-4: SSEThresh 0.67 against a floor of ~1 540
    clutter points x g^2) and ends nearer the truth, in angle and in translation, than the plain registration of the same clouds.  Both
    search the rotation box BUNNY_BOX (narrowed, as said there).  The truncated run has to END inside its time limit.  The plain run
    cannot: the clutter puts its sum of squares two orders of magnitude above SSEThresh and the search runs to exhaustion (the reason for
    this feature), so it is cancelled after BUNNY_PLAIN_LIMIT seconds and judged by the best pose it holds then -- ICP-refined like every
    pose it adopts; more time only lets it approach the plain objective's own optimum, which lies about 5e-2 rad from the truth."""
    tgt, src, Rt, tt = clutter_bunny()
    e_truth = score_f64(oracle_mod, oracle_dt_bunny, src, Rt, tt, BUNNY_G)
    res = {}
    for name, kw in (("plain", {}), ("truncated", {"trunc_dist": BUNNY_G, "max_corr_dist": BUNNY_G})):
        eng = pkg.FastGoICP(tgt, src, BUNNY_MSE, **BUNNY_BOX, **kw)
        try:
            if name == "plain":
                timer = threading.Timer(BUNNY_PLAIN_LIMIT, eng.cancel)
                timer.start()
                t0 = time.perf_counter()
                eng.run()
                wall = time.perf_counter() - t0
                timer.cancel()
            else:
                wall = _run_with_limit(eng, BUNNY_LIMIT)
            c = eng.counters
            res[name] = (float(eng.get_best_error()), rot_angle(eng.optR, Rt), float(np.linalg.norm(eng.optT.astype(np.float64) - tt)), float(eng.sse_threshold))
            print("clutter bunny %s: %.2f s, best_sse %.6g, rot_error %.3e rad, trans_error %.3e, rotation nodes %d, cube bounds %d, icp iterations %d"
                  % (name, wall, res[name][0], res[name][1], res[name][2], c.rot_pops, c.cubes, c.icp_iters))
        finally:
            eng.registration.close()
    sse, ang, dtr, thr = res["truncated"]
    print("E_g(truth) %.6g, SSEThresh %.4g" % (e_truth, thr))
    assert sse <= e_truth + thr, (sse, e_truth, thr)
    assert ang < res["plain"][1] and dtr < res["plain"][2], (res["truncated"], res["plain"])
    voxel, radius = 1.0 / oracle_dt_bunny.scale, float(np.linalg.norm(tgt.astype(np.float64), axis=1).max())
    assert ang <= BUNNY_TWIN_ROT + 2 * voxel / radius and dtr <= BUNNY_TWIN_TRANS + 2 * voxel, (ang, dtr, voxel, radius)


# ----------------------------------------------------------------------------------------------
# 6. refusals on a live handle
# ----------------------------------------------------------------------------------------------
def test_refusals_and_switching_off(pkg, bunny_model, bunny_data10):
    reg = pkg.Registration(bunny_model, bunny_data10, 1e-3)
    lib = reg._lib
    rng = np.random.default_rng(5)
    R = pkg.fgoicp.rodrigues([0.3, -0.2, 0.9])
    cubes = _cubes(rng, 64)
    t = np.array([0.01, 0.02, -0.01], np.float32)
    before = (reg.eval_bounds(R, cubes, 4), reg.compute_sse_error(R, t), reg.inner_bnb(R, 3, 1e10)[0])
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert lib.goicp_set_search_truncation(reg.handle, bad) == INVALID
    assert reg.search_truncation() == 0.0
    reg.set_search_truncation(0.02)
    during = (reg.eval_bounds(R, cubes, 4), reg.compute_sse_error(R, t), reg.inner_bnb(R, 3, 1e10)[0])
    assert np.all(during[0][0] <= before[0][0]) and np.any(during[0][0] < before[0][0]) and during[1] < before[1] and during[2] <= before[2]
    reg.set_search_truncation(0.0)                                       # off again: the plain bits
    after = (reg.eval_bounds(R, cubes, 4), reg.compute_sse_error(R, t), reg.inner_bnb(R, 3, 1e10)[0])
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and before[1] == after[1] and before[2] == after[2]
    reg.close()
    trimmed = pkg.Registration(bunny_model, bunny_data10, 1e-3, trim_fraction=0.1)
    assert lib.goicp_set_search_truncation(trimmed.handle, 0.05) == INVALID and b"trim" in lib.goicp_last_error()
    assert lib.goicp_set_search_truncation(trimmed.handle, 0.0) == 0
    trimmed.close()
    with pytest.raises(pkg.GoicpError):
        pkg.Registration(bunny_model, bunny_data10, 1e-3, trim_fraction=0.1, trunc_dist=0.05)
    # during a registration: from the progress callback, on the registering thread
    eng = pkg.FastGoICP(bunny_model, bunny_data10, 1e-3, trunc_dist=0.15)
    rcs = []
    CB = C.CFUNCTYPE(None, C.POINTER(pkg.binding.CResult), C.c_void_p)
    cb = CB(lambda r, u: rcs.append((lib.goicp_set_search_truncation(eng.registration.handle, 0.05), lib.goicp_set_search_truncation(eng.registration.handle, 0.0))))
    pkg.binding.check(lib.goicp_set_progress_callback(eng.registration.handle, C.cast(cb, C.c_void_p), None))
    th = threading.Thread(target=eng.run)
    th.start(); th.join()
    pkg.binding.check(lib.goicp_set_progress_callback(eng.registration.handle, None, None))
    assert rcs and all(rc == (INVALID, INVALID) for rc in rcs)
    assert eng.registration.search_truncation() == np.float32(0.15)
    assert lib.goicp_set_search_truncation(eng.registration.handle, 0.05) == 0
    eng.registration.close()
