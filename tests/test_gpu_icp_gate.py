"""Distance-gated ICP (goicp_set_icp_gate): a correspondence takes part in an iteration iff the walk's d^2 <= max_corr_dist^2.

What is held here, on the committed clouds and on a seeded clutter case (the bunny model as target; every 7th model point + N(0, 5e-4)
noise, moved by 10 degrees and (0.02, -0.015, 0.01), plus 30 % clutter points uniform in the bounding box grown by 0.1 as source):
identity with the ungated run while nothing is rejected, the inlier set against goicp_nn_query, an fp64 numpy twin of the semantics,
robustness against clutter, the batch, reproducibility and launch-shape independence (capped and full walk), the degenerate gate, the
refusals, and the gate inside goicp_register and the collective loop.  Every test needs the entry points this feature adds.

Bars: the project's own for ICP against its oracle: 1e-4 absolute on R, t after 1 / 2 / 10 iterations, 1e-3 converged."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import cloud, golden, load_pkg, rot_angle, skull_problem

pytestmark = pytest.mark.gpu
INVALID = -1
TRUTH_T = np.array([0.02, -0.015, 0.01])
GATES = (0.15, 0.05, 0.02)


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _rodrigues(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _truth_R(deg=10.0):
    return _rodrigues(np.array([1.0, -2.0, 1.5]) / np.linalg.norm([1.0, -2.0, 1.5]) * np.deg2rad(deg))


def clutter_case(deg=10.0, seed=20261016):
    """-> (target, source, R_true, t_true): target ~= R_true s + t_true for the non-clutter points s of the source"""
    tgt = cloud("model_bunny")
    rng = np.random.default_rng(seed)
    pts = tgt[::7].astype(np.float64) + rng.normal(scale=5e-4, size=(len(tgt[::7]), 3))
    R, t = _truth_R(deg), TRUTH_T
    moved = (pts - t) @ R                                             # s = R^T (p - t)
    lo, hi = tgt.min(0).astype(np.float64) - 0.1, tgt.max(0).astype(np.float64) + 0.1
    clutter = rng.uniform(lo, hi, (int(0.3 * len(pts)), 3))
    src = np.concatenate([moved, clutter])
    return tgt, np.ascontiguousarray(src[rng.permutation(len(src))], np.float32), R, t


def _run(reg, R=None, t=None, max_iter=10000, err_diff=1e-7):
    R = np.array(np.eye(3) if R is None else R, np.float32).reshape(9).copy()
    t = np.array(np.zeros(3) if t is None else t, np.float32).reshape(3).copy()
    err, it = C.c_float(), C.c_int32()
    rc = reg._lib.goicp_icp_run(reg.handle, _fptr(R), _fptr(t), int(max_iter), float(err_diff), C.byref(err), C.byref(it))
    assert rc == 0, reg._lib.goicp_last_error()
    return R.reshape(3, 3), t, np.float32(err.value), it.value


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _transform_f32(R, t, p):
    """the pass's expression (jly_icp3d.hpp:222-224): left-to-right float sums"""
    R, t, p = np.asarray(R, np.float32).reshape(3, 3), np.asarray(t, np.float32), np.asarray(p, np.float32)
    return np.stack([((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a] for a in range(3)], 1).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# the fp64 twin of the semantics
# ----------------------------------------------------------------------------------------------
def twin_icp(tree, tgt, src, g, max_iter, err_diff=1e-7, R=None, t=None, min_inliers=3):
    """-> (R, t, err, iters, n_in, dist of the last pass).  Neighbours: cKDTree; inliers d^2 <= g2; Kabsch over the inliers with the
    reference's carried means (jly_icp3d.hpp:244-263); stop on the truncated cost C = err + (N - n_in) g2."""
    tgt, src = tgt.astype(np.float64), src.astype(np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    N, g2 = len(src), float(np.float32(g) * np.float32(g))
    mu_m, mu_d, cost, err, n_in, iters, d = np.zeros(3), np.zeros(3), -1.0, 0.0, 0, 0, None
    for _ in range(max_iter):
        q = src @ R.T + t
        d, j = tree.query(q)
        inl = d * d <= g2
        n_in, err = int(inl.sum()), float((d[inl] ** 2).sum())
        c_new = err + (N - n_in) * g2
        if n_in < min_inliers or (cost > 0 and cost - c_new < err_diff * N):
            break
        qi, mi = q[inl], tgt[j[inl]]
        mu_d, mu_m = (mu_d + qi.sum(0)) / n_in, (mu_m + mi.sum(0)) / n_in
        H = (qi - mu_d).T @ (mi - mu_m)
        U, _, Vt = np.linalg.svd(H)
        Rk = Vt.T @ np.diag([1, 1, np.linalg.det(Vt.T @ U.T)]) @ U.T
        tk = mu_m - Rk @ mu_d
        R, t, cost, iters = Rk @ R, Rk @ t + tk, c_new, iters + 1
    return R, t, err, iters, n_in, d


@pytest.fixture(scope="module")
def clutter(pkg):
    from scipy.spatial import cKDTree
    tgt, src, Rt, tt = clutter_case()
    reg = pkg.Registration(tgt, src, 1e-3)
    yield reg, tgt, src, Rt, tt, cKDTree(tgt.astype(np.float64))
    reg.close()


# ----------------------------------------------------------------------------------------------
# 1. identity
# ----------------------------------------------------------------------------------------------
def _pairs():
    skull_t, skull_s, _, _ = skull_problem()
    return {"bunny": (cloud("model_bunny"), cloud("data_bunny")), "skull": (skull_t, skull_s),
            "spanner": (cloud("spanner_target"), cloud("spanner_source"))}


@pytest.mark.parametrize("name", ["bunny", "skull", "spanner"])
def test_identity_when_nothing_is_rejected(pkg, name):
    tgt, src = _pairs()[name]
    extent = float(max((tgt.max(0) - tgt.min(0)).max(), (src.max(0) - src.min(0)).max()))
    reg = pkg.Registration(tgt, src, 1e-3)
    try:
        for metric in (0, 1):
            reg.set_icp_options(metric, 16)
            for max_iter in (3, 60):
                reg.set_icp_gate(0.0)
                ref = _run(reg, max_iter=max_iter)
                assert list(reg.icp_inliers(1)) == [len(src)]
                for capped in (1, 0):
                    reg.set_icp_gate(10 * extent, capped_walk=capped)
                    out = _run(reg, max_iter=max_iter)
                    assert _same(out, ref), (name, metric, max_iter, capped, out[2:], ref[2:])
                    assert list(reg.icp_inliers(1)) == [len(src)]
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 2. inlier set
# ----------------------------------------------------------------------------------------------
def test_inlier_set_is_nn_query_thresholded(pkg, clutter):
    reg, tgt, src, Rt, tt, _ = clutter
    poses = [(np.eye(3), np.zeros(3)), (Rt, tt), (_rodrigues([0.3, -0.2, 0.5]), np.array([0.05, 0.02, -0.04]))]
    for g in GATES:
        g2 = np.float32(g) * np.float32(g)
        for R, t in poses:
            q = _transform_f32(R, t, src)
            idx, d2 = reg.nn_query(q)
            inl = d2 <= g2
            eidx, ed2, n, sse = reg.eval_correspondences(R, t, g)
            assert np.array_equal(ed2.view(np.uint32), d2.view(np.uint32))
            assert np.array_equal(eidx, np.where(inl, idx, -1))
            assert n == int(inl.sum()) and 0 < n < len(src)
            assert sse == np.float32(np.cumsum(d2[inl].astype(np.float64))[-1])    # the operator's sum: double, in source order
            for capped in (1, 0):
                reg.set_icp_gate(g, capped_walk=capped)
                _, _, err, _ = _run(reg, R, t, max_iter=1)
                assert list(reg.icp_inliers(1)) == [n]
                assert abs(float(err) - float(sse)) <= 1e-5 * float(sse)         # the same terms, summed in another order
    # no gate: every point, the plain neighbour
    eidx, ed2, n, _ = reg.eval_correspondences(Rt, tt, 0.0)
    idx, d2 = reg.nn_query(_transform_f32(Rt, tt, src))
    assert n == len(src) and np.array_equal(eidx, idx) and np.array_equal(ed2, d2)
    reg.set_icp_gate(0.0)


# ----------------------------------------------------------------------------------------------
# 3. twin, 4. robustness
# ----------------------------------------------------------------------------------------------
def _boundary_points(d, g, tol, src):
    """points of the twin's last pass whose distance lies within the pose disagreement of the gate: a pose within `tol` per element of
    R and t moves a point p by at most ||dR||_F |p| + |dt| <= 3 tol |p| + sqrt(3) tol"""
    delta = 3 * tol * float(np.linalg.norm(src, axis=1).max()) + np.sqrt(3) * tol
    return int((np.abs(d - g) <= delta).sum()), delta


@pytest.mark.parametrize("g", GATES)
def test_twin(pkg, clutter, g):
    reg, tgt, src, Rt, tt, tree = clutter
    reg.set_icp_options(0, 16)
    reg.set_icp_gate(g)
    try:
        for max_iter, tol in ((1, 1e-4), (2, 1e-4), (10, 1e-4), (10000, 1e-3)):
            R, t, err, it = _run(reg, max_iter=max_iter)
            n = int(reg.icp_inliers(1)[0])
            tR, tt_, terr, tit, tn, td = twin_icp(tree, tgt, src, g, max_iter)
            dR, dt = float(np.abs(R - tR).max()), float(np.abs(t - tt_).max())
            nb, delta = _boundary_points(td, g, tol, src)
            print("gate %.2f max_iter %5d: |dR| %.2e |dt| %.2e (bar %.0e); iters %d / twin %d; inliers %d / twin %d (boundary points within %.1e: %d); "
                  "err %.6g / twin %.6g" % (g, max_iter, dR, dt, tol, it, tit, n, tn, delta, nb, err, terr))
            assert dR <= tol and dt <= tol, (g, max_iter, dR, dt)
            assert abs(n - tn) <= nb, (g, max_iter, n, tn, nb)
            if max_iter <= 10:
                assert it == tit
    finally:
        reg.set_icp_gate(0.0)


def test_robust_to_clutter(pkg, clutter):
    reg, tgt, src, Rt, tt, tree = clutter
    reg.set_icp_options(0, 16)
    reg.set_icp_gate(0.0)
    R0, t0, _, it0 = _run(reg)
    ang0, d0 = rot_angle(R0, Rt), float(np.linalg.norm(t0 - tt))
    print("ungated: %.3e rad / %.3e from the truth, %d iterations" % (ang0, d0, it0))
    try:
        for g in GATES:
            reg.set_icp_gate(g)
            R, t, _, it = _run(reg)
            tR, tt_, _, tit, _, _ = twin_icp(tree, tgt, src, g, 10000)
            ang, d = rot_angle(R, Rt), float(np.linalg.norm(t - tt))
            tang, td = rot_angle(tR, Rt), float(np.linalg.norm(tt_ - tt))
            print("gate %.2f: %.3e rad / %.3e from the truth, %d iterations (twin %.3e / %.3e, %d)" % (g, ang, d, it, tang, td, tit))
            # within the twin's distance of the truth plus the converged bar (1e-3 per element: 3e-3 as a rotation's chord, sqrt(3) e-3 as a vector)
            assert ang <= tang + 3e-3 and d <= td + np.sqrt(3) * 1e-3, (g, ang, tang, d, td)
            assert ang0 >= 10 * ang, (g, ang0, ang)
    finally:
        reg.set_icp_gate(0.0)


# ----------------------------------------------------------------------------------------------
# 5. batch
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_batch_equals_single_runs(pkg, clutter, metric):
    reg = clutter[0]
    rng = np.random.default_rng(5)
    # eight starts near the identity (one basin), eight far from it (turns of up to ~90 degrees, shifts of up to 0.3: other local minima)
    R0 = np.array([_rodrigues(rng.normal(size=3) * (0.12 if k < 8 else 0.9)) for k in range(16)], np.float32)
    t0 = np.array([rng.uniform(-1, 1, 3) * (0.04 if k < 8 else 0.3) for k in range(16)], np.float32)
    R0[0], t0[0] = np.eye(3), 0
    reg.set_icp_options(metric, 16)
    try:
        for g, capped in ((0.05, 1), (0.02, 0)):
            reg.set_icp_gate(g, capped_walk=capped)
            R, t, err, it = reg.icp_run_batch(R0, t0, 200, 1e-7)
            nb = reg.icp_inliers(16)
            with pytest.raises(pkg.GoicpError):
                reg.icp_inliers(15)                                  # K must be the last run's
            for k in range(16):
                sR, st, se, si = _run(reg, R0[k], t0[k], 200, 1e-7)
                assert np.array_equal(R[k], sR) and np.array_equal(t[k], st) and err[k] == se and it[k] == si, (metric, g, k)
                assert int(reg.icp_inliers(1)[0]) == int(nb[k]), (metric, g, k)
            print("batch metric %d gate %.2f: inliers %s iters %s" % (metric, g, sorted(set(nb.tolist())), sorted(set(it.tolist()))))
            assert len(set(nb.tolist())) > 1                          # starts that end with different inlier sets are among them
    finally:
        reg.set_icp_gate(0.0)
        reg.set_icp_options(0, 16)


# ----------------------------------------------------------------------------------------------
# 6. reproducibility, launch shape, capped and full walk
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_reproducible_and_walk_independent(pkg, clutter, metric):
    reg = clutter[0]
    reg.set_icp_options(metric, 16)
    try:
        for g in GATES:
            outs = []
            for capped in (1, 1, 0):
                reg.set_icp_gate(g, capped_walk=capped)
                outs.append(_run(reg, max_iter=300) + (int(reg.icp_inliers(1)[0]),))
            assert _same(outs[0], outs[1]) and _same(outs[0], outs[2]), (metric, g, [o[2:] for o in outs])
    finally:
        reg.set_icp_gate(0.0)
        reg.set_icp_options(0, 16)


def test_million_points_reproducible(pkg):
    """S2 (N = M = 1 M: the neighbour pass, a three-level tree): the same gated run twice and with the full walk, bit-equal; the inlier
    count of the first pass is goicp_eval_correspondences' at the start pose"""
    from cuda_go_icp_amd import synth
    model, data, Rgt, tgt = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"])
    reg = pkg.Registration(model, data, 1e-3, dt_size=synth.S2["V"])
    try:
        R0, t0 = _rodrigues([0.02, -0.03, 0.01]) @ Rgt, tgt + np.array([0.01, -0.02, 0.015])    # near the truth: part of the cloud inside the gate
        g = 0.03
        outs = []
        for capped in (1, 1, 0):
            reg.set_icp_gate(g, capped_walk=capped)
            outs.append(_run(reg, R0, t0, max_iter=4) + (int(reg.icp_inliers(1)[0]),))
        assert _same(outs[0], outs[1]) and _same(outs[0], outs[2]), [o[2:] for o in outs]
        _run(reg, R0, t0, max_iter=1)
        n = reg.eval_correspondences(R0, t0, g)[2]
        assert int(reg.icp_inliers(1)[0]) == n and 0 < n < len(data)
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 7. degenerate, refusals
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_gate_below_every_distance(pkg, clutter, metric):
    reg, _, src, _, _, _ = clutter
    d2 = reg.eval_correspondences(np.eye(3), np.zeros(3), 0.0)[1]
    g = float(np.sqrt(d2.min())) * 0.5
    assert g > 0
    reg.set_icp_options(metric, 16)
    try:
        for capped in (1, 0):
            reg.set_icp_gate(g, capped_walk=capped)
            R, t, err, it = _run(reg)                                # status GOICP_OK (asserted in _run)
            assert np.array_equal(R, np.eye(3, dtype=np.float32)) and not t.any() and it == 0 and err == 0
            assert int(reg.icp_inliers(1)[0]) == 0
            # a settable floor: more inliers than the floor asks for are still too few for a larger min_inliers
            reg.set_icp_gate(0.05, min_inliers=len(src), capped_walk=capped)
            R, t, err, it = _run(reg)
            n = int(reg.icp_inliers(1)[0])
            assert np.array_equal(R, np.eye(3, dtype=np.float32)) and not t.any() and it == 0 and 6 < n < len(src) and err > 0
    finally:
        reg.set_icp_gate(0.0)
        reg.set_icp_options(0, 16)


def _set(reg, dist, min_inliers=0, capped=1):
    g = reg._lib.goicp_set_icp_gate.argtypes[1]._type_(dist, min_inliers, capped)
    return reg._lib.goicp_set_icp_gate(reg.handle, C.byref(g))


def test_refusals(pkg):
    model, data = cloud("model_bunny"), cloud("data_bunny", 10)
    reg = pkg.Registration(model, data, 1e-3)
    lib = reg._lib
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert _set(reg, bad) == INVALID
    assert _set(reg, 0.1, min_inliers=2) == INVALID and _set(reg, 0.1, min_inliers=-1) == INVALID and _set(reg, 0.1, capped=2) == INVALID
    assert _set(reg, 0.1, min_inliers=3) == 0 and _set(reg, 0.1) == 0    # back to the metric's own floor: the metric may change
    reg.set_icp_options(1, 16)
    assert _set(reg, 0.1, min_inliers=5) == INVALID and _set(reg, 0.1, min_inliers=6) == 0
    reg.set_icp_options(0, 16)
    assert _set(reg, 0.1, min_inliers=4) == 0
    with pytest.raises(pkg.GoicpError):
        reg.set_icp_options(1, 16)                                  # the gate's explicit floor is below point-to-plane's
    assert _set(reg, 0.1) == 0
    _run(reg, max_iter=2)
    out = np.zeros(4, np.int32)
    assert lib.goicp_icp_inliers(reg.handle, 2, out.ctypes.data_as(C.POINTER(C.c_int32))) == INVALID
    assert lib.goicp_icp_inliers(reg.handle, 1, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0 and 0 < out[0] <= len(data)
    I, Z = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
    assert lib.goicp_eval_correspondences(reg.handle, _fptr(I), _fptr(Z), -1.0, None, None, None, None) == INVALID
    assert lib.goicp_eval_correspondences(reg.handle, _fptr(I), _fptr(Z), 0.1, None, None, None, None) == 0
    reg.close()
    trimmed = pkg.Registration(model, data, 1e-3, trim_fraction=0.1)
    assert _set(trimmed, 0.1) == INVALID and b"trim" in lib.goicp_last_error() and _set(trimmed, 0.0) == 0
    trimmed.close()
    linear = pkg.Registration(model, data, 1e-3, dt_layout=0, dt_size=96)
    assert _set(linear, 0.1) == INVALID and b"dt_layout" in lib.goicp_last_error()
    linear.close()
    fused = pkg.Registration(model, data, 1e-3, icp_fused=1)
    assert _set(fused, 0.1) == INVALID and b"icp_fused" in lib.goicp_last_error()
    fused.close()
    with pytest.raises(pkg.GoicpError):
        pkg.Registration(model, data, 1e-3, trim_fraction=0.1, max_corr_dist=0.1)
    # during a registration: from the progress callback, on the registering thread
    eng = pkg.FastGoICP(model, data, 1e-3)
    rcs = []
    CB = C.CFUNCTYPE(None, C.POINTER(pkg.binding.CResult), C.c_void_p)
    cb = CB(lambda r, u: rcs.append(_set(eng.registration, 0.1)))
    pkg.binding.check(lib.goicp_set_progress_callback(eng.registration.handle, C.cast(cb, C.c_void_p), None))
    th = threading.Thread(target=eng.run)
    th.start(); th.join()
    pkg.binding.check(lib.goicp_set_progress_callback(eng.registration.handle, None, None))
    assert rcs and all(rc == INVALID for rc in rcs)
    assert _set(eng.registration, 0.1) == 0
    eng.registration.close()


# ----------------------------------------------------------------------------------------------
# 8. registration, collective loop
# ----------------------------------------------------------------------------------------------
def test_register_with_a_gate_that_holds_every_point(pkg):
    from test_gpu_parity import POSE_TOL, _pose_close
    model, data = cloud("model_bunny"), cloud("data_bunny", 10)
    g = golden("e2e_bunny10")
    eng = pkg.FastGoICP(model, data, g["mse_threshold"], max_corr_dist=0.5)
    try:
        eng.run()
        sse = float(eng.get_best_error())
        _pose_close("gated register bunny/10", eng.optR, eng.optT, g, POSE_TOL, sse=sse)
        assert sse < g["sse_threshold"]
        assert eng.registration.eval_correspondences(eng.optR, eng.optT, 0.5)[2] == len(data)   # the gate holds every point at the optimum
    finally:
        eng.registration.close()


def test_collective_gate(pkg):
    from cuda_go_icp_amd import sharded
    tgt, src, _, _ = clutter_case()
    R0, t0 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    regs = [pkg.Registration(tgt, src, 1e-3) for _ in range(2)]
    try:
        regs[0].set_icp_gate(0.05)
        out = sharded.icp_run_thread_ranks(regs, R0, t0, raise_on_error=False)      # one rank gated, one not
        assert [o[0] for o in out] == [INVALID, INVALID]
        regs[1].set_icp_gate(0.02)
        out = sharded.icp_run_thread_ranks(regs, R0, t0, raise_on_error=False)      # different gates
        assert [o[0] for o in out] == [INVALID, INVALID]
        regs[1].set_icp_gate(0.05)
        ref = _run(regs[0], R0, t0)
        w1 = sharded.icp_run_thread_ranks(regs[:1], R0, t0)[0]
        assert w1[0] == 0 and _same((w1[2], w1[3], w1[1], w1[4]), ref)
        for rc, e, R, t, it in sharded.icp_run_thread_ranks(regs, R0, t0):
            assert rc == 0 and _same((R, t, e, it), ref)
        assert regs[0].icp_shard_stats()["sliced"] == 0                            # replicated, as point-to-plane
    finally:
        for r in regs:
            r.close()
