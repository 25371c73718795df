"""The ICP pose solvers on planar, linear and singular correspondences: the three-lane Kabsch routine (device.hip kabsch_rows) alone, and the
6x6 Gauss-Newton solve (icp_plane_finalize_body) through one iteration and through the loop, each against the fp64 references of
tests/degenerate_twin.py.  tests/test_icp_degenerate_host.py holds those references and the inputs on the CPU: the ranks asserted here, the
eigenvalue gaps around the rank rule and the margin by which every correspondence is fixed.

  a  goicp_debug_kabsch on 36 matrices H: rank 2, 1, near-rank-1, tied and sign-flipped singular values, scales 1e-30 and 1e+30, the exact forms
     diag(1, .5, 0) and e_i e_j^T.  Every result is finite, |R^T R - I| <= 1e-5, det > 0 and attains tr(R H) >= (1 - 1e-5) (s1 + s2 + d s3); where
     the optimum is unique, (s2 + d s3) / s1 >= KABSCH_COND, |R - kabsch64(H)| <= 1e-5, the bar of test_device_svd_golden
  b  one iteration on the 17 x 17 lattice plane at five tilts, metric 1 plain, gated and Huber, symmetric, generalized: nn_query == nn_brute, the
     matrix has the rank the host test established, the pose equals the twin's minimum-norm step within 1e-5 (PLANE_POSE; the bar of
     test_one_iteration_vs_fp64_twin of the symmetric and the generalized file), iters == 1 and the pose moved; a batch of two reproduces the bits
  c  the metric-1 loop, max_iter 20, err_diff 1e-9: it stops before 20, ends within iters x PLANE_POSE of the twin loop, on the plane (rms <=
     1e-5), and its motion in the plane's three free directions is the twin's within the same bar
  d  point-to-point on the line at five tilts and on a target of which only one point is ever matched: every pose of five iterations (five
     chained one-iteration runs, see _five_iterations) is a rotation, the error never increases beyond the float rounding of the pose, and the
     single matched point gives a pure translation

Every test prints what it measured.  On MI355X, 72 tests, 2.2 s in all:

The build before the fixes (the same tests, the library of the parent commit): 29 of 72 fail.
  a  all nine e_i e_j^T: the result is H^T itself, two zero rows, det 0 -- not a rotation.  The other 27 pass, the rank-2 cross product, every tie
     and both scales among them
  b  14 of 25: a zero step (iters 1, pose unchanged, |dR| 1.7e-2 .. 2.1e-2, |dt| 7.1e-3 .. 1.0e-2 from the twin) for metric 1 plain, gated and
     Huber at the three general tilts and for the symmetric form at all five.  Axis-parallel and 45-degree planes pass metric 1 (the null block
     is exact zeros there and the shift alone keeps the pivots positive); the generalized form is full rank and passes everywhere
  c  the three general tilts: the loop counts the zero step, the next pass sees the same error and it reports convergence after "1
     iteration" at the start pose, plane rms 1.13e-2
  d  the line parallel to x and the one at 45 degrees: R with a zero row (H has two exact zero columns).  The three general tilts return
     rotations (the float rounding of the line makes H full rank).  The one-point target: a turn of |R1 - R0| = 1.47 from an H that is the
     rounding of its own terms (the error does not see it: every point has the same neighbour)
With the fixes all 72 pass; the worst deviation against each bar:
  a  |R^T R - I| 6.4e-8 (bar 1e-5); objective short of the optimum by 2.0e-8 of s1 (1e-5); |R - kabsch64| 3.0e-8 over the 23 unique cases (1e-5)
  b  metric 1 plain and gated |dR| 2.8e-8 |dt| 6.1e-10, Huber 2.8e-8 / 1.4e-9, symmetric 2.8e-8 / 9.7e-10, generalized 2.6e-7 / 6.2e-7 (1e-5 each);
     ranks 3, 3, 3, 3, 6; every batch slot the single run's bits
  c  2 iterations at every tilt; |dR| 2.8e-8 |dt| 7.5e-10 (bar 2e-5); plane rms 6.0e-9 (1e-5); turn about the normal within 2.6e-10 of the
     twin's (2e-5); the slide is 2.12e-4 as the twin's -- the second-order motion of the minimum-norm step itself -- and the loop does not spin
  d  line: errors 2.166e-3 -> <= 1.6e-14 and never above 1.9e-14 afterwards (floor 2 DQ sqrt(5 a) + 5 DQ^2 = 1.4e-11 there), landed within 6.0e-8
     of the matched points; one point: 2.171e-2 -> 1.250e-2 and flat, R1 == R0, the moved centroid 3.4e-9 from the point
"""
import ctypes as C

import numpy as np
import pytest

import degenerate_twin as D
from conftest import load_pkg
from test_gpu_icp_gate import _run, _same
from test_gpu_scale_parity import TOL_ICP
from test_gpu_small_shapes import KABSCH_COND, PLANE_POSE, _is_rotation
from test_icp_robust_host import HUBER, robust_w

pytestmark = pytest.mark.gpu
f32 = np.float32
KABSCH_BAR = 1e-5            # test_device_svd_golden's
ONE_ITER_POSE = {1: PLANE_POSE, 2: 1e-5, 3: 1e-5}     # test_one_iteration_vs_fp64_twin (symmetric), test_one_iteration_vs_twin (generalized)
HUBER_SCALE = 0.01           # the plane residuals at the start pose lie in 0 .. 0.02: the weights differ
FORMS = ["plain", "gate", "huber", "symmetric", "generalized"]
KABSCH = D.kabsch_cases()


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


# ----------------------------------------------------------------------------------------------
# a. the Kabsch routine alone
# ----------------------------------------------------------------------------------------------
def _device_kabsch(pkg, H):
    lib = pkg.load_library()
    H = np.ascontiguousarray(H, f32).reshape(9)
    R = np.full(9, np.nan, f32)
    fp = C.POINTER(C.c_float)
    pkg.binding.check(lib.goicp_debug_kabsch(H.ctypes.data_as(fp), R.ctypes.data_as(fp)))
    return R.reshape(3, 3)


@pytest.mark.parametrize("name", list(KABSCH))
def test_kabsch_on_degenerate_covariances(pkg, name):
    H = KABSCH[name]
    R = _device_kabsch(pkg, H)
    R64 = R.astype(np.float64)
    Rt, s, d = D.kabsch64(H)
    gap, best = D.kabsch_gap(H), D.kabsch_optimum(H)
    got = D.kabsch_objective(R, H)
    orth = float(np.abs(R64.T @ R64 - np.eye(3)).max()) if np.isfinite(R).all() else float("nan")
    dev = float(np.abs(R64 - Rt).max())
    print("%-16s gap %.3e: |R^T R - I| %.2e det %+.6f objective %.9g of %.9g (short by %.2e rel)%s"
          % (name, gap, orth, np.linalg.det(R64), got, best, (best - got) / s[0], ", |R - kabsch64| %.2e" % dev if gap >= KABSCH_COND else ""))
    assert np.isfinite(R).all(), (name, R)
    assert orth <= 1e-5 and np.linalg.det(R64) > 0, (name, orth, np.linalg.det(R64), R)
    assert got >= (1 - 1e-5) * best, (name, got, best)
    if gap >= KABSCH_COND:
        assert dev <= KABSCH_BAR, (name, dev)


# ----------------------------------------------------------------------------------------------
# b. one iteration on the planes
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(range(len(D.TILTS))), ids=D.TILT_IDS)
def plane_case(pkg, request):
    tilt = D.TILTS[request.param]
    tgt, src, sel = D.plane(tilt)
    reg = pkg.Registration(tgt, src, 1e-3, icp_metric=1, normal_k=8, source_normal_k=8, dt_size=32)
    R0, t0 = D.start(tilt)
    yield {"tilt": tilt, "reg": reg, "tgt": tgt, "src": src, "sel": sel, "R0": R0, "t0": t0, "n0": D.frame(tilt)[:, 2]}
    reg.close()


def _set_form(reg, form):
    """-> (the metric the pass runs, the twin's weight function)"""
    if form == "gate":
        reg.set_icp_gate(10.0)                                         # above every distance
    if form == "huber":
        reg.set_icp_robust(HUBER, HUBER_SCALE)
        return 1, lambda r: robust_w(HUBER, HUBER_SCALE, r)
    if form == "symmetric":
        reg.set_icp_symmetric(True, 8)
        return 2, None
    if form == "generalized":
        reg.set_icp_generalized(True, D.GICP_EPS, 8)
        return 3, None
    return 1, None


def _clear_form(reg):
    reg.set_icp_gate(0.0)
    reg.set_icp_robust(0)
    reg.set_icp_symmetric(False, 8)
    reg.set_icp_generalized(False, D.GICP_EPS, 8)


def _twin_system(c, metric, R, t, weight=None):
    """(A, b) at the pose from the device's own neighbours and normals"""
    reg = c["reg"]
    idx, _ = reg.nn_query(D.q32(R, t, c["src"]))
    ns = reg.source_normals() if metric >= 2 else None
    return D.system(metric, c["src"], c["tgt"], R, t, idx, reg.target_normals(), ns, weight)


@pytest.mark.parametrize("form", FORMS)
def test_one_iteration_on_a_plane(pkg, oracle_mod, plane_case, form):
    c = plane_case
    reg, R0, t0 = c["reg"], c["R0"], c["t0"]
    try:
        metric, weight = _set_form(reg, form)
        q = D.q32(R0, t0, c["src"])
        idx, d2 = reg.nn_query(q)
        bi, bd2 = oracle_mod.nn_brute(c["tgt"], q)
        assert np.array_equal(idx, bi) and np.array_equal(d2.view(np.uint32), bd2.view(np.uint32)) and np.array_equal(idx, c["sel"])
        nm = reg.target_normals()
        if not any(c["tilt"]):
            assert np.array_equal(np.abs(nm), np.tile(np.array([0, 0, 1], f32), (len(nm), 1)))
        assert np.abs(np.abs(nm.astype(np.float64) @ c["n0"]) - 1).max() <= 1e-6
        A, b = _twin_system(c, metric, R0, t0, weight)
        x, rank = D.min_norm_step(A, b)
        assert rank == D.PLANE_RANK[metric], (form, rank, D.spectrum(A))
        Rt, tt = D.compose(c["src"], R0, t0, x)
        R1, t1, e1, it = _run(reg, R0, t0, max_iter=1)
        dR, dt = float(np.abs(R1 - Rt).max()), float(np.abs(t1 - tt).max())
        moved = float(np.abs(t1.astype(np.float64) - t0).max())
        print("%s %s: rank %d, |dR| %.2e |dt| %.2e (bar %.0e), iters %d, moved %.2e of the twin's %.2e"
              % (D.TILT_IDS[D.TILTS.index(c["tilt"])], form, rank, dR, dt, ONE_ITER_POSE[metric], it, moved, np.abs(tt - t0).max()))
        assert it == 1, (form, it)
        assert moved >= 1e-3 and R1.tobytes() != R0.tobytes(), (form, moved)          # a zero step cannot pass
        assert dR <= ONE_ITER_POSE[metric] and dt <= ONE_ITER_POSE[metric], (form, dR, dt)
        # a batch of two, this start in either slot, reproduces the single run bit for bit
        Rb, tb = np.stack([R0, np.eye(3, dtype=f32)]), np.stack([t0, np.zeros(3, f32)])
        for slot in (0, 1):
            bR, bt, berr, bit = reg.icp_run_batch(Rb[::-1] if slot else Rb, tb[::-1] if slot else tb, 1, 1e-7)
            assert np.array_equal(bR[slot], R1) and np.array_equal(bt[slot], t1) and berr[slot] == e1 and bit[slot] == it, (form, slot)
    finally:
        _clear_form(reg)


# ----------------------------------------------------------------------------------------------
# c. the loop
# ----------------------------------------------------------------------------------------------
def test_loop_on_a_plane(pkg, plane_case):
    c = plane_case
    reg, src, R0, t0, n0 = c["reg"], c["src"], c["R0"], c["t0"], c["n0"]
    R1, t1, err, it = _run(reg, R0, t0, max_iter=20, err_diff=1e-9)
    R, t = R0.astype(np.float64), t0.astype(np.float64)
    for _ in range(it):
        A, b = _twin_system(c, 1, R, t)
        x, rank = D.min_norm_step(A, b)
        assert rank == 3
        R, t = D.compose(src, R, t, x)
    bar = max(it, 1) * PLANE_POSE
    dR, dt = float(np.abs(R1 - R).max()), float(np.abs(t1 - t).max())
    rms = float(np.sqrt(np.mean(((src.astype(np.float64) @ R1.astype(np.float64).T + t1.astype(np.float64)) @ n0) ** 2)))
    spin, slide = D.null_motion(R1, t1, R0, t0, n0)
    spin_t, slide_t = D.null_motion(R, t, R0, t0, n0)
    print("%s: %d iterations, |dR| %.2e |dt| %.2e (bar %.0e), plane rms %.2e, turn about the normal %.2e (twin %.2e), slide %.2e (twin %.2e)"
          % (D.TILT_IDS[D.TILTS.index(c["tilt"])], it, dR, dt, bar, rms, spin, spin_t, np.linalg.norm(slide), np.linalg.norm(slide_t)))
    assert 1 <= it < 20, it
    assert dR <= bar and dt <= bar, (it, dR, dt)
    assert rms <= 1e-5, rms
    assert abs(spin - spin_t) <= bar and np.abs(slide - slide_t).max() <= bar, (spin, spin_t, slide, slide_t)


# ----------------------------------------------------------------------------------------------
# d. point-to-point on the line and on a single matched target point
# ----------------------------------------------------------------------------------------------
# Five iterations are five one-iteration runs, each from the pose the last one returned: every step is then the solver's alone.  (Inside one
# run the loop adds the previous iteration's means to the new sums before it divides by n -- the reference's rule, jly_icp3d.hpp:244-263,
# kept for parity -- which displaces a five-point cloud by |mu| / 5 per iteration, whatever the solver does: measured on the one-point target
# 0.02171, 0.01250, 0.01287 over max_iter = 1, 2, 3, before and after this file's fixes.)
# The error of a pass is known to the float rounding of the pose and of q = R p + t: 3 + 1 roundings of the pose's entries and 4 of the
# row expression, each <= 2^-24 of a magnitude <= 2, so |dq| <= DQ = sqrt(3) * 16 * 2^-24 per point, and a sum of N squared distances a
# moves by at most 2 DQ sqrt(N a) + N DQ^2 (Cauchy-Schwarz).  An increase within that is the rounding, not the solver.
DQ = np.sqrt(3.0) * 16 * 2.0 ** -24


def _err_floor(a, n=5):
    return 2 * DQ * np.sqrt(n * a) + n * DQ * DQ


def _five_iterations(reg, R0, t0):
    """-> [(R, t, err of the pass at the pose before, iters)] of five chained one-iteration runs, and the five errors followed by the error at the last pose"""
    outs, R, t = [], R0, t0
    for k in range(6):
        R1, t1, err, it = _run(reg, R, t, max_iter=1)
        if k == 5:
            break                                                      # the sixth run only scores the fifth pose
        assert it == 1, (k + 1, it)
        assert _is_rotation(R1, t1), (k + 1, R1, t1)
        assert np.abs(R1.astype(np.float64).T @ R1.astype(np.float64) - np.eye(3)).max() <= 1e-5, (k + 1, R1)
        outs.append((R1, t1, err, it))
        R, t = R1, t1
    errs = [float(o[2]) for o in outs] + [float(err)]
    for a, b in zip(errs, errs[1:]):
        assert b <= a + _err_floor(a), errs
    return outs, errs


@pytest.mark.parametrize("ti", list(range(len(D.TILTS))), ids=D.TILT_IDS)
def test_point_to_point_on_a_line(pkg, oracle_mod, ti):
    tilt = D.TILTS[ti]
    tgt, src = D.line(tilt)
    R0, t0 = D.start(tilt)
    reg = pkg.Registration(tgt, src, 1e-3, dt_size=32)
    try:
        idx, _ = reg.nn_query(D.q32(R0, t0, src))
        assert np.array_equal(idx, oracle_mod.nn_brute(tgt, D.q32(R0, t0, src))[0]) and np.array_equal(idx, [0, 3, 7, 12, 16])
        outs, errs = _five_iterations(reg, R0, t0)
        R, t = outs[-1][0], outs[-1][1]
        landed = D.q32(R, t, src).astype(np.float64) - tgt[[0, 3, 7, 12, 16]].astype(np.float64)
        print("%s: errors %s, |landed - matched| %.2e" % (D.TILT_IDS[ti], ["%.3e" % e for e in errs], np.abs(landed).max()))
        # the first pass sees the start pose; a rigid motion carries the five points exactly onto their neighbours, and the loop finds it within
        # the 1e-5 per coordinate every pose bar here allows
        assert errs[0] >= 1e-4 and errs[-1] <= 5 * 3 * 1e-5 ** 2, errs
    finally:
        reg.close()


def test_point_to_point_on_one_target_point(pkg, oracle_mod):
    tgt, src = D.one_target_point()
    R0, t0 = D.start(D.TILTS[2])
    reg = pkg.Registration(tgt, src, 1e-3, dt_size=32)
    try:
        q = D.q32(R0, t0, src)
        idx, d2 = reg.nn_query(q)
        assert not idx.any() and np.array_equal(idx, oracle_mod.nn_brute(tgt, q)[0])
        outs, errs = _five_iterations(reg, R0, t0)
        R1, t1, e1, it = outs[0]
        # H = 0: the rotation stays, the translation carries the moved centroid onto the one matched point
        turned = float(np.abs(R1.astype(np.float64) - R0).max())
        landed = D.q32(R1, t1, src).astype(np.float64).mean(0) - tgt[0].astype(np.float64)
        looped = [float(_run(reg, R0, t0, max_iter=k)[2]) for k in (1, 2, 3)]         # informative: the carried means inside one run
        print("one target point: errors %s (one run of max_iter 1, 2, 3: %s), |R1 - R0| %.2e, |moved centroid - point 0| %.2e"
              % (["%.3e" % e for e in errs], ["%.5f" % e for e in looped], turned, np.abs(landed).max()))
        assert it == 1
        assert np.abs(landed).max() <= TOL_ICP, landed
        assert np.array_equal(R1, R0), (R1, R0)
    finally:
        reg.close()
