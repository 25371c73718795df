"""The ICP passes, the neighbour searches and the cube bounds at tiny and ragged cloud sizes: source sizes on and around the wavefront (4 queries),
workgroup (16 queries), strided-switch (40 000) and bound-chunk (256 points, eight chunk sets from 7 937) boundaries, target sizes on the k-d
hierarchy's depth boundaries (1 024, 65 536) and down to two points.  Every kernel is held to a plain reference of the same operation:
oracle.nn_brute for neighbours, float64 Kabsch / Gauss-Newton steps on those correspondences for poses, float64 sums of the oracle's
per-point terms for bounds -- at the project's existing bars:
  5e-6 rel   first-pass error against the brute-force sum        (test_icp_first_pass_error_is_bruteforce_nn_sum)
  1e-6       R, t of one point-to-point iteration, TOL_ICP       (test_gpu_scale_parity)
  1e-5 rel   gated error against the inliers' sum                (test_inlier_set_is_nn_query_thresholded)
  1e-4, 1e-3 robust pose after one iteration, W (and C) rel      (test_gpu_icp_robust._against_twin)
  1e-5, 1e-6 point-to-plane pose, its error against the plain    (test_one_iteration_vs_fp64_twin)
  2e-6 rel   bounds, floor max(ref, 1e-3), TOL                   (test_gpu_scale_parity)
Every test prints the worst deviation it saw.

Clouds: synth.make_pair(SEED, M, N, noise = 0.002) with far points appended (twins.make_case) where a gate or a kernel needs outliers; the start
pose is a fixed small turn and shift on top of the ground truth.  Poses are compared only where the system solved is well conditioned --
sigma_3 / sigma_1 >= 1e-2 of the Kabsch covariance, lambda_min / lambda_max >= 1e-6 of the point-to-plane normal matrix -- and the tests ASSERT
that condition for every size it is meant to hold at, so a change of seed cannot silently drop cases.  Checked on the CPU for SEED = 20261017
(oracle.nn_brute's neighbours; PCA normals from 8 neighbours): the Kabsch condition holds at every listed N >= 4 for the plain (worst 0.050, N = 4),
gated (0.065, N = 5) and both robust steps (0.106), the point-to-plane one at every listed N >= 15 (worst 3.7e-3, N = 15); a point-to-plane system of N < 6 rows has rank <= N < 6 whatever the seed, so
at N = 4 and 5 only its error is held.  At N <= 3 a pose is only asked to be finite and a rotation.

A gate or a robust kernel stops a loop whose inlier count / weight sum is below the metric's floor (3 point-to-point, 6 point-to-plane: the documented
rule, test_gate_below_every_distance) and leaves the pose; below the floor the identities with the plain run therefore read "the start pose, unchanged".

The defect these shapes found: with a single correspondence (N = 1, plain pass) the covariance H is exactly 0 and kabsch_rows returned the zero
matrix as the "rotation"; it now returns the identity (a pure translation).  Guards: test_plain_pass_ragged[1] and
test_kabsch_of_a_zero_covariance_is_the_identity.

Teeth (done once on scratch copies of device.hip, on MI355X, the whole GPU suite per mutant; both mutants read valid memory only):
  A  icp_pass_body's `valid` without `i < N`, surplus rows counting the last point again:   11 of the 256 earlier tests fail, 72 of the 144 here
  B  bounds_work's tail without the clamp to N, the last point again up to the chunk's end: 69 of the 256 earlier tests fail, 25 of the 144 here
     (the 25: every size and layout of test_bounds_ragged bar N = 256, 7 936 and 8 192, where the last chunk ends on N; the doubled clouds
     bar 2 x 256; both single-point cubes.  The trimmed kernel has its own loop and was not mutated.)
Wall time on MI355X: this file 4.4 s (144 tests, the slowest 0.2 s); the suite without it 223 s.
"""
import functools

import numpy as np
import pytest

import twins
from conftest import load_pkg
from test_gpu_icp_gate import _run, _same, _transform_f32
from test_gpu_point_to_plane import _knn_brute, _twin_step
from test_gpu_scale_parity import TOL, TOL_ICP, _icp_one_f64, _rel, _sibling_cubes, _trim_reg
from test_icp_robust_host import HUBER, NAMES, TUKEY, robust_rho, robust_w

pytestmark = pytest.mark.gpu
INVALID = -1
SEED = 20261017
M_ICP = 2000
N_RAGGED = [1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 255, 257, 1023, 1025]
N_SWITCH = [39999, 40000, 40001, 40003]
M_DEPTH = [2, 3, 16, 17, 1024, 1025, 65537]
N_BOUNDS = [1, 2, 7, 255, 256, 257, 511, 513, 7936, 7937, 8192, 8193]
KABSCH_COND, PLANE_COND = 1e-2, 1e-6
# The bars, each with the worst deviation measured on MI355X over every case of this file that is held to it:
ERR_REL = 5e-6          # first-pass error against the brute-force sum: 8.1e-8
GATE_ERR_REL = 1e-5     # gated error against the inliers' sum: 1.4e-7
ROBUST_POSE = 1e-4      # robust pose after one iteration: R 9.1e-8, t 3.8e-8
ROBUST_SUM_REL = 1e-3   # W = sum w: 8.5e-8.  C = sum rho is held to the same bar (measured 1.5e-7): _against_twin only prints C, so that bar is this file's own,
                        # taken over from W because both are column sums of the same pass, scaled and added the same way
PLANE_POSE = 1e-5       # point-to-plane pose after one iteration: R 1.2e-6, t 2.6e-7
PLANE_ERR_REL = 1e-6    # point-to-plane first-pass error against the plain pass's: 0 (the same bits)
# TOL_ICP = 1e-6 (imported), R and t of one point-to-point iteration: plain R 8.4e-8, t 2.6e-8; gated R 7.4e-8, t 5.1e-8; N around 40 000 R 6.2e-8, t 2.4e-8
# TOL = 2e-6 (imported), cube bounds: plain 3.1e-7, truncated 3.7e-7, trimmed 2.6e-7, doubled cloud 1.8e-7


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _case(M, N, out_idx=None, outliers=True):
    """the clouds, the start pose, the moved source q (float32, the pass's expression) and oracle.nn_brute's neighbours of q: built once, read-only"""
    import oracle
    load_pkg()
    from cuda_go_icp_amd import synth
    c = twins.make_case(synth, SEED, M, N, out_idx=out_idx if outliers else ())
    c["q"] = _transform_f32(c["R0"], c["t0"], c["source"])
    c["bi"], c["bd2"] = oracle.nn_brute(c["target"], c["q"])
    return _frozen(c)


def _reg(pkg, c, **kw):
    kw.setdefault("dt_size", 32)
    return pkg.Registration(c["target"], c["source"], 1e-3, **kw)


def _pose_dev(R, t, fR, ft):
    return float(np.abs(R - fR).max()), float(np.abs(t - ft).max())


def _is_rotation(R, t):
    R64 = R.astype(np.float64)
    return bool(np.isfinite(R).all() and np.isfinite(t).all() and abs(np.linalg.det(R64) - 1) <= 1e-5)


def _unchanged(out, c):
    return np.array_equal(out[0], c["R0"]) and np.array_equal(out[1], c["t0"]) and out[3] == 0


# ----------------------------------------------------------------------------------------------
# the checks (a) .. (e): each takes a handle and its case and prints what it measured
# ----------------------------------------------------------------------------------------------
def check_plain(reg, c, pose=True):
    """(a) nn_query == nn_brute bit for bit; the first pass's error == their float64 sum; one iteration == the float64 Kabsch step"""
    N = c["N"]
    reg.set_icp_options(0, 16)
    idx, d2 = reg.nn_query(c["q"])
    assert np.array_equal(d2.view(np.uint32), c["bd2"].view(np.uint32)) and np.array_equal(idx, c["bi"]), ("nn", c["M"], N, int(np.sum(idx != c["bi"])))
    R, t, err, it = _run(reg, c["R0"], c["t0"], max_iter=1)
    ref = float(np.sum(d2.astype(np.float64)))
    e_rel = abs(float(err) - ref) / ref
    assert e_rel <= ERR_REL, (c["M"], N, float(err), ref)
    assert list(reg.icp_inliers(1)) == [N]
    assert _is_rotation(R, t), (c["M"], N, R, t)
    dR = dt = cond = float("nan")
    if N == 1:
        # one correspondence: the pivot cq is the moved point itself, every centred term is exactly 0, H = 0, and the step is a pure translation
        # onto the neighbour -- the rotation stays bit for bit, the moved point lands on target[idx] within the float rounding of the means
        assert np.array_equal(R, c["R0"]), (R, c["R0"])
        landed = _transform_f32(R, t, c["source"])[0].astype(np.float64)
        assert np.abs(landed - c["target"][idx[0]].astype(np.float64)).max() <= TOL_ICP, (landed, c["target"][idx[0]])
    if pose and N >= 4:
        cond = twins.kabsch_condition(c["target"], c["q"], idx)
        assert cond >= KABSCH_COND, ("conditioning", c["M"], N, cond)
        _, fR, ft = _icp_one_f64(c["target"], c["q"], idx, d2, N, c["R0"], c["t0"])
        dR, dt = _pose_dev(R, t, fR, ft)
        assert it == 1 and dR <= TOL_ICP and dt <= TOL_ICP, (c["M"], N, dR, dt, cond)
    print("plain M %d N %d: err rel %.2e, |dR| %.2e |dt| %.2e (sigma3/sigma1 %.3g)" % (c["M"], N, e_rel, dR, dt, cond))


def check_gate(reg, c, pose=True):
    """(b) the gate from the data; inlier count, error and pose against nn_query thresholded; capped and full walk give the same bits"""
    N = c["N"]
    reg.set_icp_options(0, 16)
    idx, d2 = reg.nn_query(c["q"])
    g, margin = twins.pick_gate(np.sqrt(d2.astype(np.float64)), c["out_idx"])
    assert margin >= 1e-4, (N, g, margin)                       # no distance near the gate: the inlier set cannot flip
    g2 = np.float32(g) * np.float32(g)
    inl = d2 <= g2
    n = int(inl.sum())
    if len(c["out_idx"]):                                      # the gate separates exactly the appended far points
        want = np.ones(N, bool)
        want[c["out_idx"]] = False
        assert np.array_equal(inl, want), (N, g)
    ref = float(np.sum(d2[inl].astype(np.float64)))
    outs, e_rel, dR, dt, cond = [], 0.0, float("nan"), float("nan"), float("nan")
    try:
        for capped in (1, 0):
            reg.set_icp_gate(g, capped_walk=capped)
            R, t, err, it = _run(reg, c["R0"], c["t0"], max_iter=1)
            cnt = int(reg.icp_inliers(1)[0])
            outs.append((R, t, err, it, cnt))
            assert cnt == n, (N, capped, cnt, n)
            if n:
                e_rel = max(e_rel, abs(float(err) - ref) / ref)
                assert abs(float(err) - ref) <= GATE_ERR_REL * ref, (N, capped, float(err), ref)
            else:
                assert float(err) == 0.0
            assert _is_rotation(R, t)
            if n < 3:
                assert _unchanged((R, t, err, it), c), (N, capped, n)
            elif pose and n >= 4:
                cond = twins.kabsch_condition(c["target"], c["q"][inl], idx[inl])
                assert cond >= KABSCH_COND, ("conditioning", N, n, cond)
                _, fR, ft = _icp_one_f64(c["target"], c["q"][inl], idx[inl], d2[inl], n, c["R0"], c["t0"])
                dR, dt = _pose_dev(R, t, fR, ft)
                assert it == 1 and dR <= TOL_ICP and dt <= TOL_ICP, (N, capped, n, dR, dt, cond)
        assert _same(outs[0], outs[1]), (N, [o[2:] for o in outs])
    finally:
        reg.set_icp_gate(0.0)
    print("gate M %d N %d: g %.4f (nearest distance %.1e away), inliers %d, err rel %.2e, |dR| %.2e |dt| %.2e (sigma3/sigma1 %.3g)"
          % (c["M"], N, g, margin, n, e_rel, dR, dt, cond))


def check_robust(reg, c, pose=True):
    """(c) Huber at the median distance, Tukey at 1.5 x it: W and C against the float64 sums of the table's w and rho on nn_query's distances,
    the pose against the weighted Kabsch step"""
    N = c["N"]
    reg.set_icp_options(0, 16)
    idx, d2 = reg.nn_query(c["q"])
    d = np.sqrt(d2.astype(np.float64))
    try:
        for kernel, scale in ((HUBER, float(np.float32(np.median(d)))), (TUKEY, float(np.float32(1.5 * np.median(d))))):
            w, rho = robust_w(kernel, scale, d), robust_rho(kernel, scale, d)
            tW, tC = float(w.sum()), float(rho.sum())
            if N >= 4:
                assert w.max() - w.min() > 0.05                 # the scale lies inside the spread of the distances: the weights differ
            reg.set_icp_robust(kernel, scale)
            R, t, err, it = _run(reg, c["R0"], c["t0"], max_iter=1)
            cost, W = reg.icp_robust_stats(1)
            cost, W = float(cost[0]), float(W[0])
            dW, dC = abs(W - tW) / tW, abs(cost - tC) / tC
            assert dW <= ROBUST_SUM_REL and dC <= ROBUST_SUM_REL, (N, kernel, W, tW, cost, tC)
            assert abs(float(err) - float(np.sum(d2.astype(np.float64)))) <= ERR_REL * float(np.sum(d2.astype(np.float64)))   # err is over all N points
            assert _is_rotation(R, t)
            dR = dt = cond = float("nan")
            # W within 0.01 of the floor of 3 could fall on either side of it in float: there only "finite, a rotation" (above) is held
            if tW <= 2.99:
                assert _unchanged((R, t, err, it), c), (N, kernel, tW)
            elif pose and N >= 4 and tW >= 3.01:
                cond = twins.kabsch_condition(c["target"], c["q"], idx, w)
                assert cond >= KABSCH_COND, ("conditioning", N, kernel, cond)
                fR, ft, _ = twins.kabsch_weighted_f64(c["target"], c["q"], idx, w, c["R0"], c["t0"])
                dR, dt = _pose_dev(R, t, fR, ft)
                assert it == 1 and dR <= ROBUST_POSE and dt <= ROBUST_POSE, (N, kernel, dR, dt, cond)
            print("robust M %d N %d %s c %.4f: W %.3f (rel %.2e) C %.6g (rel %.2e), |dR| %.2e |dt| %.2e (sigma3/sigma1 %.3g)"
                  % (c["M"], N, NAMES[kernel], scale, W, dW, cost, dC, dR, dt, cond))
    finally:
        reg.set_icp_robust(0)


def check_plane(reg, c, pose=True):
    """(d) one point-to-plane iteration (normals from 8 neighbours) against the float64 Gauss-Newton twin; its error is the plain pass's"""
    N = c["N"]
    R64, t64 = c["R0"].astype(np.float64), c["t0"].astype(np.float64)
    try:
        reg.set_icp_options(1, 8)
        fR, ft, _ = _twin_step(reg, c["source"], c["target"], R64, t64)
        R1, t1, e1, it1 = _run(reg, c["R0"], c["t0"], max_iter=1)
        reg.set_icp_options(0, 8)
        _, _, e0, _ = _run(reg, c["R0"], c["t0"], max_iter=1)
        e_rel = abs(float(e1) - float(e0)) / float(e0)
        assert e_rel <= PLANE_ERR_REL, (N, e1, e0)
        assert np.isfinite(R1).all() and np.isfinite(t1).all()
        dR = dt = cond = float("nan")
        if pose and N >= 15:
            idx, _ = reg.nn_query(c["q"])
            pivot = R64 @ c["source"].astype(np.float64).mean(0) + t64
            cond = twins.plane_condition(c["q"], reg.target_normals()[idx], pivot)
            assert cond >= PLANE_COND, ("conditioning", c["M"], N, cond)
            dR, dt = _pose_dev(R1, t1, fR, ft)
            assert it1 == 1 and dR <= PLANE_POSE and dt <= PLANE_POSE, (c["M"], N, dR, dt, cond)
    finally:
        reg.set_icp_options(0, 16)
    print("plane M %d N %d: err rel to plain %.2e, |dR| %.2e |dt| %.2e (lambda_min/lambda_max %.3g)" % (c["M"], N, e_rel, dR, dt, cond))


def check_identities(reg, c, metrics=(0, 1), batch=True, normal_k=8):
    """(e) a gate and a Huber scale of ten extents reproduce the plain run's bits; a batch of three starts, two of them equal, reproduces
    three single runs -- either metric, after 1 and after 5 iterations.  Below the metric's floor the gated / robust loop leaves the start pose."""
    N, big = c["N"], 10 * c["extent"]
    R1 = (twins.rodrigues64([-0.03, 0.01, 0.02]) @ c["R0"].astype(np.float64)).astype(np.float32)
    t1 = (c["t0"] + np.array([-0.01, 0.015, 0.005], np.float32)).astype(np.float32)
    try:
        for metric in metrics:
            floor = 6 if metric else 3
            reg.set_icp_options(metric, normal_k)
            for iters in (1, 5):
                ref = _run(reg, c["R0"], c["t0"], max_iter=iters)
                for capped in (1, 0):
                    reg.set_icp_gate(big, capped_walk=capped)
                    out = _run(reg, c["R0"], c["t0"], max_iter=iters)
                    assert list(reg.icp_inliers(1)) == [N]
                    assert (_same(out, ref) if N >= floor else _unchanged(out, c)), ("gate", c["M"], N, metric, iters, capped, out[2:], ref[2:])
                reg.set_icp_gate(0.0)
                reg.set_icp_robust(HUBER, big)
                out = _run(reg, c["R0"], c["t0"], max_iter=iters)
                cost, W = reg.icp_robust_stats(1)
                assert float(W[0]) == float(N)
                assert (_same(out, ref) if N >= floor else _unchanged(out, c)), ("huber", c["M"], N, metric, iters, out[2:], ref[2:])
                reg.set_icp_robust(0)
                if batch:
                    Rb, tb = np.stack([c["R0"], R1, c["R0"]]), np.stack([c["t0"], t1, c["t0"]])
                    bR, bt, berr, bit = reg.icp_run_batch(Rb, tb, iters, 1e-7)
                    for k in range(3):
                        sR, st, se, si = _run(reg, Rb[k], tb[k], max_iter=iters)
                        assert np.array_equal(bR[k], sR) and np.array_equal(bt[k], st) and berr[k] == se and bit[k] == si, ("batch", c["M"], N, metric, iters, k)
                    assert np.array_equal(bR[0], bR[2]) and np.array_equal(bt[0], bt[2]) and berr[0] == berr[2]
    finally:
        reg.set_icp_gate(0.0)
        reg.set_icp_robust(0)
        reg.set_icp_options(0, 16)


# ----------------------------------------------------------------------------------------------
# 1. the pass family over ragged N (target 2 000 points: two box levels; strided addressing throughout)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", N_RAGGED)
def test_plain_pass_ragged(pkg, N):
    c = _case(M_ICP, N)
    reg = _reg(pkg, c)
    try:
        check_plain(reg, c)
    finally:
        reg.close()


@pytest.mark.parametrize("N", N_RAGGED)
def test_gated_pass_ragged(pkg, N):
    c = _case(M_ICP, N)
    reg = _reg(pkg, c)
    try:
        check_gate(reg, c)
    finally:
        reg.close()


def test_gated_pass_row_without_owner(pkg):
    """N = 65 in input order (morton_sort 0): nw = 17, so the last wavefront of workgroup 0 walks the points 3, 20, 37 and 54 -- all four far
    points (and 64, the ragged last row's only query, a fifth).  Under the capped walk none of that wavefront's rows has an owning lane."""
    c = _case(M_ICP, 65, out_idx=(3, 20, 37, 54, 64))
    reg = _reg(pkg, c, morton_sort=0)
    try:
        check_gate(reg, c)
    finally:
        reg.close()


@pytest.mark.parametrize("N", N_RAGGED)
def test_robust_pass_ragged(pkg, N):
    c = _case(M_ICP, N)
    reg = _reg(pkg, c)
    try:
        check_robust(reg, c)
    finally:
        reg.close()


@pytest.mark.parametrize("N", N_RAGGED)
def test_plane_pass_ragged(pkg, N):
    c = _case(M_ICP, N)
    reg = _reg(pkg, c)
    try:
        check_plane(reg, c)
    finally:
        reg.close()


@pytest.mark.parametrize("N", N_RAGGED)
def test_identities_ragged(pkg, N):
    c = _case(M_ICP, N)
    reg = _reg(pkg, c)
    try:
        check_identities(reg, c)
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 2. the strided switch (N around 40 000) and the hierarchy depth (M around 1 024 and 65 536, down to 2)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", N_SWITCH)
def test_strided_switch(pkg, N):
    """39 999 and 40 000: strided addressing; 40 001 and 40 003: neighbours, a ragged last wavefront."""
    c = _case(M_ICP, N, outliers=False)
    reg = _reg(pkg, c)
    try:
        check_plain(reg, c)
        check_identities(reg, c)
    finally:
        reg.close()


@pytest.mark.parametrize("M", M_DEPTH)
def test_hierarchy_depth(pkg, M):
    """N = 257 against targets of one, two and three box levels.  Two, three and sixteen target points make every pose step ill-posed: there only
    the error, the inlier count and W / C are held."""
    c = _case(M, 257, outliers=False)
    pose = M >= 17
    for kw in ({}, {"kd_gpu_build": 1}) if M == 65537 else ({},):
        reg = _reg(pkg, c, **kw)
        try:
            check_plain(reg, c, pose=pose)
            if kw:
                continue
            check_gate(reg, c, pose=False)         # no far points here: the widest gap lies inside the cloud; count and error only
            check_robust(reg, c, pose=pose)
            # point-to-plane needs normal_k >= 3 neighbours among the target points: both metrics from M = 3 on, point-to-point alone at M = 2
            check_identities(reg, c, metrics=(0, 1) if M >= 3 else (0,), batch=False, normal_k=max(3, min(8, M)))
            if M >= 17:
                check_plane(reg, c)
        finally:
            reg.close()


def test_kabsch_of_a_zero_covariance_is_the_identity(pkg):
    """goicp_debug_kabsch (the finalize's own routine) on H = 0, the covariance of a single correspondence: the identity, as the reference's
    SVD gives it (U = V = I) -- not the zero matrix; and an H of full rank is left as it was (a rotation)"""
    import ctypes as C
    lib = pkg.load_library()
    fp = C.POINTER(C.c_float)
    for H, want in ((np.zeros(9, np.float32), np.eye(3, dtype=np.float32)), (np.eye(3, dtype=np.float32).reshape(9) * np.float32(0.25), np.eye(3, dtype=np.float32))):
        R = np.full(9, np.nan, np.float32)
        pkg.binding.check(lib.goicp_debug_kabsch(H.ctypes.data_as(fp), R.ctypes.data_as(fp)))
        assert np.array_equal(R.reshape(3, 3), want), (H, R)


def _knn_queries(target, n, seed):
    """test_gpu_point_to_plane._queries for targets of any size (it draws target points without replacement): a quarter each on target points,
    near them, around the cloud and far outside the DT grid"""
    rng = np.random.default_rng(seed)
    lo, hi = target.min(0), target.max(0)
    ext = float((hi - lo).max())
    m = n // 4
    on = target[rng.integers(0, len(target), m)] + rng.normal(scale=1e-5 * ext, size=(m, 3))
    near = target[rng.integers(0, len(target), m)] + rng.normal(scale=2e-2 * ext, size=(m, 3))
    around = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (m, 3))
    out = rng.uniform(-1, 1, (n - 3 * m, 3)) * 4 * ext + (lo + hi) / 2 + 3 * ext
    return np.concatenate([on, near, around, out]).astype(np.float32)


@pytest.mark.parametrize("M,k", [(2, 1), (2, 2), (16, 16), (17, 17), (33, 32), (1025, 32)])
def test_knn_small_targets(pkg, M, k):
    c = _case(M, 257, outliers=False)
    reg = _reg(pkg, c)
    try:
        q = _knn_queries(c["target"], 256, 17 + M)
        bi, bd = _knn_brute(c["target"], q, k)
        idx, d2 = reg.knn_query(q, k)
        assert idx.shape == (len(q), k)
        assert np.array_equal(idx, bi), (M, k, int(np.sum(idx != bi)))
        assert np.array_equal(d2.view(np.uint32), bd.view(np.uint32)), (M, k)
        if M + 1 <= 32:
            with pytest.raises(pkg.GoicpError) as e:
                reg.knn_query(q[:4], M + 1)
            assert e.value.code == INVALID
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 3. cube bounds over ragged N
# ----------------------------------------------------------------------------------------------
ROTS = ([0.9, -1.7, 2.3], [-1.1, 0.4, 0.2], [0.05, 1.7, -0.6])
V_BOUNDS = 64
LEVEL = 5


@functools.lru_cache(maxsize=None)
def _bounds_target():
    import oracle
    load_pkg()
    from cuda_go_icp_amd import synth
    target = synth.make_pair(seed=SEED, M=M_ICP, N=1, noise=0.002)[0]
    return target, oracle.DistanceTransform(target, V_BOUNDS, 2.0)


@functools.lru_cache(maxsize=None)
def _bounds_case(N):
    """the launches of one source size and the oracle's per-point terms of every cube in them (computed once; they depend neither on the
    layout nor on the truncation nor on the inlier count): [(kind, argument, level or None, [(terms, child width)])]"""
    import oracle as O
    pkg = load_pkg()
    from cuda_go_icp_amd import synth
    target, dt = _bounds_target()
    source = synth.make_pair(seed=SEED, M=M_ICP, N=N, noise=0.002)[1]
    _, rho = O.rot_radii(source)
    rots = np.stack([pkg.fgoicp.rodrigues(v) for v in ROTS])
    prots = [O.rotate(R, source) for R in rots]
    coeff, lib = O.rot_coeff(LEVEL), pkg.load_library()
    rng = np.random.default_rng(N)
    calls = []
    for n in (1, 8, 77):                                     # eval_bounds: unrelated cubes of one rotation, a ragged last group
        cubes = np.concatenate([rng.uniform(-0.4, 0.4, (n, 3)), rng.choice([1 / 8, 1 / 16, 1 / 32], (n, 1))], 1).astype(np.float32)
        for level in (-1, LEVEL):
            calls.append(("eval", cubes, level, [(O.cube_terms(dt, prots[0], rho[level] if level >= 0 else None, c[:3], c[3]), c[3]) for c in cubes]))
    kids = _sibling_cubes(rng, 2, 1.0 / 8)                   # the 8 children of two parents, one per pass: the sibling path
    recs, terms = [], []
    for i, k in enumerate(kids):
        lower = i >= 8
        recs.append((k[0], k[1], k[2], lib.goicp_trans_delta(float(k[3])), float(coeff) if lower else 0.0, 0))
        terms.append((O.cube_terms(dt, prots[0], rho[LEVEL] if lower else None, k[:3], k[3]), k[3]))
    calls.append(("batch", recs, None, terms))
    cen = rng.uniform(-0.4, 0.4, (13, 3)).astype(np.float32)  # three rotations and both passes inside every group: the generic kernel
    w = np.float32(1.0 / 16)
    recs = [(cen[i, 0], cen[i, 1], cen[i, 2], lib.goicp_trans_delta(float(w)), float(coeff) if i % 2 else 0.0, i % 3) for i in range(13)]
    terms = [(O.cube_terms(dt, prots[i % 3], rho[LEVEL] if i % 2 else None, cen[i], w), w) for i in range(13)]
    calls.append(("batch", recs, None, terms))
    source.setflags(write=False)
    return source, rots, calls


def _check_bounds(reg, rots, calls, tag, trunc=0.0, inliers=None, factor=1.0):
    """every launch of `calls` on reg against twins.bound_ref (x factor); -> worst relative deviation"""
    worst = 0.0
    for kind, arg, level, terms in calls:
        ub, lb = reg.eval_bounds(rots[0], arg, level) if kind == "eval" else reg.eval_bounds_batch(rots, arg)
        assert len(ub) == len(terms)
        for i, (m, w) in enumerate(terms):
            fu, fl = twins.bound_ref(m, w, trunc, inliers)
            d = max(_rel(ub[i], factor * fu), _rel(lb[i], factor * fl))
            worst = max(worst, d)
            assert d <= TOL and lb[i] <= ub[i], (tag, kind, len(terms), level, i, ub[i], factor * fu, lb[i], factor * fl)
    return worst


@pytest.mark.parametrize("N,layout", [(n, 1) for n in N_BOUNDS] + [(n, 0) for n in N_BOUNDS if n < 1000])
def test_bounds_ragged(pkg, oracle_mod, N, layout):
    """Plain and truncated (g = 0.05) bounds; the linear layout for the six sizes below 1 000."""
    target, _ = _bounds_target()
    source, rots, calls = _bounds_case(N)
    reg = pkg.Registration(target, source, 1e-3, dt_size=V_BOUNDS, dt_layout=layout)
    try:
        assert reg.rot_coeff(LEVEL) == oracle_mod.rot_coeff(LEVEL)
        a = _check_bounds(reg, rots, calls, "N %d layout %d" % (N, layout))
        reg.set_search_truncation(0.05)
        b = _check_bounds(reg, rots, calls, "N %d layout %d truncated" % (N, layout), trunc=0.05)
        reg.set_search_truncation(0.0)
        print("bounds N %d layout %d: worst rel deviation %.2e plain, %.2e truncated" % (N, layout, a, b))
    finally:
        reg.close()


@pytest.mark.parametrize("N", [n for n in N_BOUNDS if n >= 7])
def test_bounds_trimmed_ragged(pkg, N):
    """inliers N - 1 and ceil(0.9 N) (at N = 7 the latter is N itself: untrimmed, left out): the float64 sum of that many smallest terms per cube."""
    target, _ = _bounds_target()
    source, rots, calls = _bounds_case(N)
    for k in sorted({N - 1, int(np.ceil(0.9 * N))} - {N}):
        for layout in (1, 0) if N < 1000 else (1,):
            reg = _trim_reg(pkg, target, source, k, dt_size=V_BOUNDS, dt_layout=layout)
            try:
                worst = _check_bounds(reg, rots, calls, "N %d inliers %d layout %d" % (N, k, layout), inliers=k)
                print("trimmed bounds N %d inliers %d layout %d: worst rel deviation %.2e" % (N, k, layout, worst))
            finally:
                reg.close()


@pytest.mark.parametrize("N", [n for n in N_BOUNDS if n <= 513])
def test_bounds_double_with_the_cloud(pkg, N):
    """every point twice: every bound is twice the single cloud's reference."""
    target, _ = _bounds_target()
    source, rots, calls = _bounds_case(N)
    reg = pkg.Registration(target, np.concatenate([source, source]), 1e-3, dt_size=V_BOUNDS)
    try:
        worst = _check_bounds(reg, rots, calls, "N 2 x %d" % N, factor=2.0)
        print("doubled cloud 2 x %d: worst rel deviation %.2e" % (N, worst))
    finally:
        reg.close()


@pytest.mark.parametrize("layout", [1, 0])
def test_single_point_far_outside_the_grid(pkg, oracle_mod, layout):
    """N = 1, a cube far outside the grid: the upper bound is the one DT lookup squared and the lower bound its clamped difference squared, bit for bit"""
    target, dt = _bounds_target()
    source, rots, _ = _bounds_case(1)
    reg = pkg.Registration(target, source, 1e-3, dt_size=V_BOUNDS, dt_layout=layout)
    try:
        cube = np.array([[50.0, -40.0, 30.0, 0.125]], np.float32)
        prot = oracle_mod.rotate(rots[0], source)
        m = oracle_mod.cube_terms(dt, prot, None, cube[0, :3], cube[0, 3])[0]
        assert m == dt.distance(prot[0] + cube[0, :3])[0] and m > 10
        ub, lb = reg.eval_bounds(rots[0], cube, -1)
        dis = np.float32(max(m - np.float32(reg._lib.goicp_trans_delta(0.125)), np.float32(0)))
        assert ub[0].tobytes() == np.float32(m * m).tobytes() and lb[0].tobytes() == np.float32(dis * dis).tobytes(), (ub, lb, m, dis)
        assert lb[0] <= ub[0]
    finally:
        reg.close()
