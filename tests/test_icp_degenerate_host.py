"""CPU checks of tests/degenerate_twin.py: the references and the inputs of tests/test_gpu_icp_degenerate.py, so that the GPU tests cannot
pass or fail by construction.

  kabsch64 reproduces the 32 golden rotations of tests/golden/svd3x3.json to 1e-5: its convention is the device routine's
  every 3x3 case has the singular value ratios and the uniqueness gap (s2 + d s3) / s1 it is named for
  every plane, at the start pose and at each pose of the five-iteration twin loop: rank 3 under the 1e-6 rule for metrics 1 and 2 with the
    retained eigenvalues >= 1e-3 and the dropped ones <= 1e-7 of the largest; the metric-3 matrix is full rank (eigenvalues >= 1e-5: the
    plane's free directions carry eps = 1e-3 of an ordinary eigenvalue, nothing within a decade of the rule); every source point's
    second-nearest squared distance exceeds its nearest by >= 1e-4 (oracle.nn_brute), so no correspondence can flip
  the line's covariance has s2 / s1 <= 1e-6 at every tilt, with exact zeros where the line is parallel to x
  a transcription of the finalize's present solve on float32-rounded terms, per tilt: informative, printed, nothing asserted of the device
"""
import numpy as np
import pytest

import degenerate_twin as D
from conftest import golden

f32 = np.float32


def test_kabsch64_reproduces_the_golden_rotations():
    worst = 0.0
    for c in golden("svd3x3")["cases"]:
        R, s, d = D.kabsch64(c["H"])
        worst = max(worst, float(np.abs(R.reshape(9) - np.array(c["R"], np.float64)).max()))
        assert abs(np.linalg.det(R) - 1) <= 1e-12
        assert abs(D.kabsch_objective(R, c["H"]) - D.kabsch_optimum(c["H"])) <= 1e-12 * s[0]
    print("kabsch64 against the golden rotations: worst %.2e" % worst)
    assert worst <= 1e-5, worst


def test_kabsch_cases_are_what_they_are_named_for():
    cases = D.kabsch_cases()
    assert len(cases) == 13 + 8 + 6 + 9
    for name, H in cases.items():
        _, s, d = D.kabsch64(H)
        r2, r3, gap = s[1] / s[0], s[2] / s[0], D.kabsch_gap(H)
        print("%-16s s1 %.3e  s2/s1 %.3e  s3/s1 %.3e  d %+d  gap %.3e" % (name, s[0], r2, r3, d, gap))
        assert np.isfinite(H).all() and s[0] > 0
        base = name.split("@")[0]
        if "@1e-30" in name:
            assert 0.5e-30 <= s[0] <= 2e-30
        elif "@1e+30" in name:
            assert 0.5e+30 <= s[0] <= 2e+30
        else:
            assert abs(s[0] - 1) <= 1e-6
        if base in D.KABSCH_S:
            want = D.KABSCH_S[base]
            # the float rounding of H moves a singular value by at most |dH|_2 <= 3 * 2^-24 * s1
            assert abs(r2 - abs(want[1])) <= 2e-7 and abs(r3 - abs(want[2])) <= 2e-7, (name, r2, r3)
            if abs(want[2]) >= 1e-6:
                assert d == np.sign(want[2])
        if base in ("rank2", "s3=+1e-8", "s3=-1e-8", "near-tie12", "tie12+", "tie12-") or base.startswith("diag-zero"):
            assert gap >= 0.49, (name, gap)                            # unique, held to kabsch64
        if base == "reflect":
            assert abs(gap - 0.1) <= 1e-6
        if base in ("tie23-", "tie123-", "rank1", "near-rank1") or base.startswith("e"):
            assert gap <= 1e-6, (name, gap)                            # not unique (or nearly not): only the objective is held
        if base.startswith("e"):
            assert r2 == 0 and r3 == 0
        if base.startswith("diag-zero"):
            assert r2 == 0.5 and r3 == 0


def _brute_two(oracle, target, q):
    """nearest index and squared distance, and the squared distance of the second nearest"""
    idx, d1 = oracle.nn_brute(target, q)
    d2 = np.empty(len(q), f32)
    for k in range(len(q)):
        _, d = oracle.nn_brute(np.delete(target, idx[k], axis=0), q[k:k + 1])
        d2[k] = d[0]
    return idx, d1, d2


@pytest.mark.parametrize("tilt", D.TILTS, ids=D.TILT_IDS)
def test_planes_have_rank_three_and_fixed_correspondences(oracle_mod, tilt):
    tgt, src, sel = D.plane(tilt)
    assert tgt.shape == (289, 3) and src.shape == (101, 3) and tgt.dtype == src.dtype == f32
    F = D.frame(tilt)
    n0 = F[:, 2]
    nm = np.tile(n0.astype(f32), (len(tgt), 1))
    ns = np.tile(n0.astype(f32), (len(src), 1))
    if not any(tilt):
        assert np.all(tgt * 16 == np.round(tgt * 16)) and np.all(tgt[:, 2] == 0) and np.all(src * 64 == np.round(src * 64))
    R, t = (x.astype(np.float64) for x in D.start(tilt))
    for it in range(6):
        q = D.q32(R, t, src)
        idx, d1, d2 = _brute_two(oracle_mod, tgt, q)
        assert np.array_equal(idx, sel), (tilt, it)
        margin = float((d2.astype(np.float64) - d1.astype(np.float64)).min())
        assert margin >= 1e-4, (tilt, it, margin)
        ranks = {}
        for metric in (1, 2, 3):
            A, b = D.system(metric, src, tgt, R, t, idx, nm, ns)
            lam = D.spectrum(A)
            _, rank = D.min_norm_step(A, b)
            ranks[metric] = rank
            assert rank == D.PLANE_RANK[metric], (tilt, it, metric, lam)
            if metric == 3:
                assert lam[0] >= 1e-5, (tilt, it, lam)
            else:
                assert lam[3] >= 1e-3 and np.abs(lam[:3]).max() <= 1e-7, (tilt, it, metric, lam)
        A, b = D.system(1, src, tgt, R, t, idx, nm)
        x, _ = D.min_norm_step(A, b)
        rms = float(np.sqrt(np.mean(((q.astype(np.float64)) @ n0) ** 2)))
        print("%s pose %d: NN margin %.2e, ranks %s, |x| %.3e, plane rms %.2e" % (tilt, it, margin, ranks, np.linalg.norm(x), rms))
        if it == 0:
            assert 0.02 <= np.linalg.norm(x) <= 0.03                   # the start pose is 0.01 off the plane and 0.022 rad turned
        R, t = D.compose(src, R, t, x)
    assert rms <= 1e-6                                                 # the min-norm loop lands on the plane


@pytest.mark.parametrize("tilt", D.TILTS, ids=D.TILT_IDS)
def test_line_covariance_has_rank_one(oracle_mod, tilt):
    tgt, src = D.line(tilt)
    assert tgt.shape == (17, 3) and src.shape == (5, 3)
    R0, t0 = D.start(tilt)
    idx, _ = oracle_mod.nn_brute(tgt, D.q32(R0, t0, src))
    assert np.array_equal(idx, [0, 3, 7, 12, 16])
    H = D.covariance(src, tgt, R0, t0, idx)
    s = np.linalg.svd(H, compute_uv=False)
    print("%s: s2/s1 %.2e s3/s1 %.2e" % (tilt, s[1] / s[0], s[2] / s[0]))
    assert s[1] <= 1e-6 * s[0]
    if not any(tilt):
        assert not H[:, 1:].any() and H[:, 0].any()                    # the centred target terms are exact zeros in y and z


def test_one_target_point_covariance_vanishes(oracle_mod):
    tgt, src = D.one_target_point()
    R0, t0 = D.start(D.TILTS[2])
    idx, d1, d2 = _brute_two(oracle_mod, tgt, D.q32(R0, t0, src))
    assert not idx.any() and float((d2 - d1).min()) >= 0.5
    assert not D.covariance(src, tgt, R0, t0, idx).any()
    assert np.abs(tgt.astype(np.float64).mean(0)).min() >= 0.1       # the pass's pivot, the target's centroid, is not the matched point


@pytest.mark.parametrize("tilt", D.TILTS, ids=D.TILT_IDS)
def test_present_solve_emulated(oracle_mod, tilt):
    """informative: the shift-and-Cholesky solve on the float32-rounded terms of the start pose.  Nothing here speaks for the device: the
    emulation leaves out the fixed-point rounding of the sums and the workgroup order.  Only the twin's own consistency is asserted."""
    tgt, src, sel = D.plane(tilt)
    nm = np.tile(D.frame(tilt)[:, 2].astype(f32), (len(tgt), 1))
    R0, t0 = D.start(tilt)
    A, b = D.system_f32_terms(src, tgt, R0, t0, sel, nm)
    x, ok, piv = D.finalize_solve(A, b)
    xm, rank = D.min_norm_step(A, b)
    lam = D.spectrum(A)
    n0 = D.frame(tilt)[:, 2]
    print("%s: Cholesky ok %s, pivots/trace %s, null eigenvalues/largest %s, |x - min-norm| %.3g, |min-norm| %.3g, rotation about the normal %.3g"
          % (tilt, ok, np.array2string(piv, precision=2), np.array2string(lam[:3], precision=2), np.abs(x - xm).max(), np.linalg.norm(xm), x[:3] @ n0))
    assert rank == 3 and 0.02 <= np.linalg.norm(xm) <= 0.03
    if not ok:
        assert not x.any()
    # on a well-conditioned system the transcription is an ordinary solve
    rng = np.random.default_rng(5)
    J = rng.normal(size=(40, 6))
    A2, b2 = J.T @ J, J.T @ rng.normal(size=40)
    x2, ok2, _ = D.finalize_solve(A2, b2)
    assert ok2 and np.abs(x2 - np.linalg.solve(A2, -b2)).max() <= 1e-9
    assert np.abs(x2 - D.min_norm_step(A2, b2)[0]).max() <= 1e-9
