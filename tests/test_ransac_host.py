"""goicp_ransac_pose_host / goicp_select_matches: RANSAC pose estimation from correspondences on the host (no handle, no GPU) against the
numpy twin of its definition (tests/ransac_twin.py) -- pose records (every field, as bytes) and the inlier mask bit for bit over the shared
cases -- and what the definition promises on named cases: degenerate inputs, the exact copy (the tie goes to the smallest t), a
min_inliers above M, every refusal with the outputs untouched, select_matches against its statement, the rotation property of every
returned pose, and the recovery of a known pose from 30 % true correspondences.

The recovery input (tests/ransac_twin.py recovery(): scene seed 7, RANSAC seed 0, distance 0.03, noise sigma 0.01) is the first one
tried; the twin meets the bounds on it, so neither the input nor a bound was changed."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ransac_twin as RT
from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_ransac_pose_select_default", "goicp_ransac_pose_host", "goicp_ransac_pose", "goicp_select_matches", "goicp_ransac_pose_tile",
       "goicp_ransac_pose_block"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def assert_equal(got, want, what):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, g[:4], w[:4])


def assert_rotations(poses, what):
    for p in poses:
        R = p["R"].astype(np.float64)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and np.linalg.det(R) > 0, (what, R)


@pytest.mark.parametrize("name", list(RT.cases()))
def test_library_equals_twin(pkg, name):
    src, tgt, corr, kw = RT.cases()[name]
    poses, mask = RT.twin_of(name)
    assert poses.dtype == pkg.fgoicp.RANSAC_POSE_DTYPE and poses.dtype.itemsize == 60
    got = pkg.ransac_pose(src, tgt, corr, **kw)
    assert_equal(got, (poses, mask), name)
    # the properties, on the library's output: proper rotations, descending keys, the mask counts pose 0's inliers
    assert_rotations(got[0], name)
    key = [(-int(p["inliers"]), int(p["hypothesis"])) for p in got[0]]
    if not kw.get("refine", 1):
        assert key == sorted(key) and np.all(got[0]["refined"] == 0), name
    assert len(got[0]) <= (kw.get("max_poses", 1) or 1) and np.all(got[0]["inliers"] >= max(kw.get("min_inliers", 0), 3))
    assert int(got[1].sum()) == (int(got[0][0]["inliers"]) if len(got[0]) else 0)


def test_sizes_straddle_the_kernel_shapes(pkg):
    lib = pkg.load_library()
    assert lib.goicp_ransac_pose_tile() == RT.TILE and lib.goicp_ransac_pose_block() == RT.BLOCK
    for v in (RT.BLOCK - 1, RT.BLOCK, RT.BLOCK + 1):
        assert v in RT.SIZES
    for v in (RT.TILE - 1, RT.TILE, RT.TILE + 1, 2 * RT.TILE + 1):
        assert v in RT.ITERATIONS


def test_degenerate_inputs_have_no_pose(pkg):
    for name in ("collinear", "coincident_source", "min_inliers_above_M"):
        src, tgt, corr, kw = RT.cases()[name]
        poses, mask = pkg.ransac_pose(src, tgt, corr, **kw)
        assert len(poses) == 0 and not mask.any() and len(mask) == len(corr), name


def test_more_poses_asked_for_than_qualify(pkg):
    src, tgt, corr, kw = RT.cases()["min_inliers_cuts"]
    poses, _ = pkg.ransac_pose(src, tgt, corr, **kw)
    assert 0 < len(poses) < 64 and np.all(poses["inliers"] >= 100)
    src, tgt, corr, kw = RT.cases()["scene65_T1"]
    assert len(pkg.ransac_pose(src, tgt, corr, **dict(kw, max_poses=64))[0]) <= 1       # one hypothesis, 64 poses asked for


@pytest.mark.parametrize("refine", [0, 1])
def test_exact_copy_ties_go_to_the_smallest_hypothesis(pkg, refine):
    src, tgt, corr, kw = RT.cases()["exact_copy_r%d" % refine]
    counts = RT.hypothesis_counts(src, tgt, corr, kw["distance"], kw["iterations"], kw["edge_similarity"], 0)[2]
    full = np.flatnonzero(counts == len(corr))
    assert len(full) >= 8                                        # a real tie
    poses, mask = pkg.ransac_pose(src, tgt, corr, **kw)
    assert len(poses) == 1 and poses[0]["inliers"] == len(corr) and poses[0]["hypothesis"] == full[0] and mask.all()
    assert np.abs(poses[0]["R"] - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() <= 1e-6 and np.abs(poses[0]["t"]).max() <= 1e-6


def test_offset_of_1000_and_duplicate_indices(pkg):
    src, tgt, corr, kw = RT.cases()["offset1000_r1"]
    poses, _ = pkg.ransac_pose(src, tgt, corr, **kw)
    assert len(poses) == 2 and np.all(poses["refined"] == 1) and poses[0]["inliers"] >= 0.45 * len(corr)
    src, tgt, corr, kw = RT.cases()["duplicate_indices"]
    assert len(np.unique(corr[:, 0])) < len(corr) and len(pkg.ransac_pose(src, tgt, corr, **kw)[0]) >= 1


def _pose_error(pose):
    R = pose["R"].astype(np.float64)
    angle = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R @ RT.TRUE_R.T) - 1) / 2))))
    return angle, float(np.linalg.norm(pose["t"].astype(np.float64) - RT.TRUE_T))


def test_recovers_a_known_pose_from_30_percent_true_pairs(pkg):
    """M = 400, 30 % true under a rotation of 100 degrees about a skew axis, noise sigma = distance / 3, T = 2 000, refit: pose 0 within
    1 degree and 2 x distance of the truth with at least 90 % of the true pairs -- first of the twin, then of the library"""
    src, tgt, corr, is_true, kw = RT.recovery()
    assert len(corr) == 400 and 110 <= is_true.sum() <= 130 and kw["iterations"] == 2000 and kw["refine"] == 1
    for what, fn in (("twin", RT.ransac_pose), ("library", pkg.ransac_pose)):
        poses, mask = fn(src, tgt, corr, **kw)
        assert len(poses) == 1, what
        angle, shift = _pose_error(poses[0])
        share = (mask.astype(bool) & is_true).sum() / is_true.sum()
        print("%s: angle %.4f deg, shift %.5f, share of the true pairs %.4f, inliers %d" % (what, angle, shift, share, poses[0]["inliers"]))
        assert angle <= 1.0 and shift <= 2 * kw["distance"] and share >= 0.9, (what, angle, shift, share)


def test_select_matches(pkg):
    rng = np.random.default_rng(3)
    n = 300
    index = rng.integers(0, 500, n).astype(np.int32)
    d2 = rng.uniform(0, 1, n).astype(np.float32)
    second = (d2 * rng.uniform(1, 2, n)).astype(np.float32)
    second[::7] = np.inf
    second[3] = d2[3] = 0                                        # 0 <= r^2 * 0 passes
    mutual = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    for ratio in (0.0, 0.9, 1.0, 0.5):
        for mut, req in ((mutual, True), (mutual, False), (None, True), (None, False)):
            got = pkg.select_matches(index, d2, second, mut, ratio, req)
            # the statement
            r = np.float32(ratio)
            keep = (np.ones(n, bool) if (mut is None or not req) else mut != 0) & (np.ones(n, bool) if ratio == 0 else d2 <= (r * r) * second)
            want = np.stack([np.flatnonzero(keep), index[keep]], 1).astype(np.int32)
            assert got.dtype == np.int32 and got.tobytes() == want.tobytes() and RT.select_matches(index, d2, second, mut, ratio, req).tobytes() == want.tobytes()
            assert ratio != 0 or mut is not None and req or len(got) == n
    assert np.all(np.isin(np.arange(0, n, 7)[mutual[::7] != 0], pkg.select_matches(index, d2, second, mutual, 0.9)[:, 0]))   # +inf seconds pass


def test_refusals_write_nothing(pkg):
    lib = pkg.load_library()
    from cuda_go_icp_amd import binding as B
    fp, ip, bp, pp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(B.CRansacPose)
    src, tgt, corr, _ = RT.scene(65)
    corr = np.array(corr)
    ns, nt, M = len(src), len(tgt), len(corr)
    s, t, c = src.ctypes.data_as(fp), tgt.ctypes.data_as(fp), corr.ctypes.data_as(ip)
    poses, mask, count = np.full(64 * 15, -7, np.int32), np.full(M, 7, np.uint8), C.c_size_t(99)
    P, K, N = poses.ctypes.data_as(pp), mask.ctypes.data_as(bp), C.byref(count)
    limit = (2 ** 31 - 1) // 8

    def sel(distance=0.03, iterations=8, refine=1, max_poses=1, min_inliers=0, edge_similarity=0.9, seed=0):
        return C.byref(B.CRansacPoseSelect(distance, iterations, refine, max_poses, min_inliers, edge_similarity, seed))

    def call(s_=s, ns_=ns, t_=t, nt_=nt, c_=c, M_=M, **kw):
        return lib.goicp_ransac_pose_host(s_, ns_, t_, nt_, c_, M_, sel(**kw), P, N, K)

    assert call(s_=None) == INVALID and call(t_=None) == INVALID and call(c_=None) == INVALID
    assert lib.goicp_ransac_pose_host(s, ns, t, nt, c, M, None, P, N, K) == INVALID
    assert lib.goicp_ransac_pose_host(s, ns, t, nt, c, M, sel(), None, N, K) == INVALID
    assert lib.goicp_ransac_pose_host(s, ns, t, nt, c, M, sel(), P, None, K) == INVALID
    for m in (0, 1, 2):
        assert call(M_=m) == INVALID and b"three" in lib.goicp_last_error()
    assert call(M_=limit + 1) == INVALID and call(ns_=limit + 1) == INVALID and call(nt_=limit + 1) == INVALID
    for col, bad_index in ((0, -1), (0, ns), (1, -1), (1, nt)):
        bad = np.array(corr)
        bad[40, col] = bad_index
        assert call(c_=bad.ctypes.data_as(ip)) == INVALID and b"out of range" in lib.goicp_last_error()
    for bad_value in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            bad = np.array(tgt if which else src)
            bad[7, 1] = bad_value
            b = bad.ctypes.data_as(fp)
            assert (call(t_=b) if which else call(s_=b)) == INVALID and b"non-finite" in lib.goicp_last_error()
    for d in (0.0, -0.1, float("nan"), float("inf")):
        assert call(distance=d) == INVALID and b"distance" in lib.goicp_last_error(), d
    for kw, word in ((dict(iterations=-1), b"iterations"), (dict(iterations=B.RANSAC_POSE_MAX_ITERATIONS + 1), b"iterations"), (dict(max_poses=-1), b"max_poses"),
                     (dict(max_poses=B.RANSAC_POSE_MAX_POSES + 1), b"max_poses"), (dict(min_inliers=-1), b"min_inliers"), (dict(refine=2), b"refine"),
                     (dict(refine=-1), b"refine"), (dict(edge_similarity=-0.1), b"edge_similarity"), (dict(edge_similarity=1.5), b"edge_similarity"),
                     (dict(edge_similarity=float("nan")), b"edge_similarity")):
        assert call(**kw) == INVALID and word in lib.goicp_last_error(), kw
    assert np.all(poses == -7) and np.all(mask == 7) and count.value == 99
    # select_matches
    n = 10
    index, d2 = np.arange(n, dtype=np.int32), np.ones(n, np.float32)
    mut, out, m = np.ones(n, np.uint8), np.full((n, 2), -7, np.int32), C.c_size_t(99)
    I, D, U, O = index.ctypes.data_as(ip), d2.ctypes.data_as(fp), mut.ctypes.data_as(bp), out.ctypes.data_as(ip)
    assert lib.goicp_select_matches(None, D, D, U, n, 0.9, 1, O, C.byref(m)) == INVALID
    assert lib.goicp_select_matches(I, None, D, U, n, 0.9, 1, O, C.byref(m)) == INVALID
    assert lib.goicp_select_matches(I, D, None, U, n, 0.9, 1, O, C.byref(m)) == INVALID
    assert lib.goicp_select_matches(I, D, D, None, n, 0.9, 1, O, C.byref(m)) == INVALID
    assert lib.goicp_select_matches(I, D, D, U, n, 0.9, 1, None, C.byref(m)) == INVALID
    assert lib.goicp_select_matches(I, D, D, U, n, 0.9, 1, O, None) == INVALID
    assert lib.goicp_select_matches(I, D, D, U, 0, 0.9, 1, O, C.byref(m)) == INVALID
    assert lib.goicp_select_matches(I, D, D, U, limit + 1, 0.9, 1, O, C.byref(m)) == INVALID
    for ratio in (-0.5, float("nan"), float("inf")):
        assert lib.goicp_select_matches(I, D, D, U, n, ratio, 1, O, C.byref(m)) == INVALID and b"ratio" in lib.goicp_last_error()
    assert lib.goicp_select_matches(I, D, D, U, n, 0.9, 2, O, C.byref(m)) == INVALID
    assert np.all(out == -7) and m.value == 99
    assert lib.goicp_select_matches(I, D, D, None, n, 0.0, 0, O, C.byref(m)) == 0 and m.value == n
    # the defaults (iterations 0 = 100000 is too slow for a test: max_poses 0 = 1), the optional mask
    assert lib.goicp_ransac_pose_host(s, ns, t, nt, c, M, sel(max_poses=0), P, N, None) == 0 and count.value == 1 and np.all(mask == 7)


def test_shim_call_sites_compile():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_ransac.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_boundary(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    assert C.sizeof(B.CRansacPoseSelect) == 32 and C.sizeof(B.CRansacPose) == 60 and B.CRansacPoseSelect.seed.offset == 24
    assert NEW <= set(B.SYMBOLS) and all(hasattr(lib, name) for name in NEW)
    with open(os.path.join(ROOT, "include", "goicp_mi355.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NEW) and "GOICP_RANSAC_POSE_MAX_ITERATIONS (1 << 20)" in header and "GOICP_RANSAC_POSE_MAX_POSES 64" in header
    s = B.CRansacPoseSelect(1.0, 2, 0, 4, 5, 0.5, 6)
    lib.goicp_ransac_pose_select_default(C.byref(s))
    assert (s.distance, s.iterations, s.refine, s.max_poses, s.min_inliers, s.seed) == (0.0, 0, 1, 0, 0, 0) and abs(s.edge_similarity - 0.9) < 1e-7
    lib.goicp_ransac_pose_select_default(None)
    for name in ("ransac_pose", "select_matches", "feature_poses"):
        assert callable(getattr(pkg, name))
    for name in ("ransac_pose", "feature_poses", "register_features"):
        assert callable(getattr(pkg.Registration, name))
