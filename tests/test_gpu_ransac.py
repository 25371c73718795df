"""goicp_ransac_pose on the device.

The kernels of kdbuild.hip (gather, hypothesis, score, keys + rocPRIM sort, take, moments, mask) against the host function, pose records
and inlier mask byte for byte, over the cases of tests/ransac_twin.py (M around the score workgroup's 1 024 correspondences, T around the
256-hypothesis LDS tile and two tiles + 1, refine 0 / 1, max_poses 1 / 2 / 64, edge_similarity 0 / 0.9 / 1, the degenerate inputs), and
on a larger case with many workgroups in both grid directions.  Two device runs give the same bytes.  goicp_ransac_pose leaves the
handle's fingerprint (tests/test_gpu_voxel_downsample.py) as it was, and so does every refused call.  Registration.feature_poses on the
device equals the composition of the host functions; Registration.register_features returns the candidate with the smallest
icp_run_batch error; the C++ shim's call sites run; goicp_cli --feature-init parses and finishes, and without the flag the CLI prints
what it printed before."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_twin as RT
from conftest import ROOT, load_pkg
from test_gpu_voxel_downsample import _make, assert_same, fingerprint, source, target

pytestmark = pytest.mark.gpu
INVALID = -1
DT = 48
FEATURE = dict(voxel=0.05, k=32, distance=0.075, normal_k=32, iterations=4000, max_poses=8, seed=1)


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def reg(pkg):
    r = pkg.Registration(target(), source(37), 1e-3, dt_size=DT)
    yield r
    r.close()


def same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(RT.cases()))
def test_device_equals_host(pkg, reg, name):
    src, tgt, corr, kw = RT.cases()[name]
    want, got = pkg.ransac_pose(src, tgt, corr, **kw), reg.ransac_pose(src, tgt, corr, **kw)
    assert same(got, want), (name, got[0], want[0], int(np.sum(got[1] != want[1])))


def test_two_runs_give_identical_bytes(pkg, reg):
    for name in ("scene1025_T513", "offset1000_r1"):
        src, tgt, corr, kw = RT.cases()[name]
        assert same(reg.ransac_pose(src, tgt, corr, **kw), reg.ransac_pose(src, tgt, corr, **kw)), name


def test_a_larger_case_with_many_workgroups(pkg, reg):
    """M = 5 000 and T = 3 000: five workgroups of correspondences times twelve tiles of hypotheses, atomics between them, eight poses refit"""
    src, tgt, corr, _ = RT.scene(5000, 0.4, 0.005, seed=9)
    kw = dict(distance=0.03, iterations=3000, refine=1, max_poses=8, edge_similarity=0.9, seed=2)
    want, got = pkg.ransac_pose(src, tgt, corr, **kw), reg.ransac_pose(src, tgt, corr, **kw)
    assert same(got, want), (got[0], want[0])
    assert len(want[0]) == 8 and want[0][0]["inliers"] >= 1800


def test_operator_and_refusals_leave_the_handle_as_it_was(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    fp, ip, bp, pp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(B.CRansacPose)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        src, tgt, corr, _ = RT.scene(257)
        corr = np.array(corr)
        ns, nt, M = len(src), len(tgt), len(corr)
        s, t, c = src.ctypes.data_as(fp), tgt.ctypes.data_as(fp), corr.ctypes.data_as(ip)
        poses, mask, count = np.full(64 * 15, -7, np.int32), np.full(M, 7, np.uint8), C.c_size_t(99)
        P, K, N = poses.ctypes.data_as(pp), mask.ctypes.data_as(bp), C.byref(count)
        limit = (2 ** 31 - 1) // 8

        def sel(distance=0.03, iterations=64, refine=1, max_poses=1, min_inliers=0, edge_similarity=0.9, seed=0):
            return C.byref(B.CRansacPoseSelect(distance, iterations, refine, max_poses, min_inliers, edge_similarity, seed))

        def call(s_=s, ns_=ns, t_=t, nt_=nt, c_=c, M_=M, **kw):
            return lib.goicp_ransac_pose(a.handle, s_, ns_, t_, nt_, c_, M_, sel(**kw), P, N, K)

        assert call(s_=None) == INVALID and call(t_=None) == INVALID and call(c_=None) == INVALID
        assert lib.goicp_ransac_pose(None, s, ns, t, nt, c, M, sel(), P, N, K) == INVALID
        assert lib.goicp_ransac_pose(a.handle, s, ns, t, nt, c, M, None, P, N, K) == INVALID
        assert lib.goicp_ransac_pose(a.handle, s, ns, t, nt, c, M, sel(), None, N, K) == INVALID
        assert lib.goicp_ransac_pose(a.handle, s, ns, t, nt, c, M, sel(), P, None, K) == INVALID
        for m in (0, 2, limit + 1):
            assert call(M_=m) == INVALID
        assert call(ns_=limit + 1) == INVALID and call(nt_=limit + 1) == INVALID
        for col, bad_index in ((0, -1), (0, ns), (1, -1), (1, nt)):
            bad = np.array(corr)
            bad[40, col] = bad_index
            assert call(c_=bad.ctypes.data_as(ip)) == INVALID and b"out of range" in lib.goicp_last_error()
        for bad_value in (np.nan, np.inf):
            bad = np.array(src)
            bad[7, 1] = bad_value
            assert call(s_=bad.ctypes.data_as(fp)) == INVALID and b"non-finite" in lib.goicp_last_error()
        for d in (0.0, -0.1, float("nan"), float("inf")):
            assert call(distance=d) == INVALID, d
        for kw in (dict(iterations=-1), dict(iterations=B.RANSAC_POSE_MAX_ITERATIONS + 1), dict(max_poses=-1), dict(max_poses=65), dict(min_inliers=-1),
                   dict(refine=2), dict(edge_similarity=-0.1), dict(edge_similarity=1.5), dict(edge_similarity=float("nan"))):
            assert call(**kw) == INVALID, kw
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        assert call() == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert np.all(poses == -7) and np.all(mask == 7) and count.value == 99
        # the operator itself leaves the handle alone
        got = a.ransac_pose(src, tgt, corr, 0.03, 300, max_poses=4)
        assert len(got[0]) >= 1
        assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0      # the same history without the refused calls
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the operator and the refusals")
    finally:
        a.close(); b.close()


@functools.lru_cache(maxsize=None)
def turned_pair():
    """2 000 points of the bunny scan, and a copy turned by 100 degrees about a skew axis and moved"""
    src = source(2000)
    tgt = np.ascontiguousarray((src.astype(np.float64) @ RT.TRUE_R.T + RT.TRUE_T).astype(np.float32))
    tgt.setflags(write=False)
    vp = np.array([0.0, 0.0, 3.0])
    return src, tgt, tuple(vp), tuple(RT.TRUE_R @ vp + RT.TRUE_T)


def test_feature_poses_equal_the_composition_of_the_host_functions(pkg, reg):
    src, tgt, vps, vpt = turned_pair()
    want = pkg.feature_poses(src, tgt, viewpoint_src=vps, viewpoint_tgt=vpt, **FEATURE)
    got = reg.feature_poses(src, tgt, viewpoint_src=vps, viewpoint_tgt=vpt, **FEATURE)
    assert same((got[0],), (want[0],)), (got[0], want[0])
    for key in ("src", "tgt", "corr", "inlier"):
        assert got[1][key].dtype == want[1][key].dtype and got[1][key].tobytes() == want[1][key].tobytes(), key
    # the composition, spelled out
    ds, dt = pkg.voxel_downsample(src, FEATURE["voxel"])[0], pkg.voxel_downsample(tgt, FEATURE["voxel"])[0]
    fs = pkg.fpfh(ds, FEATURE["k"], normals=pkg.estimate_normals(ds, FEATURE["normal_k"], vps)[0])[0]
    ft = pkg.fpfh(dt, FEATURE["k"], normals=pkg.estimate_normals(dt, FEATURE["normal_k"], vpt)[0])[0]
    corr = pkg.select_matches(*pkg.match_features(fs, ft))
    assert corr.tobytes() == want[1]["corr"].tobytes() and len(corr) >= 3
    poses = pkg.ransac_pose(ds, dt, corr, FEATURE["distance"], FEATURE["iterations"], max_poses=FEATURE["max_poses"], seed=FEATURE["seed"])[0]
    assert poses.tobytes() == want[0].tobytes()


def test_register_features_returns_the_candidate_with_the_smallest_batch_error(pkg):
    src, tgt, vps, vpt = turned_pair()
    r = pkg.Registration(tgt, src, 1e-3, dt_size=DT)
    try:
        poses, _ = r.feature_poses(r.pcs, r.pct, viewpoint_src=vps, viewpoint_tgt=vpt, **FEATURE)
        assert len(poses) >= 1
        R, t, err, it = r.icp_run_batch(poses["R"], poses["t"], 60, 1e-7)
        best = int(np.argmin(err))
        gR, gt, gerr, info = r.register_features(max_iter=60, err_diff=1e-7, viewpoint_src=vps, viewpoint_tgt=vpt, **FEATURE)
        assert info["best"] == best and gR.tobytes() == R[best].tobytes() and gt.tobytes() == t[best].tobytes() and np.float32(gerr).tobytes() == err[best].tobytes()
        assert info["err"].tobytes() == err.tobytes() and np.array_equal(info["inliers"], poses["inliers"]) and len(info["err"]) == len(poses)
    finally:
        r.close()


def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_ransac.cpp as a program: icp::Registration::select_matches / ransac_pose agree with the host functions (pose records and
    mask as bytes) and find the pose the target was made with"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_ransac")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_RANSAC_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_ransac.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "operators agree" in r.stdout and "is the pose" in r.stdout, (r.returncode, r.stdout, r.stderr)


def _write_cloud(path, pts):
    with open(path, "w") as f:
        f.write("%d\n" % len(pts))
        for q in pts:
            f.write("%.9g %.9g %.9g\n" % tuple(q))


def _cli(tmp_path, *args, io=""):
    src, tgt, _, _ = turned_pair()
    _write_cloud(tmp_path / "model.txt", tgt)
    _write_cloud(tmp_path / "scan.txt", src)
    (tmp_path / "cfg.toml").write_text('[info]\ndescription = "feature init"\n[io]\ntarget = "model.txt"\nsource = "scan.txt"\n' + io +
                                       '[params]\nmode = 1\nsubsample = 1.0\nmse_threshold = 1e-3\nresize = 1.0\n')
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    return subprocess.run([exe, str(tmp_path / "cfg.toml"), "--iters", "20"] + list(args), capture_output=True, text=True, timeout=120)


def test_cli_feature_init(pkg, tmp_path):
    r = _cli(tmp_path, "--feature-init", "--feature-voxel", str(FEATURE["voxel"]), "--fpfh-k", "32", "--normal-k", "32", "--match-ratio", "0",
             "--ransac-distance", str(FEATURE["distance"]), "--ransac-iterations", "4000", "--ransac-poses", "8", "--ransac-seed", "1")
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert re.search(r"feature init: \d+ x \d+ points, fpfh k 32, normal k 32, ratio 0: \d+ correspondences; ransac distance 0.075 iterations 4000: \d+ poses", r.stdout), r.stdout
    assert "ICP from the feature pose after" in r.stdout and "Optimal Rotation Matrix:" in r.stdout
    bad = _cli(tmp_path, "--ransac-distance", "0.1")
    assert bad.returncode == 2 and "needs --feature-init" in bad.stderr
    bad = _cli(tmp_path, "--feature-init", "--ransac-poses", "65", "--ransac-distance", "0.1")
    assert bad.returncode == 2 and "--ransac-poses" in bad.stderr
    bad = _cli(tmp_path, "--feature-init", "--ransac-distance", "0.1", io='output = "out.toml"\n')
    assert bad.returncode == 1 and "cannot be combined with [io] output" in bad.stderr and not (tmp_path / "out.toml").exists()


def test_cli_without_the_flag_prints_what_it_printed(pkg, tmp_path):
    r = _cli(tmp_path)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert "feature" not in r.stdout
    i = [k for k, l in enumerate(lines) if l.startswith("mode 1: source 2000 points, target 2000 points, mse_threshold")]
    assert len(i) == 1
    tail = lines[i[0] + 1:]
    assert re.fullmatch(r"ICP after 20 iterations: SSE \S+", tail[0]) and tail[1] == "Optimal Rotation Matrix:" and tail[5] == "Optimal Translation Vector:"
    assert all(len(l.split()) == 3 for l in tail[2:5]) and all(len(l.split()) == 1 for l in tail[6:9])
