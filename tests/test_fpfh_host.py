"""goicp_fpfh_host and goicp_match_features_host: the FPFH descriptors and the descriptor matching on the host (no handle, no GPU) against
the numpy twin of their definition (tests/fpfh_twin.py) -- descriptors, SPFH counts, indices, distances and mutual flags bit for bit over
the cloud kinds of the self k-NN's grid and over clouds constructed to hit the skip rules and the bin edges -- the table rule of the theta
bin against arctan2, the properties the definition promises (sub-histograms of 200, descriptors that turn with the cloud), every refusal,
the boundary (header, nm, binding, ABI version), the shim's call sites, the CLI mode, and the stand-alone selftest under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fpfh_twin as FT
import normals_twin as NT
from conftest import ROOT, cloud, load_pkg

INVALID = -1
NEW = {"goicp_fpfh_host", "goicp_fpfh", "goicp_match_features_host", "goicp_match_features", "goicp_match_features_tile"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def assert_fpfh(got, want, tag):
    (g, gc), (w, wc) = got, want
    assert gc.dtype == np.uint8 and np.array_equal(gc, wc), (tag, int(np.sum(np.any(gc != wc, axis=1))))
    assert FT.same_bits(g, w), (tag, int(np.sum(np.any(g.view(np.uint32) != w.view(np.uint32), axis=1))))


def assert_match(got, want, tag):
    assert np.array_equal(got[0], want[0]), (tag, int(np.sum(got[0] != want[0])))
    assert FT.same_bits(got[1], want[1]) and FT.same_bits(got[2], want[2]), tag
    assert got[3].dtype == np.uint8 and np.array_equal(got[3], want[3]), (tag, int(np.sum(got[3] != want[3])))


def normals_for(pkg, xyz, n, k):
    """random unit normals, and from 4 points up the library's own estimate as well"""
    out = [("random", FT.unit_normals(n, 100 * n + k))]
    if n >= 4:
        out.append(("estimated", pkg.estimate_normals(xyz, min(16, n))[0]))
    return out


@pytest.mark.parametrize("kind", FT.KINDS)
@pytest.mark.parametrize("n", FT.SIZES)
def test_library_equals_twin_over_the_grid(pkg, kind, n):
    xyz = FT.make_cloud(kind, n)
    keys = NT.keys_of(kind, n)
    for k in FT.ks_for(n):
        for name, nrm in normals_for(pkg, xyz, n, k):
            assert_fpfh(pkg.fpfh(xyz, k, nrm), FT.fpfh_twin(xyz, nrm, k, keys), (kind, n, k, name))


@pytest.mark.parametrize("name", sorted(FT.constructed()))
def test_constructed_clouds(pkg, name):
    xyz, nrm, k = FT.constructed()[name]
    want = FT.fpfh_twin(xyz, nrm, k)
    got = pkg.fpfh(xyz, k, nrm)
    assert_fpfh(got, want, name)
    cnt = got[1].astype(np.int64)
    idx, d2 = NT.knn_twin(xyz, k)
    f = FT.pair_features(xyz, nrm, idx)
    if name == "duplicates":
        # a duplicate is a neighbour at d2 == 0: its pair is skipped and its weight left out
        assert (d2 == 0).any() and np.array_equal(f["skip"], d2 == 0)
        assert np.array_equal(cnt[:, :11].sum(1), (d2 != 0).sum(1))
    elif name.startswith("lattice"):
        # axis normals on a unit lattice: a pair whose source normal lies along the offset is skipped (vl2 == 0), x is -1, 0 or 1, and
        # with the diagonal neighbours (k = 26) theta hits 0, pi / 2, -pi / 2 and pi exactly: the bin edges and the wrap
        ok = ~f["skip"]
        x, y = f["x"][ok], f["y"][ok]
        assert ok.any() and f["skip"].any() and set(np.unique(x)) <= {-1.0, 0.0, 1.0}
        assert ((x == 1) & (y == 0)).any() and ((x == -1) & (y == 0)).any() and ((x == 0) & (y == 0)).any()
        if k == 26:
            assert ((x == 0) & (y == 1)).any() and ((x == 0) & (y == -1)).any()
            b1 = f["b1"][ok]
            assert np.all(b1[(x == 1) & (y == 0)] == 5) and np.all(b1[(x == -1) & (y == 0)] == 0)
            assert np.all(b1[(x == 0) & (y == 1)] == 8) and np.all(b1[(x == 0) & (y == -1)] == 2)
    elif name == "plane":
        # equal normals across the plane: x = 1, y = 0, f2 = 0, f3 = 0 for every pair: one bin per group holds all k
        assert not f["skip"].any()
        want_cnt = np.zeros((len(xyz), 33), np.int64)
        want_cnt[:, [5, 16, 27]] = k
        assert np.array_equal(cnt, want_cnt)
    elif name == "anti-parallel":
        # x = 1 (theta 0, bin 5) between equal normals, x = -1, y = 0 (theta' = 2 pi = 0, bin 0) between opposite ones
        assert not f["skip"].any() and np.array_equal(cnt[:, 0] + cnt[:, 5], np.full(len(xyz), k)) and cnt[:, 0].any() and cnt[:, 5].any()
    elif name == "zero normals":
        zero = ~(nrm != 0).any(1)
        assert zero.sum() >= 50 and zero[3] and not cnt[zero].any()
        assert np.array_equal(f["skip"], zero[:, None] | zero[idx])
    elif name == "normal along d":
        # the pairs of the line: the offset is parallel to both normals, vl2 == 0
        line = np.arange(len(xyz)) < 40
        on_line = line[:, None] & line[idx]
        assert on_line.any() and f["skip"][on_line].all() and not f["skip"][~on_line].any()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_table_rule_is_the_theta_binning(seed):
    """on random clouds the twin's theta bin equals floor(11 (arctan2(y, x) + pi) / (2 pi)) for every pair whose theta lies at least 1e-9 rad
    from a bin edge (arctan2 and the scaling are good to a few 1e-16; the table's entries are within 2^-53 of the true cosines and sines and
    the cross product of two unit-size vectors is good to about 2e-16, so the rule can differ from the real angle only within about 1e-15 of
    an edge); at most 1e-4 of the pairs may lie that close"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (4000, 3)).astype(np.float32)
    nrm = FT.unit_normals(4000, 50 + seed)
    idx = NT.knn_twin(xyz, 16)[0]
    f = FT.pair_features(xyz, nrm, idx)
    ok = ~f["skip"]
    assert ok.mean() > 0.99
    theta = np.arctan2(f["y"][ok], f["x"][ok]) + np.pi
    step = 2 * np.pi / 11
    off = np.abs(theta / step - np.round(theta / step)) * step
    clear = off >= 1e-9
    share = 1.0 - clear.mean()
    print("seed %d: %d pairs, %.3g within 1e-9 rad of an edge" % (seed, ok.sum(), share))
    assert share <= 1e-4
    want = np.minimum(np.floor(theta / step).astype(np.int64), 10)
    assert np.array_equal(f["b1"][ok][clear], want[clear])
    assert len(np.unique(want)) == 11


def test_subhistograms_sum_to_200(pkg):
    """a point without a skipped pair: its own part sums to k * inc = 100 per group, the weighted part is scaled to 100"""
    xyz = FT.make_cloud("uniform", 1000)
    nrm = FT.unit_normals(1000, 9)
    for k in (1, 16, 32):
        out, cnt = pkg.fpfh(xyz, k, nrm)
        full = (cnt[:, :11].sum(1) == k) & (cnt[:, 11:22].sum(1) == k) & (cnt[:, 22:].sum(1) == k)
        assert full.mean() > 0.99
        sums = out.astype(np.float64).reshape(-1, 3, 11).sum(2)
        assert np.all(np.abs(sums[full] - 200.0) <= 1e-3), float(np.abs(sums[full] - 200.0).max())
        assert np.all(out >= 0)


def test_descriptors_turn_with_the_cloud(pkg):
    """a quarter turn about z maps (x, y, z) to (-y, x, z) exactly, points and normals: every sum of the definition only exchanges two
    addends of its first pair, so neighbours, counts and descriptors are the same bits"""
    xyz = cloud("data_bunny")[::10][:3000].copy()
    nrm = pkg.estimate_normals(xyz, 16)[0]
    turn = lambda a: np.ascontiguousarray(np.stack([-a[:, 1], a[:, 0], a[:, 2]], 1))
    for k in (5, 16):
        a, ca = pkg.fpfh(xyz, k, nrm)
        b, cb = pkg.fpfh(turn(xyz), k, turn(nrm))
        assert np.array_equal(ca, cb) and FT.same_bits(a, b), k


def test_convenience_path_is_the_composition(pkg):
    xyz = cloud("data_bunny")[::20][:1500].copy()
    vp = np.float32([0, 0, 5])
    nrm = pkg.estimate_normals(xyz, 12, vp)[0]
    assert_fpfh(pkg.fpfh(xyz, 10, normal_k=12, viewpoint=vp), pkg.fpfh(xyz, 10, nrm), "normals=None")
    assert_fpfh(pkg.fpfh(xyz, 10), pkg.fpfh(xyz, 10, pkg.estimate_normals(xyz, 16)[0]), "defaults")


# ----------------------------------------------------------------------------------------------
# matching
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", FT.MATCH_SIZES)
def test_matching_equals_twin_over_the_sizes(pkg, nq):
    for nt in FT.MATCH_SIZES:
        q, t = FT.descriptors(nq, nq), FT.descriptors(nt, 1000 + nt)
        got = pkg.match_features(q, t)
        assert_match(got, FT.match_twin(q, t), (nq, nt))
        if nt == 1:
            assert np.all(np.isposinf(got[2])) and not got[0].any() and got[3].sum() == 1
        without = pkg.match_features(q, t, mutual=False)
        assert without[3] is None and np.array_equal(without[0], got[0]) and FT.same_bits(without[2], got[2])


def test_matching_real_descriptors(pkg):
    a, b = cloud("data_bunny")[::23][:700].copy(), cloud("data_bunny")[5::29][:600].copy()
    fa, fb = pkg.fpfh(a, 16)[0], pkg.fpfh(b, 16)[0]
    got = pkg.match_features(fa, fb)
    assert_match(got, FT.match_twin(fa, fb), "bunny")
    assert got[3].sum() > 50 and np.all(got[1] <= got[2])


def test_duplicated_targets_tie_to_the_smaller_index(pkg):
    t = FT.descriptors(100, 7)
    t[100 - 37:] = t[:37]                                          # 37 targets appear twice
    q = np.ascontiguousarray(np.concatenate([t[:37] + np.float32(0.25), FT.descriptors(30, 8)]))
    got = pkg.match_features(q, t)
    assert_match(got, FT.match_twin(q, t), "duplicates")
    assert np.array_equal(got[0][:37], np.arange(37)) and FT.same_bits(got[1][:37], got[2][:37])


def test_identical_descriptors(pkg):
    q, t = np.full((70, 33), 1.5, np.float32), np.full((65, 33), 1.5, np.float32)
    idx, d2, second, mutual = pkg.match_features(q, t)
    assert not idx.any() and not d2.any() and not second.any()
    assert mutual[0] == 1 and not mutual[1:].any()
    assert_match((idx, d2, second, mutual), FT.match_twin(q, t), "identical")


# ----------------------------------------------------------------------------------------------
# refusals and the boundary
# ----------------------------------------------------------------------------------------------
def test_refusals_without_a_device(pkg):
    lib = pkg.load_library()
    fp, ip, bp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    xyz, nrm = FT.make_cloud("uniform", 16), FT.unit_normals(16, 1)
    out, cnt = np.full((16, 33), -7, np.float32), np.full((16, 33), 7, np.uint8)
    x, m, o, c = xyz.ctypes.data_as(fp), nrm.ctypes.data_as(fp), out.ctypes.data_as(fp), cnt.ctypes.data_as(bp)
    fpfh = lib.goicp_fpfh_host
    assert fpfh(None, m, 16, 3, o, c) == INVALID and fpfh(x, None, 16, 3, o, c) == INVALID and fpfh(x, m, 16, 3, None, c) == INVALID
    assert fpfh(x, m, 0, 3, o, c) == INVALID and fpfh(x, m, (2 ** 31 - 1) // 8 + 1, 3, o, c) == INVALID
    for k in (0, -1, -2 ** 31, 33, 1000):
        assert fpfh(x, m, 16, k, o, c) == INVALID and b"k must be" in lib.goicp_last_error(), k
    assert fpfh(x, m, 16, 16, o, c) == INVALID and b"n - 1" in lib.goicp_last_error()
    assert fpfh(x, m, 1, 1, o, c) == INVALID
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[7, 1] = bad_value
        assert fpfh(bad.ctypes.data_as(fp), m, 16, 3, o, c) == INVALID and b"non-finite" in lib.goicp_last_error()
        bad = nrm.copy()
        bad[15, 2] = bad_value
        assert fpfh(x, bad.ctypes.data_as(fp), 16, 3, o, c) == INVALID and b"non-finite normal" in lib.goicp_last_error()
    assert np.all(out == -7) and np.all(cnt == 7)
    assert fpfh(x, m, 16, 3, o, None) == 0 and FT.same_bits(out, FT.fpfh_twin(xyz, nrm, 3)[0])

    q, t = FT.descriptors(16, 1), FT.descriptors(9, 2)
    idx, d2, second, mut = np.full(16, -7, np.int32), np.full(16, -7, np.float32), np.full(16, -7, np.float32), np.full(16, 7, np.uint8)
    qp, tp, i, d, s, u = q.ctypes.data_as(fp), t.ctypes.data_as(fp), idx.ctypes.data_as(ip), d2.ctypes.data_as(fp), second.ctypes.data_as(fp), mut.ctypes.data_as(bp)
    match = lib.goicp_match_features_host
    assert match(None, 16, tp, 9, i, d, s, u) == INVALID and match(qp, 16, None, 9, i, d, s, u) == INVALID
    assert match(qp, 16, tp, 9, None, d, s, u) == INVALID and match(qp, 16, tp, 9, i, None, s, u) == INVALID and match(qp, 16, tp, 9, i, d, None, u) == INVALID
    assert match(qp, 0, tp, 9, i, d, s, u) == INVALID and match(qp, 16, tp, 0, i, d, s, u) == INVALID
    big = (2 ** 31 - 1) // 8 + 1
    assert match(qp, big, tp, 9, i, d, s, u) == INVALID and match(qp, 16, tp, big, i, d, s, u) == INVALID
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = q.copy()
        bad[15, 32] = bad_value
        assert match(bad.ctypes.data_as(fp), 16, tp, 9, i, d, s, u) == INVALID and b"non-finite" in lib.goicp_last_error()
        bad = t.copy()
        bad[8, 0] = bad_value
        assert match(qp, 16, bad.ctypes.data_as(fp), 9, i, d, s, u) == INVALID and b"non-finite" in lib.goicp_last_error()
    assert np.all(idx == -7) and np.all(d2 == -7) and np.all(second == -7) and np.all(mut == 7)
    assert match(qp, 16, tp, 9, i, d, s, None) == 0 and np.array_equal(idx, FT.match_twin(q, t)[0]) and np.all(mut == 7)
    # the handle-taking forms refuse a NULL handle before anything else
    assert lib.goicp_fpfh(None, x, m, 16, 3, o, c) == INVALID
    assert lib.goicp_match_features(None, qp, 16, tp, 9, i, d, s, u) == INVALID


def test_header_nm_and_binding_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    for decl in (r"int goicp_fpfh_host\(const float\* xyz, const float\* normals, size_t n, int32_t k, float\* out_fpfh, uint8_t\* out_spfh_counts\);",
                 r"int goicp_fpfh\(goicp_handle h, const float\* xyz, const float\* normals, size_t n, int32_t k, float\* out_fpfh, uint8_t\* out_spfh_counts\);",
                 r"int goicp_match_features_host\(const float\* query, size_t n_q, const float\* target, size_t n_t, int32_t\* out_index, float\* out_d2, float\* out_d2_second,\s+uint8_t\* out_mutual\);",
                 r"int goicp_match_features\(goicp_handle h, const float\* query, size_t n_q, const float\* target, size_t n_t, int32_t\* out_index, float\* out_d2,\s+float\* out_d2_second, uint8_t\* out_mutual\);",
                 r"#define GOICP_FPFH_DIM 33\b"):
        assert re.search(decl, hdr), decl
    assert re.search(r"#define GOICP_ABI_VERSION 4\b", hdr)
    # the table: twenty literals, the cosines and sines of 2 pi k / 11.  numpy's own differ by the rounding of the angle, up to
    # 5.8 * 2^-52 = 1.3e-15, and a few 1e-16 of the function: within 2e-15; the pairs lie on the unit circle and mirror about pi
    ang = 2 * np.pi * np.arange(1, 11) / 11
    assert np.all(np.abs(FT.COS - np.cos(ang)) <= 2e-15) and np.all(np.abs(FT.SIN - np.sin(ang)) <= 2e-15)
    assert np.all(np.abs(FT.COS * FT.COS + FT.SIN * FT.SIN - 1.0) <= 4 * 2.0 ** -52)
    assert np.array_equal(FT.COS, FT.COS[::-1]) and np.array_equal(FT.SIN, -FT.SIN[::-1])
    from cuda_go_icp_amd import binding
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("goicp_") and " T " in l}
    assert NEW <= exported and NEW <= set(binding.SYMBOLS)
    lib = pkg.load_library()
    assert lib.goicp_abi_version() == 4 and lib.goicp_match_features_tile() >= 1
    fp, ip, bp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    assert lib.goicp_fpfh_host.argtypes == [fp, fp, C.c_size_t, C.c_int32, fp, bp]
    assert lib.goicp_fpfh.argtypes == [C.c_void_p, fp, fp, C.c_size_t, C.c_int32, fp, bp]
    assert lib.goicp_match_features_host.argtypes == [fp, C.c_size_t, fp, C.c_size_t, ip, fp, fp, bp]
    assert lib.goicp_match_features.argtypes == [C.c_void_p, fp, C.c_size_t, fp, C.c_size_t, ip, fp, fp, bp]
    assert callable(pkg.fpfh) and callable(pkg.match_features)
    assert hasattr(pkg.Registration, "fpfh") and hasattr(pkg.Registration, "match_features")
    shim = open(os.path.join(ROOT, "include", "goicp_mi355.hpp")).read()
    assert "goicp_fpfh(h_" in shim and "goicp_match_features(h_" in shim


def test_shim_fpfh_call_sites_compile():
    """tests/shim_fpfh.cpp, compiled as tests/shim_normals.cpp is: syntax only"""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_fpfh.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_fpfh_match_refusals_before_any_device(pkg, tmp_path):
    """exit status 2 with the reason; the inputs named do not exist, so a run that got as far as loading them would end with status 1"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    src, tgt, out = str(tmp_path / "a.txt"), str(tmp_path / "b.txt"), str(tmp_path / "out.txt")
    for args, word in ((["--ranks", "2"], "--ranks"), (["--fpfh-k", "0"], "--fpfh-k"), (["--fpfh-k", "33"], "--fpfh-k"), (["--fpfh-k"], "--fpfh-k"),
                       (["--normal-k", "2"], "--normal-k"), (["--normal-k", "k"], "--normal-k"), (["--voxel", "0"], "--voxel"),
                       (["--voxel", "nan"], "--voxel"), (["--viewpoint", "1,2,3"], "--viewpoint")):
        r = subprocess.run([exe, "--fpfh-match", src, tgt, out] + args, capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([exe, "--fpfh-match", src, tgt], capture_output=True, text=True)
    assert r.returncode == 2 and "SRC, TGT and OUT" in r.stderr
    assert not os.path.exists(out)


def test_cli_fpfh_match_writes_the_host_functions_matches(pkg, tmp_path):
    """goicp_cli --fpfh-match on two samples of a golden cloud, wherever it runs (the device when there is one, the host otherwise: the same
    bits): one line i j d2 d2_second per mutual match of the composition of the host functions (%.9g round-trips a float)"""
    clouds = [cloud("data_bunny")[::31][:500], cloud("data_bunny")[7::37][:450]]
    for name, pts in zip(("a.txt", "b.txt"), clouds):
        with open(tmp_path / name, "w") as f:
            f.write("%d\n" % len(pts))
            for q in pts:
                f.write("%.9g %.9g %.9g\n" % tuple(q))
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    out = tmp_path / "matches.txt"
    r = subprocess.run([exe, "--fpfh-match", str(tmp_path / "a.txt"), str(tmp_path / "b.txt"), str(out), "--fpfh-k", "12", "--normal-k", "10"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fpfh match: 500 x 450 points, k 12, normal k 10" in r.stdout, (r.returncode, r.stdout, r.stderr)
    fa, fb = (pkg.fpfh(np.ascontiguousarray(c), 12, normal_k=10)[0] for c in clouds)
    idx, d2, second, mutual = pkg.match_features(fa, fb)
    keep = np.flatnonzero(mutual)
    body = np.array([l.split() for l in out.read_text().splitlines()], np.float64)
    assert len(keep) > 20 and body.shape == (len(keep), 4)
    assert np.array_equal(body[:, 0].astype(np.int64), keep) and np.array_equal(body[:, 1].astype(np.int32), idx[keep])
    assert FT.same_bits(body[:, 2].astype(np.float32), d2[keep]) and FT.same_bits(body[:, 3].astype(np.float32), second[keep])


@pytest.mark.parametrize("target", ["fpfh-asan", "fpfh-tsan"])
def test_fpfh_selftest_under_the_sanitizers(target):
    """csrc/fpfh_selftest.cpp: the host functions against an all-pairs restatement, the threaded paths included, built with
    -fsanitize=address,undefined / -fsanitize=thread and run as a program of its own"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cuda-go-icp_amd", "csrc"), target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "fpfh selftest ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
