"""goicp_fpfh and goicp_match_features on the device.

The device path (kdbuild.hip: the self k-NN launch with its rows left on the device, spfh_kernel, fpfh_kernel; match_tile_kernel,
match_merge_kernel, match_mutual_kernel) against the host functions, element for element, over the grid and the constructed clouds of
tests/test_fpfh_host.py, and on inputs placed to cut the kernels' edges: the sorted cells of tests/test_gpu_normals.py (runs of 1, 63, 64,
65, 255, 256, 257 and 511 points) at the tier edges of k, point counts around the 15 points of an fpfh_kernel workgroup, target counts one
below, at and one above the matcher's LDS tile (the constant the library exports), more tiles than chunks, and ties.  Two runs give the
same bytes, and both calls leave the handle's fingerprint as it was, as does every refused call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fpfh_twin as FT
from conftest import ROOT, cloud, load_pkg
from test_gpu_normals import _cells
from test_gpu_voxel_downsample import _make, assert_same, fingerprint, source, target

pytestmark = pytest.mark.gpu
INVALID = -1
DT = 48


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


def assert_fpfh_equals_host(pkg, reg, xyz, k, nrm, tag):
    w, wc = pkg.fpfh(xyz, k, nrm)
    g, gc = reg.fpfh(xyz, k, nrm)
    assert np.array_equal(gc, wc), (tag, int(np.sum(np.any(gc != wc, axis=1))))
    assert FT.same_bits(g, w), (tag, int(np.sum(np.any(g.view(np.uint32) != w.view(np.uint32), axis=1))))
    return g, gc


def assert_match_equals_host(pkg, reg, q, t, tag):
    want, got = pkg.match_features(q, t), reg.match_features(q, t)
    assert np.array_equal(got[0], want[0]), (tag, int(np.sum(got[0] != want[0])))
    assert FT.same_bits(got[1], want[1]) and FT.same_bits(got[2], want[2]), tag
    assert np.array_equal(got[3], want[3]), (tag, int(np.sum(got[3] != want[3])))
    return got


# ----------------------------------------------------------------------------------------------
# descriptors
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FT.KINDS)
def test_device_equals_host_over_the_grid(pkg, reg, kind):
    for n in FT.SIZES:
        xyz = FT.make_cloud(kind, n)
        for k in FT.ks_for(n):
            assert_fpfh_equals_host(pkg, reg, xyz, k, FT.unit_normals(n, 100 * n + k), (kind, n, k, "random"))
            if n >= 4:
                assert_fpfh_equals_host(pkg, reg, xyz, k, pkg.estimate_normals(xyz, min(16, n))[0], (kind, n, k, "estimated"))


@pytest.mark.parametrize("name", sorted(FT.constructed()))
def test_constructed_clouds(pkg, reg, name):
    xyz, nrm, k = FT.constructed()[name]
    assert_fpfh_equals_host(pkg, reg, xyz, k, nrm, name)


def test_cells_cut_the_wave_and_workgroup_edges(pkg, reg):
    """the sorted runs of 1, 63, 64, 65, 255, 256, 257, 1, 1 and 511 points, at the tier edges of k"""
    xyz = _cells()
    for k in (1, 16, 17, 32):
        assert_fpfh_equals_host(pkg, reg, xyz, k, FT.unit_normals(len(xyz), k), ("cells", k))


@pytest.mark.parametrize("n", [14, 15, 16, 29, 30, 31, 255, 256, 257])
def test_point_counts_around_the_workgroups(pkg, reg, n):
    """15 points per fpfh_kernel workgroup, 256 per spfh_kernel workgroup: one below, at and one above"""
    xyz = np.ascontiguousarray(cloud("data_bunny")[::7][:n])
    for k in (1, 13):
        assert_fpfh_equals_host(pkg, reg, xyz, k, FT.unit_normals(n, n), (n, k))


def test_convenience_path_is_the_composition_of_the_host_functions(pkg, reg):
    xyz = cloud("data_bunny")[::9][:4000].copy()
    vp = np.float32([0, 0, 5])
    want = pkg.fpfh(xyz, 16, pkg.estimate_normals(xyz, 12, vp)[0])
    got = reg.fpfh(xyz, 16, normal_k=12, viewpoint=vp)
    assert np.array_equal(got[1], want[1]) and FT.same_bits(got[0], want[0])
    want = pkg.fpfh(xyz, 8, pkg.estimate_normals(xyz, 16)[0])
    got = reg.fpfh(xyz, 8)
    assert np.array_equal(got[1], want[1]) and FT.same_bits(got[0], want[0])


# ----------------------------------------------------------------------------------------------
# matching
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", FT.MATCH_SIZES)
def test_matching_equals_host_over_the_sizes(pkg, reg, nq):
    for nt in FT.MATCH_SIZES:
        got = assert_match_equals_host(pkg, reg, FT.descriptors(nq, nq), FT.descriptors(nt, 1000 + nt), (nq, nt))
        if nt == 1:
            assert np.all(np.isposinf(got[2]))


def test_target_tile_edges(pkg, reg):
    """n_t one below, at and one above one and two LDS tiles of the kernel, the size taken from the library"""
    tile = pkg.load_library().goicp_match_features_tile()
    assert tile >= 2
    q = FT.descriptors(300, 5)
    for nt in (tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1):
        assert_match_equals_host(pkg, reg, q, FT.descriptors(nt, nt), ("tile", nt))
        assert_match_equals_host(pkg, reg, FT.descriptors(nt, nt), q, ("tile, transposed", nt))


def test_more_tiles_than_chunks(pkg, reg):
    """64 workgroups of queries leave 32 chunks for 36 tiles of targets: a chunk walks two tiles, the last chunk ends inside its second"""
    tile = pkg.load_library().goicp_match_features_tile()
    q, t = FT.descriptors(64 * 256, 11), FT.descriptors(35 * tile + 5, 12)
    assert_match_equals_host(pkg, reg, q, t, "chunks")


def test_ties_and_identical_descriptors(pkg, reg):
    tile = pkg.load_library().goicp_match_features_tile()
    t = FT.descriptors(3 * tile, 7)
    t[2 * tile:] = t[:tile]                                        # a tile of targets twice, a tile and a chunk apart
    q = np.ascontiguousarray(np.concatenate([t[:tile] + np.float32(0.25), FT.descriptors(30, 8)]))
    got = assert_match_equals_host(pkg, reg, q, t, "duplicates")
    assert np.array_equal(got[0][:tile], np.arange(tile)) and FT.same_bits(got[1][:tile], got[2][:tile])
    same = np.full((300, 33), 1.5, np.float32)
    got = assert_match_equals_host(pkg, reg, same, same[:257], "identical")
    assert not got[0].any() and got[3][0] == 1 and not got[3][1:].any()


def test_real_descriptors_and_two_runs_give_the_same_bytes(pkg, reg):
    a, b = cloud("data_bunny")[::11][:3000].copy(), cloud("data_bunny")[5::13][:2500].copy()
    fa, ca = reg.fpfh(a, 16)
    fb, _ = reg.fpfh(b, 16)
    fa2, ca2 = reg.fpfh(a, 16)
    assert fa.tobytes() == fa2.tobytes() and ca.tobytes() == ca2.tobytes()
    m1 = assert_match_equals_host(pkg, reg, fa, fb, "bunny")
    m2 = reg.match_features(fa, fb)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(m1, m2))
    assert m1[3].sum() > 100


def test_null_optional_outputs(pkg, reg):
    lib = reg._lib
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz, nrm = FT.make_cloud("uniform", 1000), FT.unit_normals(1000, 3)
    out = np.zeros((1000, 33), np.float32)
    assert lib.goicp_fpfh(reg.handle, xyz.ctypes.data_as(fp), nrm.ctypes.data_as(fp), 1000, 9, out.ctypes.data_as(fp), None) == 0
    assert FT.same_bits(out, pkg.fpfh(xyz, 9, nrm)[0])
    q, t = FT.descriptors(100, 1), FT.descriptors(90, 2)
    idx, d2, second = np.zeros(100, np.int32), np.zeros(100, np.float32), np.zeros(100, np.float32)
    assert lib.goicp_match_features(reg.handle, q.ctypes.data_as(fp), 100, t.ctypes.data_as(fp), 90, idx.ctypes.data_as(ip), d2.ctypes.data_as(fp),
                                    second.ctypes.data_as(fp), None) == 0
    want = pkg.match_features(q, t)
    assert np.array_equal(idx, want[0]) and FT.same_bits(d2, want[1]) and FT.same_bits(second, want[2])


# ----------------------------------------------------------------------------------------------
# the handle
# ----------------------------------------------------------------------------------------------
def test_the_calls_leave_the_handle_untouched(pkg):
    a = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    b = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    try:
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), "before")
        f = a.fpfh(source(6000), 16)[0]
        a.fpfh(FT.make_cloud("identical", 300), 32, FT.unit_normals(300, 1))
        a.match_features(f[:2500], f[2500:])
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the calls")
    finally:
        a.close(); b.close()


def test_refusals_leave_the_handle_as_it_was(pkg):
    lib = pkg.load_library()
    fp, ip, bp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        good, nrm = source(2000), FT.unit_normals(2000, 2)
        g, m = good.ctypes.data_as(fp), nrm.ctypes.data_as(fp)
        out, cnt = np.full((2000, 33), -7, np.float32), np.full((2000, 33), 7, np.uint8)
        o, c = out.ctypes.data_as(fp), cnt.ctypes.data_as(bp)
        fpfh = lambda x, nm, n, k: lib.goicp_fpfh(a.handle, x, nm, n, k, o, c)
        for bad_value in (np.nan, np.inf):
            bad = np.array(good)
            bad[1234, 2] = bad_value
            assert fpfh(bad.ctypes.data_as(fp), m, 2000, 16) == INVALID and b"non-finite" in lib.goicp_last_error()
            bad = np.array(nrm)
            bad[1999, 0] = bad_value
            assert fpfh(g, bad.ctypes.data_as(fp), 2000, 16) == INVALID and b"non-finite normal" in lib.goicp_last_error()
        assert fpfh(g, m, 0, 16) == INVALID and fpfh(None, m, 2000, 16) == INVALID and fpfh(g, None, 2000, 16) == INVALID
        assert fpfh(g, m, (2 ** 31 - 1) // 8 + 1, 16) == INVALID                  # refused before a byte is read
        for k in (0, -1, 33, 2000):
            assert fpfh(g, m, 2000, k) == INVALID, k
        assert fpfh(g, m, 16, 16) == INVALID and b"n - 1" in lib.goicp_last_error()
        assert lib.goicp_fpfh(a.handle, g, m, 2000, 16, None, c) == INVALID
        q, t = FT.descriptors(2000, 1), FT.descriptors(900, 2)
        idx, d2, second, mut = np.full(2000, -7, np.int32), np.full(2000, -7, np.float32), np.full(2000, -7, np.float32), np.full(2000, 7, np.uint8)
        qp, tp, i, d, s, u = q.ctypes.data_as(fp), t.ctypes.data_as(fp), idx.ctypes.data_as(ip), d2.ctypes.data_as(fp), second.ctypes.data_as(fp), mut.ctypes.data_as(bp)
        match = lambda x, nq, y, nt: lib.goicp_match_features(a.handle, x, nq, y, nt, i, d, s, u)
        assert match(None, 2000, tp, 900) == INVALID and match(qp, 2000, None, 900) == INVALID
        assert match(qp, 0, tp, 900) == INVALID and match(qp, 2000, tp, 0) == INVALID
        big = (2 ** 31 - 1) // 8 + 1
        assert match(qp, big, tp, 900) == INVALID and match(qp, 2000, tp, big) == INVALID
        for bad_value in (np.nan, np.inf):
            bad = q.copy()
            bad[1999, 32] = bad_value
            assert match(bad.ctypes.data_as(fp), 2000, tp, 900) == INVALID and b"non-finite" in lib.goicp_last_error()
            bad = t.copy()
            bad[899, 0] = bad_value
            assert match(qp, 2000, bad.ctypes.data_as(fp), 900) == INVALID and b"non-finite" in lib.goicp_last_error()
        assert lib.goicp_match_features(a.handle, qp, 2000, tp, 900, None, d, s, u) == INVALID
        assert lib.goicp_match_features(a.handle, qp, 2000, tp, 900, i, None, s, u) == INVALID
        assert lib.goicp_match_features(a.handle, qp, 2000, tp, 900, i, d, None, u) == INVALID
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        assert fpfh(g, m, 2000, 16) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert match(qp, 2000, tp, 900) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert np.all(out == -7) and np.all(cnt == 7) and np.all(idx == -7) and np.all(d2 == -7) and np.all(second == -7) and np.all(mut == 7)
        assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0      # the same history without the refused calls
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the refusals")
        assert fpfh(g, m, 2000, 16) == 0 and match(qp, 2000, tp, 900) == 0       # and good calls still work
        assert FT.same_bits(out, pkg.fpfh(good, 16, nrm)[0]) and np.array_equal(idx, pkg.match_features(q, t)[0])
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------------------------
# the other ways in
# ----------------------------------------------------------------------------------------------
def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_fpfh.cpp as a program: icp::Registration::fpfh and match_features on the device give the bits of the host functions
    (exit status 0)"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_fpfh")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_FPFH_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_fpfh.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32"), "12"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "same bits" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_fpfh_match_end_to_end(pkg, tmp_path):
    """goicp_cli --fpfh-match SRC TGT OUT.txt --voxel V on two samples of a golden cloud: the lines are the mutual matches of the
    composition of the host functions on the voxel-reduced clouds"""
    clouds = [np.ascontiguousarray(cloud("data_bunny")[::3]), np.ascontiguousarray(cloud("data_bunny")[1::4])]
    for name, pts in zip(("a.txt", "b.txt"), clouds):
        with open(tmp_path / name, "w") as f:
            f.write("%d\n" % len(pts))
            for q in pts:
                f.write("%.9g %.9g %.9g\n" % tuple(q))
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    out = tmp_path / "matches.txt"
    r = subprocess.run([exe, "--fpfh-match", str(tmp_path / "a.txt"), str(tmp_path / "b.txt"), str(out), "--voxel", "0.02"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "on the device" in r.stdout, (r.returncode, r.stdout, r.stderr)
    small = [pkg.voxel_downsample(c, 0.02)[0] for c in clouds]
    fa, fb = (pkg.fpfh(c, 16)[0] for c in small)
    idx, d2, second, mutual = pkg.match_features(fa, fb)
    keep = np.flatnonzero(mutual)
    body = np.array([l.split() for l in out.read_text().splitlines()], np.float64)
    assert len(keep) > 20 and body.shape == (len(keep), 4)
    assert np.array_equal(body[:, 0].astype(np.int64), keep) and np.array_equal(body[:, 1].astype(np.int32), idx[keep])
    assert FT.same_bits(body[:, 2].astype(np.float32), d2[keep]) and FT.same_bits(body[:, 3].astype(np.float32), second[keep])
