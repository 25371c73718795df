"""goicp_knn_self and goicp_estimate_normals on the device.

The device path (kdbuild.hip: per level the voxel operator's key kernel, rocPRIM radix sort and the gather into sorted records; level 0
grid_knn_block_kernel, later levels and the top level grid_knn_wave_kernel, both with keys; normal_pca_kernel) against the host functions, element for
element, over the grid of tests/test_normals_host.py, and on clouds placed to cut the kernels' edges: sorted cells of exactly 1, 63, 64, 65,
255, 256, 257, 1, 1 and 511 points at the tier edges of k, 20 001 identical points (every candidate ties at 0: the rows are the smallest
other indices), a 12 x 12 x 12 unit lattice (every shell is a tie), a cluster with isolated points up to 10^4 cluster diameters away
(several levels, the wave kernel and its list), clouds without a first radius (the top level alone), k = n - 1 at n = 33, the grid's faces,
and viewpoints inside and outside the cloud.  Both calls leave the handle's fingerprint as it was, and so does every refused call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import normals_twin as NT
from conftest import ROOT, cloud, load_pkg
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


def assert_knn_equals_host(pkg, reg, xyz, k, tag, want=None):
    widx, wd2 = want if want is not None else pkg.knn_self(xyz, k)
    idx, d2 = reg.knn_self(xyz, k)
    assert np.array_equal(idx, widx), (tag, int(np.sum(np.any(idx != widx, axis=1))))
    assert NT.same_bits(d2, wd2), tag
    return idx, d2


def assert_normals_equal_host(pkg, reg, xyz, k, vp, tag, want=None):
    wn, wv, widx = want if want is not None else pkg.estimate_normals(xyz, k, vp)
    nrm, var, idx = reg.estimate_normals(xyz, k, vp)
    assert np.array_equal(idx, widx), (tag, int(np.sum(np.any(idx != widx, axis=1))))
    assert NT.same_bits(nrm, wn), (tag, int(np.sum(np.any(nrm.view(np.uint32) != wn.view(np.uint32), axis=1))))
    assert NT.same_bits(var, wv), (tag, int(np.sum(var.view(np.uint32) != wv.view(np.uint32))))
    return nrm, var, idx


# ----------------------------------------------------------------------------------------------
# the device against the host functions
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", NT.KINDS)
def test_device_equals_host_over_the_grid(pkg, reg, kind):
    for n in NT.SIZES:
        xyz = NT.make_cloud(kind, n)
        for k in NT.knn_ks_for(n):
            assert_knn_equals_host(pkg, reg, xyz, k, (kind, n, k))
        for k in NT.normal_ks_for(n):
            for vp in (None, NT.viewpoint_of(xyz)):
                assert_normals_equal_host(pkg, reg, xyz, k, vp, (kind, n, k, vp is not None))


def _cells():
    sizes = [1, 63, 64, 65, 255, 256, 257, 1, 1, 511]
    rng = np.random.default_rng(11)
    pts = np.concatenate([np.stack([c + rng.uniform(0.02, 0.98, s), rng.uniform(0.02, 0.98, s), rng.uniform(0.02, 0.98, s)], 1) for c, s in enumerate(sizes)])
    pts[0] = 0.0
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], np.float32)


def test_cells_cut_the_wave_and_workgroup_edges(pkg, reg):
    """cells of a unit grid along x with exactly these populations (shuffled input): sorted runs that end on, one before and one after a
    wave edge and a workgroup edge, with singletons between long ones -- at the tier edges of k, against the twin"""
    xyz = _cells()
    keys = NT.knn_keys(xyz, 32)
    for k in (1, 16, 17, 32):
        assert_knn_equals_host(pkg, reg, xyz, k, ("cells", k), NT.split(keys, k))
    for k in (17, 18):                                           # k - 1 on either side of the tier edge
        assert_normals_equal_host(pkg, reg, xyz, k, None, ("cells normals", k), NT.normals_twin(xyz, k, None, keys))


def test_20001_identical_points(pkg, reg):
    """every candidate ties at d2 = 0: row i is the k smallest indices other than i"""
    n = 20001
    xyz = NT.make_cloud("identical", n)
    for k in (1, 32):
        idx, d2 = reg.knn_self(xyz, k)
        want = np.tile(np.arange(k, dtype=np.int32), (n, 1))
        for i in range(k):
            want[i] = np.delete(np.arange(k + 1, dtype=np.int32), i)
        assert np.array_equal(idx, want) and not d2.any()
    nrm, var, idx = reg.estimate_normals(xyz, 8, np.float32([1, 2, 3]))
    assert not nrm.any() and not var.any() and not np.signbit(nrm).any()


def test_unit_lattice_where_every_shell_is_a_tie(pkg, reg):
    g = np.arange(12, dtype=np.float32)
    xyz = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[np.random.default_rng(4).permutation(1728)])
    keys = NT.knn_keys(xyz, 32)
    for k in (1, 6, 7, 18, 19, 26, 27, 32):                      # the shells hold 6, 12 and 8 points
        assert_knn_equals_host(pkg, reg, xyz, k, ("lattice", k), NT.split(keys, k))
    for k in (7, 19, 27):
        assert_normals_equal_host(pkg, reg, xyz, k, np.float32([5.5, 5.5, 40]), ("lattice normals", k),
                                  NT.normals_twin(xyz, k, np.float32([5.5, 5.5, 40]), keys))


def test_cluster_and_isolated_points_take_several_levels(pkg, capfd):
    """4 000 points in a cluster of diameter 1 and 50 points alone at 10 .. 10^4 diameters: the isolated points resolve only at radii far
    above the first level's, in the wave kernel.  The verbose line reports the levels that ran"""
    rng = np.random.default_rng(5)
    cluster = rng.uniform(-0.5, 0.5, (4000, 3))
    far = rng.normal(size=(50, 3))
    far = far / np.linalg.norm(far, axis=1)[:, None] * np.geomspace(10, 1e4, 50)[:, None]
    xyz = np.ascontiguousarray(np.concatenate([cluster, far])[rng.permutation(4050)], np.float32)
    keys = NT.knn_keys(xyz, 20)
    r = load_pkg().Registration(target(), source(37), 1e-3, dt_size=DT, verbose=1)
    try:
        for what, call in (("knn_self", lambda: r.knn_self(xyz, 20)), ("estimate_normals", lambda: r.estimate_normals(xyz, 21))):
            capfd.readouterr()
            got = call()
            err = capfd.readouterr().err
            line = re.search(what + r": 4050 -> 4050 points, levels (\d+), resolved((?: \d+)+), top (\d+)", err)
            assert line, err
            resolved = [int(v) for v in line.group(2).split()]
            assert int(line.group(1)) > 2 and sum(resolved) + int(line.group(3)) == 4050 and sum(v > 0 for v in resolved[1:]) >= 1, line.group(0)
            if what == "knn_self":
                widx, wd2 = NT.split(keys, 20)
                assert np.array_equal(got[0], widx) and NT.same_bits(got[1], wd2)
            else:
                wn, wv, widx = NT.normals_twin(xyz, 21, None, keys)
                assert np.array_equal(got[2], widx) and NT.same_bits(got[0], wn) and NT.same_bits(got[1], wv)
    finally:
        r.close()


@pytest.mark.parametrize("kind", ["zeros", "denormal", "identical"])
def test_clouds_without_a_first_radius_go_to_the_top_level(pkg, kind, capfd):
    """no r_0 whose square is a normal float (or no extent at all): no grid level runs and the top level serves every point"""
    xyz = NT.make_cloud(kind, 257)
    if kind == "zeros":
        xyz = np.ascontiguousarray(np.where(np.abs(xyz) > 1e-20, 0, xyz), np.float32)      # extent 2e-30: r_0 * r_0 underflows
    r = load_pkg().Registration(target(), source(37), 1e-3, dt_size=DT, verbose=1)
    try:
        capfd.readouterr()
        idx, d2 = r.knn_self(xyz, 5)
        err = capfd.readouterr().err
        assert re.search(r"knn_self: 257 -> 257 points, levels 1, resolved, top 257", err), err
        widx, wd2 = NT.knn_twin(xyz, 5)
        assert np.array_equal(idx, widx) and NT.same_bits(d2, wd2)
        assert_normals_equal_host(pkg, r, xyz, 6, np.float32([0, 0, 1]), (kind, "top level"), NT.normals_twin(xyz, 6, np.float32([0, 0, 1])))
    finally:
        r.close()


def test_k_equals_n_minus_1_at_33_points(pkg, reg):
    for kind in ("uniform", "duplicates", "denormal", "lattice"):
        xyz = NT.make_cloud(kind, 4097)[:33].copy()
        assert_knn_equals_host(pkg, reg, xyz, 32, (kind, "k = n - 1"), NT.knn_twin(xyz, 32))
        assert_normals_equal_host(pkg, reg, xyz, 32, None, (kind, "k - 1 = n - 2"), NT.normals_twin(xyz, 32))


def test_grid_faces(pkg, reg):
    """the "edge" cloud: both faces of every axis are occupied, with close pairs in the lowest and the highest cell"""
    xyz = NT.make_cloud("edge", 4097)
    keys = NT.keys_of("edge", 4097)
    for k in (1, 20):
        assert_knn_equals_host(pkg, reg, xyz, k, ("faces", k), NT.split(keys, k))
    assert_normals_equal_host(pkg, reg, xyz, 10, None, "faces normals", NT.normals_twin(xyz, 10, None, keys))


def test_viewpoint_inside_and_outside_the_cloud(pkg, reg):
    """a noisy sphere shell of radius 0.5: seen from its centre the normals point inwards, seen from far outside towards the viewer's side,
    and the two differ by the sign alone wherever both dot products are non-zero"""
    rng = np.random.default_rng(7)
    p = rng.normal(size=(3000, 3))
    xyz = np.ascontiguousarray(p / np.linalg.norm(p, axis=1)[:, None] * 0.5 + rng.normal(scale=0.002, size=(3000, 3)), np.float32)
    keys = NT.knn_keys(xyz, 15)
    inside, outside = np.float32([0, 0, 0]), np.float32([0, 0, 100])
    n_in = assert_normals_equal_host(pkg, reg, xyz, 16, inside, "inside", NT.normals_twin(xyz, 16, inside, keys))[0]
    n_out = assert_normals_equal_host(pkg, reg, xyz, 16, outside, "outside", NT.normals_twin(xyz, 16, outside, keys))[0]
    radial = np.einsum("ij,ij->i", n_in.astype(np.float64), xyz.astype(np.float64))
    assert np.all(radial < 0) and np.mean(radial / 0.5 < -0.95) > 0.95
    assert np.all(np.einsum("ij,ij->i", n_out.astype(np.float64), outside.astype(np.float64) - xyz) >= 0)
    assert np.all((n_in == n_out).all(1) | (n_in == -n_out).all(1))


def test_null_outputs(pkg, reg):
    lib = reg._lib
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = NT.make_cloud("uniform", 1000)
    widx = pkg.knn_self(xyz, 5)[0]
    wn = pkg.estimate_normals(xyz, 6)[0]
    idx, nrm = np.zeros((1000, 5), np.int32), np.zeros((1000, 3), np.float32)
    assert lib.goicp_knn_self(reg.handle, xyz.ctypes.data_as(fp), 1000, 5, idx.ctypes.data_as(ip), None) == 0
    assert np.array_equal(idx, widx)
    assert lib.goicp_estimate_normals(reg.handle, xyz.ctypes.data_as(fp), 1000, 6, None, nrm.ctypes.data_as(fp), None, None) == 0
    assert NT.same_bits(nrm, wn)


# ----------------------------------------------------------------------------------------------
# the handle
# ----------------------------------------------------------------------------------------------
def test_the_calls_leave_the_handle_untouched(pkg):
    a = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    b = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    try:
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), "before")
        a.knn_self(source(6000), 16)
        a.estimate_normals(source(6000), 16, np.float32([0, 0, 5]))
        a.estimate_normals(NT.make_cloud("identical", 300), 32)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the calls")
    finally:
        a.close(); b.close()


def test_refusals_leave_the_handle_as_it_was(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        good = source(2000)
        g = good.ctypes.data_as(fp)
        idx, d2 = np.full((2000, 32), -7, np.int32), np.full((2000, 32), -7, np.float32)
        nrm, var = np.full((2000, 3), -7, np.float32), np.full(2000, -7, np.float32)
        i, d, o, v = idx.ctypes.data_as(ip), d2.ctypes.data_as(fp), nrm.ctypes.data_as(fp), var.ctypes.data_as(fp)
        knn = lambda x, n, k: lib.goicp_knn_self(a.handle, x, n, k, i, d)
        nor = lambda x, n, k, vp=None: lib.goicp_estimate_normals(a.handle, x, n, k, vp, o, v, i)
        for call in (knn, nor):
            for bad_value in (np.nan, np.inf):
                bad = np.array(good)
                bad[1234, 2] = bad_value
                assert call(bad.ctypes.data_as(fp), 2000, 16) == INVALID and b"non-finite" in lib.goicp_last_error()
            assert call(g, 0, 16) == INVALID
            assert call(None, 2000, 16) == INVALID
            assert call(g, (2 ** 31 - 1) // 8 + 1, 16) == INVALID            # refused before a byte is read
            for k in (0, -1, 33, 2000):
                assert call(g, 2000, k) == INVALID, k
        assert knn(g, 16, 16) == INVALID and b"n - 1" in lib.goicp_last_error()
        assert nor(g, 16, 17) == INVALID and b"n - 1" in lib.goicp_last_error()
        assert nor(g, 2000, 2) == INVALID and nor(g, 2000, 1) == INVALID
        for bad_value in (np.nan, np.inf, -np.inf):
            vp = np.float32([0, bad_value, 0])
            assert nor(g, 2000, 16, vp.ctypes.data_as(fp)) == INVALID and b"viewpoint" in lib.goicp_last_error()
        assert lib.goicp_knn_self(a.handle, g, 2000, 16, None, d) == INVALID
        assert lib.goicp_estimate_normals(a.handle, g, 2000, 16, None, None, v, i) == INVALID
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        assert knn(g, 2000, 16) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert nor(g, 2000, 16) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert np.all(idx == -7) and np.all(d2 == -7) and np.all(nrm == -7) and np.all(var == -7)
        assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0      # the same history without the refused calls
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the refusals")
        assert knn(g, 2000, 16) == 0                                              # and a good call still works
        assert np.array_equal(idx.reshape(-1)[:2000 * 16].reshape(2000, 16), pkg.knn_self(good, 16)[0])
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------------------------
# the other ways in
# ----------------------------------------------------------------------------------------------
def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_normals.cpp as a program: icp::Registration::knn_self and estimate_normals on the device give the bits of the host
    functions (exit status 0)"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_normals")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_NORMALS_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_normals.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32"), "16"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "same bits" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_estimate_normals_end_to_end(pkg, tmp_path):
    """goicp_cli --estimate-normals IN OUT.ply --normal-k K --viewpoint X,Y,Z on a golden cloud: the PLY parsed back is the cloud with the
    host function's normals and variation (%.9g round-trips a float)"""
    pts = cloud("data_bunny")[:3000]
    with open(tmp_path / "scan.txt", "w") as f:
        f.write("%d\n" % len(pts))
        for q in pts:
            f.write("%.9g %.9g %.9g\n" % tuple(q))
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    for extra, vp in ((["--viewpoint", "0.5,-2,3.25"], np.float32([0.5, -2, 3.25])), ([], None)):
        out = tmp_path / "normals.ply"
        r = subprocess.run([exe, "--estimate-normals", str(tmp_path / "scan.txt"), str(out), "--normal-k", "12"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "on the device" in r.stdout, (r.returncode, r.stdout, r.stderr)
        lines = out.read_text().splitlines()
        end = lines.index("end_header")
        assert lines[0] == "ply" and "element vertex %d" % len(pts) in lines[:end]
        assert [l.split()[2] for l in lines[:end] if l.startswith("property")] == ["x", "y", "z", "nx", "ny", "nz", "curvature"]
        body = np.array([l.split() for l in lines[end + 1:]], np.float64).astype(np.float32)
        wn, wv, _ = pkg.estimate_normals(pts, 12, vp)
        assert body.shape == (len(pts), 7) and NT.same_bits(body[:, :3], pts) and NT.same_bits(body[:, 3:6], wn) and NT.same_bits(body[:, 6], wv)
