"""goicp_statistical_outlier_removal and goicp_set_source_pipeline on the device.

The device filter (kdbuild.hip: per level the voxel operator's key kernel, rocPRIM radix sort and the gather into sorted records; level 0
grid_knn_block_kernel, later levels and the top level grid_knn_wave_kernel, both with distances; then the maximum, the exact sums, the finishing thread, the
flags, rocPRIM scan and the compaction) against the host function, element for element, over the grid of
tests/test_stat_outlier_host.py, and on clouds placed to cut the kernels' edges: sorted cells of exactly 1, 63, 64, 65, 255, 256, 257, 1, 1
and 511 points at the tier edges of k, 20 001 identical points, a cluster with isolated points up to 10^4 cluster diameters away (several
levels), k = n - 1, and the grid's faces.

goicp_set_source_pipeline: handle A swaps to the raw cloud behind the chain, handle B swaps to the composition of the host functions with
goicp_set_source, and every answer of the C ABI must be the same BYTES (the fingerprint of tests/test_gpu_voxel_downsample.py).
goicp_statistical_outlier_removal leaves the handle's fingerprint as it was, and so does every refused call."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import stat_outlier_twin as ST
from conftest import ROOT, cloud, load_pkg
from test_gpu_voxel_downsample import VARIANTS, _make, assert_same, fingerprint, reduced, source, target

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


@functools.lru_cache(maxsize=None)
def composed(n, voxel, k, alpha, radius, min_neighbors):
    """the composition of the host functions for source(n): computed once, shared, never changed"""
    pkg = load_pkg()
    d = reduced(n, voxel) if voxel else source(n)
    if k:
        d = pkg.statistical_outlier_removal(d, k, alpha)[0]
    if radius:
        d = pkg.radius_outlier_removal(d, radius, min_neighbors)[0]
    d.setflags(write=False)
    return d


def assert_device_equals_host(pkg, reg, xyz, k, alpha, tag, want=None):
    want, widx, wu, wthr = want if want is not None else pkg.statistical_outlier_removal(xyz, k, alpha)
    got, idx, u, thr = reg.statistical_outlier_removal(xyz, k, alpha)
    assert ST.same_bits(u, wu), (tag, int(np.sum(u.view(np.uint32) != wu.view(np.uint32))))
    assert np.float64(thr).tobytes() == np.float64(wthr).tobytes(), (tag, thr, wthr)
    assert len(got) == len(want) and np.array_equal(idx, widx), (tag, len(got), len(want))
    assert ST.same_bits(got, want), tag
    return got, idx, u, thr


# ----------------------------------------------------------------------------------------------
# the device filter against the host function
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ST.KINDS)
def test_device_equals_host_over_the_grid(pkg, reg, kind):
    for n in ST.SIZES:
        xyz = ST.make_cloud(kind, n)
        for k in ST.ks_for(n):
            for alpha in ST.ALPHAS:
                assert_device_equals_host(pkg, reg, xyz, k, alpha, (kind, n, k, alpha))


def test_cells_cut_the_wave_and_workgroup_edges(pkg, reg):
    """cells of a unit grid along x with exactly these populations (shuffled input): sorted runs that end on, one before and one after a
    wave edge and a workgroup edge, with singletons between long ones -- at the tier edges of k, against the twin"""
    sizes = [1, 63, 64, 65, 255, 256, 257, 1, 1, 511]
    rng = np.random.default_rng(11)
    pts = np.concatenate([np.stack([c + rng.uniform(0.02, 0.98, s), rng.uniform(0.02, 0.98, s), rng.uniform(0.02, 0.98, s)], 1) for c, s in enumerate(sizes)])
    pts[0] = 0.0
    xyz = np.ascontiguousarray(pts[rng.permutation(len(pts))], np.float32)
    nearest = ST.nearest_d2(xyz, 64)
    for k in (1, 16, 17, 32, 33, 64):
        assert_device_equals_host(pkg, reg, xyz, k, 1.0, ("cells", k), ST.twin(xyz, k, 1.0, nearest))


def test_20001_identical_points(pkg, reg):
    n = 20001
    xyz = ST.make_cloud("identical", n)
    got, idx, u, thr = reg.statistical_outlier_removal(xyz, 64, 2.0)      # the answer is known: every distance is 0
    assert len(got) == n and np.array_equal(idx, np.arange(n)) and not u.any() and thr == 0.0 and ST.same_bits(got, xyz)


def test_cluster_and_isolated_points_take_several_levels(pkg, capfd):
    """4 000 points in a cluster of diameter 1 and 50 points alone at 10 .. 10^4 diameters: the isolated points resolve only at radii far
    above the first level's.  The verbose line reports the levels that ran"""
    rng = np.random.default_rng(5)
    cluster = rng.uniform(-0.5, 0.5, (4000, 3))
    far = rng.normal(size=(50, 3))
    far = far / np.linalg.norm(far, axis=1)[:, None] * np.geomspace(10, 1e4, 50)[:, None]
    xyz = np.ascontiguousarray(np.concatenate([cluster, far])[rng.permutation(4050)], np.float32)
    r = load_pkg().Registration(target(), source(37), 1e-3, dt_size=DT, verbose=1)
    try:
        capfd.readouterr()
        got, idx, u, thr = r.statistical_outlier_removal(xyz, 20, 2.0)
        err = capfd.readouterr().err
    finally:
        r.close()
    line = re.search(r"statistical_outlier_removal: 4050 -> (\d+) points, levels (\d+), resolved((?: \d+)+), top (\d+)", err)
    assert line, err
    resolved = [int(v) for v in line.group(3).split()]
    assert int(line.group(2)) > 2 and sum(resolved) + int(line.group(4)) == 4050 and sum(v > 0 for v in resolved) > 2, line.group(0)
    want = ST.twin(xyz, 20, 2.0)
    assert len(want[1]) == int(line.group(1)) < 4050
    assert ST.same_bits(u, want[2]) and np.array_equal(idx, want[1]) and ST.same_bits(got, want[0]) and thr == want[3]


def test_k_equals_n_minus_1(pkg, reg):
    for kind in ("uniform", "duplicates", "denormal"):
        xyz = ST.make_cloud(kind, 65)
        assert_device_equals_host(pkg, reg, xyz, 64, 1.0, (kind, "k = n - 1"), ST.twin(xyz, 64, 1.0))


def test_grid_faces(pkg, reg):
    """the "edge" cloud: both faces of every axis are occupied, with close pairs in the lowest and the highest cell"""
    xyz = ST.make_cloud("edge", 4097)
    for k in (1, 20):
        assert_device_equals_host(pkg, reg, xyz, k, 2.0, ("faces", k), ST.twin(xyz, k, 2.0, ST.nearest_of("edge", 4097)))


def test_null_outputs(pkg, reg):
    lib = reg._lib
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = ST.make_cloud("uniform", 4097)
    want, widx, wu, wthr = pkg.statistical_outlier_removal(xyz, 20, 1.0)
    assert 0 < len(want) < 4097
    out, idx, m = np.zeros((4097, 3), np.float32), np.zeros(4097, np.int32), C.c_size_t(0)
    assert lib.goicp_statistical_outlier_removal(reg.handle, xyz.ctypes.data_as(fp), 4097, 20, 1.0, out.ctypes.data_as(fp), None, None, None, C.byref(m)) == 0
    assert m.value == len(want) and ST.same_bits(out[:m.value], want)
    assert lib.goicp_statistical_outlier_removal(reg.handle, xyz.ctypes.data_as(fp), 4097, 20, 1.0, out.ctypes.data_as(fp), idx.ctypes.data_as(ip), None, None,
                                                 C.byref(m)) == 0
    assert np.array_equal(idx[:m.value], widx)


@functools.lru_cache(maxsize=None)
def _cluttered_bunny():
    bunny = source(2000)
    rng = np.random.default_rng(3)
    clutter = np.float32(rng.uniform(bunny.min(0), bunny.max(0), (100, 3)))
    order = rng.permutation(2100)
    xyz = np.ascontiguousarray(np.concatenate([bunny, clutter])[order], np.float32)
    xyz.setflags(write=False)
    return xyz, order < 2000


def test_bunny_with_box_clutter(pkg, reg):
    """2 000 bunny points and 5 % uniform clutter in their box, k = 20, alpha = 2: at least half of the clutter is dropped and at most 5 % of
    the surface points -- conditions on the twin; the device has to return the twin's set"""
    xyz, is_bunny = _cluttered_bunny()
    want = ST.twin(xyz, 20, 2.0)
    keep = np.zeros(len(xyz), bool)
    keep[want[1]] = True
    print("bunny dropped %.4f, clutter dropped %.4f" % ((~keep[is_bunny]).mean(), (~keep[~is_bunny]).mean()))
    assert (~keep[~is_bunny]).mean() >= 0.5 and (~keep[is_bunny]).mean() <= 0.05, ((~keep[is_bunny]).mean(), (~keep[~is_bunny]).mean())
    assert_device_equals_host(pkg, reg, xyz, 20, 2.0, "clutter", want)


# ----------------------------------------------------------------------------------------------
# the handle
# ----------------------------------------------------------------------------------------------
def test_statistical_outlier_removal_leaves_the_handle_untouched(pkg):
    a = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    b = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    try:
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), "before")
        a.statistical_outlier_removal(source(6000), 20, 2.0)
        a.statistical_outlier_removal(ST.make_cloud("identical", 300), 64, 0.0)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after two filters")
    finally:
        a.close(); b.close()


def _swap(lib, reg, raw, voxel, k, alpha, radius, min_neighbors, kept=None):
    from cuda_go_icp_amd import binding
    p = binding.CSourcePipeline(voxel, k, alpha, radius, min_neighbors)
    return lib.goicp_set_source_pipeline(reg.handle, raw.ctypes.data_as(C.POINTER(C.c_float)), len(raw), C.byref(p), None if kept is None else C.byref(kept))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_set_source_pipeline_equals_set_source_of_the_host_output(pkg, variant):
    """stat only (growth 500 -> most of 6 000), voxel + stat, voxel + stat + radius, then stat only on 2 000 (shrink); both handles were
    used before"""
    lib = pkg.load_library()
    a, b = _make(pkg, 500, variant), _make(pkg, 500, variant)
    try:
        fingerprint(pkg, a, register=False); fingerprint(pkg, b, register=False)
        for n, v, k, alpha, r, mn in ((6000, 0.0, 20, 2.0, 0.0, 0), (6000, 0.05, 8, 1.0, 0.0, 0), (6000, 0.05, 8, 1.0, 0.06, 5), (2000, 0.0, 5, 0.5, 0.0, 0)):
            D = composed(n, v, k, alpha, r, mn)
            kept = C.c_size_t(0)
            assert _swap(lib, a, source(n), v, k, alpha, r, mn, kept) == 0, lib.goicp_last_error()
            assert kept.value == len(D) and 1 < len(D) < (len(reduced(n, v)) if v else n)
            a.ns, a.pcs = len(D), D
            b.set_source(D)
            full = n == 6000 and v > 0 and r > 0
            assert_same(fingerprint(pkg, a, register=full), fingerprint(pkg, b, register=full), (variant, n, v, k, alpha, r, mn))
        # n_kept may be NULL, and the original order is D's
        assert _swap(lib, a, source(6000), 0.05, 8, 1.0, 0.06, 5) == 0
        D = composed(6000, 0.05, 8, 1.0, 0.06, 5)
        a.ns = len(D)
        assert ST.same_bits(a.transform_source(np.eye(3, dtype=np.float32), np.zeros(3, np.float32)) + np.float32(0), D + np.float32(0))
    finally:
        a.close(); b.close()


def test_statistical_stage_off_is_the_filtered_swap(pkg):
    lib = pkg.load_library()
    from cuda_go_icp_amd import binding
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        kept, kept_b = C.c_size_t(0), C.c_size_t(0)
        raw = source(6000)
        assert _swap(lib, a, raw, 0.05, 0, 7.0, 0.06, 5, kept) == 0, lib.goicp_last_error()          # std_ratio is not looked at without a k
        f = binding.CSourceFilter(0.05, 0.06, 5)
        assert lib.goicp_set_source_filtered(b.handle, raw.ctypes.data_as(C.POINTER(C.c_float)), 6000, C.byref(f), C.byref(kept_b)) == 0
        D = composed(6000, 0.05, 0, 0.0, 0.06, 5)
        assert kept.value == kept_b.value == len(D)
        a.ns = b.ns = len(D)
        a.pcs = b.pcs = D
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "stat off")
        raw = source(2000)
        assert _swap(lib, a, raw, 0.0, 0, 0.0, 0.0, -3, kept) == 0 and kept.value == 2000
        a.ns, a.pcs = 2000, raw
        b.set_source(raw)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "all off")
    finally:
        a.close(); b.close()


def test_refusals_leave_the_handle_as_it_was(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        good = source(2000)
        g = good.ctypes.data_as(fp)
        out, idx, u = np.full((2000, 3), -7, np.float32), np.full(2000, -7, np.int32), np.full(2000, -7, np.float32)
        thr, m = C.c_double(-7.0), C.c_size_t(99)
        o, i, d = out.ctypes.data_as(fp), idx.ctypes.data_as(ip), u.ctypes.data_as(fp)
        from cuda_go_icp_amd import binding

        def swap(x, n, k, alpha, v=0.0, r=0.0, mn=0):
            p = binding.CSourcePipeline(v, k, alpha, r, mn)
            return lib.goicp_set_source_pipeline(a.handle, x, n, C.byref(p), None)
        filt = lambda x, n, k, alpha: lib.goicp_statistical_outlier_removal(a.handle, x, n, k, alpha, o, i, d, C.byref(thr), C.byref(m))
        for call in (swap, filt):
            for bad_value in (np.nan, np.inf):
                bad = np.array(good)
                bad[1234, 2] = bad_value
                assert call(bad.ctypes.data_as(fp), 2000, 20, 2.0) == INVALID and b"non-finite" in lib.goicp_last_error()
            assert call(g, 0, 20, 2.0) == INVALID
            assert call(None, 2000, 20, 2.0) == INVALID
            assert call(g, (2 ** 31 - 1) // 8 + 1, 20, 2.0) == INVALID          # refused before a byte is read
            for k in (-1, 65, 2000):
                assert call(g, 2000, k, 2.0) == INVALID, k
            assert call(g, 20, 20, 2.0) == INVALID and b"n - 1" in lib.goicp_last_error()
            for alpha in (-1.0, float("nan"), float("inf")):
                assert call(g, 2000, 20, alpha) == INVALID and b"std_ratio" in lib.goicp_last_error(), alpha
        assert filt(g, 2000, 0, 2.0) == INVALID                                # k = 0 is "no stage" for the swap alone
        assert lib.goicp_set_source_pipeline(a.handle, g, 2000, None, None) == INVALID
        assert lib.goicp_statistical_outlier_removal(a.handle, g, 2000, 20, 2.0, None, i, d, C.byref(thr), C.byref(m)) == INVALID
        assert lib.goicp_statistical_outlier_removal(a.handle, g, 2000, 20, 2.0, o, i, d, C.byref(thr), None) == INVALID
        # what the stages refuse, behind one another: a bad voxel, k above the REDUCED cloud's size minus one, a bad radius stage, and a
        # radius stage that keeps nothing
        for v in (-0.05, float("nan"), float("inf"), 2.0 ** -22):
            assert swap(g, 2000, 20, 2.0, v) == INVALID, v
        n_red = len(reduced(2000, 0.3))
        assert 1 < n_red <= 64
        assert swap(g, 2000, n_red, 2.0, 0.3) == INVALID and b"n - 1" in lib.goicp_last_error()
        assert swap(g, 2000, 20, 2.0, 0.0, 0.05, 0) == INVALID and b"min_neighbors" in lib.goicp_last_error()
        assert swap(g, 2000, 20, 2.0, 0.0, 1e-30, 3) == INVALID
        assert swap(g, 2000, 20, 2.0, 0.0, 2.0 ** -17, 3) == INVALID and b"16 bits" in lib.goicp_last_error()
        assert swap(g, 2000, 20, 2.0, 0.0, 0.05, 2000) == INVALID and b"keeps no point" in lib.goicp_last_error()
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        assert swap(g, 2000, 20, 2.0) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert swap(g, 2000, 20, 2.0, 0.05) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert filt(g, 2000, 20, 2.0) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert np.all(out == -7) and np.all(idx == -7) and np.all(u == -7) and thr.value == -7.0 and m.value == 99
        assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0      # the same history without the refused calls
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the refusals")
        kept = C.c_size_t(0)
        assert _swap(lib, a, good, 0.0, 5, 0.5, 0.0, 0, kept) == 0 and kept.value == len(composed(2000, 0.0, 5, 0.5, 0.0, 0))    # and a good swap still works
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------------------------
# the other ways in
# ----------------------------------------------------------------------------------------------
def test_fastgoicp_set_source_pipeline(pkg):
    D = composed(6000, 0.05, 8, 1.0, 0.06, 5)
    eng = pkg.FastGoICP(target(), source(500), 1e-3, dt_size=DT)
    ref = pkg.FastGoICP(target(), D, 1e-3, dt_size=DT)
    try:
        with pytest.raises(ValueError):
            eng.set_source(source(6000), stat_neighbors=8)
        eng.set_source(source(6000), voxel=0.05, radius=0.06, min_neighbors=5, stat_neighbors=8, std_ratio=1.0)
        assert not eng.finished and eng.sse_threshold == ref.sse_threshold and eng.registration.ns == len(D) and ST.same_bits(eng.registration.pcs, D)
        eng.run(); ref.run()
        assert eng.get_best_error().tobytes() == ref.get_best_error().tobytes()
        assert eng.optR.tobytes() == ref.optR.tobytes() and eng.optT.tobytes() == ref.optT.tobytes()
        # stat only, through the Registration
        eng.registration.set_source(source(2000), stat_neighbors=5, std_ratio=0.5)
        assert eng.registration.ns == len(composed(2000, 0.0, 5, 0.5, 0.0, 0)) and ST.same_bits(eng.registration.pcs, composed(2000, 0.0, 5, 0.5, 0.0, 0))
    finally:
        eng.registration.close(); ref.registration.close()


def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_stat_outlier.cpp as a program: icp::FastGoICP::set_source(scan, pipeline) ends on the bits of a fresh engine created with
    the host functions' output (exit status 0)"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_stat")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_STAT_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_stat_outlier.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32"), "0.05", "8", "1.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "swapped" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_stat_with_source_list(pkg, tmp_path):
    """goicp_cli --stat-neighbors K --stat-std-ratio A --source-list: the config's source is filtered on the host, the listed cloud on the
    device inside its swap; the listed cloud's line and numbered outputs are those of a run of its own with the same flags (host filter,
    fresh engine), bit for bit"""
    K, A = 5, 1.0
    def write(name, pts):
        with open(tmp_path / (name + ".txt"), "w") as f:
            f.write("%d\n" % len(pts))
            for q in pts:
                f.write("%.9g %.9g %.9g\n" % tuple(q))
    write("model", cloud("model_rand"))
    write("scan0", cloud("data_rand")[:60])
    write("scan1", cloud("data_rand"))
    n1 = len(cloud("data_rand"))
    m0, m1 = len(pkg.statistical_outlier_removal(cloud("data_rand")[:60], K, A)[0]), len(pkg.statistical_outlier_removal(cloud("data_rand"), K, A)[0])
    assert 0 < m0 < 60 and 0 < m1 < n1
    cfg = ('[info]\ndescription = "stat source list"\n[io]\ntarget = "model.txt"\nsource = "%s.txt"\noutput = "%s"\nvisualization = "%s"\n'
           '[params]\nmode = 4\nsubsample = 1.0\nmse_threshold = 1e-3\nresize = 1.0\n')
    (tmp_path / "cfg.toml").write_text(cfg % ("scan0", tmp_path / "out.toml", tmp_path / "viz.ply"))
    (tmp_path / "own.toml").write_text(cfg % ("scan1", tmp_path / "own_out.toml", tmp_path / "own_viz.ply"))
    (tmp_path / "scans.lst").write_text("scan1.txt\n")
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    flags = ["--stat-neighbors", str(K), "--stat-std-ratio", str(A)]
    out = subprocess.run([exe, str(tmp_path / "cfg.toml")] + flags + ["--source-list", str(tmp_path / "scans.lst")], check=True, capture_output=True,
                         text=True, timeout=120).stdout
    own = subprocess.run([exe, str(tmp_path / "own.toml")] + flags, check=True, capture_output=True, text=True, timeout=120).stdout
    assert "source stat neighbors %d std ratio %g: kept %d of 60 points" % (K, A, m0) in out and "mode 4: source %d points" % m0 in out, out
    assert "source stat neighbors %d std ratio %g: kept %d of %d points" % (K, A, m1, n1) in own, own
    assert "source 1 stat neighbors %d std ratio %g: kept %d of %d points" % (K, A, m1, n1) in out, out
    line = [l for l in out.splitlines() if l.startswith("source 1 (")]
    assert len(line) == 1 and "%d points, swap " % m1 in line[0], out
    best_own = [l for l in own.splitlines() if l.startswith("Searching over!")][0].split("Best Error:")[1].split()[0]
    rot_own = [l for l in own.splitlines() if l.startswith("Total Rotation Nodes Searched")][0].split(":")[1].strip()
    assert "Best Error: %s," % best_own in line[0] and line[0].endswith("rotation nodes " + rot_own), (line[0], own)
    keep = lambda p: [l for l in (tmp_path / p).read_text().splitlines() if "_ms" not in l]      # the two wall-clock fields
    assert keep("out.1.toml") == keep("own_out.toml")
    assert np.array_equal(pkg.load_cloud(tmp_path / "viz.1.ply"), pkg.load_cloud(tmp_path / "own_viz.ply"))
    # --target-stat-*: the target is filtered on the host before the engine is created
    tv = subprocess.run([exe, str(tmp_path / "own.toml"), "--target-stat-neighbors", str(K), "--target-stat-std-ratio", str(A)], check=True,
                        capture_output=True, text=True, timeout=120).stdout
    mt = len(pkg.statistical_outlier_removal(cloud("model_rand"), K, A)[0])
    assert "target stat neighbors %d std ratio %g: kept %d of %d points" % (K, A, mt, len(cloud("model_rand"))) in tv and "target %d points" % mt in tv, tv
