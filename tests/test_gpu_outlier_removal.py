"""goicp_radius_outlier_removal and goicp_set_source_filtered on the device.

The device filter (kdbuild.hip: the voxel operator's key kernel at pitch 1.03125 r, rocPRIM radix sort, the gather into sorted 16-byte
records, ror_count_kernel, rocPRIM scan, the compaction) against the host function, element for element, over the grid of
tests/test_outlier_removal_host.py, and on clouds placed to cut the count kernel's edges: sorted cells of exactly 1, 63, 64, 65, 255, 256,
257, 1, 1 and 511 points (shuffled input) with neighbours inside one cell only and across three cells, 20 001 identical points (a lane
has to scan up to 20 000 candidates, or none of them when it saturates at once), 70 001 points each alone, and points in cell 0 and in
the highest cell of every axis at the smallest radius the grid takes.

goicp_set_source_filtered: handle A swaps to the raw cloud behind the filters, handle B swaps to the composition of the host functions
with goicp_set_source, and every answer of the C ABI must be the same BYTES (the fingerprint of tests/test_gpu_voxel_downsample.py):
radius only, voxel and radius, growth and shrink, morton_sort 0 / 1 / 2, and a handle with a gate and point-to-plane; voxel only equals
goicp_set_source_voxel and both stages off goicp_set_source.  goicp_radius_outlier_removal leaves the handle's fingerprint as it was, and so
does every refused call, the filter that keeps nothing included."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import outlier_twin as OT
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
def cleaned(n, voxel, radius, k):
    """the composition of the host functions for source(n): computed once, shared, never changed"""
    pkg = load_pkg()
    d = reduced(n, voxel) if voxel else source(n)
    d = pkg.radius_outlier_removal(d, radius, k)[0]
    d.setflags(write=False)
    return d


def assert_device_equals_host(pkg, reg, xyz, r, k, tag, want=None):
    want, widx, wcnt = want if want is not None else pkg.radius_outlier_removal(xyz, r, k)
    got, idx, cnt = reg.radius_outlier_removal(xyz, r, k)
    assert len(got) == len(want), (tag, len(got), len(want))
    assert np.array_equal(idx, widx) and np.array_equal(cnt, wcnt), (tag, int(np.sum(cnt != wcnt)))
    assert OT.same_bits(got, want), tag
    return got, idx, cnt


# ----------------------------------------------------------------------------------------------
# the device filter against the host function
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", OT.KINDS)
def test_device_equals_host_over_the_grid(pkg, reg, kind):
    for n in OT.SIZES:
        xyz = OT.make_cloud(kind, n)
        taken = 0
        for r in OT.radii_for(kind, xyz):
            if not OT.valid(xyz, r):
                with pytest.raises(pkg.GoicpError):
                    reg.radius_outlier_removal(xyz, r, 1)
                continue
            taken += 1
            for k in OT.ks_for(n):
                assert_device_equals_host(pkg, reg, xyz, r, k, (kind, n, r, k))
        assert taken >= 1


def _cells_along_x(sizes, pitch, spread, stride, rng):
    """cell stride * k of a grid of that pitch holds exactly sizes[k] points, inside a cube of edge `spread` * pitch at the cell's centre"""
    lo, hi = 0.5 - spread / 2, 0.5 + spread / 2
    pts = np.concatenate([np.stack([stride * k + rng.uniform(lo, hi, s), rng.uniform(lo, hi, s), rng.uniform(lo, hi, s)], 1) * pitch for k, s in enumerate(sizes)])
    pts[0] = 0.0                                         # the frame's minimum: cell j is [j, j + 1) * pitch along x
    return pts


def test_spans_cut_the_wave_and_workgroup_edges(pkg, reg):
    """sorted positions 0 | 1..63 | 64..127 | 128..192 | ...: runs that end on, one before and one after a wave edge and a workgroup edge, span
    several workgroups, with three singletons between long ones.  First with every point's neighbours inside its own cell (cells two
    apart, points in the middle 40 % of each: any two of a cell are within r, the count is known), then with the cells adjacent and
    filled, so that the neighbours span three cells (against the twin)"""
    sizes = [1, 63, 64, 65, 255, 256, 257, 1, 1, 511]
    r = np.float32(1.0)
    pitch = float(r * np.float32(1.03125))
    rng = np.random.default_rng(11)
    pts = _cells_along_x(sizes, pitch, 0.4, 2, rng)
    order = rng.permutation(len(pts))
    xyz = np.ascontiguousarray(pts[order], np.float32)
    own = np.concatenate([np.full(s, s - 1) for s in sizes])[order]
    for k in (1, 5, 62, 64, 256, 510, 511):
        got, idx, cnt = assert_device_equals_host(pkg, reg, xyz, float(r), k, ("one cell", k))
        assert np.array_equal(cnt, np.minimum(own, k)), k
    pts = _cells_along_x(sizes, pitch, 0.98, 1, rng)
    xyz = np.ascontiguousarray(pts[rng.permutation(len(pts))], np.float32)
    counts = OT.neighbour_counts(xyz, r)
    cell = np.floor((xyz[:, 0] - xyz[:, 0].min()) / np.float32(pitch)).astype(int)
    assert np.bincount(cell).tolist() == sizes
    for k in (1, 5, 64, 200, int(counts.max())):
        assert_device_equals_host(pkg, reg, xyz, float(r), k, ("three cells", k), OT.twin(xyz, r, k, counts))


def test_dense_and_empty_extremes(pkg, reg):
    n = 20001
    xyz = OT.make_cloud("identical", n)
    for k in (5, n - 1):
        got, idx, cnt = reg.radius_outlier_removal(xyz, 1e-3, k)          # the answer is known: everybody has n - 1 neighbours
        assert len(got) == n and np.array_equal(idx, np.arange(n)) and np.all(cnt == k) and OT.same_bits(got, xyz), k
    got, idx, cnt = reg.radius_outlier_removal(xyz, 1e-3, n)
    assert len(got) == 0 and len(idx) == 0 and np.all(cnt == n - 1)
    n = 70001
    xyz = OT.make_cloud("uniform", n)
    got, idx, cnt = assert_device_equals_host(pkg, reg, xyz, float(OT.extent(xyz)) * 2.0 ** -15, 1, "alone")
    assert len(got) == 0 and not cnt.any()
    # and a middling radius on the same cloud: 275 workgroups, the candidate intervals of most of them overlap
    got, idx, cnt = assert_device_equals_host(pkg, reg, xyz, float(OT.extent(xyz)) / 37.0, 9, "middling")
    assert 0 < len(got) < n


def test_grid_faces(pkg, reg):
    """the "edge" cloud at the smallest radius its grid takes: cell 0 and cell 63 550 of every axis are occupied, and the pairs placed in
    them are found (against the twin)"""
    xyz = OT.make_cloud("edge", 4097)
    r = OT.smallest_radius(xyz)
    assert OT.valid(xyz, r) and not OT.valid(xyz, np.nextafter(r, np.float32(0)))
    assert int(np.floor(np.float32(1.0) / (r * np.float32(1.03125)))) > 60000
    want = OT.twin(xyz, r, 1)
    assert {0, 1, 2, 3, 4, 5} <= set(want[1].tolist())   # (0,0,0) twice and (h,0,0) in cell 0; (1,1,1) twice and (1-h,1-h,1-h) in the highest cell
    assert 1000 < len(want[1]) < 3100                    # half of the rest are pairs, the others alone
    assert_device_equals_host(pkg, reg, xyz, float(r), 1, "faces", want)
    with pytest.raises(pkg.GoicpError):
        reg.radius_outlier_removal(xyz, float(np.nextafter(r, np.float32(0))), 1)


def test_null_outputs(pkg, reg):
    lib = reg._lib
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = OT.make_cloud("duplicates", 4097)
    want, widx, wcnt = pkg.radius_outlier_removal(xyz, 0.05, 5)
    assert 0 < len(want) < 4097
    out, idx, m = np.zeros((4097, 3), np.float32), np.zeros(4097, np.int32), C.c_size_t(0)
    assert lib.goicp_radius_outlier_removal(reg.handle, xyz.ctypes.data_as(fp), 4097, 0.05, 5, out.ctypes.data_as(fp), None, None, C.byref(m)) == 0
    assert m.value == len(want) and OT.same_bits(out[:m.value], want)
    assert lib.goicp_radius_outlier_removal(reg.handle, xyz.ctypes.data_as(fp), 4097, 0.05, 5, out.ctypes.data_as(fp), idx.ctypes.data_as(ip), None, C.byref(m)) == 0
    assert np.array_equal(idx[:m.value], widx)


def test_bunny_with_box_clutter(pkg, reg):
    """6 000 bunny points and 5 % uniform clutter in their box, k = 4.  r is derived on the CPU from the bunny alone: the 99.3 % quantile
    of the distance to a bunny point's 4th neighbour.  That the rule then keeps 99 % of the bunny and drops 90 % of the clutter are
    conditions on the twin; the device has to return the twin's set"""
    bunny, k = source(6000), 4
    rng = np.random.default_rng(3)
    clutter = np.float32(rng.uniform(bunny.min(0), bunny.max(0), (300, 3)))
    order = rng.permutation(6300)
    xyz = np.ascontiguousarray(np.concatenate([bunny, clutter])[order], np.float32)
    is_bunny = order < 6000
    kth = np.concatenate([np.partition(((bunny[a:a + 500, None, :] - bunny[None, :, :]) ** 2).sum(2), k, axis=1)[:, k] for a in range(0, 6000, 500)])
    r = np.float32(np.sqrt(np.quantile(kth, 0.993)))
    want = OT.twin(xyz, r, k)
    keep = np.zeros(len(xyz), bool)
    keep[want[1]] = True
    print("r %.5f: bunny kept %.4f, clutter dropped %.4f" % (r, keep[is_bunny].mean(), (~keep[~is_bunny]).mean()))
    assert keep[is_bunny].mean() >= 0.99 and (~keep[~is_bunny]).mean() >= 0.90, (r, keep[is_bunny].mean(), (~keep[~is_bunny]).mean())
    assert_device_equals_host(pkg, reg, xyz, float(r), k, "clutter", want)


# ----------------------------------------------------------------------------------------------
# the handle
# ----------------------------------------------------------------------------------------------
def test_radius_outlier_removal_leaves_the_handle_untouched(pkg):
    a = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    b = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    try:
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), "before")
        a.radius_outlier_removal(source(6000), 0.03, 3)
        a.radius_outlier_removal(OT.make_cloud("identical", 300), 0.5, 300)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after two filters")
    finally:
        a.close(); b.close()


def _swap_filtered(lib, reg, raw, voxel, radius, k, kept=None):
    from cuda_go_icp_amd import binding
    f = binding.CSourceFilter(voxel, radius, k)
    return lib.goicp_set_source_filtered(reg.handle, raw.ctypes.data_as(C.POINTER(C.c_float)), len(raw), C.byref(f), None if kept is None else C.byref(kept))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_set_source_filtered_equals_set_source_of_the_host_output(pkg, variant):
    """growth 500 -> 5 221 of 6 000 raw points (radius only), then voxel and radius (6 000 -> 1 459 cells -> 1 006), then shrink to 205 of
    2 000 (radius only); both handles were used before"""
    lib = pkg.load_library()
    a, b = _make(pkg, 500, variant), _make(pkg, 500, variant)
    try:
        fingerprint(pkg, a, register=False); fingerprint(pkg, b, register=False)
        for n, v, r, k in ((6000, 0.0, 0.03, 3), (6000, 0.05, 0.06, 5), (2000, 0.0, 0.03, 5)):
            D = cleaned(n, v, r, k)
            kept = C.c_size_t(0)
            assert _swap_filtered(lib, a, source(n), v, r, k, kept) == 0, lib.goicp_last_error()
            assert kept.value == len(D) and 1 < len(D) < (len(reduced(n, v)) if v else n)
            a.ns, a.pcs = len(D), D
            b.set_source(D)
            assert_same(fingerprint(pkg, a, register=(n == 6000 and v > 0)), fingerprint(pkg, b, register=(n == 6000 and v > 0)), (variant, n, v, r, k))
        # n_kept may be NULL, and the original order is D's
        assert _swap_filtered(lib, a, source(6000), 0.05, 0.06, 5) == 0
        D = cleaned(6000, 0.05, 0.06, 5)
        a.ns = len(D)
        assert OT.same_bits(a.transform_source(np.eye(3, dtype=np.float32), np.zeros(3, np.float32)) + np.float32(0), D + np.float32(0))
    finally:
        a.close(); b.close()


def test_stages_off_are_the_existing_swaps(pkg):
    """voxel only is goicp_set_source_voxel, both stages off goicp_set_source (min_neighbors is not looked at without a radius)"""
    lib = pkg.load_library()
    fp = C.POINTER(C.c_float)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        kept = C.c_size_t(0)
        raw = source(6000)
        assert _swap_filtered(lib, a, raw, 0.05, 0.0, 0, kept) == 0, lib.goicp_last_error()
        assert lib.goicp_set_source_voxel(b.handle, raw.ctypes.data_as(fp), 6000, 0.05, None) == 0
        assert kept.value == len(reduced(6000, 0.05))
        a.ns = b.ns = kept.value
        a.pcs = b.pcs = reduced(6000, 0.05)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "voxel only")
        raw = source(2000)
        assert _swap_filtered(lib, a, raw, 0.0, 0.0, -3, kept) == 0, lib.goicp_last_error()
        assert kept.value == 2000
        a.ns, a.pcs = 2000, raw
        b.set_source(raw)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "both off")
    finally:
        a.close(); b.close()


def test_refusals_leave_the_handle_as_it_was(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        good = source(2000)
        g = good.ctypes.data_as(fp)
        out, idx, cnt, m = np.full((2000, 3), -7, np.float32), np.full(2000, -7, np.int32), np.full(2000, -7, np.int32), C.c_size_t(99)
        o, i, c = out.ctypes.data_as(fp), idx.ctypes.data_as(ip), cnt.ctypes.data_as(ip)
        from cuda_go_icp_amd import binding

        def swap(x, n, r, k, v=0.0):
            f = binding.CSourceFilter(v, r, k)
            return lib.goicp_set_source_filtered(a.handle, x, n, C.byref(f), None)
        filt = lambda x, n, r, k: lib.goicp_radius_outlier_removal(a.handle, x, n, r, k, o, i, c, C.byref(m))
        for call in (swap, filt):
            for bad_value in (np.nan, np.inf):
                bad = np.array(good)
                bad[1234, 2] = bad_value
                assert call(bad.ctypes.data_as(fp), 2000, 0.05, 3) == INVALID and b"non-finite" in lib.goicp_last_error()
            assert call(g, 0, 0.05, 3) == INVALID
            assert call(None, 2000, 0.05, 3) == INVALID
            assert call(g, (2 ** 31 - 1) // 8 + 1, 0.05, 3) == INVALID          # refused before a byte is read
            for r in (-0.05, float("nan"), float("inf"), 1e-30, 1e25):
                assert call(g, 2000, r, 3) == INVALID, r
            for k in (0, -1):
                assert call(g, 2000, 0.05, k) == INVALID and b"min_neighbors" in lib.goicp_last_error()
            assert call(g, 2000, 2.0 ** -17, 3) == INVALID and b"16 bits" in lib.goicp_last_error()
        assert filt(g, 2000, 0.0, 3) == INVALID                                # radius 0 is "no stage" for the swap alone
        assert lib.goicp_set_source_filtered(a.handle, g, 2000, None, None) == INVALID
        assert lib.goicp_radius_outlier_removal(a.handle, g, 2000, 0.05, 3, None, i, c, C.byref(m)) == INVALID
        assert lib.goicp_radius_outlier_removal(a.handle, g, 2000, 0.05, 3, o, i, c, None) == INVALID
        # what the stages refuse, behind one another: a bad voxel, and a radius too small for the REDUCED cloud's extent
        for v in (-0.05, float("nan"), float("inf"), 2.0 ** -22):
            assert swap(g, 2000, 0.05, 3, v) == INVALID, v
        assert swap(g, 2000, 2.0 ** -17, 3, 0.05) == INVALID and b"16 bits" in lib.goicp_last_error()
        assert swap(g, 2000, 0.05, 0, 0.05) == INVALID and b"min_neighbors" in lib.goicp_last_error()
        # a filter that keeps no point: alone (no point has 2 000 neighbours) and behind the voxel grid
        assert swap(g, 2000, 0.05, 2000) == INVALID and b"keeps no point" in lib.goicp_last_error()
        assert swap(g, 2000, 0.05, 2000, 0.05) == INVALID and b"keeps no point" in lib.goicp_last_error()
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        assert swap(g, 2000, 0.05, 3) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert swap(g, 2000, 0.05, 3, 0.05) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert filt(g, 2000, 0.05, 3) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert np.all(out == -7) and np.all(idx == -7) and np.all(cnt == -7) and m.value == 99
        assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0      # the same history without the refused calls
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the refusals")
        assert filt(g, 2000, 0.05, 2000) == 0 and m.value == 0                                        # m == 0 is a result of the filter itself
        kept = C.c_size_t(0)
        assert _swap_filtered(lib, a, good, 0.0, 0.03, 5, kept) == 0 and kept.value == len(cleaned(2000, 0.0, 0.03, 5))    # and a good swap still works
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------------------------
# the other ways in
# ----------------------------------------------------------------------------------------------
def test_fastgoicp_set_source_filtered(pkg):
    D = cleaned(6000, 0.05, 0.06, 5)
    eng = pkg.FastGoICP(target(), source(500), 1e-3, dt_size=DT)
    ref = pkg.FastGoICP(target(), D, 1e-3, dt_size=DT)
    try:
        eng.run()
        assert eng.finished
        with pytest.raises(ValueError):
            eng.set_source(source(6000), radius=0.06)
        eng.set_source(source(6000), voxel=0.05, radius=0.06, min_neighbors=5)
        assert not eng.finished and np.array_equal(eng.optR, np.eye(3, dtype=np.float32)) and eng.get_best_error() == np.float32(1e10)
        assert eng.sse_threshold == ref.sse_threshold and eng.registration.ns == len(D) and OT.same_bits(eng.registration.pcs, D)
        eng.run(); ref.run()
        assert eng.get_best_error().tobytes() == ref.get_best_error().tobytes()
        assert eng.optR.tobytes() == ref.optR.tobytes() and eng.optT.tobytes() == ref.optT.tobytes()
        assert tuple(getattr(eng.counters, k) for k, _ in eng.counters._fields_) == tuple(getattr(ref.counters, k) for k, _ in ref.counters._fields_)
        # radius only, through the Registration
        eng.registration.set_source(source(2000), radius=0.03, min_neighbors=5)
        assert eng.registration.ns == len(cleaned(2000, 0.0, 0.03, 5)) and OT.same_bits(eng.registration.pcs, cleaned(2000, 0.0, 0.03, 5))
    finally:
        eng.registration.close(); ref.registration.close()


def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_outlier.cpp as a program: icp::FastGoICP::set_source(scan, filter) ends on the bits of a fresh engine created with the
    host functions' output (exit status 0)"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_outlier")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_OUTLIER_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_outlier.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32"), "0.05", "0.06", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "swapped" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_outlier_with_source_list(pkg, tmp_path):
    """goicp_cli --outlier-radius R --outlier-min-neighbors K --source-list: the config's source is filtered on the host, the listed cloud
    on the device inside its swap; the listed cloud's line and numbered outputs are those of a run of its own with the same flags (host
    filter, fresh engine), bit for bit"""
    R, K = 0.3, 1
    def write(name, pts):
        with open(tmp_path / (name + ".txt"), "w") as f:
            f.write("%d\n" % len(pts))
            for q in pts:
                f.write("%.9g %.9g %.9g\n" % tuple(q))
    write("model", cloud("model_rand"))
    write("scan0", cloud("data_rand")[:60])
    write("scan1", cloud("data_rand"))
    m0, m1 = len(pkg.radius_outlier_removal(cloud("data_rand")[:60], R, K)[0]), len(pkg.radius_outlier_removal(cloud("data_rand"), R, K)[0])
    n1 = len(cloud("data_rand"))
    assert 0 < m0 < 60 and 0 < m1 < n1
    cfg = ('[info]\ndescription = "outlier source list"\n[io]\ntarget = "model.txt"\nsource = "%s.txt"\noutput = "%s"\nvisualization = "%s"\n'
           '[params]\nmode = 4\nsubsample = 1.0\nmse_threshold = 1e-3\nresize = 1.0\n')
    (tmp_path / "cfg.toml").write_text(cfg % ("scan0", tmp_path / "out.toml", tmp_path / "viz.ply"))
    (tmp_path / "own.toml").write_text(cfg % ("scan1", tmp_path / "own_out.toml", tmp_path / "own_viz.ply"))
    (tmp_path / "scans.lst").write_text("scan1.txt\n")
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    flags = ["--outlier-radius", str(R), "--outlier-min-neighbors", str(K)]
    out = subprocess.run([exe, str(tmp_path / "cfg.toml")] + flags + ["--source-list", str(tmp_path / "scans.lst")], check=True, capture_output=True,
                         text=True, timeout=120).stdout
    own = subprocess.run([exe, str(tmp_path / "own.toml")] + flags, check=True, capture_output=True, text=True, timeout=120).stdout
    assert "source outlier radius %g min neighbors %d: kept %d of 60 points" % (R, K, m0) in out and "mode 4: source %d points" % m0 in out, out
    assert "source outlier radius %g min neighbors %d: kept %d of %d points" % (R, K, m1, n1) in own, own
    assert "source 1 outlier radius %g min neighbors %d: kept %d of %d points" % (R, K, m1, n1) in out, out
    line = [l for l in out.splitlines() if l.startswith("source 1 (")]
    assert len(line) == 1 and "%d points, swap " % m1 in line[0], out
    best_own = [l for l in own.splitlines() if l.startswith("Searching over!")][0].split("Best Error:")[1].split()[0]
    rot_own = [l for l in own.splitlines() if l.startswith("Total Rotation Nodes Searched")][0].split(":")[1].strip()
    assert "Best Error: %s," % best_own in line[0] and line[0].endswith("rotation nodes " + rot_own), (line[0], own)
    keep = lambda p: [l for l in (tmp_path / p).read_text().splitlines() if "_ms" not in l]      # the two wall-clock fields
    assert keep("out.1.toml") == keep("own_out.toml")
    assert np.array_equal(pkg.load_cloud(tmp_path / "viz.1.ply"), pkg.load_cloud(tmp_path / "own_viz.ply"))
    # with --voxel in front of it, on the list as well: the chain on the device against the chain on the host
    V = 0.1
    both = subprocess.run([exe, str(tmp_path / "cfg.toml"), "--voxel", str(V)] + flags + ["--source-list", str(tmp_path / "scans.lst")], check=True,
                          capture_output=True, text=True, timeout=120).stdout
    red = pkg.voxel_downsample(cloud("data_rand"), V)[0]
    mb = len(pkg.radius_outlier_removal(red, R, K)[0])
    assert 0 < mb and "source 1 outlier radius %g min neighbors %d: kept %d of %d points" % (R, K, mb, n1) in both, both
    # --target-outlier-*: the target is filtered on the host before the engine is created
    tv = subprocess.run([exe, str(tmp_path / "own.toml"), "--target-outlier-radius", str(R), "--target-outlier-min-neighbors", str(K)], check=True,
                        capture_output=True, text=True, timeout=120).stdout
    mt = len(pkg.radius_outlier_removal(cloud("model_rand"), R, K)[0])
    assert "target outlier radius %g min neighbors %d: kept %d of %d points" % (R, K, mt, len(cloud("model_rand"))) in tv and "target %d points" % mt in tv, tv
