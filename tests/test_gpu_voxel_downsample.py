"""goicp_voxel_downsample and goicp_set_source_voxel on the device.

The device reduction (kdbuild.hip: key kernel, rocPRIM radix sort and scan, the wave-level segmented sum with 64-bit integer atomics at the
wave edges, the finishing kernel) against the host function, element for element and bit for bit, over the grid of
tests/test_voxel_downsample_host.py, and on clouds whose segments are placed to cut the kernel's edges: cells along x holding exactly
1, 63, 64, 65, 255, 256, 257, 1, 1 and 511 points (shuffled input), 70 001 points in one cell (1 094 waves add into one accumulator), and
70 001 points each alone.

goicp_set_source_voxel: handle A swaps to the raw cloud behind the grid, handle B swaps to the host function's output with
goicp_set_source, and every answer of the C ABI must be the same BYTES (the fingerprint of tests/test_gpu_set_source.py, copied here):
growth, shrink, morton_sort 0 / 1 / 2, and a handle with a gate and point-to-plane.  goicp_voxel_downsample leaves the handle's
fingerprint as it was, and so does every refused call."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import voxel_twin as VT
from conftest import ROOT, cloud, load_pkg

pytestmark = pytest.mark.gpu
INVALID = -1
DT = 48


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@functools.lru_cache(maxsize=None)
def target():
    t = cloud("model_bunny", 20)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def source(n):
    d = cloud("data_bunny")
    s = np.ascontiguousarray(d[np.linspace(0, len(d) - 1, n).astype(np.int64)])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def reduced(n, voxel):
    """the host function's output for source(n): computed once, shared, never changed"""
    d = load_pkg().voxel_downsample(source(n), voxel)[0]
    d.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def reg(pkg):
    r = pkg.Registration(target(), source(37), 1e-3, dt_size=DT)
    yield r
    r.close()


def _rot(v):
    load_pkg()
    from cuda_go_icp_amd import fgoicp
    return fgoicp.rodrigues(v)


@functools.lru_cache(maxsize=None)
def _cubes():
    rng = np.random.default_rng(5)
    c = np.concatenate([rng.uniform(-0.3, 0.3, (64, 3)), np.full((64, 1), 0.125)], 1).astype(np.float32)
    c.setflags(write=False)
    return c


def _try(pkg, fn):
    """the operator's answer, or the status it refused with: a refusal must be the same on both handles"""
    try:
        return fn()
    except pkg.GoicpError as e:
        return ("refused", getattr(e, "code", None) if getattr(e, "code", None) is not None else str(e)[:40])


def _poll_bytes(reg):
    r = reg.poll()
    cnt = tuple(getattr(r.counters, k) for k, _ in r.counters._fields_)
    return (bytes(bytearray(np.array(list(r.optR) + list(r.optT) + list(r.curR) + list(r.curT) + [r.best_sse], np.float32).tobytes())), int(r.finished), cnt)


def fingerprint(pkg, reg, register=True):
    """bounds, pose score, transform, thresholds, single and batched ICP, correspondences, pose information, one inner search, an ICP step
    and a whole registration, as bytes / ints, in a fixed order of calls (a copy of tests/test_gpu_set_source.py's)"""
    lib = reg._lib
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    R1, R2 = _rot([0.3, -0.2, 0.9]), _rot([-1.1, 0.4, 0.2])
    t1 = np.array([0.02, -0.03, 0.01], np.float32)
    out = {}
    thr, inl = C.c_float(), C.c_int32()
    assert lib.goicp_thresholds(reg.handle, C.byref(thr), C.byref(inl)) == 0
    out["thresholds"] = (np.float32(thr.value).tobytes(), inl.value)
    out["poll0"] = _poll_bytes(reg)
    for name, R, level in (("bounds_R1_fix", R1, -1), ("bounds_R2_fix", R2, -1), ("bounds_R1_l3", R1, 3)):
        ub, lb = reg.eval_bounds(R, _cubes(), level)
        out[name] = (ub.tobytes(), lb.tobytes())
    sse = C.c_float()
    assert lib.goicp_eval_sse(reg.handle, R1.ctypes.data_as(C.POINTER(C.c_float)), t1.ctypes.data_as(C.POINTER(C.c_float)), C.byref(sse)) == 0
    out["sse"] = np.float32(sse.value).tobytes()
    out["transform"] = reg.transform_source(R1, t1).tobytes()

    def icp():
        it = pkg.IterativeClosestPoint3D(reg, 40, 1e-7)
        err, R, t = it.run()
        return (np.float32(err).tobytes(), R.tobytes(), t.tobytes(), it.iters)
    out["icp_run"] = _try(pkg, icp)
    out["icp_inliers"] = _try(pkg, lambda: reg.icp_inliers(1).tobytes())

    def batch():
        Rs = np.stack([I, R1, _rot([0.05, 0.02, -0.04])])
        ts = np.stack([z, t1, z])
        R, t, err, it = reg.icp_run_batch(Rs, ts, 40, 1e-7)
        return (R.tobytes(), t.tobytes(), err.tobytes(), it.tobytes())
    out["icp_batch"] = _try(pkg, batch)

    def corr():
        idx, d2, n, s = reg.eval_correspondences(R1, t1, 0.05)
        return (idx.tobytes(), d2.tobytes(), n, np.float32(s).tobytes())
    out["correspondences"] = _try(pkg, corr)

    def info():
        d = reg.pose_information(I, z)
        return tuple(np.asarray(d[k]).tobytes() for k in sorted(d))
    out["pose_information"] = _try(pkg, info)

    def inner():
        v, node, cnt = reg.inner_bnb(R1, -1, 1e10)
        return (np.float32(v).tobytes(), None if node is None else node.tobytes(), cnt.trans_pops, cnt.cubes)
    out["inner_bnb"] = _try(pkg, inner)
    reg.icp_step()
    out["icp_step"] = _poll_bytes(reg)
    if register:
        assert lib.goicp_register(reg.handle) == 0, lib.goicp_last_error()
        out["register"] = _poll_bytes(reg)
        assert out["register"][1] == 1
        out["result_information"] = _try(pkg, lambda: tuple(np.asarray(v).tobytes() for _, v in sorted(reg.result_information().items())))
    return out


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], (tag, k)


def assert_device_equals_host(pkg, reg, xyz, v, tag):
    want, wcnt = pkg.voxel_downsample(xyz, v)
    got, cnt = reg.voxel_downsample(xyz, v)
    assert len(got) == len(want), (tag, len(got), len(want))
    assert np.array_equal(cnt, wcnt), tag
    assert VT.same_bits(got, want), (tag, int(np.sum(got.view(np.uint32) != want.view(np.uint32))))
    return got, cnt


# ----------------------------------------------------------------------------------------------
# the device reduction against the host function
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", VT.KINDS)
def test_device_equals_host_over_the_grid(pkg, reg, kind):
    for n in VT.SIZES:
        xyz = VT.make_cloud(kind, n)
        for v in VT.voxels_for(kind, xyz):
            assert_device_equals_host(pkg, reg, xyz, v, (kind, n, v))


def test_segments_cut_the_wave_edges(pkg, reg):
    """cells along x with exactly these sizes, in key order: sorted positions 0 | 1..63 | 64..127 | 128..192 | ... so segments end on, one
    before and one after a wave edge, span several waves, and three singletons sit between long ones"""
    sizes = [1, 63, 64, 65, 255, 256, 257, 1, 1, 511]
    rng = np.random.default_rng(11)
    pts = np.concatenate([np.stack([k + rng.uniform(0.05, 0.95, s), rng.uniform(0.05, 0.95, s), rng.uniform(0.05, 0.95, s)], 1) for k, s in enumerate(sizes)])
    pts[0] = 0.0                                         # the frame's minimum: cell k is [k, k + 1) along x
    xyz = np.ascontiguousarray(pts[rng.permutation(len(pts))], np.float32)
    got, cnt = assert_device_equals_host(pkg, reg, xyz, 1.0, "edges")
    assert cnt.tolist() == sizes
    want64 = np.array([pts[a:b].mean(0) for a, b in zip(np.cumsum([0] + sizes[:-1]), np.cumsum(sizes))])
    assert np.abs(got.astype(np.float64) - want64).max() <= VT.bound(xyz) + 2.0 ** -24 * 10     # pts were rounded to float32 once


def test_one_cell_of_70001_and_70001_alone(pkg, reg):
    n = 70001
    xyz = VT.make_cloud("uniform", n)
    ext = float(np.max(xyz.max(0) - xyz.min(0)))
    got, cnt = assert_device_equals_host(pkg, reg, xyz, ext * 4.0, "one cell")
    assert len(got) == 1 and cnt[0] == n
    assert np.abs(got[0].astype(np.float64) - xyz.astype(np.float64).mean(0)).max() <= VT.bound(xyz)
    got, cnt = assert_device_equals_host(pkg, reg, xyz, ext * 2.0 ** -20, "alone")
    assert len(got) == n and np.all(cnt == 1)
    # against the numpy twin as well, at a middling voxel on the same cloud
    want, wcnt, _, _ = VT.twin(xyz, ext / 37.0)
    got, cnt = reg.voxel_downsample(xyz, ext / 37.0)
    assert VT.same_bits(got, want) and np.array_equal(cnt, wcnt)


def test_out_count_may_be_null(pkg, reg):
    lib = reg._lib
    fp = C.POINTER(C.c_float)
    xyz = VT.make_cloud("duplicates", 4097)
    out, m = np.zeros((4097, 3), np.float32), C.c_size_t(0)
    assert lib.goicp_voxel_downsample(reg.handle, xyz.ctypes.data_as(fp), 4097, 0.3, out.ctypes.data_as(fp), None, C.byref(m)) == 0
    want = pkg.voxel_downsample(xyz, 0.3)[0]
    assert m.value == len(want) and VT.same_bits(out[:m.value], want)


# ----------------------------------------------------------------------------------------------
# the handle
# ----------------------------------------------------------------------------------------------
def test_voxel_downsample_leaves_the_handle_untouched(pkg):
    a = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    b = pkg.Registration(target(), source(500), 1e-3, dt_size=DT)
    try:
        # two handles with the same history; only a reduces clouds in between (a fingerprint moves the ICP step pose, so it is b that shows
        # what a must still answer)
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), "before")
        a.voxel_downsample(source(6000), 0.05)
        a.voxel_downsample(VT.make_cloud("identical", 300), 0.5)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after two reductions")
    finally:
        a.close(); b.close()


VARIANTS = {
    "default": (dict(), None),                           # morton_sort 2
    "morton0": (dict(morton_sort=0), None),
    "morton1": (dict(morton_sort=1), None),
    "plane_gate": (dict(), lambda r: (r.set_icp_options(1, 8), r.set_icp_gate(0.08))),
}


def _make(pkg, n, variant):
    kw, opts = VARIANTS[variant]
    r = pkg.Registration(target(), source(n), 1e-3, dt_size=DT, **kw)
    if opts:
        opts(r)
    return r


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_set_source_voxel_equals_set_source_of_the_host_output(pkg, variant):
    """growth 500 -> 1 459 cells of 6 000 raw points, then shrink to the 22 cells of 2 000 raw points; both handles were used before"""
    lib = pkg.load_library()
    fp = C.POINTER(C.c_float)
    a, b = _make(pkg, 500, variant), _make(pkg, 500, variant)
    try:
        fingerprint(pkg, a, register=False); fingerprint(pkg, b, register=False)
        for n, v in ((6000, 0.05), (2000, 0.5)):
            D = reduced(n, v)
            kept = C.c_size_t(0)
            raw = source(n)
            assert lib.goicp_set_source_voxel(a.handle, raw.ctypes.data_as(fp), n, v, C.byref(kept)) == 0, lib.goicp_last_error()
            assert kept.value == len(D) and 1 < len(D) < n
            a.ns, a.pcs = len(D), D
            b.set_source(D)
            assert_same(fingerprint(pkg, a), fingerprint(pkg, b), (variant, n, v))
        # n_kept may be NULL, and the original order is D's
        assert lib.goicp_set_source_voxel(a.handle, source(6000).ctypes.data_as(fp), 6000, 0.05, None) == 0
        a.ns = len(reduced(6000, 0.05))
        assert VT.same_bits(a.transform_source(np.eye(3, dtype=np.float32), np.zeros(3, np.float32)) + np.float32(0), reduced(6000, 0.05) + np.float32(0))
    finally:
        a.close(); b.close()


def test_refusals_leave_the_handle_as_it_was(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        good = source(2000)
        g = good.ctypes.data_as(fp)
        out, cnt, m = np.full((2000, 3), -7, np.float32), np.full(2000, -7, np.int32), C.c_size_t(99)
        o, c = out.ctypes.data_as(fp), cnt.ctypes.data_as(ip)
        swap = lambda x, n, v: lib.goicp_set_source_voxel(a.handle, x, n, v, None)
        down = lambda x, n, v: lib.goicp_voxel_downsample(a.handle, x, n, v, o, c, C.byref(m))
        for call in (swap, down):
            for bad_value in (np.nan, np.inf):
                bad = np.array(good)
                bad[1234, 2] = bad_value
                assert call(bad.ctypes.data_as(fp), 2000, 0.05) == INVALID and b"non-finite" in lib.goicp_last_error()
            assert call(g, 0, 0.05) == INVALID
            assert call(None, 2000, 0.05) == INVALID
            assert call(g, (2 ** 31 - 1) // 8 + 1, 0.05) == INVALID            # refused before a byte is read
            for v in (0.0, -0.05, float("nan"), float("inf")):
                assert call(g, 2000, v) == INVALID, v
            assert call(g, 2000, 2.0 ** -22) == INVALID and b"21 bits" in lib.goicp_last_error()
        unit = np.zeros((2, 3), np.float32)
        unit[1, 0] = 1.0                                                      # E = 1, v = 2^-22
        assert swap(unit.ctypes.data_as(fp), 2, 2.0 ** -22) == INVALID and down(unit.ctypes.data_as(fp), 2, 2.0 ** -22) == INVALID
        assert lib.goicp_voxel_downsample(a.handle, g, 2000, 0.05, None, c, C.byref(m)) == INVALID
        assert lib.goicp_voxel_downsample(a.handle, g, 2000, 0.05, o, c, None) == INVALID
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        assert swap(g, 2000, 0.05) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert down(g, 2000, 0.05) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert np.all(out == -7) and np.all(cnt == -7) and m.value == 99
        assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0      # the same history without the refused calls
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the refusals")
        kept = C.c_size_t(0)
        assert lib.goicp_set_source_voxel(a.handle, g, 2000, 0.05, C.byref(kept)) == 0                # and a good swap still works
        assert kept.value == len(reduced(2000, 0.05))
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------------------------
# the other ways in
# ----------------------------------------------------------------------------------------------
def test_fastgoicp_set_source_voxel(pkg):
    D = reduced(6000, 0.05)
    eng = pkg.FastGoICP(target(), source(500), 1e-3, dt_size=DT)
    ref = pkg.FastGoICP(target(), D, 1e-3, dt_size=DT)
    try:
        eng.run()
        assert eng.finished
        eng.set_source(source(6000), voxel=0.05)
        assert not eng.finished and np.array_equal(eng.optR, np.eye(3, dtype=np.float32)) and eng.get_best_error() == np.float32(1e10)
        assert eng.sse_threshold == ref.sse_threshold and eng.registration.ns == len(D) and VT.same_bits(eng.registration.pcs, D)
        eng.run(); ref.run()
        assert eng.get_best_error().tobytes() == ref.get_best_error().tobytes()
        assert eng.optR.tobytes() == ref.optR.tobytes() and eng.optT.tobytes() == ref.optT.tobytes()
        assert tuple(getattr(eng.counters, k) for k, _ in eng.counters._fields_) == tuple(getattr(ref.counters, k) for k, _ in ref.counters._fields_)
    finally:
        eng.registration.close(); ref.registration.close()


def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_voxel.cpp as a program: icp::FastGoICP::set_source(scan, voxel) ends on the bits of a fresh engine created with the host
    function's output (exit status 0)"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_voxel")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_VOXEL_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_voxel.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32"), "0.05"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "swapped" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_voxel_with_source_list(pkg, tmp_path):
    """goicp_cli --voxel V --source-list: the config's source is reduced on the host, the listed cloud on the device inside its swap; the
    listed cloud's line and numbered outputs are those of a run of its own with --voxel V (host reduction, fresh engine), bit for bit"""
    V = 0.3
    def write(name, pts):
        with open(tmp_path / (name + ".txt"), "w") as f:
            f.write("%d\n" % len(pts))
            for q in pts:
                f.write("%.9g %.9g %.9g\n" % tuple(q))
    write("model", cloud("model_rand"))
    write("scan0", cloud("data_rand")[:60])
    write("scan1", cloud("data_rand"))
    m0, m1 = len(pkg.voxel_downsample(cloud("data_rand")[:60], V)[0]), len(pkg.voxel_downsample(cloud("data_rand"), V)[0])
    assert m0 < 60 and m1 < len(cloud("data_rand"))
    cfg = ('[info]\ndescription = "voxel source list"\n[io]\ntarget = "model.txt"\nsource = "%s.txt"\noutput = "%s"\nvisualization = "%s"\n'
           '[params]\nmode = 4\nsubsample = 1.0\nmse_threshold = 1e-3\nresize = 1.0\n')
    (tmp_path / "cfg.toml").write_text(cfg % ("scan0", tmp_path / "out.toml", tmp_path / "viz.ply"))
    (tmp_path / "own.toml").write_text(cfg % ("scan1", tmp_path / "own_out.toml", tmp_path / "own_viz.ply"))
    (tmp_path / "scans.lst").write_text("scan1.txt\n")
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    out = subprocess.run([exe, str(tmp_path / "cfg.toml"), "--voxel", str(V), "--source-list", str(tmp_path / "scans.lst")], check=True, capture_output=True,
                         text=True, timeout=120).stdout
    own = subprocess.run([exe, str(tmp_path / "own.toml"), "--voxel", str(V)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "source voxel %g: %d of 60 points kept" % (V, m0) in out and "mode 4: source %d points" % m0 in out, out
    assert "source voxel %g: %d of %d points kept" % (V, m1, len(cloud("data_rand"))) in own, own
    line = [l for l in out.splitlines() if l.startswith("source 1 (")]
    assert len(line) == 1 and "%d points, swap " % m1 in line[0], out
    best_own = [l for l in own.splitlines() if l.startswith("Searching over!")][0].split("Best Error:")[1].split()[0]
    rot_own = [l for l in own.splitlines() if l.startswith("Total Rotation Nodes Searched")][0].split(":")[1].strip()
    assert "Best Error: %s," % best_own in line[0] and line[0].endswith("rotation nodes " + rot_own), (line[0], own)
    keep = lambda p: [l for l in (tmp_path / p).read_text().splitlines() if "_ms" not in l]      # the two wall-clock fields
    assert keep("out.1.toml") == keep("own_out.toml")
    assert np.array_equal(pkg.load_cloud(tmp_path / "viz.1.ply"), pkg.load_cloud(tmp_path / "own_viz.ply"))
    # --target-voxel: the target is reduced on the host before the engine is created
    tv = subprocess.run([exe, str(tmp_path / "own.toml"), "--target-voxel", str(V)], check=True, capture_output=True, text=True, timeout=120).stdout
    mt = len(pkg.voxel_downsample(cloud("model_rand"), V)[0])
    assert "target voxel %g: %d of %d points kept" % (V, mt, len(cloud("model_rand"))) in tv and "target %d points" % mt in tv, tv
