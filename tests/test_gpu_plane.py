"""goicp_segment_plane, goicp_plane_filter and goicp_set_source_segmented on the device.

The device path (kdbuild.hip launch_segment_plane: pl_hyp_kernel, pl_score_kernel -- points in registers, a tile of hypotheses in LDS,
ballot + popcount, one global atomic per hypothesis per workgroup --, pl_argmax_kernel, pl_moment_kernel, pl_label_kernel, the filters'
scan and compaction) against the host functions, element for element, over the cases of tests/plane_twin.py: labels, plane records as
bytes, kept cloud bits and indices.  The sizes 3 .. 1 025 and the iteration counts 1 .. 1 000 put the ends of the cloud and of the
hypotheses on, one before and one after a wave (64), the tile (256) and a workgroup's points (1 024).

goicp_set_source_segmented: handle A swaps to the raw cloud behind the chain, handle B swaps to the composition of the host functions
with goicp_set_source, and every answer of the C ABI must be the same BYTES (the fingerprint of tests/test_gpu_voxel_downsample.py).
goicp_segment_plane and goicp_plane_filter leave the handle's fingerprint as it was, and so does every refused call."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import plane_twin as PT
from conftest import ROOT, load_pkg
from test_gpu_cluster import scan_with_blob
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


def same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(PT.cases()))
def test_device_equals_host(pkg, reg, name):
    xyz, kw = PT.cases()[name]
    want, got = pkg.segment_plane(xyz, **kw), reg.segment_plane(xyz, **kw)
    assert same(got, want), (name, got[1], want[1], int(np.sum(got[0] != want[0])))
    wantf, gotf = pkg.plane_filter(xyz, **kw), reg.plane_filter(xyz, **kw)
    assert same(gotf, wantf), (name, len(gotf[0]), len(wantf[0]))


def test_two_runs_give_identical_bytes(pkg, reg):
    xyz, kw = PT.cases()["floor_wall_object_P2"]
    assert same(reg.segment_plane(xyz, **kw), reg.segment_plane(xyz, **kw))
    assert same(reg.plane_filter(xyz, **kw), reg.plane_filter(xyz, **kw))


@functools.lru_cache(maxsize=None)
def scan_on_floor(n, nf):
    """source(n) (the bunny scan) on a floor of nf points at its min y (noise sigma 0.004), shuffled"""
    rng = np.random.default_rng(21)
    s = source(n).astype(np.float64)
    lo, hi = s.min(0), s.max(0)
    floor = np.c_[rng.uniform(lo[0] - 0.3, hi[0] + 0.3, nf), lo[1] + rng.normal(0, 0.004, nf), rng.uniform(lo[2] - 0.3, hi[2] + 0.3, nf)]
    out = np.ascontiguousarray(np.concatenate([s, floor])[rng.permutation(n + nf)], np.float32)
    out.setflags(write=False)
    return out


def test_a_larger_cloud_with_many_workgroups(pkg, reg):
    """20 000 scan points + 8 000 floor points: 28 workgroups of points times two tiles of hypotheses, atomics between them, two rounds"""
    xyz = scan_on_floor(20000, 8000)
    kw = dict(distance=0.012, iterations=300, refine=1, max_planes=2, min_inliers=2000, seed=4)
    want, got = pkg.segment_plane(xyz, **kw), reg.segment_plane(xyz, **kw)
    assert same(got, want), (got[1], want[1])
    assert len(want[1]) >= 1 and want[1][0]["inliers"] >= 7000
    assert same(reg.plane_filter(xyz, **kw), pkg.plane_filter(xyz, **kw))


# ----------------------------------------------------------------------------------------------
# the handle
# ----------------------------------------------------------------------------------------------
PLANE = (0.015, 128, 1, 1, 0, 7)                                  # distance, iterations, refine, max_planes, min_inliers, seed
CLUSTER = (0.08, 2, 10, 1)
STAGES = {
    "plane_only": (dict(), False),
    "plane_cluster": (dict(), True),
    "all_stages": (dict(voxel=0.03, radius=0.1, min_neighbors=3), True),
}


@functools.lru_cache(maxsize=None)
def raw_cloud():
    """the scan with its blob (tests/test_gpu_cluster.py) on a floor"""
    rng = np.random.default_rng(22)
    s = scan_with_blob(3000, 300).astype(np.float64)
    lo, hi = s.min(0), s.max(0)
    floor = np.c_[rng.uniform(lo[0], hi[0], 1500), lo[1] + rng.normal(0, 0.004, 1500), rng.uniform(lo[2], hi[2], 1500)]
    out = np.ascontiguousarray(np.concatenate([s, floor])[rng.permutation(len(s) + 1500)], np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def composed(stages):
    """the composition of the host functions: computed once, shared, never changed"""
    pkg = load_pkg()
    kw, with_cluster = STAGES[stages]
    d = raw_cloud()
    if "voxel" in kw:
        d = pkg.voxel_downsample(d, kw["voxel"])[0]
    if "radius" in kw:
        d = pkg.radius_outlier_removal(d, kw["radius"], kw["min_neighbors"])[0]
    before = len(d)
    d = pkg.plane_filter(d, *PLANE)[0]
    after_plane = len(d)
    if with_cluster:
        d = pkg.cluster_filter(d, *CLUSTER)[0]
    d.setflags(write=False)
    return d, before, after_plane


def _swap(lib, handle, xyz, stages, plane, cluster, kept=None):
    from cuda_go_icp_amd import binding as B
    kw, with_cluster = STAGES[stages]
    p = B.CSourcePipeline(kw.get("voxel", 0.0), 0, 0.0, kw.get("radius", 0.0), kw.get("min_neighbors", 0))
    pl = None if plane is None else B.CPlaneSelect(*plane)
    s = B.CClusterSelect(*cluster) if with_cluster and cluster is not None else None
    return lib.goicp_set_source_segmented(handle, xyz.ctypes.data_as(C.POINTER(C.c_float)), len(xyz), C.byref(p) if kw else None,
                                          None if pl is None else C.byref(pl), None if s is None else C.byref(s), None if kept is None else C.byref(kept))


@pytest.mark.parametrize("stages", list(STAGES))
def test_set_source_segmented_equals_set_source_of_the_host_output(pkg, stages):
    lib = pkg.load_library()
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        fingerprint(pkg, a, register=False); fingerprint(pkg, b, register=False)
        D, before, after_plane = composed(stages)
        assert 100 < len(D) <= after_plane < before - 500          # the floor went
        kept = C.c_size_t(0)
        assert _swap(lib, a.handle, raw_cloud(), stages, PLANE, CLUSTER, kept) == 0, lib.goicp_last_error()
        assert kept.value == len(D)
        a.ns, a.pcs = len(D), D
        b.set_source(D)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), stages)
        # the Python form, and the original order is D's
        kw, with_cluster = STAGES[stages]
        ckw = dict(cluster_radius=CLUSTER[0], cluster_min_neighbors=CLUSTER[1], cluster_min_size=CLUSTER[2], cluster_keep=CLUSTER[3]) if with_cluster else {}
        a.set_source(raw_cloud(), plane_distance=PLANE[0], plane_iterations=PLANE[1], plane_refine=PLANE[2], plane_max=PLANE[3], plane_min_inliers=PLANE[4],
                     plane_seed=PLANE[5], **ckw, **kw)
        assert a.ns == len(D) and PT.same_bits(a.pcs, D)
        assert PT.same_bits(a.transform_source(np.eye(3, dtype=np.float32), np.zeros(3, np.float32)) + np.float32(0), D + np.float32(0))
    finally:
        a.close(); b.close()


def test_no_plane_stage_is_the_clustered_swap(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        raw = raw_cloud()
        kept, kept_b = C.c_size_t(0), C.c_size_t(0)
        for plane in (None, (0.0, 0, 0, 0, 0, 0)):
            assert _swap(lib, a.handle, raw, "all_stages", plane, CLUSTER, kept) == 0, lib.goicp_last_error()
        p = B.CSourcePipeline(0.03, 0, 0.0, 0.1, 3)
        for _ in range(2):
            assert lib.goicp_set_source_clustered(b.handle, raw.ctypes.data_as(C.POINTER(C.c_float)), len(raw), C.byref(p), C.byref(B.CClusterSelect(*CLUSTER)),
                                                  C.byref(kept_b)) == 0
        assert kept.value == kept_b.value
        D = pkg.cluster_filter(pkg.radius_outlier_removal(pkg.voxel_downsample(raw, 0.03)[0], 0.1, 3)[0], *CLUSTER)[0]
        a.ns = b.ns = len(D)
        a.pcs = b.pcs = D
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), "no plane stage")
    finally:
        a.close(); b.close()


def test_operators_and_refusals_leave_the_handle_as_it_was(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    fp, ip, pp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(B.CPlane)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        good = raw_cloud()
        g, n = good.ctypes.data_as(fp), len(good)
        lab, out, idx, planes = np.full(n, -7, np.int32), np.full((n, 3), -7, np.float32), np.full(n, -7, np.int32), np.full(80, -7, np.int32)
        c, m = C.c_size_t(99), C.c_size_t(99)
        L, O, X, P = lab.ctypes.data_as(ip), out.ctypes.data_as(fp), idx.ctypes.data_as(ip), planes.ctypes.data_as(pp)
        sel = lambda distance=0.015, iterations=64, refine=1, max_planes=1, min_inliers=0, seed=0: C.byref(
            B.CPlaneSelect(distance, iterations, refine, max_planes, min_inliers, seed))
        plain = lambda x, n_, **kw: lib.goicp_segment_plane(a.handle, x, n_, sel(**kw), L, P, C.byref(c))
        filt = lambda x, n_, **kw: lib.goicp_plane_filter(a.handle, x, n_, sel(**kw), O, X, P, C.byref(c), C.byref(m))
        swap = lambda x, n_, **kw: lib.goicp_set_source_segmented(a.handle, x, n_, None, sel(**kw), None, None)
        for call in (plain, filt, swap):
            for bad_value in (np.nan, np.inf):
                bad = np.array(good)
                bad[1234, 2] = bad_value
                assert call(bad.ctypes.data_as(fp), n) == INVALID and b"non-finite" in lib.goicp_last_error()
            assert call(g, 0) == INVALID and call(None, n) == INVALID
            assert call(g, (2 ** 31 - 1) // 8 + 1) == INVALID
            for d in (-0.1, float("nan")) + (() if call is swap else (0.0, float("inf"))):
                assert call(g, n, distance=d) == INVALID, d
            for kw in (dict(iterations=-1), dict(iterations=65537), dict(max_planes=-1), dict(max_planes=9), dict(min_inliers=-1), dict(refine=2)):
                assert call(g, n, **kw) == INVALID, kw
        assert swap(g, n, distance=float("inf")) == INVALID
        # a chain that keeps no point: refused for the swap, a valid m == 0 for the operator
        flat = np.ascontiguousarray(PT.exact_plane())
        assert lib.goicp_set_source_segmented(a.handle, flat.ctypes.data_as(fp), len(flat), None, sel(0.01), None, None) == INVALID
        assert b"keeps no point" in lib.goicp_last_error()
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        for call in (plain, filt, swap):
            assert call(g, n) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert np.all(lab == -7) and np.all(out == -7) and np.all(idx == -7) and np.all(planes == -7) and c.value == 99 and m.value == 99
        # the operators themselves leave the handle alone
        a.segment_plane(good, 0.015, 64)
        a.plane_filter(good, 0.015, 64, max_planes=2)
        assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0      # the same history without the refused calls
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the operators and the refusals")
        kept = C.c_size_t(0)
        assert _swap(lib, a.handle, good, "plane_only", PLANE, None, kept) == 0 and kept.value == len(composed("plane_only")[0])   # a good swap still works
    finally:
        a.close(); b.close()


def test_fastgoicp_set_source_segmented(pkg):
    f = pkg.FastGoICP(target(), source(500), 1e-3, dt_size=DT)
    try:
        D = composed("plane_cluster")[0]
        f.set_source(raw_cloud(), cluster_radius=CLUSTER[0], cluster_min_neighbors=CLUSTER[1], cluster_min_size=CLUSTER[2], cluster_keep=CLUSTER[3],
                     plane_distance=PLANE[0], plane_iterations=PLANE[1], plane_refine=PLANE[2], plane_max=PLANE[3], plane_min_inliers=PLANE[4], plane_seed=PLANE[5])
        assert f.registration.ns == len(D) and PT.same_bits(f.registration.pcs, D)
    finally:
        f.registration.close()


def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_plane.cpp as a program: icp::Registration::segment_plane / plane_filter agree with the host functions (labels, plane
    records as bytes, kept cloud, indices), and icp::FastGoICP::set_source(scan, nullptr, select, nullptr) ends on the bits of a fresh
    engine created with the host function's output"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_plane")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_PLANE_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_plane.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32"), "0.015", "128"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "operators agree" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_plane_with_source_list(pkg, tmp_path):
    """one goicp_cli run with --plane-distance, --cluster-radius and --source-list: the config's source loses its floor on the host
    (goicp_plane_filter_host), the listed cloud on the device inside its swap (goicp_set_source_segmented), the target on the host with
    the --target-plane-* forms; each prints the count the host functions give for the cloud as the CLI loads it"""
    def write(name, pts):
        with open(tmp_path / (name + ".txt"), "w") as f:
            f.write("%d\n" % len(pts))
            for q in pts:
                f.write("%.9g %.9g %.9g\n" % tuple(q))
    write("model", scan_on_floor(1500, 1500))
    write("scan0", raw_cloud()[::3])
    write("scan1", raw_cloud())
    loaded = [pkg.load_cloud(tmp_path / (n + ".txt")) for n in ("scan0", "scan1", "model")]
    assert PT.same_bits(loaded[1], raw_cloud())
    after_plane = [pkg.plane_filter(c, *PLANE)[0] for c in loaded[:2]]
    m = [len(pkg.cluster_filter(c, *CLUSTER)[0]) for c in after_plane]
    mt = len(pkg.plane_filter(loaded[2], 0.012, 128, 0, 1, 0, 3)[0])
    assert 0 < m[0] <= len(after_plane[0]) < len(loaded[0]) - 300 and m[1] == len(composed("plane_cluster")[0]) and 1300 < mt < 1520
    (tmp_path / "cfg.toml").write_text('[info]\ndescription = "plane source list"\n[io]\ntarget = "model.txt"\nsource = "scan0.txt"\n'
                                       '[params]\nmode = 1\nsubsample = 1.0\nmse_threshold = 1e-3\nresize = 1.0\n')
    (tmp_path / "scans.lst").write_text("scan1.txt\n")
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "cfg.toml"), "--iters", "3", "--plane-distance", str(PLANE[0]), "--plane-iterations", str(PLANE[1]), "--plane-seed",
                        str(PLANE[5]), "--cluster-radius", str(CLUSTER[0]), "--cluster-min-neighbors", str(CLUSTER[1]), "--cluster-min-size", str(CLUSTER[2]),
                        "--target-plane-distance", "0.012", "--target-plane-iterations", "128", "--target-plane-seed", "3", "--target-plane-no-refine",
                        "--source-list", str(tmp_path / "scans.lst")], capture_output=True, text=True, timeout=120)
    out = r.stdout
    assert r.returncode == 0, (r.returncode, out, r.stderr)
    head = "plane distance %g iterations %d max 0 min inliers 0 refine 1: " % (PLANE[0], PLANE[1])
    assert "source " + head + "1 planes, kept %d of %d points" % (len(after_plane[0]), len(loaded[0])) in out, out
    assert "target plane distance 0.012 iterations 128 max 0 min inliers 0 refine 0: 1 planes, kept %d of %d points" % (mt, len(loaded[2])) in out, out
    assert "mode 1: source %d points, target %d points" % (m[0], mt) in out, out
    assert "source 1 " + head + "kept %d of %d points" % (m[1], len(loaded[1])) in out, out
    line = [l for l in out.splitlines() if l.startswith("source 1 (")]
    assert len(line) == 1 and "%d points, swap " % m[1] in line[0], out
