"""goicp_cluster, goicp_cluster_filter and goicp_set_source_clustered on the device.

The device path (kdbuild.hip launch_cluster: the voxel operator's key kernel, rocPRIM radix sort, the radius filter's gather and count
kernel for the core flag, then cl_union_kernel -- a single-pass lock-free union-find --, cl_flatten_kernel, cl_border_kernel, the root
flags, rocPRIM scan and cl_label_kernel; launch_cluster_compact for the filter) against the host function, element for element, over the
cases of tests/cluster_twin.py: labels, sizes, kept cloud bits, indices and kept labels.

The chain (4 096 points on a line at spacing 0.9 r, shuffled) is one cluster.  The component kernel is the single-pass form: it runs
once, whatever the cloud, so there is no number of rounds to report or to bound; plain label propagation would need thousands.

goicp_set_source_clustered: handle A swaps to the raw cloud behind the chain, handle B swaps to the composition of the host functions
with goicp_set_source, and every answer of the C ABI must be the same BYTES (the fingerprint of tests/test_gpu_voxel_downsample.py).
goicp_cluster and goicp_cluster_filter leave the handle's fingerprint as it was, and so does every refused call."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cluster_twin as CT
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


@functools.lru_cache(maxsize=None)
def host_of(name, k):
    """the host function's answer for a case: computed once, shared, never changed"""
    xyz, r, _ = CT.cases()[name]
    labels, sizes = load_pkg().cluster(xyz, r, k)
    labels.setflags(write=False)
    sizes.setflags(write=False)
    return labels, sizes


# ----------------------------------------------------------------------------------------------
# the device operators against the host functions
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CT.cases()))
def test_device_equals_host(pkg, reg, name):
    xyz, r, ks = CT.cases()[name]
    for k in ks:
        want, wsizes = host_of(name, k)
        got, sizes = reg.cluster(xyz, r, k)
        assert np.array_equal(sizes, wsizes), (name, k, sizes[:8], wsizes[:8])
        assert np.array_equal(got, want), (name, k, int(np.sum(got != want)))


@pytest.mark.parametrize("name", CT.SELECT_CASES)
def test_device_filter_equals_host(pkg, reg, name):
    xyz, r, ks = CT.cases()[name]
    for k in ks:
        for min_size, keep in CT.SELECTIONS:
            want, widx, wlab = pkg.cluster_filter(xyz, r, k, min_size, keep)
            got, idx, lab = reg.cluster_filter(xyz, r, k, min_size, keep)
            assert np.array_equal(idx, widx) and np.array_equal(lab, wlab), (name, k, min_size, keep, len(idx), len(widx))
            assert CT.same_bits(got, want), (name, k, min_size, keep)


def test_chain_is_one_cluster_in_a_single_pass(pkg, reg):
    xyz, r, _ = CT.cases()["chain"]
    for k in (0, 2):
        labels, sizes = reg.cluster(xyz, r, k)
        assert sizes.tolist() == [4096] and not labels.any()
    labels, sizes = reg.cluster(xyz, r, 3)                       # nobody has three neighbours: all noise, c == 0
    assert len(sizes) == 0 and np.all(labels == -1)
    cloud, idx, lab = reg.cluster_filter(xyz, r, 3, 0, 0)        # and m == 0
    assert cloud.shape == (0, 3) and len(idx) == 0 and len(lab) == 0


def test_border_point_flips_with_one_ulp(pkg, reg):
    for name, tip in (("bridge_at", 8), ("bridge_below", 17), ("bridge_above", 8)):
        xyz, r, (k,) = CT.cases()[name]
        labels, sizes = reg.cluster(xyz, r, k)
        assert len(sizes) == 2 and labels[18] == labels[tip] and labels[8] != labels[17], (name, labels.tolist())


def test_two_runs_give_identical_bytes(pkg, reg):
    xyz, r, _ = CT.cases()["uniform1025_sparse"]
    for k in (0, 1, 3):
        a, b = reg.cluster(xyz, r, k), reg.cluster(xyz, r, k)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        fa, fb = reg.cluster_filter(xyz, r, k, 2, 5), reg.cluster_filter(xyz, r, k, 2, 5)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb))


def test_a_larger_cloud_with_dense_cells(pkg, reg):
    """20 000 points of the bunny scan and a blob of 2 000 beside it: some 80 tiles, cells of hundreds of points, several components"""
    xyz = scan_with_blob(20000, 2000)
    for r, k in ((0.04, 0), (0.03, 4)):
        want, wsizes = pkg.cluster(xyz, r, k)
        got, sizes = reg.cluster(xyz, r, k)
        assert np.array_equal(sizes, wsizes) and np.array_equal(got, want), (r, k, len(sizes), len(wsizes))
        assert len(sizes) >= 2


def test_null_outputs(pkg, reg):
    from cuda_go_icp_amd import binding as B
    lib = reg._lib
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz, r, _ = CT.cases()["uniform1025_sparse"]
    n = len(xyz)
    want, wsizes = host_of("uniform1025_sparse", 1)
    lab, c = np.zeros(n, np.int32), C.c_size_t(0)
    assert lib.goicp_cluster(reg.handle, xyz.ctypes.data_as(fp), n, r, 1, lab.ctypes.data_as(ip), None, C.byref(c)) == 0
    assert c.value == len(wsizes) and np.array_equal(lab, want)
    wf = pkg.cluster_filter(xyz, r, 1, 2, 3)
    out, m = np.zeros((n, 3), np.float32), C.c_size_t(0)
    s = B.CClusterSelect(r, 1, 2, 3)
    assert lib.goicp_cluster_filter(reg.handle, xyz.ctypes.data_as(fp), n, C.byref(s), out.ctypes.data_as(fp), None, None, C.byref(m)) == 0
    assert m.value == len(wf[0]) and CT.same_bits(out[:m.value], wf[0])


# ----------------------------------------------------------------------------------------------
# the handle
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_with_blob(n, nb):
    """source(n) (the bunny scan) with a dense foreign object: a ball of nb points beside the scan's box, shuffled in"""
    rng = np.random.default_rng(9)
    s = source(n)
    v = rng.normal(size=(nb, 3))
    ball = v / np.linalg.norm(v, axis=1)[:, None] * (0.1 * rng.uniform(0, 1, (nb, 1)) ** (1.0 / 3.0))
    ball += np.array([s[:, 0].max() + 0.4, s[:, 1].mean(), s[:, 2].mean()])
    out = np.ascontiguousarray(np.concatenate([s, ball])[rng.permutation(n + nb)], np.float32)
    out.setflags(write=False)
    return out


CLUSTER = (0.08, 2, 10, 1)                                       # radius, min_neighbors, min_size, keep: the largest cluster
STAGES = {
    "cluster_only": dict(),
    "all_stages": dict(voxel=0.03, stat_neighbors=8, std_ratio=2.0, radius=0.1, min_neighbors=3),
    "voxel_radius": dict(voxel=0.03, radius=0.1, min_neighbors=3),
}


@functools.lru_cache(maxsize=None)
def composed(stages):
    """the composition of the host functions for the scan with its blob: computed once, shared, never changed"""
    pkg = load_pkg()
    kw = STAGES[stages]
    d = scan_with_blob(3000, 300)
    if "voxel" in kw:
        d = pkg.voxel_downsample(d, kw["voxel"])[0]
    if "stat_neighbors" in kw:
        d = pkg.statistical_outlier_removal(d, kw["stat_neighbors"], kw["std_ratio"])[0]
    if "radius" in kw:
        d = pkg.radius_outlier_removal(d, kw["radius"], kw["min_neighbors"])[0]
    before = len(d)
    d = pkg.cluster_filter(d, *CLUSTER)[0]
    d.setflags(write=False)
    return d, before


def _swap(lib, handle, xyz, stages, cluster, kept=None):
    from cuda_go_icp_amd import binding as B
    kw = STAGES[stages]
    p = B.CSourcePipeline(kw.get("voxel", 0.0), kw.get("stat_neighbors", 0), kw.get("std_ratio", 0.0), kw.get("radius", 0.0), kw.get("min_neighbors", 0))
    s = B.CClusterSelect(*cluster)
    return lib.goicp_set_source_clustered(handle, xyz.ctypes.data_as(C.POINTER(C.c_float)), len(xyz), C.byref(p) if kw else None, C.byref(s),
                                          None if kept is None else C.byref(kept))


@pytest.mark.parametrize("stages", list(STAGES))
def test_set_source_clustered_equals_set_source_of_the_host_output(pkg, stages):
    lib = pkg.load_library()
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        fingerprint(pkg, a, register=False); fingerprint(pkg, b, register=False)
        D, before = composed(stages)
        assert 100 < len(D) < before                             # the blob (and what else is no part of the largest cluster) went
        kept = C.c_size_t(0)
        assert _swap(lib, a.handle, scan_with_blob(3000, 300), stages, CLUSTER, kept) == 0, lib.goicp_last_error()
        assert kept.value == len(D)
        a.ns, a.pcs = len(D), D
        b.set_source(D)
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), stages)
        # the Python form, and the original order is D's
        a.set_source(scan_with_blob(3000, 300), cluster_radius=CLUSTER[0], cluster_min_neighbors=CLUSTER[1], cluster_min_size=CLUSTER[2],
                     cluster_keep=CLUSTER[3], **STAGES[stages])
        assert a.ns == len(D) and CT.same_bits(a.pcs, D)
        assert CT.same_bits(a.transform_source(np.eye(3, dtype=np.float32), np.zeros(3, np.float32)) + np.float32(0), D + np.float32(0))
    finally:
        a.close(); b.close()


def test_no_cluster_stage_is_the_pipeline_swap(pkg):
    lib = pkg.load_library()
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        raw = scan_with_blob(3000, 300)
        kept = C.c_size_t(0)
        assert _swap(lib, a.handle, raw, "voxel_radius", (0.0, 0, 0, 0), kept) == 0, lib.goicp_last_error()
        b.set_source(raw, **STAGES["voxel_radius"])
        assert kept.value == b.ns
        a.ns, a.pcs = b.ns, b.pcs
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), "no cluster stage")
    finally:
        a.close(); b.close()


def test_operators_and_refusals_leave_the_handle_as_it_was(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        good = scan_with_blob(3000, 300)
        g, n = good.ctypes.data_as(fp), len(good)
        lab, siz, out, idx = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full((n, 3), -7, np.float32), np.full(n, -7, np.int32)
        c = C.c_size_t(99)
        L, S, O, X = lab.ctypes.data_as(ip), siz.ctypes.data_as(ip), out.ctypes.data_as(fp), idx.ctypes.data_as(ip)
        plain = lambda x, n_, r, k, ms=0, mc=0: lib.goicp_cluster(a.handle, x, n_, r, k, L, S, C.byref(c))
        filt = lambda x, n_, r, k, ms=0, mc=0: lib.goicp_cluster_filter(a.handle, x, n_, C.byref(B.CClusterSelect(r, k, ms, mc)), O, X, L, C.byref(c))
        swap = lambda x, n_, r, k, ms=0, mc=0: lib.goicp_set_source_clustered(a.handle, x, n_, None, C.byref(B.CClusterSelect(r, k, ms, mc)), None)
        for call in (plain, filt, swap):
            for bad_value in (np.nan, np.inf):
                bad = np.array(good)
                bad[1234, 2] = bad_value
                assert call(bad.ctypes.data_as(fp), n, 0.08, 1) == INVALID and b"non-finite" in lib.goicp_last_error()
            assert call(g, 0, 0.08, 1) == INVALID and call(None, n, 0.08, 1) == INVALID
            assert call(g, (2 ** 31 - 1) // 8 + 1, 0.08, 1) == INVALID
            for r in (-0.1, float("nan"), float("inf"), 1e-25, 1e25) + (() if call is swap else (0.0,)):   # 0 = no stage for the swap
                assert call(g, n, r, 1) == INVALID, r
            assert call(g, n, 1e-7, 1) == INVALID and b"16 bits" in lib.goicp_last_error()
            assert call(g, n, 0.08, -1) == INVALID and b"min_neighbors" in lib.goicp_last_error()
        for call in (filt, swap):
            assert call(g, n, 0.08, 1, -1, 0) == INVALID and b"min_size" in lib.goicp_last_error()
            assert call(g, n, 0.08, 1, 0, -1) == INVALID and b"max_clusters" in lib.goicp_last_error()
        # a selection that keeps nothing: refused for the swap (all noise; no cluster that large), a valid m == 0 for the operator
        assert swap(g, n, 0.08, 3300) == INVALID and b"keeps no point" in lib.goicp_last_error()
        assert swap(g, n, 0.08, 1, 10 ** 6, 0) == INVALID and b"keeps no point" in lib.goicp_last_error()
        # the pipeline's own refusals come through, and a chain that dies before the cluster stage
        bad_p = B.CSourcePipeline(0.0, 65, 1.0, 0.0, 0)
        assert lib.goicp_set_source_clustered(a.handle, g, n, C.byref(bad_p), C.byref(B.CClusterSelect(0.08, 1, 0, 0)), None) == INVALID
        assert lib.goicp_set_source_clustered(a.handle, g, n, None, None, None) == INVALID
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        for call in (plain, filt, swap):
            assert call(g, n, 0.08, 1) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert np.all(lab == -7) and np.all(siz == -7) and np.all(out == -7) and np.all(idx == -7) and c.value == 99
        # the operators themselves leave the handle alone
        a.cluster(good, 0.08, 2)
        a.cluster_filter(good, 0.08, 2, 10, 1)
        assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0      # the same history without the refused calls
        assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the operators and the refusals")
        kept = C.c_size_t(0)
        assert _swap(lib, a.handle, good, "cluster_only", CLUSTER, kept) == 0 and kept.value == len(composed("cluster_only")[0])   # a good swap still works
    finally:
        a.close(); b.close()


def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_cluster.cpp as a program: icp::Registration::cluster / cluster_filter agree with the host functions, and
    icp::FastGoICP::set_source(scan, nullptr, select) ends on the bits of a fresh engine created with the host function's output"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_cluster")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_CLUSTER_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_cluster.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32"), "0.08", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "operators agree" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_cluster_with_source_list(pkg, tmp_path):
    """goicp_cli --cluster-radius R --source-list: the config's source is filtered on the host, the listed cloud on the device inside its
    swap; the listed cloud's line and numbered outputs are those of a run of its own with the same options (host filter, fresh engine)"""
    R = 0.5
    def write(name, pts):
        with open(tmp_path / (name + ".txt"), "w") as f:
            f.write("%d\n" % len(pts))
            for q in pts:
                f.write("%.9g %.9g %.9g\n" % tuple(q))
    write("model", cloud("model_rand"))
    write("scan0", cloud("data_rand")[:60])
    write("scan1", cloud("data_rand"))
    m0, m1 = len(pkg.cluster_filter(cloud("data_rand")[:60], R, 0, 0, 1)[0]), len(pkg.cluster_filter(cloud("data_rand"), R, 0, 0, 1)[0])
    assert 0 < m0 < 60 and 0 < m1 < len(cloud("data_rand"))
    cfg = ('[info]\ndescription = "cluster source list"\n[io]\ntarget = "model.txt"\nsource = "%s.txt"\noutput = "%s"\nvisualization = "%s"\n'
           '[params]\nmode = 4\nsubsample = 1.0\nmse_threshold = 1e-3\nresize = 1.0\n')
    (tmp_path / "cfg.toml").write_text(cfg % ("scan0", tmp_path / "out.toml", tmp_path / "viz.ply"))
    (tmp_path / "own.toml").write_text(cfg % ("scan1", tmp_path / "own_out.toml", tmp_path / "own_viz.ply"))
    (tmp_path / "scans.lst").write_text("scan1.txt\n")
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    out = subprocess.run([exe, str(tmp_path / "cfg.toml"), "--cluster-radius", str(R), "--source-list", str(tmp_path / "scans.lst")], check=True,
                         capture_output=True, text=True, timeout=120).stdout
    own = subprocess.run([exe, str(tmp_path / "own.toml"), "--cluster-radius", str(R)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "source cluster radius %g min neighbors 0 min size 0 keep 1: kept %d of 60 points" % (R, m0) in out and "mode 4: source %d points" % m0 in out, out
    assert "source cluster radius %g min neighbors 0 min size 0 keep 1: kept %d of %d points" % (R, m1, len(cloud("data_rand"))) in own, own
    assert "source 1 cluster radius %g min neighbors 0 min size 0 keep 1: kept %d of %d points" % (R, m1, len(cloud("data_rand"))) in out, out
    line = [l for l in out.splitlines() if l.startswith("source 1 (")]
    assert len(line) == 1 and "%d points, swap " % m1 in line[0], out
    best_own = [l for l in own.splitlines() if l.startswith("Searching over!")][0].split("Best Error:")[1].split()[0]
    rot_own = [l for l in own.splitlines() if l.startswith("Total Rotation Nodes Searched")][0].split(":")[1].strip()
    assert "Best Error: %s," % best_own in line[0] and line[0].endswith("rotation nodes " + rot_own), (line[0], own)
    keep = lambda p: [l for l in (tmp_path / p).read_text().splitlines() if "_ms" not in l]      # the two wall-clock fields
    assert keep("out.1.toml") == keep("own_out.toml")
    assert np.array_equal(pkg.load_cloud(tmp_path / "viz.1.ply"), pkg.load_cloud(tmp_path / "own_viz.ply"))
    # --target-cluster-radius: the target is filtered on the host before the engine is created
    tv = subprocess.run([exe, str(tmp_path / "own.toml"), "--target-cluster-radius", str(R), "--target-cluster-keep", "2"], check=True, capture_output=True,
                        text=True, timeout=120).stdout
    mt = len(pkg.cluster_filter(cloud("model_rand"), R, 0, 0, 2)[0])
    assert "target cluster radius %g min neighbors 0 min size 0 keep 2: kept %d of %d points" % (R, mt, len(cloud("model_rand"))) in tv and "target %d points" % mt in tv, tv


def test_fastgoicp_set_source_clustered(pkg):
    f = pkg.FastGoICP(target(), source(500), 1e-3, dt_size=DT)
    try:
        D, _ = composed("cluster_only")
        f.set_source(scan_with_blob(3000, 300), cluster_radius=CLUSTER[0], cluster_min_neighbors=CLUSTER[1], cluster_min_size=CLUSTER[2], cluster_keep=CLUSTER[3])
        assert f.registration.ns == len(D) and CT.same_bits(f.registration.pcs, D)
    finally:
        f.registration.close()
