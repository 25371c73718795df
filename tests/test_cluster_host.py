"""goicp_cluster_host / goicp_cluster_filter_host: Euclidean / DBSCAN clustering on the host (no handle, no GPU) against the numpy twin of
its definition (tests/cluster_twin.py) -- labels, sizes, kept cloud, indices and kept labels bit for bit over the shared cases -- and what
the definition promises on named cases: the pair exactly at d2 == r2, one ulp beyond, duplicates, a border point that never joins two
clusters and flips with one ulp, equal sizes ranked by label, the chain.  Also here: the boundary (ABI version, struct sizes, the new
symbols) and every refusal that needs no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_twin as CT
from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_cluster_host", "goicp_cluster", "goicp_cluster_select_default", "goicp_cluster_filter_host", "goicp_cluster_filter",
       "goicp_set_source_clustered"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


@pytest.mark.parametrize("name", list(CT.cases()))
def test_library_equals_twin(pkg, name):
    xyz, r, ks = CT.cases()[name]
    for k in ks:
        want, wsizes = CT.twin_of(name, k)
        got, sizes = pkg.cluster(xyz, r, k)
        assert np.array_equal(sizes, wsizes), (name, k, sizes[:8], wsizes[:8])
        assert np.array_equal(got, want), (name, k, int(np.sum(got != want)))
        # the properties, on the library's output: labels dense, sizes their counts, clusters numbered by their first member that is core
        assert got.min() >= -1 and got.max() == len(sizes) - 1
        assert np.array_equal(np.bincount(got[got >= 0], minlength=len(sizes)), sizes)


@pytest.mark.parametrize("name", CT.SELECT_CASES)
def test_filter_equals_twin(pkg, name):
    xyz, r, ks = CT.cases()[name]
    for k in ks:
        labels, sizes = CT.twin_of(name, k)
        for min_size, keep in CT.SELECTIONS:
            want, widx, wlab = CT.select(xyz, labels, sizes, min_size, keep)
            got, idx, lab = pkg.cluster_filter(xyz, r, k, min_size, keep)
            assert np.array_equal(idx, widx) and np.array_equal(lab, wlab), (name, k, min_size, keep, len(idx), len(widx))
            assert CT.same_bits(got, want) and CT.same_bits(got, xyz[idx]), (name, k, min_size, keep)
            assert np.all(np.diff(idx) > 0)


def test_small_and_boundary_answers(pkg):
    one = CT.cases()["n1"][0]
    assert [a.tolist() for a in pkg.cluster(one, 0.5, 0)] == [[0], [1]]
    assert [a.tolist() for a in pkg.cluster(one, 0.5, 1)] == [[-1], []]
    at, beyond, dup = (CT.cases()[k][0] for k in ("n2_at_r2", "n2_one_ulp_beyond", "n2_duplicates"))
    assert [a.tolist() for a in pkg.cluster(at, 0.5, 1)] == [[0, 0], [2]]                 # d2 == r2 joins
    assert [a.tolist() for a in pkg.cluster(at, 0.5, 2)] == [[-1, -1], []]
    assert [a.tolist() for a in pkg.cluster(beyond, 0.5, 0)] == [[0, 1], [1, 1]]          # one ulp beyond: apart
    assert [a.tolist() for a in pkg.cluster(beyond, 0.5, 1)] == [[-1, -1], []]
    assert [a.tolist() for a in pkg.cluster(dup, 0.5, 1)] == [[0, 0], [2]]                # a duplicate is a neighbour
    # all noise: c == 0 and m == 0 are valid results
    cloud, idx, lab = pkg.cluster_filter(beyond, 0.5, 1, 0, 0)
    assert cloud.shape == (0, 3) and len(idx) == 0 and len(lab) == 0


def test_border_point_joins_one_cluster_and_flips_with_one_ulp(pkg):
    """tests/cluster_twin.py bridge(): b has index 8, a index 17, the bridging point P index 18"""
    for name, tip in (("bridge_at", 8), ("bridge_below", 17), ("bridge_above", 8)):
        xyz, r, (k,) = CT.cases()[name]
        labels, sizes = pkg.cluster(xyz, r, k)
        assert len(sizes) == 2 and labels[8] == 0 and labels[17] == 1, (name, labels.tolist())
        assert labels[18] == labels[tip] and sorted(sizes.tolist()) == [9, 10], (name, labels.tolist(), sizes.tolist())
        counts = pkg.radius_outlier_removal(xyz, r, k)[2]
        assert counts[18] < k and counts[8] == k and counts[17] == k             # P is no core point, the tips are


def test_equal_sizes_rank_by_label(pkg):
    xyz, r, _ = CT.cases()["equal_sizes"]
    labels, sizes = pkg.cluster(xyz, r, 0)
    assert sizes.tolist() == [50, 50]
    cloud, idx, lab = pkg.cluster_filter(xyz, r, 0, 0, 1)
    assert len(idx) == 50 and not lab.any() and np.array_equal(idx, np.flatnonzero(labels == 0))


def test_chain_is_one_cluster(pkg):
    xyz, r, _ = CT.cases()["chain"]
    for k in (0, 2):                                            # k = 2: the two end points are border points
        labels, sizes = pkg.cluster(xyz, r, k)
        assert sizes.tolist() == [4096] and not labels.any()
    assert pkg.cluster(xyz, r, 3)[1].tolist() == []


def test_permuted_input_gives_the_same_partition(pkg):
    xyz, r, _ = CT.cases()["uniform1025_sparse"]
    perm = np.random.default_rng(2).permutation(len(xyz))
    for k in (0, 1):                                            # k = 0, 1: no border point, whose key depends on the indices
        a, sa = pkg.cluster(xyz, r, k)
        b, sb = pkg.cluster(xyz[perm], r, k)
        assert sorted(sa.tolist()) == sorted(sb.tolist())
        pairs = set(zip(a[perm].tolist(), b.tolist()))
        assert len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))      # a bijection of the labels


def test_refusals_write_nothing(pkg):
    lib = pkg.load_library()
    from cuda_go_icp_amd import binding as B
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    good = CT.cases()["uniform257_dense"][0]
    g, n = good.ctypes.data_as(fp), len(good)
    lab, siz, out, idx = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full((n, 3), -7, np.float32), np.full(n, -7, np.int32)
    c = C.c_size_t(99)
    L, S, O, X = lab.ctypes.data_as(ip), siz.ctypes.data_as(ip), out.ctypes.data_as(fp), idx.ctypes.data_as(ip)

    def plain(x, n_, r, k):
        return lib.goicp_cluster_host(x, n_, r, k, L, S, C.byref(c))

    def filt(x, n_, r, k, min_size=0, keep=0):
        s = B.CClusterSelect(r, k, min_size, keep)
        return lib.goicp_cluster_filter_host(x, n_, C.byref(s), O, X, L, C.byref(c))

    for call in (plain, filt):
        for bad_value in (np.nan, np.inf):
            bad = np.array(good)
            bad[100, 1] = bad_value
            assert call(bad.ctypes.data_as(fp), n, 0.1, 1) == INVALID and b"non-finite" in lib.goicp_last_error()
        assert call(g, 0, 0.1, 1) == INVALID and call(None, n, 0.1, 1) == INVALID
        assert call(g, (2 ** 31 - 1) // 8 + 1, 0.1, 1) == INVALID
        for r in (0.0, -0.1, float("nan"), float("inf"), 1e-25, 1e25):
            assert call(g, n, r, 1) == INVALID, r
        assert call(g, n, 1e-6, 1) == INVALID and b"16 bits" in lib.goicp_last_error()
        assert call(g, n, 0.1, -1) == INVALID and b"min_neighbors" in lib.goicp_last_error()
        assert call(g, n, 0.1, 0) == 0                                          # 0 is legal here
        lab[:], siz[:], out[:], idx[:] = -7, -7, -7, -7
        c.value = 99
    assert filt(g, n, 0.1, 1, -1, 0) == INVALID and b"min_size" in lib.goicp_last_error()
    assert filt(g, n, 0.1, 1, 0, -1) == INVALID and b"max_clusters" in lib.goicp_last_error()
    assert lib.goicp_cluster_host(g, n, 0.1, 1, None, S, C.byref(c)) == INVALID and lib.goicp_cluster_host(g, n, 0.1, 1, L, S, None) == INVALID
    s = B.CClusterSelect(0.1, 1, 0, 0)
    assert lib.goicp_cluster_filter_host(g, n, None, O, X, L, C.byref(c)) == INVALID
    assert lib.goicp_cluster_filter_host(g, n, C.byref(s), None, X, L, C.byref(c)) == INVALID
    assert lib.goicp_cluster_filter_host(g, n, C.byref(s), O, X, L, None) == INVALID
    assert np.all(lab == -7) and np.all(siz == -7) and np.all(out == -7) and np.all(idx == -7) and c.value == 99
    # the optional outputs
    assert lib.goicp_cluster_host(g, n, 0.1, 1, L, None, C.byref(c)) == 0 and np.all(siz == -7)
    want = pkg.cluster_filter(good, 0.1, 1, 2, 3)
    assert lib.goicp_cluster_filter_host(g, n, C.byref(B.CClusterSelect(0.1, 1, 2, 3)), O, None, None, C.byref(c)) == 0
    assert c.value == len(want[0]) and CT.same_bits(out[:c.value], want[0]) and np.all(idx == -7)


def test_shim_call_sites_compile():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_cluster.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_refuses_bad_cluster_values_before_any_device(pkg, tmp_path):
    """every bad --cluster-* / --target-cluster-* value ends with status 2 and a line that names the option; the config named does not even
    exist, so nothing was loaded and no device was touched"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    cfg = str(tmp_path / "missing.toml")
    for pre in ("--cluster", "--target-cluster"):
        for args, word in (([pre + "-radius", "0"], "-radius"), ([pre + "-radius", "-0.1"], "-radius"), ([pre + "-radius", "nan"], "-radius"),
                           ([pre + "-radius", "inf"], "-radius"), ([pre + "-radius", "1e-25"], "-radius"), ([pre + "-radius", "0.1x"], "-radius"),
                           ([pre + "-radius"], "-radius"), ([pre + "-radius", "0.1", pre + "-min-neighbors", "-1"], "-min-neighbors"),
                           ([pre + "-radius", "0.1", pre + "-min-neighbors", "1.5"], "-min-neighbors"),
                           ([pre + "-radius", "0.1", pre + "-min-size", "-2"], "-min-size"), ([pre + "-radius", "0.1", pre + "-keep", "x"], "-keep"),
                           ([pre + "-keep", "1"], "-radius"), ([pre + "-min-neighbors", "3"], "-radius"), ([pre + "-min-size", "3"], "-radius")):
            r = subprocess.run([exe, cfg] + args, capture_output=True, text=True, timeout=60)
            assert r.returncode == 2 and (pre + word) in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
    r = subprocess.run([exe, cfg, "--cluster-radius", "0.1", "--cluster-keep", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--cluster" not in r.stderr and "cannot open" in r.stderr      # good values: the run gets as far as the missing config


def test_boundary(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    assert lib.goicp_abi_version() == 4
    assert C.sizeof(B.CClusterSelect) == 16 and C.sizeof(B.CSourcePipeline) == 20 and C.sizeof(B.CSourceFilter) == 12
    assert NEW <= set(B.SYMBOLS) and all(hasattr(lib, name) for name in NEW)
    s = B.CClusterSelect(1.0, 2, 3, 4)
    lib.goicp_cluster_select_default(C.byref(s))
    assert (s.radius, s.min_neighbors, s.min_size, s.max_clusters) == (0.0, 0, 0, 0)
    lib.goicp_cluster_select_default(None)
    assert callable(pkg.cluster) and callable(pkg.cluster_filter) and callable(pkg.Registration.cluster) and callable(pkg.Registration.cluster_filter)
