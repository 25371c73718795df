"""goicp_statistical_outlier_removal_host: the statistical outlier removal operator on the host (no handle, no GPU) against the numpy twin of
its definition (tests/stat_outlier_twin.py) -- kept cloud, indices, mean distances and threshold bit for bit over the grid of sizes, cloud
kinds, k and std_ratio -- the properties the definition promises (at least one point is kept, indices ascend, kept points carry the
input's bits, a permuted input permutes the mean distances, U == 0 keeps everything), the agreement of its decisions with the textbook
form in float64 outside a band around the threshold, every refusal, the boundary (header, nm, binding, ABI version, struct sizes), and the
stand-alone selftest under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stat_outlier_twin as ST
from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_statistical_outlier_removal_host", "goicp_statistical_outlier_removal", "goicp_source_pipeline_default", "goicp_set_source_pipeline"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


@pytest.mark.parametrize("kind", ST.KINDS)
@pytest.mark.parametrize("n", ST.SIZES)
def test_library_equals_twin_and_properties(pkg, kind, n):
    xyz = ST.make_cloud(kind, n)
    nearest = ST.nearest_of(kind, n)
    perm = np.random.default_rng(n).permutation(n)
    for k in ST.ks_for(n):
        for alpha in ST.ALPHAS:
            want, widx, wu, wthr = ST.twin(xyz, k, alpha, nearest)
            got, idx, u, thr = pkg.statistical_outlier_removal(xyz, k, alpha)
            assert ST.same_bits(u, wu), (kind, n, k, alpha, int(np.sum(u.view(np.uint32) != wu.view(np.uint32))))
            assert np.float64(thr).tobytes() == np.float64(wthr).tobytes(), (kind, n, k, alpha, thr, wthr)
            assert np.array_equal(idx, widx), (kind, n, k, alpha, len(idx), len(widx))
            assert ST.same_bits(got, want), (kind, n, k, alpha)
            # the properties, on the library's output
            assert len(got) >= 1 and np.all(np.diff(idx) > 0) and ST.same_bits(got, xyz[idx])
            assert int(np.argmin(u)) in set(idx.tolist())
            if u.max() == 0:
                assert len(got) == n and thr == 0.0
            else:
                assert np.all(u[idx] <= np.float64(thr) + np.float64(u.max()) * 2.0 ** -30)
        got2, idx2, u2, thr2 = pkg.statistical_outlier_removal(xyz[perm], k, 1.0)
        got1, idx1, u1, thr1 = pkg.statistical_outlier_removal(xyz, k, 1.0)
        assert ST.same_bits(u2, u1[perm]) and thr2 == thr1, (kind, n, k)
        assert np.array_equal(np.sort(perm[idx2]), idx1) and ST.same_bits(got2, xyz[perm][idx2]), (kind, n, k)


@pytest.mark.parametrize("kind", ["identical", "denormal"])
def test_a_cloud_without_distances_keeps_everything(pkg, kind):
    """every d2 is 0 (the denormal cloud's squares underflow): u == 0, every point is kept, the threshold is 0"""
    for n in (2, 65, 1000):
        xyz = ST.make_cloud(kind, n)
        for k in ST.ks_for(n):
            got, idx, u, thr = pkg.statistical_outlier_removal(xyz, k, 0.0)
            assert len(got) == n and np.array_equal(idx, np.arange(n)) and not u.any() and thr == 0.0 and ST.same_bits(got, xyz)


@pytest.mark.parametrize("kind", ST.TEXTBOOK_KINDS)
def test_decisions_agree_with_the_textbook_form(pkg, kind):
    """the mean of the k smallest float64 distances and T = mu + alpha sigma (ddof = 1): the library's keep set is the textbook's for
    every point outside the band |m_i - T| <= 2^-18 max m, and at most 1 % of a case's points lie inside the band"""
    for n in (65, 255, 256, 257, 1000, 4097):
        xyz = ST.make_cloud(kind, n)
        nearest = ST.textbook_nearest(xyz, min(64, n - 1))
        for k in (1, 5, 20, 64):
            if k > n - 1:
                continue
            for alpha in ST.ALPHAS:
                m, T = ST.textbook(nearest, k, alpha)
                idx = pkg.statistical_outlier_removal(xyz, k, alpha)[1]
                keep = np.zeros(n, bool)
                keep[idx] = True
                band = np.abs(m - T) <= 2.0 ** -18 * m.max()
                wrong = int(np.sum((keep != (m <= T)) & ~band))
                print("%s n %d k %d alpha %g: %d in the band, %d disagreements outside" % (kind, n, k, alpha, int(band.sum()), wrong))
                assert wrong == 0, (kind, n, k, alpha, wrong)
                assert band.sum() <= 0.01 * n, (kind, n, k, alpha, int(band.sum()))


def test_null_outputs(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = ST.make_cloud("uniform", 257)
    want, widx, wu, wthr = pkg.statistical_outlier_removal(xyz, 5, 1.0)
    assert 0 < len(want) < 257
    host = lib.goicp_statistical_outlier_removal_host
    out, idx, u, thr, m = np.zeros((257, 3), np.float32), np.zeros(257, np.int32), np.zeros(257, np.float32), C.c_double(-1), C.c_size_t(0)
    assert host(xyz.ctypes.data_as(fp), 257, 5, 1.0, out.ctypes.data_as(fp), None, None, None, C.byref(m)) == 0
    assert m.value == len(want) and ST.same_bits(out[:m.value], want)
    assert host(xyz.ctypes.data_as(fp), 257, 5, 1.0, out.ctypes.data_as(fp), idx.ctypes.data_as(ip), None, None, C.byref(m)) == 0
    assert np.array_equal(idx[:m.value], widx)
    assert host(xyz.ctypes.data_as(fp), 257, 5, 1.0, out.ctypes.data_as(fp), None, u.ctypes.data_as(fp), C.byref(thr), C.byref(m)) == 0
    assert ST.same_bits(u, wu) and thr.value == wthr


def test_refusals_without_a_device(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = ST.make_cloud("uniform", 16)
    out, idx, u = np.full((16, 3), -7, np.float32), np.full(16, -7, np.int32), np.full(16, -7, np.float32)
    thr, m = C.c_double(-7.0), C.c_size_t(99)
    x, o, i, d = xyz.ctypes.data_as(fp), out.ctypes.data_as(fp), idx.ctypes.data_as(ip), u.ctypes.data_as(fp)
    host = lib.goicp_statistical_outlier_removal_host
    assert host(None, 16, 3, 1.0, o, i, d, C.byref(thr), C.byref(m)) == INVALID
    assert host(x, 16, 3, 1.0, None, i, d, C.byref(thr), C.byref(m)) == INVALID
    assert host(x, 16, 3, 1.0, o, i, d, C.byref(thr), None) == INVALID
    assert host(x, 0, 3, 1.0, o, i, d, C.byref(thr), C.byref(m)) == INVALID
    assert host(x, (2 ** 31 - 1) // 8 + 1, 3, 1.0, o, i, d, C.byref(thr), C.byref(m)) == INVALID   # goicp_create's limit, refused before anything is read
    for k in (0, -1, -2 ** 31, 65, 1000):
        assert host(x, 16, k, 1.0, o, i, d, C.byref(thr), C.byref(m)) == INVALID and b"neighbors" in lib.goicp_last_error(), k
    assert host(x, 16, 16, 1.0, o, i, d, C.byref(thr), C.byref(m)) == INVALID and b"n - 1" in lib.goicp_last_error()
    assert host(x, 1, 1, 1.0, o, i, d, C.byref(thr), C.byref(m)) == INVALID
    for a in (-0.5, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert host(x, 16, 3, a, o, i, d, C.byref(thr), C.byref(m)) == INVALID and b"std_ratio" in lib.goicp_last_error(), a
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[7, 1] = bad_value
        assert host(bad.ctypes.data_as(fp), 16, 3, 1.0, o, i, d, C.byref(thr), C.byref(m)) == INVALID and b"non-finite" in lib.goicp_last_error()
    assert np.all(out == -7) and np.all(idx == -7) and np.all(u == -7) and thr.value == -7.0 and m.value == 99
    # nothing about the extent is refused: a cloud spread over 2^40 times its closest pair, k = n - 1, and alpha == 0
    wide = np.zeros((16, 3), np.float32)
    wide[1:, 0] = np.float32(2.0) ** np.arange(-20, 25, 3)[:15]
    assert host(wide.ctypes.data_as(fp), 16, 15, 0.0, o, i, d, C.byref(thr), C.byref(m)) == 0 and 1 <= m.value <= 16
    # the handle-taking forms refuse a NULL handle before anything else
    from cuda_go_icp_amd import binding
    p = binding.CSourcePipeline(0.0, 3, 1.0, 0.0, 0)
    assert lib.goicp_statistical_outlier_removal(None, x, 16, 3, 1.0, o, i, d, C.byref(thr), C.byref(m)) == INVALID
    assert lib.goicp_set_source_pipeline(None, x, 16, C.byref(p), None) == INVALID


def test_header_nm_and_binding_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    args = r"const float\* xyz, size_t n, int32_t neighbors, float std_ratio, float\* out_xyz, int32_t\* out_index, float\* out_mean_dist, double\* threshold, size_t\* m\);"
    for decl in (r"int goicp_statistical_outlier_removal_host\(" + args, r"int goicp_statistical_outlier_removal\(goicp_handle h, " + args,
                 r"typedef struct goicp_source_pipeline \{ float voxel; int32_t stat_neighbors; float stat_std_ratio; float radius; int32_t min_neighbors; \} goicp_source_pipeline;",
                 r"void goicp_source_pipeline_default\(goicp_source_pipeline\* out\);",
                 r"int goicp_set_source_pipeline\(goicp_handle h, const float\* xyz, size_t n, const goicp_source_pipeline\* p, size_t\* n_kept\);",
                 r"#define GOICP_STAT_MAX_NEIGHBORS 64\b"):
        assert re.search(decl, hdr), decl
    assert re.search(r"#define GOICP_ABI_VERSION 4\b", hdr)
    from cuda_go_icp_amd import binding
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("goicp_") and " T " in l}
    assert NEW <= exported and NEW <= set(binding.SYMBOLS)
    lib = pkg.load_library()
    assert lib.goicp_abi_version() == 4
    fp, ip, sp, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.POINTER(C.c_double)
    assert lib.goicp_statistical_outlier_removal_host.argtypes == [fp, C.c_size_t, C.c_int32, C.c_float, fp, ip, fp, dp, sp]
    assert lib.goicp_statistical_outlier_removal.argtypes == [C.c_void_p, fp, C.c_size_t, C.c_int32, C.c_float, fp, ip, fp, dp, sp]
    assert lib.goicp_set_source_pipeline.argtypes == [C.c_void_p, fp, C.c_size_t, C.POINTER(binding.CSourcePipeline), sp]
    # the new struct, its defaults, and the sizes the ABI had before
    assert C.sizeof(binding.CSourcePipeline) == 20
    p = binding.CSourcePipeline(1.0, 2, 3.0, 4.0, 5)
    lib.goicp_source_pipeline_default(C.byref(p))
    assert (p.voxel, p.stat_neighbors, p.stat_std_ratio, p.radius, p.min_neighbors) == (0.0, 0, 0.0, 0.0, 0)
    assert C.sizeof(binding.CSourceFilter) == 12 and C.sizeof(binding.CCube) == 24 and C.sizeof(binding.CCounters) == 80
    assert callable(pkg.statistical_outlier_removal) and hasattr(pkg.Registration, "statistical_outlier_removal")
    shim = open(os.path.join(ROOT, "include", "goicp_mi355.hpp")).read()
    assert "goicp_set_source_pipeline(h_" in shim


def test_shim_stat_outlier_call_sites_compile():
    """tests/shim_stat_outlier.cpp, compiled as tests/shim_outlier.cpp is: syntax only"""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_stat_outlier.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_stat_refusals_before_any_device(pkg, tmp_path):
    """exit status 2 with the reason; the config named does not exist, so a run that got as far as loading it would end with status 1"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    cfg = str(tmp_path / "missing.toml")
    for args in (["--stat-neighbors", "20"], ["--stat-std-ratio", "2"], ["--stat-neighbors", "0", "--stat-std-ratio", "2"],
                 ["--stat-neighbors", "65", "--stat-std-ratio", "2"], ["--stat-neighbors", "k", "--stat-std-ratio", "2"],
                 ["--stat-neighbors", "20", "--stat-std-ratio", "-1"], ["--stat-neighbors", "20", "--stat-std-ratio", "nan"],
                 ["--stat-neighbors", "20", "--stat-std-ratio", "inf"], ["--stat-neighbors", "20", "--stat-std-ratio"],
                 ["--target-stat-neighbors", "20"], ["--target-stat-neighbors", "-3", "--target-stat-std-ratio", "2"],
                 ["--target-stat-neighbors", "20", "--target-stat-std-ratio", "x"]):
        r = subprocess.run([exe, cfg] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "stat" in r.stderr, (args, r.returncode, r.stderr)


@pytest.mark.parametrize("target", ["stat-asan", "stat-tsan"])
def test_stat_selftest_under_the_sanitizers(target):
    """csrc/stat_selftest.cpp: the host function against all pairs, the threaded path from 65 536 points included, built with
    -fsanitize=address,undefined / -fsanitize=thread and run as a program of its own"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cuda-go-icp_amd", "csrc"), target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "stat selftest ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
