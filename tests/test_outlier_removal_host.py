"""goicp_radius_outlier_removal_host: the radius outlier removal operator on the host (no handle, no GPU) against the numpy twin of its
definition (tests/outlier_twin.py) -- cloud, indices and counts bit for bit over the grid of sizes, cloud kinds, radii and
min_neighbors -- and the properties the definition promises: indices ascend, kept points carry the input's bits, the count is saturated,
a permuted input gives the permuted keep set, the keep set never grows with min_neighbors and never shrinks with the radius.  Also here:
the boundary (header, nm, binding, ABI version, struct sizes) for the new entry points, the shim's call-site file, and every refusal that
needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import outlier_twin as OT
from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_radius_outlier_removal_host", "goicp_radius_outlier_removal", "goicp_source_filter_default", "goicp_set_source_filtered"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


@pytest.mark.parametrize("kind", OT.KINDS)
@pytest.mark.parametrize("n", OT.SIZES)
def test_library_equals_twin_and_properties(pkg, kind, n):
    xyz = OT.make_cloud(kind, n)
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)
    keep_of = {}
    taken = 0
    for r in OT.radii_for(kind, xyz):
        if not OT.valid(xyz, r):
            with pytest.raises(pkg.GoicpError):
                pkg.radius_outlier_removal(xyz, r, 1)
            continue
        taken += 1
        counts = OT.neighbour_counts(xyz, r)
        for k in OT.ks_for(n):
            want, widx, wcnt = OT.twin(xyz, r, k, counts)
            got, idx, cnt = pkg.radius_outlier_removal(xyz, r, k)
            assert len(got) == len(want), (kind, n, r, k, len(got), len(want))
            assert np.array_equal(idx, widx) and np.array_equal(cnt, wcnt), (kind, n, r, k)
            assert OT.same_bits(got, want), (kind, n, r, k)
            # the properties, on the library's output
            assert np.all(np.diff(idx) > 0) and OT.same_bits(got, xyz[idx])
            assert cnt.min() >= 0 and cnt.max() <= k and np.array_equal(np.flatnonzero(cnt == k), idx)
            keep = np.zeros(n, bool)
            keep[idx] = True
            keep_of[(r, k)] = keep
            got2, idx2, cnt2 = pkg.radius_outlier_removal(xyz[perm], r, k)
            assert np.array_equal(cnt2, cnt[perm])
            assert np.array_equal(np.sort(perm[idx2]), idx) and OT.same_bits(got2, xyz[perm][idx2]), (kind, n, r, k)
    assert taken >= 1
    # monotone: never more points with a larger min_neighbors, never fewer with a larger radius
    for (r, k), keep in keep_of.items():
        for (r2, k2), keep2 in keep_of.items():
            if r2 == r and k2 > k:
                assert not np.any(keep2 & ~keep), (kind, n, r, k, k2)
            if k2 == k and np.float32(r2) > np.float32(r):
                assert not np.any(keep & ~keep2), (kind, n, k, r, r2)


@pytest.mark.parametrize("n", [2, 65, 1000])
def test_identical_points_are_each_others_neighbours(pkg, n):
    xyz = OT.make_cloud("identical", n)
    for k in sorted({1, n - 1}):
        got, idx, cnt = pkg.radius_outlier_removal(xyz, 1e-3, k)
        assert len(got) == n and np.array_equal(idx, np.arange(n)) and np.all(cnt == k) and OT.same_bits(got, xyz)
    got, idx, cnt = pkg.radius_outlier_removal(xyz, 1e-3, n)
    assert len(got) == 0 and len(idx) == 0 and np.all(cnt == n - 1)          # nobody is its own neighbour


def test_shell_points_at_exactly_r_are_kept(pkg):
    """for the cluster points exactly at the origin d2 == r2 holds at the shell points placed at r, and the next float above r gives
    d2 > r2: the twin's counts differ between the two, and the library agrees (the comparison is <=, in float)"""
    xyz = OT.make_cloud("shell", 256)
    r = OT.SHELL_R
    d = np.abs(xyz).max(1)
    at, above = np.flatnonzero(d == r), np.flatnonzero(d == np.nextafter(r, np.float32(1)))
    assert len(at) > 5 and len(above) > 5
    counts = OT.neighbour_counts(xyz, r)
    assert counts[at].min() >= 64 and counts[above].max() < 64             # the 64 points at the origin decide
    got, idx, cnt = pkg.radius_outlier_removal(xyz, float(r), 64)
    assert set(at) <= set(idx) and not set(above) & set(idx)
    assert np.array_equal(cnt, np.minimum(counts, 64))


def test_null_outputs_and_an_empty_result(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = OT.make_cloud("duplicates", 257)
    want, widx, wcnt = pkg.radius_outlier_removal(xyz, 0.3, 5)
    assert 0 < len(want) < 257
    host = lib.goicp_radius_outlier_removal_host
    out, idx, cnt, m = np.zeros((257, 3), np.float32), np.zeros(257, np.int32), np.zeros(257, np.int32), C.c_size_t(0)
    assert host(xyz.ctypes.data_as(fp), 257, 0.3, 5, out.ctypes.data_as(fp), None, None, C.byref(m)) == 0
    assert m.value == len(want) and OT.same_bits(out[:m.value], want)
    assert host(xyz.ctypes.data_as(fp), 257, 0.3, 5, out.ctypes.data_as(fp), idx.ctypes.data_as(ip), None, C.byref(m)) == 0
    assert np.array_equal(idx[:m.value], widx)
    assert host(xyz.ctypes.data_as(fp), 257, 0.3, 5, out.ctypes.data_as(fp), None, cnt.ctypes.data_as(ip), C.byref(m)) == 0
    assert np.array_equal(cnt, wcnt)
    # m == 0 is a result, not a refusal
    m.value = 99
    assert host(xyz.ctypes.data_as(fp), 257, 0.3, 257, out.ctypes.data_as(fp), idx.ctypes.data_as(ip), cnt.ctypes.data_as(ip), C.byref(m)) == 0
    assert m.value == 0 and cnt.max() < 257
    lone = OT.make_cloud("uniform", 1)
    got, gidx, gcnt = pkg.radius_outlier_removal(lone, 1.0, 1)
    assert len(got) == 0 and gcnt.tolist() == [0]


def test_refusals_without_a_device(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = OT.make_cloud("uniform", 16)
    out, idx, cnt, m = np.full((16, 3), -7, np.float32), np.full(16, -7, np.int32), np.full(16, -7, np.int32), C.c_size_t(99)
    x, o, i, c = xyz.ctypes.data_as(fp), out.ctypes.data_as(fp), idx.ctypes.data_as(ip), cnt.ctypes.data_as(ip)
    host = lib.goicp_radius_outlier_removal_host
    assert host(None, 16, 0.1, 2, o, i, c, C.byref(m)) == INVALID
    assert host(x, 16, 0.1, 2, None, i, c, C.byref(m)) == INVALID
    assert host(x, 16, 0.1, 2, o, i, c, None) == INVALID
    assert host(x, 0, 0.1, 2, o, i, c, C.byref(m)) == INVALID
    assert host(x, (2 ** 31 - 1) // 8 + 1, 0.1, 2, o, i, c, C.byref(m)) == INVALID      # goicp_create's limit, refused before anything is read
    for r in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert host(x, 16, r, 2, o, i, c, C.byref(m)) == INVALID, r
    # r * r must be a normal float: 2^-63 squares to exactly the smallest normal and is taken (were it not for the 2^16 rule: use a
    # cloud of no extent), the float below squares to a denormal, 1e20 squares to infinity
    same = OT.make_cloud("identical", 16)
    s = same.ctypes.data_as(fp)
    assert host(s, 16, float(np.nextafter(np.float32(2.0 ** -63), np.float32(0))), 2, o, i, c, C.byref(m)) == INVALID and b"normal" in lib.goicp_last_error()
    assert host(s, 16, 1e-30, 2, o, i, c, C.byref(m)) == INVALID
    assert host(s, 16, 1e20, 2, o, i, c, C.byref(m)) == INVALID and b"normal" in lib.goicp_last_error()
    for k in (0, -1, -2 ** 31):
        assert host(x, 16, 0.1, k, o, i, c, C.byref(m)) == INVALID and b"min_neighbors" in lib.goicp_last_error()
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[7, 1] = bad_value
        assert host(bad.ctypes.data_as(fp), 16, 0.1, 2, o, i, c, C.byref(m)) == INVALID and b"non-finite" in lib.goicp_last_error()
    # the 2^16 rule: E = 1, r = 2^-16 is refused (E / r = 2^16), the next radius up is taken
    unit = np.zeros((2, 3), np.float32)
    unit[1, 0] = 1.0
    u = unit.ctypes.data_as(fp)
    assert host(u, 2, 2.0 ** -17, 1, o, i, c, C.byref(m)) == INVALID and b"16 bits" in lib.goicp_last_error()
    assert host(u, 2, 2.0 ** -16, 1, o, i, c, C.byref(m)) == INVALID
    assert np.all(out == -7) and np.all(idx == -7) and np.all(cnt == -7) and m.value == 99
    assert host(s, 16, 2.0 ** -63, 2, o, i, c, C.byref(m)) == 0 and m.value == 16
    assert host(u, 2, float(np.nextafter(np.float32(2.0 ** -16), np.float32(1))), 1, o, i, c, C.byref(m)) == 0 and m.value == 0
    # the handle-taking forms refuse a NULL handle before anything else
    from cuda_go_icp_amd import binding
    f = binding.CSourceFilter(0.0, 0.1, 2)
    assert lib.goicp_radius_outlier_removal(None, x, 16, 0.1, 2, o, i, c, C.byref(m)) == INVALID
    assert lib.goicp_set_source_filtered(None, x, 16, C.byref(f), None) == INVALID


def test_header_nm_and_binding_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    args = r"const float\* xyz, size_t n, float radius, int32_t min_neighbors, float\* out_xyz, int32_t\* out_index, int32_t\* out_count, size_t\* m\);"
    for decl in (r"int goicp_radius_outlier_removal_host\(" + args, r"int goicp_radius_outlier_removal\(goicp_handle h, " + args,
                 r"typedef struct goicp_source_filter \{ float voxel; float radius; int32_t min_neighbors; \} goicp_source_filter;",
                 r"void goicp_source_filter_default\(goicp_source_filter\* out\);",
                 r"int goicp_set_source_filtered\(goicp_handle h, const float\* xyz, size_t n, const goicp_source_filter\* f, size_t\* n_kept\);"):
        assert re.search(decl, hdr), decl
    assert re.search(r"#define GOICP_ABI_VERSION 4\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(goicp_[a-z0-9_]+)\s*\(", hdr))
    from cuda_go_icp_amd import binding
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("goicp_") and " T " in l}
    assert NEW <= declared and NEW <= exported and NEW <= set(binding.SYMBOLS)
    assert declared == set(binding.SYMBOLS) and declared <= exported, (declared ^ set(binding.SYMBOLS), declared - exported)
    lib = pkg.load_library()
    assert lib.goicp_abi_version() == 4
    fp, ip, sp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)
    assert lib.goicp_radius_outlier_removal_host.argtypes == [fp, C.c_size_t, C.c_float, C.c_int32, fp, ip, ip, sp]
    assert lib.goicp_radius_outlier_removal.argtypes == [C.c_void_p, fp, C.c_size_t, C.c_float, C.c_int32, fp, ip, ip, sp]
    assert lib.goicp_set_source_filtered.argtypes == [C.c_void_p, fp, C.c_size_t, C.POINTER(binding.CSourceFilter), sp]
    # the new struct, its defaults, and the sizes the ABI had before
    assert C.sizeof(binding.CSourceFilter) == 12
    f = binding.CSourceFilter(1.0, 2.0, 3)
    lib.goicp_source_filter_default(C.byref(f))
    assert (f.voxel, f.radius, f.min_neighbors) == (0.0, 0.0, 0)
    assert C.sizeof(binding.CCube) == 24 and C.sizeof(binding.CCounters) == 80 and C.sizeof(binding.CStepStatus) == 24
    assert C.sizeof(binding.CResult) == 4 * (9 + 3 + 9 + 3 + 1 + 1) + 80 + 16
    assert C.sizeof(binding.CIcpOptions) == 8 and C.sizeof(binding.CIcpGate) == 12 and C.sizeof(binding.CIcpRobust) == 8
    assert callable(pkg.radius_outlier_removal) and hasattr(pkg.Registration, "radius_outlier_removal")
    shim = open(os.path.join(ROOT, "include", "goicp_mi355.hpp")).read()
    assert "goicp_set_source_filtered(h_" in shim


@pytest.mark.parametrize("glm", [False, True])
def test_shim_outlier_call_sites_compile(glm):
    """tests/shim_outlier.cpp, compiled as tests/shim_voxel.cpp is: syntax only, with the shim's own Vec3 and with glm types on the
    caller's side"""
    from test_host_boundary import _glm_include_flags
    extra = ["-DSHIM_WITH_GLM"] + _glm_include_flags() if glm else []
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include")] + extra +
                       [os.path.join(ROOT, "tests", "shim_outlier.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_outlier_refusals_before_any_device(pkg, tmp_path):
    """exit status 2 with the reason; the config named does not exist, so a run that got as far as loading it would end with status 1"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    cfg = str(tmp_path / "missing.toml")
    for args in (["--outlier-radius", "0.1"], ["--outlier-min-neighbors", "3"], ["--outlier-radius", "0", "--outlier-min-neighbors", "3"],
                 ["--outlier-radius", "nan", "--outlier-min-neighbors", "3"], ["--outlier-radius", "inf", "--outlier-min-neighbors", "3"],
                 ["--outlier-radius", "1e-30", "--outlier-min-neighbors", "3"], ["--outlier-radius", "x", "--outlier-min-neighbors", "3"],
                 ["--outlier-radius", "0.1", "--outlier-min-neighbors", "0"], ["--outlier-radius", "0.1", "--outlier-min-neighbors", "k"],
                 ["--outlier-radius", "0.1", "--outlier-min-neighbors"], ["--target-outlier-radius", "0.1"],
                 ["--target-outlier-radius", "-1", "--target-outlier-min-neighbors", "2"], ["--target-outlier-radius", "0.1", "--target-outlier-min-neighbors", "-2"]):
        r = subprocess.run([exe, cfg] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "outlier" in r.stderr, (args, r.returncode, r.stderr)
