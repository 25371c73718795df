"""goicp_voxel_downsample_host: the voxel-grid operator on the host (no handle, no GPU) against the numpy twin of its definition
(tests/voxel_twin.py) -- cloud, counts and m bit for bit over the grid of sizes, cloud kinds and voxels -- and the properties the
definition promises: the counts sum to n, the keys rise strictly, a cell of one point returns the input's bits, every centroid lies within
2^-23 (E + max|x|) of the fp64 centroid of its cell (the derived bound, not a measured one), and a permuted input gives the same output
(the sums are exact integers, the cells are ordered).  Also here: the boundary (header, nm, binding, ABI version) for the three new entry
points, the shim's call-site file, and every refusal that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_twin as VT
from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_voxel_downsample_host", "goicp_voxel_downsample", "goicp_set_source_voxel"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


@pytest.mark.parametrize("kind", VT.KINDS)
@pytest.mark.parametrize("n", VT.SIZES)
def test_library_equals_twin_and_properties(pkg, kind, n):
    xyz = VT.make_cloud(kind, n)
    rng = np.random.default_rng(n)
    for v in VT.voxels_for(kind, xyz):
        want, wcnt, keys, cell = VT.twin(xyz, v)
        got, cnt = pkg.voxel_downsample(xyz, v)
        m = len(want)
        assert len(got) == m and len(cnt) == m, (kind, n, v, len(got), m)
        assert np.array_equal(cnt, wcnt), (kind, n, v)
        assert VT.same_bits(got, want), (kind, n, v, int(np.sum(got.view(np.uint32) != want.view(np.uint32))))
        # the properties, on the library's output
        assert int(cnt.sum()) == n and np.all(cnt >= 1)
        assert np.all(keys[1:] > keys[:-1])
        first = np.full(m, -1, np.int64)
        first[cell[::-1]] = np.arange(n)[::-1]
        single = cnt == 1
        assert VT.same_bits(got[single], xyz[first[single]])
        err = np.abs(got.astype(np.float64) - VT.centroids64(xyz, cell, m)).max()
        assert err <= VT.bound(xyz, kind == "denormal"), (kind, n, v, err, VT.bound(xyz, kind == "denormal"))
        perm = rng.permutation(n)
        got2, cnt2 = pkg.voxel_downsample(xyz[perm], v)
        assert VT.same_bits(got2, got) and np.array_equal(cnt2, cnt), (kind, n, v)


def test_extremes_of_the_voxel(pkg):
    xyz = VT.make_cloud("uniform", 4097)
    ext = float(np.max(xyz.max(0) - xyz.min(0)))
    alone, cnt = pkg.voxel_downsample(xyz, ext * 2.0 ** -20)
    assert len(alone) == 4097 and np.all(cnt == 1)                      # every point alone: the input, reordered by key
    assert VT.same_bits(alone[np.lexsort(alone.T)], xyz[np.lexsort(xyz.T)])
    one, cnt = pkg.voxel_downsample(xyz, ext * 4.0)
    assert len(one) == 1 and cnt[0] == 4097                             # one cell
    assert np.abs(one[0].astype(np.float64) - xyz.astype(np.float64).mean(0)).max() <= VT.bound(xyz)


def test_out_count_may_be_null(pkg):
    lib = pkg.load_library()
    fp = C.POINTER(C.c_float)
    xyz = VT.make_cloud("duplicates", 257)
    out, m = np.zeros((257, 3), np.float32), C.c_size_t(0)
    assert lib.goicp_voxel_downsample_host(xyz.ctypes.data_as(fp), 257, 0.3, out.ctypes.data_as(fp), None, C.byref(m)) == 0
    want = pkg.voxel_downsample(xyz, 0.3)[0]
    assert m.value == len(want) and VT.same_bits(out[:m.value], want)


def test_refusals_without_a_device(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = VT.make_cloud("uniform", 16)
    out, cnt, m = np.full((16, 3), -7, np.float32), np.full(16, -7, np.int32), C.c_size_t(99)
    x, o, c = xyz.ctypes.data_as(fp), out.ctypes.data_as(fp), cnt.ctypes.data_as(ip)
    host = lib.goicp_voxel_downsample_host
    assert host(None, 16, 0.1, o, c, C.byref(m)) == INVALID
    assert host(x, 16, 0.1, None, c, C.byref(m)) == INVALID
    assert host(x, 16, 0.1, o, c, None) == INVALID
    assert host(x, 0, 0.1, o, c, C.byref(m)) == INVALID
    assert host(x, (2 ** 31 - 1) // 8 + 1, 0.1, o, c, C.byref(m)) == INVALID        # goicp_create's limit, refused before anything is read
    for v in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert host(x, 16, v, o, c, C.byref(m)) == INVALID, v
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[7, 1] = bad_value
        assert host(bad.ctypes.data_as(fp), 16, 0.1, o, c, C.byref(m)) == INVALID and b"non-finite" in lib.goicp_last_error()
    # the 21-bit rule: E = 1, v = 2^-22 needs cell 2^22; v = 2^-21 is refused as well (E / v = 2^21), the next voxel up is taken
    unit = np.zeros((2, 3), np.float32)
    unit[1, 0] = 1.0
    u = unit.ctypes.data_as(fp)
    assert host(u, 2, 2.0 ** -22, o, c, C.byref(m)) == INVALID and b"21 bits" in lib.goicp_last_error()
    assert host(u, 2, 2.0 ** -21, o, c, C.byref(m)) == INVALID
    assert np.all(out == -7) and np.all(cnt == -7) and m.value == 99
    assert host(u, 2, float(np.nextafter(np.float32(2.0 ** -21), np.float32(1))), o, c, C.byref(m)) == 0 and m.value == 2
    # the handle-taking forms refuse a NULL handle before anything else
    assert lib.goicp_voxel_downsample(None, x, 16, 0.1, o, c, C.byref(m)) == INVALID
    assert lib.goicp_set_source_voxel(None, x, 16, 0.1, None) == INVALID


def test_header_nm_and_binding_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    for decl in (r"int goicp_voxel_downsample_host\(const float\* xyz, size_t n, float voxel, float\* out_xyz, int32_t\* out_count, size_t\* m\);",
                 r"int goicp_voxel_downsample\(goicp_handle h, const float\* xyz, size_t n, float voxel, float\* out_xyz, int32_t\* out_count, size_t\* m\);",
                 r"int goicp_set_source_voxel\(goicp_handle h, const float\* xyz, size_t n, float voxel, size_t\* n_kept\);"):
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
    assert lib.goicp_voxel_downsample_host.argtypes == [fp, C.c_size_t, C.c_float, fp, ip, sp]
    assert lib.goicp_voxel_downsample.argtypes == [C.c_void_p, fp, C.c_size_t, C.c_float, fp, ip, sp]
    assert lib.goicp_set_source_voxel.argtypes == [C.c_void_p, fp, C.c_size_t, C.c_float, sp]
    assert callable(pkg.voxel_downsample) and hasattr(pkg.Registration, "voxel_downsample")
    shim = open(os.path.join(ROOT, "include", "goicp_mi355.hpp")).read()
    assert "goicp_set_source_voxel(h_" in shim


@pytest.mark.parametrize("glm", [False, True])
def test_shim_voxel_call_sites_compile(glm):
    """tests/shim_voxel.cpp, compiled as tests/shim_set_source.cpp is: syntax only, with the shim's own Vec3 and with glm types on the
    caller's side"""
    from test_host_boundary import _glm_include_flags
    extra = ["-DSHIM_WITH_GLM"] + _glm_include_flags() if glm else []
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include")] + extra +
                       [os.path.join(ROOT, "tests", "shim_voxel.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_voxel_refusals_before_any_device(pkg, tmp_path):
    """exit status 2 with the reason; the config named does not exist, so a run that got as far as loading it would end with status 1"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    cfg = str(tmp_path / "missing.toml")
    for args in (["--voxel", "0"], ["--voxel", "-1"], ["--voxel", "nan"], ["--voxel", "inf"], ["--voxel", "x"], ["--voxel"],
                 ["--target-voxel", "0"], ["--target-voxel", "abc"]):
        r = subprocess.run([exe, cfg] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "voxel" in r.stderr, (args, r.returncode, r.stderr)
