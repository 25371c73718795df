"""goicp_source_order_host: the source order of goicp_params::morton_sort as a function of its own (host only, no handle, no GPU) -- the
twin of the device ordering that goicp_set_source uses (tests/test_gpu_source_order.py compares the two element for element).

Checked against an independent Python twin that shares nothing with the library but the rule:
  mode 2: a run of n points is split on the longest axis of its bounding box (float32 extents, the first axis wins a tie) after the
          left_count(n)-th element of the order (coordinate, index) -- -0.0 ties with +0.0 -- and both parts are split again, down to
          single points; left_count(n) = n / 2 rounded to a multiple of 256 / 64 / 16 / 4 / 1 (the largest unit smaller than n);
  mode 1: a stable sort by the 30-bit Morton code of ((p - min) / ext * 1024 clamped to 0..1023), ext the largest extent (>= 1e-30);
  mode 0: the input order.
The twin sorts whole runs (`sorted`), the library selects (`nth_element`, in parallel at the top from 8 192 points on): equality of the
two is the uniqueness argument of DESIGN 16 put to the test.  Also here: header <-> nm <-> binding agreement for the three new entry
points, the ABI version, and the refusals of the host function."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_set_source", "goicp_source_order_host", "goicp_debug_source_order"}
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4097, 8191, 8192, 8193, 20000]   # 8 192: the host's parallel top starts
KINDS = ["random", "duplicates", "planar", "zeros"]


# ----------------------------------------------------------------------------------------------
# clouds and the twin (imported by tests/test_gpu_source_order.py)
# ----------------------------------------------------------------------------------------------
def make_cloud(kind, n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    if kind == "random":
        p = rng.uniform(-0.5, 0.5, (n, 3))
    elif kind == "duplicates":
        # few distinct coordinate values per axis and whole points repeated: the index decides most comparisons
        p = rng.integers(-3, 4, (n, 3)) * 0.125
        p[n // 2:] = p[:n - n // 2]
    elif kind == "planar":
        p = rng.uniform(-0.5, 0.5, (n, 3))
        p[:, 1] = 0.25                                   # one axis all equal: extent 0, never chosen unless all are 0
    elif kind == "zeros":
        # -0.0 and +0.0 mixed on every axis, next to a few values on either side
        vals = np.array([-0.0, 0.0, -0.0, 0.0, -0.25, 0.25, -1e-30, 1e-30])
        p = vals[rng.integers(0, len(vals), (n, 3))]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, np.float32)


def left_count(n):
    unit = 256 if n > 256 else 64 if n > 64 else 16 if n > 16 else 4 if n > 4 else 1
    nl = ((n // 2 + unit // 2) // unit) * unit
    if nl == 0:
        nl = unit
    if nl >= n:
        nl = n - (n % unit if n % unit else unit)
    return nl


def twin_kd(xyz):
    cols = [xyz[:, k].astype(np.float64) + 0.0 for k in range(3)]      # + 0.0: -0.0 -> +0.0 (floats compare equal anyway)
    out = []

    def rec(ids):
        n = len(ids)
        if n <= 1:
            out.extend(ids)
            return
        sub = xyz[ids]
        ext = sub.max(axis=0) - sub.min(axis=0)                        # float32 differences
        ax = 0
        for k in (1, 2):
            if ext[k] > ext[ax]:
                ax = k
        col = cols[ax]
        s = sorted(ids, key=lambda i: (col[i], i))
        nl = left_count(n)
        rec(s[:nl])
        rec(s[nl:])

    rec(list(range(len(xyz))))
    return np.array(out, np.int32)


def _spread(q):
    q = q.astype(np.uint32) & 0x3ff
    q = (q ^ (q << 16)) & 0xff0000ff
    q = (q ^ (q << 8)) & 0x0300f00f
    q = (q ^ (q << 4)) & 0x030c30c3
    q = (q ^ (q << 2)) & 0x09249249
    return q


def morton_codes(xyz):
    mn = xyz.min(axis=0)
    ext = np.float32(max(np.max(xyz.max(axis=0) - mn), np.float32(1e-30)))
    code = np.zeros(len(xyz), np.uint32)
    for k in range(3):
        f = ((xyz[:, k] - mn[k]) / ext).astype(np.float32)
        q = np.minimum(np.float32(1023), np.maximum(np.float32(0), f * np.float32(1024))).astype(np.uint32)
        code |= _spread(q) << k
    return code


def twin(xyz, mode):
    if mode == 0:
        return np.arange(len(xyz), dtype=np.int32)
    if mode == 1:
        return np.argsort(morton_codes(xyz), kind="stable").astype(np.int32)
    return twin_kd(xyz)


_TWINS = {}


def twin_cached(kind, n, mode):
    """computed once per (kind, n, mode) and shared (the GPU test imports it)"""
    key = (kind, n, mode)
    if key not in _TWINS:
        _TWINS[key] = twin(make_cloud(kind, n), mode)
    return _TWINS[key]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


# ----------------------------------------------------------------------------------------------
# the ordering
# ----------------------------------------------------------------------------------------------
def test_left_count_is_a_proper_split():
    for n in range(2, 3000):
        assert 1 <= left_count(n) <= n - 1
    assert [left_count(n) for n in (2, 3, 4, 5, 16, 17, 64, 65, 256, 257, 1000)] == [1, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_host_order_equals_the_twin(pkg, kind, n):
    xyz = make_cloud(kind, n)
    for mode in (0, 1, 2):
        perm = pkg.source_order(xyz, mode)
        assert perm.dtype == np.int32 and perm.shape == (n,)
        assert np.array_equal(np.sort(perm), np.arange(n)), (kind, n, mode)              # a permutation
        assert np.array_equal(perm, twin_cached(kind, n, mode)), (kind, n, mode)
    codes = morton_codes(xyz)
    assert np.array_equal(pkg.source_order(xyz, 1), np.argsort(codes, kind="stable"))    # mode 1 = stable argsort of the codes


def test_zero_signs_tie(pkg):
    """a -0.0 and a +0.0 coordinate are equal to the comparator: flipping the signs of the zeros changes nothing"""
    xyz = make_cloud("zeros", 1000)
    flipped = xyz.copy()
    z = flipped == 0
    flipped[z] = -flipped[z]
    assert np.any(np.signbit(xyz) != np.signbit(flipped))
    for mode in (1, 2):
        assert np.array_equal(pkg.source_order(xyz, mode), pkg.source_order(flipped, mode))


# ----------------------------------------------------------------------------------------------
# the boundary
# ----------------------------------------------------------------------------------------------
def test_header_nm_and_binding_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    assert re.search(r"int goicp_set_source\(goicp_handle h, const float\* source_xyz, size_t n_source\);", hdr)
    assert re.search(r"int goicp_source_order_host\(const float\* xyz, size_t n, int32_t mode, int32_t\* perm\);", hdr)
    assert re.search(r"int goicp_debug_source_order\(goicp_handle h, const float\* xyz, size_t n, int32_t mode, int32_t\* perm\);", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(goicp_[a-z0-9_]+)\s*\(", hdr))
    from cuda_go_icp_amd import binding
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("goicp_") and " T " in l}
    assert NEW <= declared and NEW <= exported and NEW <= set(binding.SYMBOLS)
    assert declared == set(binding.SYMBOLS) and declared <= exported, (declared ^ set(binding.SYMBOLS), declared - exported)
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert lib.goicp_set_source.argtypes == [C.c_void_p, fp, C.c_size_t] and lib.goicp_set_source.restype is C.c_int
    assert lib.goicp_source_order_host.argtypes == [fp, C.c_size_t, C.c_int32, ip]
    assert lib.goicp_debug_source_order.argtypes == [C.c_void_p, fp, C.c_size_t, C.c_int32, ip]
    assert hasattr(pkg.Registration, "set_source") and hasattr(pkg.FastGoICP, "set_source") and callable(pkg.source_order)
    shim = open(os.path.join(ROOT, "include", "goicp_mi355.hpp")).read()
    assert "goicp_set_source(h_" in shim


@pytest.mark.parametrize("glm", [False, True])
def test_shim_set_source_call_sites_compile(glm):
    """tests/shim_set_source.cpp, compiled as tests/test_host_boundary.py compiles tests/shim_callsites.cpp: syntax only, with the shim's own
    Vec3 and with glm types on the caller's side"""
    from test_host_boundary import _glm_include_flags
    extra = ["-DSHIM_WITH_GLM"] + _glm_include_flags() if glm else []
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include")] + extra +
                       [os.path.join(ROOT, "tests", "shim_set_source.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_version_unchanged(pkg):
    lib = pkg.load_library()
    assert lib.goicp_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    assert re.search(r"#define GOICP_ABI_VERSION 4\b", hdr)
    from cuda_go_icp_amd import binding as B
    assert C.sizeof(B.CCube) == 24 and C.sizeof(B.CCounters) == 80 and C.sizeof(B.CStepStatus) == 24
    assert C.sizeof(B.CResult) == 4 * (9 + 3 + 9 + 3 + 1 + 1) + 80 + 16


def test_refusals_without_a_device(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = make_cloud("random", 16)
    perm = np.full(16, -7, np.int32)
    x, p = xyz.ctypes.data_as(fp), perm.ctypes.data_as(ip)
    assert lib.goicp_source_order_host(None, 16, 2, p) == INVALID
    assert lib.goicp_source_order_host(x, 16, 2, None) == INVALID
    assert lib.goicp_source_order_host(x, 0, 2, p) == INVALID
    assert lib.goicp_source_order_host(x, 16, 3, p) == INVALID and lib.goicp_source_order_host(x, 16, -1, p) == INVALID
    assert lib.goicp_source_order_host(x, (2 ** 31 - 1) // 8 + 1, 2, p) == INVALID      # goicp_create's limit, refused before anything is read
    assert np.all(perm == -7)
    assert lib.goicp_source_order_host(x, 16, 2, p) == 0 and np.array_equal(np.sort(perm), np.arange(16))
    # the handle-taking entry points refuse a NULL handle (and NULL clouds) before anything else
    assert lib.goicp_set_source(None, x, 16) == INVALID
    assert lib.goicp_debug_source_order(None, x, 16, 2, p) == INVALID


def test_cli_source_list_refusals_before_any_device(pkg, tmp_path):
    """exit status 2 with the reason; the config named does not exist, so a run that got as far as loading it would end with status 1"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    cfg = str(tmp_path / "missing.toml")
    empty = tmp_path / "empty.lst"
    empty.write_text("# nothing\n\n")
    good = tmp_path / "good.lst"
    good.write_text("# two scans\nscan1.txt\n\n  scan2.txt  \n")
    for args, reason in ((["--source-list"], "readable file"), (["--source-list", str(tmp_path / "none.lst")], "readable file"),
                         (["--source-list", str(empty)], "names no cloud"), (["--source-list", str(good), "--ranks", "2"], "--ranks N > 1"),
                         (["--ranks", "2", "--source-list", str(good)], "--ranks N > 1")):
        r = subprocess.run([exe, cfg] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--source-list" in r.stderr and reason in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([exe, cfg, "--source-list", str(good)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--source-list" not in r.stderr, (r.returncode, r.stderr)       # a good list gets as far as the (missing) config
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--source-list FILE]" in r.stderr
