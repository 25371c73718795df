"""CPU-side tests of the truncated-cost search boundary (goicp_set_search_truncation / goicp_search_truncation): the header, the library's
dynamic symbol table and binding.SYMBOLS agree on the new entry points, the ABI version and every struct size are what they were, the setter
refuses what the distance alone decides (and a NULL handle) without a device, goicp_cli --trunc-dist refuses bad values and forbidden
combinations before it touches a device and accepts a good one up to the config -- and the fp64 twin of the two bound terms that
tests/test_gpu_search_trunc.py imports, checked here on hand-worked values.  No compute calls here.

The twin restates the contract: m = the per-point clamped residual max(DT(R p + t_c) - coeff |p|, 0) (oracle.cube_terms, the engine's own
float arithmetic), g = the truncation distance, mtd = float32(1.732050808 / 2 * w) the translation radius of a cube of width w:
    ub = sum min(m, g)^2            lb = sum min(max(m - mtd, 0), g)^2            (clamp AFTER the subtractions)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_set_search_truncation", "goicp_search_truncation"}


# ----------------------------------------------------------------------------------------------
# the fp64 twin
# ----------------------------------------------------------------------------------------------
def trunc_bound_f64(m, w_child, g):
    """(ub, lb) of the truncated objective from the per-point residuals m (float32, oracle.cube_terms), float64 sums"""
    m = np.asarray(m, np.float32).astype(np.float64)
    g = float(np.float32(g))
    mtd = float(np.float32(1.732050808 / 2.0 * float(np.float32(w_child))))
    return float(np.sum(np.minimum(m, g) ** 2)), float(np.sum(np.minimum(np.maximum(m - mtd, 0.0), g) ** 2))


def test_twin_on_hand_worked_values():
    m = np.array([0.0, 0.01, 0.05, 0.2, 1.0], np.float32)
    g, w = 0.05, 0.0                                                  # no translation radius: lb == ub
    ub, lb = trunc_bound_f64(m, w, g)
    g64, m64 = float(np.float32(g)), m.astype(np.float64)
    assert ub == lb == m64[1] ** 2 + 3 * g64 ** 2
    # the clamp comes after the subtraction: with mtd = 0.1 (w = 0.2 / sqrt 3) the residual 0.2 keeps 0.1 and is THEN cut to g; a grid
    # clamped beforehand would have left max(min(0.2, g) - 0.1, 0) = 0 of it
    w = np.float32(0.2 / 1.732050808)
    mtd = float(np.float32(1.732050808 / 2.0 * float(w)))
    assert abs(mtd - 0.1) < 1e-7
    ub, lb = trunc_bound_f64(m, w, g)
    assert ub == m64[1] ** 2 + 3 * g64 ** 2
    assert lb == 2 * g64 ** 2                                          # 0.2 - 0.1 and 1.0 - 0.1, both cut to g; the others vanish
    loose = float(np.sum(np.maximum(np.minimum(m64, g64) - mtd, 0.0) ** 2))
    assert loose == 0.0 < lb <= ub <= len(m) * g64 ** 2
    # a huge g is the plain bound
    ub, lb = trunc_bound_f64(m, w, 1e30)
    assert ub == float(np.sum(m64 * m64)) and lb == float(np.sum(np.maximum(m64 - mtd, 0.0) ** 2))


# ----------------------------------------------------------------------------------------------
# the library's boundary
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def test_header_nm_and_binding_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    assert re.search(r"int goicp_set_search_truncation\(goicp_handle h, float max_dist\);", hdr)
    assert re.search(r"int goicp_search_truncation\(goicp_handle h, float\* max_dist\);", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(goicp_[a-z0-9_]+)\s*\(", hdr))
    from cuda_go_icp_amd import binding
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("goicp_") and " T " in l}
    assert NEW <= declared and NEW <= exported and NEW <= set(binding.SYMBOLS)
    assert declared == set(binding.SYMBOLS) and declared <= exported, (declared ^ set(binding.SYMBOLS), declared - exported)
    lib = pkg.load_library()
    assert lib.goicp_set_search_truncation.argtypes == [C.c_void_p, C.c_float] and lib.goicp_set_search_truncation.restype is C.c_int
    assert hasattr(pkg.Registration, "set_search_truncation") and hasattr(pkg.Registration, "search_truncation")
    shim = open(os.path.join(ROOT, "include", "goicp_mi355.hpp")).read()
    assert "goicp_set_search_truncation(h_, max_dist)" in shim


def test_abi_version_and_struct_sizes_unchanged(pkg):
    """symbols were added only: the version stays 4 and every struct keeps its size (the figures of tests/test_host_boundary.py and of the
    gate's and the robust kernel's host tests)"""
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    assert lib.goicp_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    assert re.search(r"#define GOICP_ABI_VERSION 4\b", hdr)
    assert C.sizeof(B.CCube) == 24 and C.sizeof(B.CCounters) == 80 and C.sizeof(B.CStepStatus) == 24
    assert C.sizeof(B.CResult) == 4 * (9 + 3 + 9 + 3 + 1 + 1) + 80 + 16
    assert C.sizeof(B.CIcpGate) == 12 and C.sizeof(B.CIcpOptions) == 8 and C.sizeof(B.CIcpRobust) == 8
    p = B.CParams()
    lib.goicp_params_default(C.byref(p))
    assert not hasattr(p, "trunc_dist") and not hasattr(p, "search_truncation")        # a per-handle option, not a goicp_params field


def test_setters_refuse_without_a_device(pkg):
    lib = pkg.load_library()
    g = C.c_float(7.0)
    assert lib.goicp_set_search_truncation(None, 0.05) == INVALID                     # a good distance, no handle
    assert lib.goicp_set_search_truncation(None, 0.0) == INVALID
    assert lib.goicp_search_truncation(None, C.byref(g)) == INVALID and g.value == 7.0
    # what the distance alone decides is refused before the handle is looked at: a dangling non-NULL handle is never dereferenced
    bogus = C.c_void_p(8)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert lib.goicp_set_search_truncation(bogus, bad) == INVALID, bad
        assert b"max_dist" in lib.goicp_last_error()
        assert lib.goicp_set_search_truncation(None, bad) == INVALID


BAD_CLI = [
    (["--trunc-dist"], "finite distance > 0"),
    (["--trunc-dist", "0"], "finite distance > 0"),
    (["--trunc-dist", "-0.05"], "finite distance > 0"),
    (["--trunc-dist", "nan"], "finite distance > 0"),
    (["--trunc-dist", "inf"], "finite distance > 0"),
    (["--trunc-dist", "0.05x"], "finite distance > 0"),
    (["--trunc-dist", "0.05", "--ranks", "2"], "--ranks N > 1"),
    (["--ranks", "4", "--trunc-dist", "0.05"], "--ranks N > 1"),
    (["--trunc-dist", "0.05", "--trim-fraction", "0.3"], "--trim-fraction F > 0"),
    (["--trim-fraction", "0.3", "--trunc-dist", "0.05"], "--trim-fraction F > 0"),
]


@pytest.mark.parametrize("args,reason", BAD_CLI)
def test_cli_refuses_before_any_device(pkg, tmp_path, args, reason):
    """exit status 2 with the reason; the config named does not exist, so a run that got as far as loading it (let alone creating an
    engine) would end with status 1 and another message"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml")] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--trunc-dist" in r.stderr and reason in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("extra", [[], ["--max-corr-dist", "0.05"], ["--point-to-plane"], ["--robust-kernel", "huber", "--robust-scale", "0.05"]])
def test_cli_parses_a_good_distance_up_to_the_config(pkg, tmp_path, extra):
    """a good distance -- alone or with one of the refiners it is meant to sit around -- gets as far as the (missing) config: status 1"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml"), "--trunc-dist", "0.05"] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--trunc-dist" not in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--trunc-dist D]" in r.stderr
