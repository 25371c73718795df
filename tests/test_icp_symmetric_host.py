"""Symmetric point-to-plane ICP (goicp_set_icp_symmetric), the part that needs no GPU: the four new symbols in the header, the library and the
binding, the ABI version and struct sizes they leave alone, the shim's call sites, and the CLI's refusals before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg

NEW = {"goicp_set_icp_symmetric", "goicp_get_icp_symmetric", "goicp_source_normals", "goicp_set_source_normals"}
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def test_header_nm_and_binding_agree(pkg):
    from cuda_go_icp_amd import binding as B
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int goicp_set_icp_symmetric\(goicp_handle h, int32_t enabled, int32_t source_normal_k\);", hdr)
    assert re.search(r"int goicp_get_icp_symmetric\(goicp_handle h, int32_t\* enabled, int32_t\* source_normal_k, int32_t\* user_normals\);", hdr)
    assert re.search(r"int goicp_source_normals\(goicp_handle h, float\* \w+\);", hdr)
    assert re.search(r"int goicp_set_source_normals\(goicp_handle h, const float\* \w+, size_t n\);", hdr)
    declared = set(re.findall(r"\b(goicp_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(B.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert NEW <= exported, NEW - exported
    lib = pkg.load_library()
    for name in NEW:
        assert getattr(lib, name).restype is C.c_int
    assert B.SYMBOLS["goicp_set_icp_symmetric"][1][1:] == [C.c_int32, C.c_int32]
    assert B.SYMBOLS["goicp_set_source_normals"][1][-1] is C.c_size_t


def test_abi_version_and_struct_sizes_unchanged(pkg):
    from cuda_go_icp_amd import binding as B
    assert pkg.load_library().goicp_abi_version() == 4
    # as tests/test_host_boundary.py states them
    assert C.sizeof(B.CCube) == 24
    assert C.sizeof(B.CCounters) == 80
    assert C.sizeof(B.CStepStatus) == 24
    assert C.sizeof(B.CResult) == 4 * (9 + 3 + 9 + 3 + 1 + 1) + 80 + 16
    # the option structs beside which the flag lives: it is an entry point of its own, not a field
    assert C.sizeof(B.CIcpOptions) == 8
    assert [n for n, _ in B.CIcpOptions._fields_] == ["metric", "normal_k"]


def test_null_arguments_refused(pkg):
    lib = pkg.load_library()
    e, k, u = C.c_int32(), C.c_int32(), C.c_int32()
    buf = (C.c_float * 3)()
    assert lib.goicp_set_icp_symmetric(None, 1, 16) == INVALID
    assert lib.goicp_get_icp_symmetric(None, C.byref(e), C.byref(k), C.byref(u)) == INVALID
    assert lib.goicp_source_normals(None, buf) == INVALID
    assert lib.goicp_set_source_normals(None, buf, 1) == INVALID


def test_shim_symmetric_call_sites_compile():
    """tests/shim_symmetric.cpp, compiled as tests/shim_normals.cpp is: syntax only"""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_symmetric.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


BAD_CLI = [
    (["--symmetric", "--ranks", "2"], "--ranks"),
    (["--symmetric", "--source-normal-k", "2"], "--source-normal-k"),
    (["--symmetric", "--source-normal-k", "33"], "--source-normal-k"),
    (["--symmetric", "--source-normal-k", "k"], "--source-normal-k"),
    (["--symmetric", "--source-normal-k"], "--source-normal-k"),
    (["--source-normal-k", "8"], "--symmetric"),
    (["--symmetric", "--trim-fraction", "0.1"], "--trim-fraction"),
]


@pytest.mark.parametrize("args,reason", BAD_CLI)
def test_cli_refuses_before_any_device(pkg, tmp_path, args, reason):
    """exit status 2 with the reason; the config named does not exist, so a run that got as far as loading it (let alone creating an
    engine) would end with status 1 and another message"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml")] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and reason in r.stderr, (args, r.returncode, r.stderr)


def test_cli_accepts_symmetric_up_to_the_config(pkg, tmp_path):
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml"), "--symmetric", "--source-normal-k", "8"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--symmetric" not in r.stderr, (r.returncode, r.stderr)
