"""CPU-side tests of the distance gate's boundary (goicp_set_icp_gate and friends): the header, the library's dynamic symbol table and
binding.SYMBOLS agree on the new entry points, the struct layout and defaults, the refusals the arguments alone decide (no device, no
handle), and goicp_cli --max-corr-dist refusing a bad value before it touches a device.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_icp_gate_default", "goicp_set_icp_gate", "goicp_icp_inliers", "goicp_eval_correspondences"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def test_header_nm_and_binding_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(goicp_[a-z0-9_]+)\s*\(", hdr))
    from cuda_go_icp_amd import binding
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("goicp_") and " T " in l}
    assert NEW <= declared and NEW <= exported and NEW <= set(binding.SYMBOLS)
    assert declared == set(binding.SYMBOLS) and declared <= exported, (declared ^ set(binding.SYMBOLS), declared - exported)
    assert pkg.load_library().goicp_abi_version() == 4               # symbols were added, no struct changed


def test_gate_struct_and_defaults(pkg):
    from cuda_go_icp_amd import binding as B
    assert C.sizeof(B.CIcpGate) == 12
    assert [(n, t) for n, t in B.CIcpGate._fields_] == [("max_corr_dist", C.c_float), ("min_inliers", C.c_int32), ("capped_walk", C.c_int32)]
    assert C.sizeof(B.CIcpOptions) == 8                              # goicp_icp_options is not extended
    lib = pkg.load_library()
    g = B.CIcpGate(7.0, 7, 7)
    lib.goicp_icp_gate_default(C.byref(g))
    assert (g.max_corr_dist, g.min_inliers, g.capped_walk) == (0.0, 0, 1)
    lib.goicp_icp_gate_default(None)                                 # tolerated, as goicp_icp_options_default
    d = pkg.Registration.icp_gate_default()
    assert (d.max_corr_dist, d.min_inliers, d.capped_walk) == (0.0, 0, 1)


@pytest.mark.parametrize("dist,min_inliers,capped,what", [
    (-0.5, 0, 1, b"max_corr_dist"), (float("nan"), 0, 1, b"max_corr_dist"), (float("inf"), 0, 1, b"max_corr_dist"),
    (-float("inf"), 0, 1, b"max_corr_dist"), (0.1, 2, 1, b"min_inliers"), (0.1, -3, 1, b"min_inliers"), (0.1, 0, 2, b"capped_walk"),
    (0.1, 0, -1, b"capped_walk")])
def test_gate_values_refused_without_a_device(pkg, dist, min_inliers, capped, what):
    """what the struct alone decides is refused before the handle is looked at: the message names the field, not the handle"""
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    g = B.CIcpGate(dist, min_inliers, capped)
    assert lib.goicp_set_icp_gate(None, C.byref(g)) == INVALID
    assert what in lib.goicp_last_error(), lib.goicp_last_error()


def test_null_arguments_refused(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    ok = B.CIcpGate(0.1, 0, 1)
    assert lib.goicp_set_icp_gate(None, C.byref(ok)) == INVALID and b"(h)" in lib.goicp_last_error()
    assert lib.goicp_set_icp_gate(None, None) == INVALID
    n = (C.c_int32 * 4)()
    assert lib.goicp_icp_inliers(None, 1, n) == INVALID
    I, Z = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)()
    assert lib.goicp_eval_correspondences(None, I, Z, 0.1, None, None, None, None) == INVALID
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.goicp_eval_correspondences(None, I, Z, bad, None, None, None, None) == INVALID
        assert b"max_corr_dist" in lib.goicp_last_error()


@pytest.mark.parametrize("args", [["--max-corr-dist", "-0.1"], ["--max-corr-dist", "0"], ["--max-corr-dist", "abc"], ["--max-corr-dist", "nan"],
                                  ["--max-corr-dist", "inf"], ["--max-corr-dist", "0.1x"], ["--max-corr-dist"],
                                  ["--max-corr-dist", "0.1", "--ranks", "2"], ["--max-corr-dist", "0.1", "--trim-fraction", "0.2"]])
def test_cli_refuses_a_bad_gate_before_any_device(pkg, tmp_path, args):
    """exit status 2 with a message about the flag; the config named does not exist, so a run that got as far as loading it (let alone
    creating an engine) would end with status 1 and another message"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml")] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--max-corr-dist" in r.stderr, (r.returncode, r.stderr)


def test_cli_accepts_a_good_gate_up_to_the_config(pkg, tmp_path):
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml"), "--max-corr-dist", "0.05"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--max-corr-dist" not in r.stderr, (r.returncode, r.stderr)
