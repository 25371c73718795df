"""Generalized (plane-to-plane) ICP (goicp_set_icp_generalized), the part that needs no GPU: the two new symbols in the header, the library
and the binding, the ABI version and struct sizes they leave alone, the shim's call sites, the CLI's refusals before any device is touched,
the header's definition text, and the twin's own algebra (tests/generalized_twin.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg

NEW = {"goicp_set_icp_generalized", "goicp_get_icp_generalized"}
INVALID = -1
f32 = np.float32


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def test_header_nm_and_binding_agree(pkg):
    from cuda_go_icp_amd import binding as B
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int goicp_set_icp_generalized\(goicp_handle h, int32_t enabled, float epsilon, int32_t source_normal_k\);", hdr)
    assert re.search(r"int goicp_get_icp_generalized\(goicp_handle h, int32_t\* enabled, float\* epsilon, int32_t\* source_normal_k, int32_t\* user_normals\);",
                     hdr)
    declared = set(re.findall(r"\b(goicp_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(B.SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert NEW <= exported, NEW - exported
    lib = pkg.load_library()
    for name in NEW:
        assert getattr(lib, name).restype is C.c_int
    assert B.SYMBOLS["goicp_set_icp_generalized"][1][1:] == [C.c_int32, C.c_float, C.c_int32]
    for name in ("set_icp_generalized", "get_icp_generalized"):
        assert callable(getattr(pkg.Registration, name))
    import inspect
    sig = inspect.signature(pkg.Registration.__init__).parameters
    assert sig["icp_generalized"].default is False and sig["gicp_epsilon"].default == 1e-3


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
    # as tests/test_pose_information_host.py states them
    assert C.sizeof(B.CPoseInfoOptions) == 40
    assert C.sizeof(B.CPoseInfo) == (36 + 6 + 36 + 6 + 36 + 3 + 4) * 8 + 8 + 3 * 4 + 4
    assert C.sizeof(B.CIcpGate) == 12 and C.sizeof(B.CIcpRobust) == 8


def test_null_arguments_refused(pkg):
    lib = pkg.load_library()
    e, k, u, eps = C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
    assert lib.goicp_set_icp_generalized(None, 1, 1e-3, 16) == INVALID
    assert lib.goicp_get_icp_generalized(None, C.byref(e), C.byref(eps), C.byref(k), C.byref(u)) == INVALID


def test_shim_generalized_call_sites_compile():
    """tests/shim_generalized.cpp, compiled as tests/shim_symmetric.cpp is: syntax only"""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_generalized.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


BAD_CLI = [
    (["--generalized", "--symmetric"], "--symmetric"),
    (["--symmetric", "--generalized"], "--symmetric"),
    (["--generalized", "--ranks", "2"], "--ranks"),
    (["--generalized", "--trim-fraction", "0.1"], "--trim-fraction"),
    (["--generalized", "--gicp-epsilon", "0.00005"], "--gicp-epsilon"),
    (["--generalized", "--gicp-epsilon", "1.5"], "--gicp-epsilon"),
    (["--generalized", "--gicp-epsilon", "nan"], "--gicp-epsilon"),
    (["--generalized", "--gicp-epsilon", "e"], "--gicp-epsilon"),
    (["--generalized", "--gicp-epsilon"], "--gicp-epsilon"),
    (["--gicp-epsilon", "0.01"], "--generalized"),
    (["--generalized", "--source-normal-k", "2"], "--source-normal-k"),
]


@pytest.mark.parametrize("args,reason", BAD_CLI)
def test_cli_refuses_before_any_device(pkg, tmp_path, args, reason):
    """exit status 2 with the reason; the config named does not exist, so a run that got as far as loading it (let alone creating an
    engine) would end with status 1 and another message"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml")] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and reason in r.stderr, (args, r.returncode, r.stderr)


def test_cli_accepts_generalized_up_to_the_config(pkg, tmp_path):
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml"), "--generalized", "--gicp-epsilon", "0.01", "--source-normal-k", "8"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "--generalized" not in r.stderr, (r.returncode, r.stderr)


def test_header_states_the_definition():
    """the definition lives in the header once: epsilon's range and default, the order of the float operations, the robust argument"""
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    doc = hdr[hdr.index("generalized (plane-to-plane) ICP"):hdr.index("int goicp_set_icp_generalized(")]
    for text in ("epsilon must lie in [1e-4, 1]", "the default is 1e-3", "Sxx = 2 - k * (u.x * u.x + s.x * s.x)", "C01 = Sxz * Syz - Sxy * Szz",
                 "det = Sxx * C00 + Sxy * C01 + Sxz * C02", "Wij = (h * Cij) / det", "the weight is taken of the Euclidean distance d = sqrt(d^2)",
                 "goicp_abi_version() stays 4", "goicp_set_icp_symmetric(1, ..) while this flag is on"):
        assert text in doc, text


# ---- the twin's own algebra ----
def _case(n=200, seed=3):
    rng = np.random.default_rng(seed)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)
    from generalized_twin import rodrigues64
    return rodrigues64(rng.uniform(-0.5, 0.5, 3)).astype(f32), unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3))), rng


def test_twin_weight_is_the_inverse_of_the_combined_covariance():
    import generalized_twin as T
    R, ns, u, _ = _case()
    for eps in (1e-4, 1e-3, 0.05, 0.5):
        W = T.full(T.weight32(R, ns, u, eps))
        s = ns.astype(np.float64) @ R.astype(np.float64).T
        k = 1.0 - float(f32(eps))
        Sigma = 2 * np.eye(3) - k * (np.einsum("ni,nj->nij", u.astype(np.float64), u) + np.einsum("ni,nj->nij", s, s))
        want = 2 * float(f32(eps)) * np.linalg.inv(Sigma)
        # float cofactors of entries of size <= 2: an absolute error of a few 2^-24 * 4 against a determinant >= 8 eps^2 ... 8 eps
        assert np.abs(W - want).max() <= 2e-5 / min(1.0, 100 * eps), (eps, np.abs(W - want).max())
        ev = np.linalg.eigvalsh(W)
        assert ev.min() >= eps * (1 - 1e-2) - 1e-6 and ev.max() <= 1 + 1e-5, (eps, ev.min(), ev.max())


def test_twin_sign_epsilon_one_and_zero_normals():
    import generalized_twin as T
    R, ns, u, rng = _case()
    flip = rng.random(len(ns)) < 0.5
    a = T.weight32(R, ns, u, 1e-3)
    b = T.weight32(R, np.where(flip[:, None], -ns, ns), np.where(~flip[:, None], -u, u), 1e-3)
    assert a.tobytes() == b.tobytes()                                   # no product sees a normal's sign
    one = T.weight32(R, ns, u, 1.0)
    assert np.array_equal(one, np.tile(f32([1, 0, 0, 1, 0, 1]), (len(ns), 1)))          # eps = 1: W = I exactly
    z = np.zeros_like(ns)
    for eps in (1e-4, 1e-3, 0.3):
        both = T.weight32(R, z, z, eps)
        assert np.array_equal(both, np.tile(f32([1, 0, 0, 1, 0, 1]) * f32(eps), (len(ns), 1)))   # both zero: W = eps I exactly


def test_twin_system_is_the_gauss_newton_system_of_the_weighted_cost():
    """H and b against finite differences of f(x) = 1/2 e'^T W e', e' = e + omega x a + tau"""
    import generalized_twin as T
    R, ns, u, rng = _case(8)
    W6 = T.weight32(R, ns, u, 0.01)
    a, e = rng.normal(size=(8, 3)), 0.1 * rng.normal(size=(8, 3))
    H, b = T.system64(W6, a, e)
    W = T.full(W6)

    def f(x, i):
        ep = e[i] + np.cross(x[:3], a[i]) + x[3:]
        return 0.5 * ep @ W[i] @ ep
    h = 1e-5
    for i in range(8):
        g = np.array([(f(h * np.eye(6)[k], i) - f(-h * np.eye(6)[k], i)) / (2 * h) for k in range(6)])
        assert np.abs(g - b[i]).max() <= 1e-8, (i, g, b[i])
        Hn = np.array([[(f(h * (np.eye(6)[k] + np.eye(6)[l]), i) - f(h * (np.eye(6)[k] - np.eye(6)[l]), i) - f(h * (np.eye(6)[l] - np.eye(6)[k]), i)
                         + f(-h * (np.eye(6)[k] + np.eye(6)[l]), i)) / (4 * h * h) for l in range(6)] for k in range(6)])
        assert np.abs(Hn - H[i]).max() <= 1e-5, (i, np.abs(Hn - H[i]).max())
        assert np.abs(H[i] - H[i].T).max() <= 1e-15 * (1 + np.abs(H[i]).max())
