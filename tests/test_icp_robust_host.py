"""CPU-side tests of the robust-kernel ICP boundary (goicp_set_icp_robust and friends): the header, the library's dynamic symbol table and
binding.SYMBOLS agree on the new entry points, the struct layout and defaults, goicp_cli --robust-kernel / --robust-scale refusing bad
values and forbidden combinations before it touches a device -- and the fp64 numpy twin of the semantics that tests/test_gpu_icp_robust.py
imports, checked here against the table of include/goicp_mi355.h.  No compute calls here.

The twin restates the contract: c = scale, d = the neighbour distance, r = d (metric 0) or |(q - m) . n| (metric 1), u = r / c, v = d / c;
  kernel             w(r)                               rho
  1 Huber            1 if r <= c, else c / r            d^2 if d <= c, else 2 c d - c^2
  2 Cauchy           1 / (1 + u^2)                      c^2 log1p(v^2)
  3 Geman-McClure    1 / (1 + u^2)^2                    d^2 / (1 + v^2)
  4 Tukey            (1 - u^2)^2 if r <= c, else 0      c^2/3 (1 - (1 - v^2)^3) if d <= c, else c^2/3
every term of the update times w, W = sum w in place of n (carried means included), err = sum d^2 over all points, stop iff
C_prev > 0 and C_prev - C_new < err_diff N with C = sum rho, W below 3 / 6 leaves the pose and stops."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_icp_robust_default", "goicp_set_icp_robust", "goicp_icp_robust_stats"}
HUBER, CAUCHY, GM, TUKEY = 1, 2, 3, 4
NAMES = {HUBER: "huber", CAUCHY: "cauchy", GM: "gm", TUKEY: "tukey"}


# ----------------------------------------------------------------------------------------------
# the fp64 twin
# ----------------------------------------------------------------------------------------------
def robust_w(kernel, c, r):
    r = np.asarray(r, np.float64)
    u2 = (r / c) ** 2
    if kernel == 0:
        return np.ones_like(r)
    if kernel == HUBER:
        return np.where(r <= c, 1.0, c / np.maximum(r, 1e-300))
    if kernel == CAUCHY:
        return 1.0 / (1.0 + u2)
    if kernel == GM:
        return 1.0 / (1.0 + u2) ** 2
    if kernel == TUKEY:
        return np.where(r <= c, (1.0 - u2) ** 2, 0.0)
    raise ValueError(kernel)


def robust_rho(kernel, c, r):
    r = np.asarray(r, np.float64)
    u2 = (r / c) ** 2
    if kernel == 0:
        return r * r
    if kernel == HUBER:
        return np.where(r <= c, r * r, 2 * c * r - c * c)
    if kernel == CAUCHY:
        return c * c * np.log1p(u2)
    if kernel == GM:
        return r * r / (1.0 + u2)
    if kernel == TUKEY:
        return np.where(r <= c, c * c / 3 * (1 - (1 - u2) ** 3), c * c / 3)
    raise ValueError(kernel)


def _rodrigues64(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * (W @ W)


def twin_icp(tree, tgt, src, kernel, c, max_iter, err_diff=1e-7, R=None, t=None, normals=None):
    """-> (R, t, err, iters, W, C).  Neighbours: cKDTree.  normals None: point-to-point -- weighted Kabsch with the reference's carried
    means (jly_icp3d.hpp:244-263); normals (M, 3): point-to-plane -- the weighted damped Gauss-Newton step about the pivot cq = R c_src + t."""
    tgt, src = tgt.astype(np.float64), src.astype(np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    N, floor = len(src), 3 if normals is None else 6
    sc = src.mean(0)
    mu_m, mu_d, cost, err, iters, W, Cn = np.zeros(3), np.zeros(3), -1.0, 0.0, 0, 0.0, 0.0
    for _ in range(max_iter):
        q = src @ R.T + t
        d, j = tree.query(q)
        m = tgt[j]
        err = float((d * d).sum())
        if normals is None:
            r = d
        else:
            n = normals[j].astype(np.float64)
            res = ((q - m) * n).sum(1)
            r = np.abs(res)
        w = robust_w(kernel, c, r)
        W, Cn = float(w.sum()), float(robust_rho(kernel, c, d).sum())
        if W < floor or (cost > 0 and cost - Cn < err_diff * N):
            break
        if normals is None:
            mu_d, mu_m = (mu_d + (w[:, None] * q).sum(0)) / W, (mu_m + (w[:, None] * m).sum(0)) / W
            H = (w[:, None] * (q - mu_d)).T @ (m - mu_m)
            U, _, Vt = np.linalg.svd(H)
            Rk = Vt.T @ np.diag([1, 1, np.linalg.det(Vt.T @ U.T)]) @ U.T
            tk = mu_m - Rk @ mu_d
            R, t = Rk @ R, Rk @ t + tk
        else:
            cq = R @ sc + t
            J = np.concatenate([np.cross(q - cq, n), n], 1)
            A, b = (w[:, None] * J).T @ J, (w[:, None] * J).T @ res
            A = A + 1e-12 * np.trace(A) * np.eye(6)
            x = np.linalg.solve(A, -b)
            dR = _rodrigues64(x[:3])
            R, t = dR @ R, dR @ (t - cq) + cq + x[3:]
        cost, iters = Cn, iters + 1
    return R, t, err, iters, W, Cn


# ----------------------------------------------------------------------------------------------
# the twin against the table
# ----------------------------------------------------------------------------------------------
def test_twin_weights_and_costs_match_the_table():
    c = 0.5
    r = np.array([0.0, 0.25, 0.5, 1.0, 2.0])                          # u = 0, 1/2, 1, 2, 4
    # values worked out by hand from the table (u^2 = 0, 1/4, 1, 4, 16)
    assert np.allclose(robust_w(HUBER, c, r), [1, 1, 1, 0.5, 0.25], rtol=0, atol=1e-15)
    assert np.allclose(robust_rho(HUBER, c, r), [0, 0.0625, 0.25, 0.75, 1.75], rtol=0, atol=1e-15)
    assert np.allclose(robust_w(CAUCHY, c, r), [1, 0.8, 0.5, 0.2, 1 / 17], rtol=0, atol=1e-15)
    assert np.allclose(robust_rho(CAUCHY, c, r), 0.25 * np.log([1, 1.25, 2, 5, 17]), rtol=0, atol=1e-15)
    assert np.allclose(robust_w(GM, c, r), [1, 0.64, 0.25, 0.04, 1 / 289], rtol=0, atol=1e-15)
    assert np.allclose(robust_rho(GM, c, r), [0, 0.05, 0.125, 0.2, 4 / 17], rtol=0, atol=1e-15)
    assert np.allclose(robust_w(TUKEY, c, r), [1, 0.5625, 0, 0, 0], rtol=0, atol=1e-15)
    assert np.allclose(robust_rho(TUKEY, c, r), [0, (1 - 0.421875) / 12, 1 / 12, 1 / 12, 1 / 12], rtol=0, atol=1e-15)
    assert np.array_equal(robust_w(0, c, r), np.ones(5)) and np.array_equal(robust_rho(0, c, r), r * r)
    # w and rho belong together: w = rho'(r) / (2 r); rho <= r^2; rho ~ r^2 near 0; Huber inside its scale is the plain term exactly
    x = np.linspace(1e-3, 3.0, 4001)
    x = x[np.abs(x - c) > 1e-3]                                       # Huber and Tukey have a kink / their edge at r = c
    h = 1e-6
    for k in (HUBER, CAUCHY, GM, TUKEY):
        drho = (robust_rho(k, c, x + h) - robust_rho(k, c, x - h)) / (2 * h)
        assert np.abs(drho / (2 * x) - robust_w(k, c, x)).max() <= 1e-6, k
        assert (robust_rho(k, c, x) <= x * x * (1 + 1e-15)).all() and (robust_w(k, c, x) <= 1).all() and (robust_w(k, c, x) >= 0).all()
        assert abs(robust_rho(k, c, 1e-4) / 1e-8 - 1) <= 1e-6
    inside = np.linspace(0, c, 100)
    assert np.array_equal(robust_w(HUBER, c, inside), np.ones(100)) and np.array_equal(robust_rho(HUBER, c, inside), inside * inside)


def test_twin_with_unit_weights_is_plain_kabsch():
    """a Huber scale above every distance: the twin is plain ICP, and W = N, C = err"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-0.5, 0.5, (400, 3))
    R0 = _rodrigues64(np.array([0.05, -0.04, 0.03]))
    src = (tgt[::2] - np.array([0.01, 0.02, -0.01])) @ R0
    tree = cKDTree(tgt)
    a = twin_icp(tree, tgt, src, HUBER, 100.0, 50)
    b = twin_icp(tree, tgt, src, 0, 1.0, 50)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:4] == b[2:4]
    assert a[4] == len(src) and abs(a[5] - a[2]) <= 1e-12 * max(a[2], 1e-30)
    assert np.abs(a[0] - R0).max() <= 1e-6                         # and it finds the pose: tgt = R0 src + t


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
    assert re.search(r"typedef struct goicp_icp_robust \{ int32_t kernel; float scale; \} goicp_icp_robust;", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(goicp_[a-z0-9_]+)\s*\(", hdr))
    from cuda_go_icp_amd import binding
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("goicp_") and " T " in l}
    assert NEW <= declared and NEW <= exported and NEW <= set(binding.SYMBOLS)
    assert declared == set(binding.SYMBOLS) and declared <= exported, (declared ^ set(binding.SYMBOLS), declared - exported)
    assert pkg.load_library().goicp_abi_version() == 4               # symbols were added, no struct changed


def test_robust_struct_and_defaults(pkg):
    from cuda_go_icp_amd import binding as B
    assert C.sizeof(B.CIcpRobust) == 8
    assert [(n, t) for n, t in B.CIcpRobust._fields_] == [("kernel", C.c_int32), ("scale", C.c_float)]
    assert C.sizeof(B.CIcpGate) == 12 and C.sizeof(B.CIcpOptions) == 8   # the neighbours are not extended
    lib = pkg.load_library()
    r = B.CIcpRobust(7, 7.0)
    lib.goicp_icp_robust_default(C.byref(r))
    assert (r.kernel, r.scale) == (0, 0.0)
    lib.goicp_icp_robust_default(None)                               # tolerated, as goicp_icp_gate_default
    d = pkg.Registration.icp_robust_default()
    assert (d.kernel, d.scale) == (0, 0.0)
    assert pkg.Registration.ROBUST_KERNELS["huber"] == 1 and pkg.Registration.ROBUST_KERNELS["tukey"] == 4


def test_null_arguments_refused(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    ok = B.CIcpRobust(1, 0.1)
    assert lib.goicp_set_icp_robust(None, C.byref(ok)) == INVALID
    assert lib.goicp_set_icp_robust(None, None) == INVALID
    f = (C.c_float * 4)()
    assert lib.goicp_icp_robust_stats(None, 1, f, f) == INVALID


BAD_CLI = [
    (["--robust-kernel", "huber"], "--robust-scale"),                                  # no scale
    (["--robust-kernel", "huber", "--robust-scale"], "--robust-scale"),
    (["--robust-scale", "0.05"], "--robust-kernel"),                                   # no kernel
    (["--robust-kernel", "l2", "--robust-scale", "0.05"], "huber, cauchy, gm, tukey"),
    (["--robust-kernel", "--robust-scale", "0.05"], "huber, cauchy, gm, tukey"),
    (["--robust-kernel", "cauchy", "--robust-scale", "0"], "finite scale > 0"),
    (["--robust-kernel", "cauchy", "--robust-scale", "-0.1"], "finite scale > 0"),
    (["--robust-kernel", "gm", "--robust-scale", "nan"], "finite scale > 0"),
    (["--robust-kernel", "gm", "--robust-scale", "inf"], "finite scale > 0"),
    (["--robust-kernel", "tukey", "--robust-scale", "0.1x"], "finite scale > 0"),
    (["--robust-kernel", "tukey", "--robust-scale", "0.1", "--ranks", "2"], "--ranks N > 1"),
    (["--robust-kernel", "tukey", "--robust-scale", "0.1", "--trim-fraction", "0.2"], "--trim-fraction F > 0"),
    (["--robust-kernel", "huber", "--robust-scale", "0.1", "--max-corr-dist", "0.1"], "--max-corr-dist"),
    (["--max-corr-dist", "0.1", "--robust-kernel", "huber", "--robust-scale", "0.1"], "--max-corr-dist"),
]


@pytest.mark.parametrize("args,reason", BAD_CLI)
def test_cli_refuses_before_any_device(pkg, tmp_path, args, reason):
    """exit status 2 with the reason; the config named does not exist, so a run that got as far as loading it (let alone creating an
    engine) would end with status 1 and another message"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml")] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--robust-kernel" in r.stderr and reason in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("name", ["huber", "cauchy", "gm", "tukey"])
def test_cli_accepts_a_good_kernel_up_to_the_config(pkg, tmp_path, name):
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    r = subprocess.run([exe, str(tmp_path / "missing.toml"), "--robust-kernel", name, "--robust-scale", "0.05"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--robust-kernel" not in r.stderr, (r.returncode, r.stderr)
