"""goicp_knn_self_host and goicp_estimate_normals_host: the exact self k-NN and the normal estimation on the host (no handle, no GPU) against
the numpy twin of their definition (tests/normals_twin.py) -- indices, squared distances, normals and surface variation bit for bit over the
statistical filter's grid of sizes and cloud kinds -- the properties the definition promises (rows ascend by key, no point is its own
neighbour, d2 is the float expression of the indices, unit or zero normals, the sign rule, the variation's range), every refusal, an
independent check against numpy.linalg.eigh, the boundary (header, nm, binding, ABI version), the shim's call sites, the CLI mode on the
host, and the stand-alone selftest under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import normals_twin as NT
from conftest import ROOT, cloud, load_pkg

INVALID = -1
NEW = {"goicp_knn_self_host", "goicp_knn_self", "goicp_estimate_normals_host", "goicp_estimate_normals"}
ULP = np.float32(2.0 ** -23)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def d2_of(xyz, idx):
    """the header's float expression, recomputed from the indices"""
    with np.errstate(under="ignore"):
        d = xyz[:, None, :] - xyz[idx]
        out = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    assert out.dtype == np.float32
    return out


def check_normal_properties(xyz, nrm, var, vp, tag):
    length = np.sqrt((nrm.astype(np.float64) ** 2).sum(1))
    zero = ~nrm.any(1)
    assert np.all(zero | (np.abs(length - 1.0) <= 2.0 ** -23)), tag
    assert not np.any(np.signbit(nrm) & (nrm == 0)), tag                                  # zero components are +0
    assert np.all(var[zero] == 0) and np.all(var >= 0) and np.all(var <= np.float32(1.0 / 3.0) * (1 + ULP)), tag
    lead = np.where(nrm[:, 0] != 0, nrm[:, 0], np.where(nrm[:, 1] != 0, nrm[:, 1], nrm[:, 2]))
    d = np.zeros(len(xyz))
    if vp is not None:
        X, V, n64 = xyz.astype(np.float64), np.asarray(vp, np.float32).astype(np.float64), nrm.astype(np.float64)
        d = (n64[:, 0] * (V[0] - X[:, 0]) + n64[:, 1] * (V[1] - X[:, 1])) + n64[:, 2] * (V[2] - X[:, 2])
        assert np.all(d >= 0), tag
    assert np.all((d != 0) | (lead >= 0)), tag


@pytest.mark.parametrize("kind", NT.KINDS)
@pytest.mark.parametrize("n", NT.SIZES)
def test_library_equals_twin_and_properties(pkg, kind, n):
    xyz = NT.make_cloud(kind, n)
    keys = NT.keys_of(kind, n)
    for k in NT.knn_ks_for(n):
        widx, wd2 = NT.split(keys, k)
        idx, d2 = pkg.knn_self(xyz, k)
        assert np.array_equal(idx, widx), (kind, n, k, int(np.sum(np.any(idx != widx, axis=1))))
        assert NT.same_bits(d2, wd2), (kind, n, k)
        # the properties, on the library's output
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
        assert np.all(key[:, 1:] > key[:, :-1]), (kind, n, k)
        assert np.all(idx != np.arange(n)[:, None]) and idx.min() >= 0 and idx.max() < n
        assert NT.same_bits(d2, d2_of(xyz, idx)), (kind, n, k)
    for k in NT.normal_ks_for(n):
        for vp in (None, NT.viewpoint_of(xyz)):
            wn, wv, widx = NT.normals_twin(xyz, k, vp, keys)
            nrm, var, idx = pkg.estimate_normals(xyz, k, vp)
            tag = (kind, n, k, vp is not None)
            assert np.array_equal(idx, widx), tag
            assert NT.same_bits(nrm, wn), (tag, int(np.sum(np.any(nrm.view(np.uint32) != wn.view(np.uint32), axis=1))))
            assert NT.same_bits(var, wv), (tag, int(np.sum(var.view(np.uint32) != wv.view(np.uint32))))
            check_normal_properties(xyz, nrm, var, vp, tag)


@pytest.mark.parametrize("kind", ["identical", "denormal"])
def test_ties_at_every_place_go_to_the_smaller_index(pkg, kind):
    """every d2 is 0 (the denormal cloud's squares underflow): row i is the k smallest indices other than i, the normals are 0"""
    for n in (33, 65, 1000):
        xyz = NT.make_cloud(kind, n)
        for k in (1, 32):
            idx, d2 = pkg.knn_self(xyz, k)
            want = np.tile(np.arange(k, dtype=np.int32), (n, 1))
            for i in range(k):
                want[i] = np.delete(np.arange(k + 1, dtype=np.int32), i)
            assert np.array_equal(idx, want) and not d2.any(), (kind, n, k)
    nrm, var, _ = pkg.estimate_normals(NT.make_cloud("identical", 65), 16, np.float32([1, 2, 3]))
    assert not nrm.any() and not var.any() and not np.signbit(nrm).any()


def _eigh_clouds():
    rng = np.random.default_rng(7)
    out = []
    for n in (1000, 3000):
        p = rng.normal(size=(n, 3))
        out.append(("sphere", np.ascontiguousarray(p / np.linalg.norm(p, axis=1)[:, None] * 0.5 + rng.normal(scale=0.002, size=(n, 3)), np.float32)))
        out.append(("box", np.ascontiguousarray(rng.uniform(-1, 1, (n, 3)), np.float32)))
    return out


def test_normals_agree_with_eigh(pkg):
    """independent of the Jacobi: numpy.linalg.eigh on the fp64 covariance of the twin's own neighbour sets.  For the points whose relative
    gap (l1 - l0) / l2 is >= 1e-3, |sin| of the angle between the library's normal and eigh's smallest eigenvector is <= 1e-6: an fp64
    Jacobi error of a few 2^-52 l2 over a gap of 1e-3 l2 is about 1e-12, the float rounding of the output about 1e-7.  At most 5 % of a
    case's points may fall outside the gap condition"""
    worst_share = 0.0
    for name, xyz in _eigh_clouds():
        keys = NT.knn_keys(xyz, 31)
        X = xyz.astype(np.float64)
        for k in (3, 4, 8, 16, 32):
            idx = NT.split(keys, k - 1)[0]
            nb = np.concatenate([X[:, None, :], X[idx]], 1) - X[:, None, :]
            nb = nb - nb.mean(1, keepdims=True)
            w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", nb, nb))
            ok = (w[:, 1] - w[:, 0]) / w[:, 2] >= 1e-3
            share = 1.0 - ok.mean()
            worst_share = max(worst_share, share)
            nrm = pkg.estimate_normals(xyz, k)[0].astype(np.float64)
            sin = np.linalg.norm(np.cross(nrm, v[:, :, 0]), axis=1)
            print("%s n %d k %d: %.4f below the gap, worst |sin| %.3g" % (name, len(xyz), k, share, sin[ok].max()))
            assert share <= 0.05, (name, len(xyz), k, share)
            assert sin[ok].max() <= 1e-6, (name, len(xyz), k, float(sin[ok].max()))
    assert worst_share <= 0.05


def test_null_outputs(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = NT.make_cloud("uniform", 257)
    widx, wd2 = pkg.knn_self(xyz, 5)
    wn, wv, wi = pkg.estimate_normals(xyz, 6, np.float32([0, 0, 9]))
    idx, nrm, var = np.zeros((257, 5), np.int32), np.zeros((257, 3), np.float32), np.zeros(257, np.float32)
    vp = np.float32([0, 0, 9])
    assert lib.goicp_knn_self_host(xyz.ctypes.data_as(fp), 257, 5, idx.ctypes.data_as(ip), None) == 0 and np.array_equal(idx, widx)
    assert lib.goicp_estimate_normals_host(xyz.ctypes.data_as(fp), 257, 6, vp.ctypes.data_as(fp), nrm.ctypes.data_as(fp), None, None) == 0
    assert NT.same_bits(nrm, wn)
    assert lib.goicp_estimate_normals_host(xyz.ctypes.data_as(fp), 257, 6, vp.ctypes.data_as(fp), nrm.ctypes.data_as(fp), var.ctypes.data_as(fp), idx.ctypes.data_as(ip)) == 0
    assert NT.same_bits(var, wv) and np.array_equal(idx, wi) and np.array_equal(wi, widx)


def test_refusals_without_a_device(pkg):
    lib = pkg.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xyz = NT.make_cloud("uniform", 16)
    idx, d2 = np.full((16, 32), -7, np.int32), np.full((16, 32), -7, np.float32)
    nrm, var = np.full((16, 3), -7, np.float32), np.full(16, -7, np.float32)
    x, i, d, o, v = xyz.ctypes.data_as(fp), idx.ctypes.data_as(ip), d2.ctypes.data_as(fp), nrm.ctypes.data_as(fp), var.ctypes.data_as(fp)
    knn, nor = lib.goicp_knn_self_host, lib.goicp_estimate_normals_host
    assert knn(None, 16, 3, i, d) == INVALID and knn(x, 16, 3, None, d) == INVALID and knn(x, 0, 3, i, d) == INVALID
    assert knn(x, (2 ** 31 - 1) // 8 + 1, 3, i, d) == INVALID                 # goicp_create's limit, refused before anything is read
    for k in (0, -1, -2 ** 31, 33, 1000):
        assert knn(x, 16, k, i, d) == INVALID and b"k must be" in lib.goicp_last_error(), k
    assert knn(x, 16, 16, i, d) == INVALID and b"n - 1" in lib.goicp_last_error()
    assert knn(x, 1, 1, i, d) == INVALID
    assert nor(None, 16, 3, None, o, v, i) == INVALID and nor(x, 16, 3, None, None, v, i) == INVALID and nor(x, 0, 3, None, o, v, i) == INVALID
    assert nor(x, (2 ** 31 - 1) // 8 + 1, 3, None, o, v, i) == INVALID
    for k in (0, 1, 2, -1, 33, 1000):
        assert nor(x, 16, k, None, o, v, i) == INVALID and b"k must be" in lib.goicp_last_error(), k
    assert nor(x, 16, 17, None, o, v, i) == INVALID and b"n - 1" in lib.goicp_last_error()
    assert nor(x, 2, 3, None, o, v, i) == INVALID
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[7, 1] = bad_value
        assert knn(bad.ctypes.data_as(fp), 16, 3, i, d) == INVALID and b"non-finite" in lib.goicp_last_error()
        assert nor(bad.ctypes.data_as(fp), 16, 3, None, o, v, i) == INVALID and b"non-finite" in lib.goicp_last_error()
        vp = np.float32([1, bad_value, 3])
        assert nor(x, 16, 3, vp.ctypes.data_as(fp), o, v, i) == INVALID and b"viewpoint" in lib.goicp_last_error()
    assert np.all(idx == -7) and np.all(d2 == -7) and np.all(nrm == -7) and np.all(var == -7)
    # nothing about the extent is refused: a cloud spread over 2^40 times its closest pair, k = n - 1
    wide = np.zeros((16, 3), np.float32)
    wide[1:, 0] = np.float32(2.0) ** np.arange(-20, 25, 3)[:15]
    assert knn(wide.ctypes.data_as(fp), 16, 15, i, d) == 0 and nor(wide.ctypes.data_as(fp), 16, 16, None, o, v, i) == 0
    assert np.array_equal(idx.reshape(-1)[:16 * 15].reshape(16, 15), NT.knn_twin(wide, 15)[0])
    # the handle-taking forms refuse a NULL handle before anything else
    assert lib.goicp_knn_self(None, x, 16, 3, i, d) == INVALID
    assert lib.goicp_estimate_normals(None, x, 16, 3, None, o, v, i) == INVALID


def test_header_nm_and_binding_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    for decl in (r"int goicp_knn_self_host\(const float\* xyz, size_t n, int32_t k, int32_t\* out_index, float\* out_dist_sq\);",
                 r"int goicp_knn_self\(goicp_handle h, const float\* xyz, size_t n, int32_t k, int32_t\* out_index, float\* out_dist_sq\);",
                 r"int goicp_estimate_normals_host\(const float\* xyz, size_t n, int32_t k, const float vp\[3\], float\* out_normals, float\* out_variation, int32_t\* out_index\);",
                 r"int goicp_estimate_normals\(goicp_handle h, const float\* xyz, size_t n, int32_t k, const float vp\[3\], float\* out_normals, float\* out_variation, int32_t\* out_index\);",
                 r"#define GOICP_KNN_SELF_MAX 32\b"):
        assert re.search(decl, hdr), decl
    assert re.search(r"#define GOICP_ABI_VERSION 4\b", hdr)
    from cuda_go_icp_amd import binding
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("goicp_") and " T " in l}
    assert NEW <= exported and NEW <= set(binding.SYMBOLS)
    lib = pkg.load_library()
    assert lib.goicp_abi_version() == 4
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert lib.goicp_knn_self_host.argtypes == [fp, C.c_size_t, C.c_int32, ip, fp]
    assert lib.goicp_knn_self.argtypes == [C.c_void_p, fp, C.c_size_t, C.c_int32, ip, fp]
    assert lib.goicp_estimate_normals_host.argtypes == [fp, C.c_size_t, C.c_int32, fp, fp, fp, ip]
    assert lib.goicp_estimate_normals.argtypes == [C.c_void_p, fp, C.c_size_t, C.c_int32, fp, fp, fp, ip]
    assert callable(pkg.knn_self) and callable(pkg.estimate_normals)
    assert hasattr(pkg.Registration, "knn_self") and hasattr(pkg.Registration, "estimate_normals")
    shim = open(os.path.join(ROOT, "include", "goicp_mi355.hpp")).read()
    assert "goicp_knn_self(h_" in shim and "goicp_estimate_normals(h_" in shim


def test_shim_normals_call_sites_compile():
    """tests/shim_normals.cpp, compiled as tests/shim_stat_outlier.cpp is: syntax only"""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_normals.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_estimate_normals_refusals_before_any_device(pkg, tmp_path):
    """exit status 2 with the reason; the input named does not exist, so a run that got as far as loading it would end with status 1"""
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    src, out = str(tmp_path / "missing.txt"), str(tmp_path / "out.ply")
    for args, word in ((["--ranks", "2"], "--ranks"), (["--ranks", "1"], "--ranks"), (["--normal-k", "2"], "--normal-k"), (["--normal-k", "33"], "--normal-k"),
                       (["--normal-k", "k"], "--normal-k"), (["--normal-k"], "--normal-k"), (["--viewpoint", "1,2"], "--viewpoint"),
                       (["--viewpoint", "1,2,nan"], "--viewpoint"), (["--viewpoint", "1,2,3,4"], "--viewpoint"), (["--voxel", "0.1"], "--voxel")):
        r = subprocess.run([exe, "--estimate-normals", src, out] + args, capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([exe, "--estimate-normals", src], capture_output=True, text=True)
    assert r.returncode == 2 and "IN and OUT" in r.stderr
    r = subprocess.run([exe, "--ranks", "2", "--estimate-normals", src, out], capture_output=True, text=True)
    assert r.returncode == 2 and "--ranks" in r.stderr
    assert not os.path.exists(out)


def test_cli_estimate_normals_writes_the_host_functions_bits(pkg, tmp_path):
    """goicp_cli --estimate-normals on a golden cloud, wherever it runs (the device when there is one, the host otherwise: the same bits):
    the PLY parsed back is the cloud with the host function's normals and variation (%.9g round-trips a float)"""
    pts = cloud("data_bunny")[:1500]
    with open(tmp_path / "scan.txt", "w") as f:
        f.write("%d\n" % len(pts))
        for q in pts:
            f.write("%.9g %.9g %.9g\n" % tuple(q))
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    out = tmp_path / "normals.ply"
    r = subprocess.run([exe, "--estimate-normals", str(tmp_path / "scan.txt"), str(out), "--viewpoint", "0,0,10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "estimate normals: 1500 points, k 16" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = out.read_text().splitlines()
    end = lines.index("end_header")
    assert [l.split()[2] for l in lines[:end] if l.startswith("property")] == ["x", "y", "z", "nx", "ny", "nz", "curvature"]
    body = np.array([l.split() for l in lines[end + 1:]], np.float64).astype(np.float32)
    wn, wv, _ = pkg.estimate_normals(pts, 16, np.float32([0, 0, 10]))
    assert body.shape == (1500, 7) and NT.same_bits(body[:, :3], pts) and NT.same_bits(body[:, 3:6], wn) and NT.same_bits(body[:, 6], wv)


@pytest.mark.parametrize("target", ["knn-asan", "knn-tsan"])
def test_knn_selftest_under_the_sanitizers(target):
    """csrc/knn_selftest.cpp: the host functions against all pairs, the threaded path from 65 536 points included, built with
    -fsanitize=address,undefined / -fsanitize=thread and run as a program of its own"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cuda-go-icp_amd", "csrc"), target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "knn selftest ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
