"""goicp_information_decompose: the host finishing step of the pose information -- cyclic Jacobi eigen-decomposition of a
symmetric 6x6, rank = the eigenvalues > rank_tol * lambda_max, pseudo-inverse over the retained ones.  No GPU: the function takes no handle.

Tolerances (derived, not tuned).  eps = np.finfo(float).eps = 2^-52.
  eigenvalues:  Jacobi and LAPACK's eigh are both backward stable: each returns the exact eigenvalues of A + dA with |dA| <= p(n) eps |A|_2,
                and eigenvalues of symmetric matrices move by at most |dA|_2 (Weyl).  With n = 6 and p(n) = n^2 for either side:
                    |lambda - lambda_ref| <= 2 * 36 * eps * |A|_2
  pinv:         for a perturbation that keeps the rank, |pinv(A + dA) - pinv(A)|_2 <= 3 |pinv(A)|_2^2 |dA|_2 (Wedin), i.e. relative to |pinv(A)|_2
                it is 3 * cond_r * |dA|_2 / |A|_2 with cond_r = lambda_max / (smallest RETAINED eigenvalue):
                    |P - P_ref|_2 <= 3 * cond_r * (2 * 36 * eps) * |P_ref|_2
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_pkg

EPS = np.finfo(np.float64).eps
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _raw(pkg, A, rank_tol):
    A = np.ascontiguousarray(A, np.float64).reshape(36)
    eig, vec, pinv, rank = np.empty(6), np.empty(36), np.empty(36), C.c_int32(-7)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = pkg.load_library().goicp_information_decompose(dp(A), float(rank_tol), dp(eig), dp(vec), dp(pinv), C.byref(rank))
    return rc, eig, vec.reshape(6, 6), pinv.reshape(6, 6), rank.value


def eig_tol(A):
    return 2 * 36 * EPS * np.linalg.norm(A, 2)


def pinv_tol(lam_ref, rank_tol, P_ref):
    kept = lam_ref[lam_ref > rank_tol * lam_ref.max()]
    cond_r = kept.max() / kept.min()
    return 3 * cond_r * 2 * 36 * EPS * np.linalg.norm(P_ref, 2)


def _check(pkg, A, rank_tol):
    rc, eig, vec, pinv, rank = _raw(pkg, A, rank_tol)
    assert rc == 0
    lam_ref = np.linalg.eigh(A)[0]
    P_ref = np.linalg.pinv(A, rcond=rank_tol, hermitian=True)
    e_err, e_tol = float(np.abs(eig - lam_ref).max()), eig_tol(A)
    p_err, p_tol = float(np.linalg.norm(pinv - P_ref, 2)), pinv_tol(lam_ref, rank_tol, P_ref)
    print("eig err %.3e (bar %.3e)  pinv err %.3e (bar %.3e)  rank %d" % (e_err, e_tol, p_err, p_tol, rank))
    assert np.all(np.diff(eig) >= 0), eig
    assert e_err <= e_tol
    assert rank == int((lam_ref > rank_tol * lam_ref.max()).sum())
    assert p_err <= p_tol
    # rows of vec are orthonormal eigenvectors: V^T diag(eig) V rebuilds A
    assert np.abs(vec @ vec.T - np.eye(6)).max() <= 36 * EPS
    assert np.linalg.norm(vec.T @ np.diag(eig) @ vec - A, 2) <= e_tol
    return eig, vec, pinv, rank


@pytest.mark.parametrize("seed", range(8))
def test_random_spd(pkg, seed):
    rng = np.random.default_rng(100 + seed)
    G = rng.normal(size=(6, 6 + seed))
    A = G @ G.T * 10.0 ** rng.integers(-3, 4)
    eig, vec, pinv, rank = _check(pkg, A, 1e-12)
    assert rank == 6


def test_random_spd_through_python_wrapper(pkg):
    rng = np.random.default_rng(7)
    G = rng.normal(size=(6, 9))
    A = G @ G.T
    eig, vec, pinv, rank = pkg.fgoicp.information_decompose(A, 1e-9)
    assert rank == 6 and np.abs(eig - np.linalg.eigh(A)[0]).max() <= eig_tol(A)
    assert np.linalg.norm(pinv - np.linalg.inv(A), 2) <= pinv_tol(eig, 1e-9, np.linalg.inv(A))


def test_half_rank_diagonal(pkg):
    A = np.diag([0.0, 0, 0, 1, 1, 1])
    rc, eig, vec, pinv, rank = _raw(pkg, A, 1e-6)
    assert rc == 0 and rank == 3
    assert np.array_equal(eig, [0, 0, 0, 1, 1, 1])
    assert np.array_equal(pinv, A)                      # a diagonal input is never rotated: exact


def test_zero_matrix(pkg):
    rc, eig, vec, pinv, rank = _raw(pkg, np.zeros((6, 6)), 1e-6)
    assert rc == 0 and rank == 0
    assert np.array_equal(eig, np.zeros(6)) and np.array_equal(pinv, np.zeros((6, 6)))
    rc, eig, vec, pinv, rank = _raw(pkg, np.zeros((6, 6)), 0.0)
    assert rc == 0 and rank == 0 and np.array_equal(pinv, np.zeros((6, 6)))


@pytest.mark.parametrize("where,kept", [("at", False), ("above", True), ("below", False)])
def test_eigenvalue_at_the_threshold(pkg, where, kept):
    """rank counts the eigenvalues STRICTLY above rank_tol * lambda_max.  Diagonal input, powers of two: every number here is exact."""
    tol, lmax = 2.0 ** -10, 8.0
    thr = tol * lmax
    x = {"at": thr, "above": np.nextafter(thr, 1.0), "below": np.nextafter(thr, 0.0)}[where]
    A = np.diag([lmax, 1.0, x, 2.0, 4.0, 0.5])
    rc, eig, vec, pinv, rank = _raw(pkg, A, tol)
    assert rc == 0 and rank == (6 if kept else 5)
    want = np.diag([1 / lmax, 1.0, 1 / x if kept else 0.0, 0.5, 0.25, 2.0])
    assert np.array_equal(pinv, want)
    assert np.array_equal(eig, np.sort(np.diag(A)))
    # the same rule as numpy's cutoff
    assert np.array_equal(np.linalg.pinv(A, rcond=tol, hermitian=True) != 0, want != 0)


def test_rotated_rank_deficient(pkg):
    """a rank-4 matrix in a random basis: the two null eigenvalues come out at rounding level and are dropped"""
    rng = np.random.default_rng(5)
    Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
    A = Q @ np.diag([0, 0, 1.0, 2.0, 3.0, 50.0]) @ Q.T
    A = 0.5 * (A + A.T)
    eig, vec, pinv, rank = _check(pkg, A, 1e-9)
    assert rank == 4


def test_refusals(pkg):
    lib = pkg.load_library()
    A = np.eye(6)
    A[2, 3] = np.nan
    rc = _raw(pkg, A, 1e-6)[0]
    assert rc == INVALID and b"non-finite" in lib.goicp_last_error()
    A[2, 3] = np.inf
    assert _raw(pkg, A, 1e-6)[0] == INVALID
    for bad in (-1e-3, 1.0, 2.0, float("nan")):
        rc = _raw(pkg, np.eye(6), bad)[0]
        assert rc == INVALID and b"rank_tol" in lib.goicp_last_error(), bad
    assert _raw(pkg, np.eye(6), 0.0)[0] == 0
    with pytest.raises(pkg.GoicpError):
        pkg.fgoicp.information_decompose(np.eye(6), 1.5)


def test_structs_and_defaults(pkg):
    from cuda_go_icp_amd import binding as B
    assert C.sizeof(B.CPoseInfoOptions) == 40
    assert C.sizeof(B.CPoseInfo) == (36 + 6 + 36 + 6 + 36 + 3 + 4) * 8 + 8 + 3 * 4 + 4
    o = B.CPoseInfoOptions(5, 5, (1.0, 2.0, 3.0), 0.5)
    pkg.load_library().goicp_pose_info_options_default(C.byref(o))
    assert (o.metric, o.use_pivot, list(o.pivot), o.rank_tol) == (-1, 0, [0.0, 0.0, 0.0], 1e-6)
    assert pkg.load_library().goicp_abi_version() == 4
