"""Batched multi-start ICP (goicp_icp_run_batch): every pose of a batch ends bit for bit where goicp_icp_run from the same start ends on
the same handle -- point-to-point and point-to-plane, strided and neighbour passes, every k-d tree depth -- independently of what else the
batch holds; the handle's own ICP state is left alone; the refusals.  Every test here needs the entry point this feature adds."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import cloud, golden, load_pkg, small_problem

pytestmark = pytest.mark.gpu
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def bunny(pkg):
    reg = pkg.Registration(cloud("model_bunny"), cloud("data_bunny"), 1e-3)     # N = 30 379: strided pass, kd.K = 2
    yield reg
    reg.close()


@pytest.fixture(scope="module")
def spanner(pkg):
    reg = pkg.Registration(cloud("spanner_target"), cloud("spanner_source"), 1e-3)   # N = 150 000: neighbour pass, kd.K = 3
    yield reg
    reg.close()


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _single(reg, R, t, max_iter, err_diff):
    R, t = np.array(R, np.float32).reshape(9), np.array(t, np.float32).reshape(3)
    err, it = C.c_float(), C.c_int32()
    rc = reg._lib.goicp_icp_run(reg.handle, _fptr(R), _fptr(t), int(max_iter), float(err_diff), C.byref(err), C.byref(it))
    assert rc == 0
    return R.reshape(3, 3), t, np.float32(err.value), it.value


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a) * np.deg2rad(deg)
    return _rodrigues(a)


def _rodrigues(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3, dtype=np.float32)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K).astype(np.float32)


def _starts(n_random=8, seed=0):
    """identity, 30 / 90 / 150 degree turns, a start far outside the clouds (its own fixed-point scale), seeded turns up to 90 degrees"""
    Rs = [np.eye(3, dtype=np.float32), _rot([1, 0, 0], 30), _rot([0, 1, 1], 90), _rot([1, -1, 0.5], 150), np.eye(3, dtype=np.float32)]
    ts = [np.zeros(3), np.array([0.02, -0.01, 0.0]), np.zeros(3), np.array([0.0, 0.05, -0.03]), np.array([6.0, -5.0, 4.0])]
    rng = np.random.default_rng(seed)
    for _ in range(n_random):
        Rs.append(_rot(rng.normal(size=3), rng.uniform(0, 90)))
        ts.append(rng.uniform(-0.05, 0.05, 3))
    return np.array(Rs, np.float32), np.array(ts, np.float32)


def _check_batch(reg, R0, t0, max_iter, err_diff, tag):
    R, t, err, it = reg.icp_run_batch(R0, t0, max_iter, err_diff)
    for k in range(len(R0)):
        sR, st, se, si = _single(reg, R0[k], t0[k], max_iter, err_diff)
        assert np.array_equal(R[k], sR) and np.array_equal(t[k], st), (tag, k)
        assert err[k] == se and it[k] == si, (tag, k, err[k], se, it[k], si)
    return R, t, err, it


def _golden_groups():
    g = golden("icp_iter")
    groups = {}
    for c in g["cases"]:
        groups.setdefault((c["max_iter"], c["err_diff"]), []).append((c["R0"], c["t0"]))
    return groups


@pytest.mark.parametrize("metric", [0, 1])
def test_bit_identity_bunny(pkg, bunny, metric):
    bunny.set_icp_options(metric, 16)
    try:
        R0, t0 = _starts(11)
        _, _, _, it = _check_batch(bunny, R0, t0, 10000, 1e-7, "bunny metric %d" % metric)
        assert it.max() > it.min()                       # the poses converge after different counts: the active list shrinks mid-run
        for (mi, ed), cases in _golden_groups().items():
            gR = np.array([c[0] for c in cases], np.float32).reshape(-1, 9)
            gt = np.array([c[1] for c in cases], np.float32).reshape(-1, 3)
            _check_batch(bunny, np.concatenate([gR, R0[:3].reshape(-1, 9)]), np.concatenate([gt, t0[:3]]), mi, ed, "golden %d" % mi)
    finally:
        bunny.set_icp_options(0, 16)


@pytest.mark.parametrize("metric", [0, 1])
def test_bit_identity_spanner_neighbour_pass(pkg, spanner, metric):
    spanner.set_icp_options(metric, 16)
    try:
        R0, t0 = _starts(11, seed=1)
        _check_batch(spanner, R0, t0, 60, 1e-7, "spanner metric %d" % metric)
    finally:
        spanner.set_icp_options(0, 16)


@pytest.mark.parametrize("metric", [0, 1])
def test_bit_identity_depth_one_tree(pkg, metric):
    """a 400-point target: a k-d tree of one level (kd.K = 1), which the committed clouds do not reach"""
    tgt, src, _, _ = small_problem(1)
    reg = pkg.Registration(tgt, src, 1e-3)
    try:
        reg.set_icp_options(metric, 16)
        R0, t0 = _starts(11, seed=2)
        _check_batch(reg, R0, t0, 10000, 1e-7, "small metric %d" % metric)
    finally:
        reg.close()


def test_result_independent_of_the_batch(pkg, bunny):
    R0, t0 = _starts(6, seed=3)
    Rf, tf = R0[7], t0[7]
    ref = bunny.icp_run_batch(Rf[None], tf[None], 10000, 1e-7)
    batches = [(R0, t0, 7), (R0[::-1].copy(), t0[::-1].copy(), len(R0) - 1 - 7)]
    rng = np.random.default_rng(4)
    Rb = np.array([_rot(rng.normal(size=3), rng.uniform(0, 90)) for _ in range(1024)], np.float32)
    tb = rng.uniform(-0.05, 0.05, (1024, 3)).astype(np.float32)
    copies = rng.choice(1024, 50, replace=False)
    Rb[copies], tb[copies] = Rf, tf
    Rs, ts, es, its = bunny.icp_run_batch(Rb, tb, 10000, 1e-7)
    for k in copies:
        assert np.array_equal(Rs[k], ref[0][0]) and np.array_equal(ts[k], ref[1][0]) and es[k] == ref[2][0] and its[k] == ref[3][0]
    for R, t, k in batches:
        out = bunny.icp_run_batch(R, t, 10000, 1e-7)
        assert all(np.array_equal(out[j][k], ref[j][0]) for j in range(4))
    sR, st, se, si = _single(bunny, Rf, tf, 10000, 1e-7)
    assert np.array_equal(ref[0][0], sR) and np.array_equal(ref[1][0], st) and ref[2][0] == se and ref[3][0] == si


def test_mixed_convergence_and_iteration_limits(pkg, bunny):
    R0, t0 = _starts(3, seed=5)
    # a pose that converges at once (the optimum of a full run) beside poses that need hundreds of iterations
    Ropt, topt, _, _ = _single(bunny, R0[2], t0[2], 10000, 1e-7)
    R = np.concatenate([Ropt[None], R0]); t = np.concatenate([topt[None], t0])
    _, _, _, it = _check_batch(bunny, R, t, 10000, 1e-7, "mixed")
    assert it[0] <= 1 and it.max() >= 30
    # max_iter = 0: the inputs unchanged, iters 0, the err goicp_icp_run reports at 0
    Rz, tz, ez, iz = _check_batch(bunny, R, t, 0, 1e-7, "max_iter 0")
    assert np.array_equal(Rz, R) and np.array_equal(tz, t) and not iz.any()
    _check_batch(bunny, R, t, 1, 1e-7, "max_iter 1")
    _check_batch(bunny, R, t, 23, 1e-7, "max_iter 23")                # below the convergence point, not a multiple of the chunk


def test_counters_and_handle_state_unchanged(pkg):
    model, data = cloud("model_bunny"), cloud("data_bunny", 10)
    a = pkg.Registration(model, data, 1e-3)
    b = pkg.Registration(model, data, 1e-3)
    try:
        for _ in range(5):
            a.icp_step(); b.icp_step()
        snap = a.poll()
        c0 = (snap.counters.icp_runs, snap.counters.icp_iters)
        R0, t0 = _starts(4, seed=6)
        _, _, _, it = a.icp_run_batch(R0, t0, 10000, 1e-7)
        snap2 = a.poll()
        assert list(snap2.curR) == list(snap.curR) and list(snap2.curT) == list(snap.curT) and list(snap2.optR) == list(snap.optR)
        for _ in range(5):
            ra = a.icp_step(); rb = b.icp_step()
        assert list(ra.curR) == list(rb.curR) and list(ra.curT) == list(rb.curT)
        assert ra.counters.icp_runs - rb.counters.icp_runs == len(R0)
        assert ra.counters.icp_iters - rb.counters.icp_iters >= int(it.sum())
        assert (snap2.counters.icp_runs, snap2.counters.icp_iters) == c0 and snap2.best_sse == snap.best_sse   # the poll snapshot untouched
    finally:
        a.close(); b.close()
    # a registration after a batch equals one on a fresh handle
    e1 = pkg.FastGoICP(model, data, 1e-3)
    e2 = pkg.FastGoICP(model, data, 1e-3)
    try:
        e1.registration.icp_run_batch(R0, t0, 10000, 1e-7)
        e1.run(); e2.run()
        assert np.array_equal(e1.optR, e2.optR) and np.array_equal(e1.optT, e2.optT) and e1.get_best_error() == e2.get_best_error()
        c1, c2 = e1.counters, e2.counters
        for f in ("rot_pops", "trans_pops", "cubes", "inner_calls", "bounds_launches"):
            assert getattr(c1, f) == getattr(c2, f), f
    finally:
        e1.registration.close(); e2.registration.close()


def _call(reg, K, R=True, t=True, max_iter=10):
    lib = reg._lib
    Rb = np.tile(np.eye(3, dtype=np.float32).reshape(9), max(K, 1))
    tb = np.zeros(3 * max(K, 1), np.float32)
    return lib.goicp_icp_run_batch(reg.handle, K, _fptr(Rb) if R else None, _fptr(tb) if t else None, max_iter, 1e-7, None, None)


def test_refusals(pkg, bunny):
    lib = bunny._lib
    assert _call(bunny, 0) == INVALID and _call(bunny, 1025) == INVALID
    assert _call(bunny, 2, R=False) == INVALID and _call(bunny, 2, t=False) == INVALID and _call(bunny, 2, max_iter=-1) == INVALID
    assert _call(bunny, 1024, max_iter=0) == 0
    model, data = cloud("model_bunny"), cloud("data_bunny", 10)
    trimmed = pkg.Registration(model, data, 1e-3, trim_fraction=0.1)
    assert _call(trimmed, 2) == INVALID and b"trim" in lib.goicp_last_error()
    trimmed.close()
    linear = pkg.Registration(model, data, 1e-3, dt_layout=0, dt_size=96)
    assert _call(linear, 2) == INVALID and b"dt_layout" in lib.goicp_last_error()
    linear.set_icp_options(1, 16)                          # point-to-plane has its fixed-point pass in either layout
    assert _call(linear, 2) == 0
    linear.close()
    # during a registration: from the progress callback, on the registering thread
    eng = pkg.FastGoICP(model, data, 1e-3)
    rcs = []
    CB = C.CFUNCTYPE(None, C.POINTER(pkg.binding.CResult), C.c_void_p)
    cb = CB(lambda r, u: rcs.append(_call(eng.registration, 2)))
    pkg.binding.check(lib.goicp_set_progress_callback(eng.registration.handle, C.cast(cb, C.c_void_p), None))
    th = threading.Thread(target=eng.run)
    th.start(); th.join()
    pkg.binding.check(lib.goicp_set_progress_callback(eng.registration.handle, None, None))
    assert rcs and all(rc == INVALID for rc in rcs)
    assert _call(eng.registration, 2) == 0                  # and accepted again once it has ended
    eng.registration.close()
