"""Robust-kernel ICP (goicp_set_icp_robust): Huber, Cauchy, Geman-McClure and Tukey weights on every correspondence of every iteration.

What is held here, on the committed clouds and on the seeded clutter case of tests/test_gpu_icp_gate.py (the bunny model as target; every
7th model point + noise, moved by 10 degrees and (0.02, -0.015, 0.01), plus 30 % clutter as source; 6 676 points): identity with the plain
run while every weight is 1, the fp64 numpy twin of tests/test_icp_robust_host.py (both metrics), robustness against clutter, a too-small
scale being visible in the weight sum, the batch, reproducibility, the refusals, and the kernel inside goicp_register and the collective
loop.  Every test needs the entry points this feature adds.

Bars: the project's own for ICP against its oracle: 1e-4 absolute on R, t after 1 / 2 / 10 iterations, 1e-3 converged."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import cloud, golden, load_pkg, rot_angle, skull_problem
from test_gpu_icp_gate import _rodrigues, _run, _same, clutter_case
from test_icp_robust_host import CAUCHY, GM, HUBER, NAMES, TUKEY, twin_icp

pytestmark = pytest.mark.gpu
INVALID = -1
# the kernels and scales of the CPU table
TABLE = [(HUBER, 0.05), (HUBER, 0.01), (HUBER, 0.002), (CAUCHY, 0.05), (CAUCHY, 0.01), (GM, 0.05), (TUKEY, 0.15), (TUKEY, 0.05)]
TWIN_CASES = [(HUBER, 0.05), (HUBER, 0.01), (CAUCHY, 0.05), (CAUCHY, 0.01), (GM, 0.05), (TUKEY, 0.15), (TUKEY, 0.05)]
PLANE_TWIN_CASES = [(HUBER, 0.05), (TUKEY, 0.15)]


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def clutter(pkg):
    from scipy.spatial import cKDTree
    tgt, src, Rt, tt = clutter_case()
    reg = pkg.Registration(tgt, src, 1e-3)
    yield reg, tgt, src, Rt, tt, cKDTree(tgt.astype(np.float64))
    reg.close()


def _stats(reg, K=1):
    c, w = reg.icp_robust_stats(K)
    return (c[0], w[0]) if K == 1 else (c, w)


# ----------------------------------------------------------------------------------------------
# 1. identity
# ----------------------------------------------------------------------------------------------
def _pairs():
    skull_t, skull_s, _, _ = skull_problem()
    return {"bunny": (cloud("model_bunny"), cloud("data_bunny")), "skull": (skull_t, skull_s),
            "spanner": (cloud("spanner_target"), cloud("spanner_source"))}


@pytest.mark.parametrize("name", ["bunny", "skull", "spanner"])
def test_identity_while_every_weight_is_one(pkg, name):
    tgt, src = _pairs()[name]
    extent = float(max((tgt.max(0) - tgt.min(0)).max(), (src.max(0) - src.min(0)).max()))
    reg = pkg.Registration(tgt, src, 1e-3)
    try:
        for metric in (0, 1):
            reg.set_icp_options(metric, 16)
            for max_iter in (3, 60):
                reg.set_icp_robust(0)
                ref = _run(reg, max_iter=max_iter)
                reg.set_icp_robust(HUBER, 10 * extent)
                out = _run(reg, max_iter=max_iter)
                cost, W = _stats(reg)
                print("%s metric %d max_iter %d: iters %d err %.7g cost %.7g W %.1f" % (name, metric, max_iter, out[3], out[2], cost, W))
                assert _same(out, ref), (name, metric, max_iter, out[2:], ref[2:])
                assert float(W) == float(len(src))
                assert abs(float(cost) - float(out[2])) <= 1e-5 * float(out[2])
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 2. twin
# ----------------------------------------------------------------------------------------------
def _against_twin(reg, tgt, src, tree, kernel, c, normals):
    for max_iter, tol in ((1, 1e-4), (2, 1e-4), (10, 1e-4), (10000, 1e-3)):
        R, t, err, it = _run(reg, max_iter=max_iter)
        cost, W = _stats(reg)
        tR, tt_, terr, tit, tW, tC = twin_icp(tree, tgt, src, kernel, c, max_iter, normals=normals)
        dR, dt = float(np.abs(R - tR).max()), float(np.abs(t - tt_).max())
        print("%s c %.3g metric %d max_iter %5d: |dR| %.2e |dt| %.2e (bar %.0e); iters %d / twin %d; W %.2f / twin %.2f; C %.6g / twin %.6g; "
              "err %.6g / twin %.6g" % (NAMES[kernel], c, 0 if normals is None else 1, max_iter, dR, dt, tol, it, tit, W, tW, cost, tC, err, terr))
        assert dR <= tol and dt <= tol, (kernel, c, max_iter, dR, dt)
        assert abs(float(W) - tW) <= 1e-3 * tW, (kernel, c, max_iter, W, tW)
        if max_iter <= 10:
            assert it == tit, (kernel, c, max_iter, it, tit)


@pytest.mark.parametrize("kernel,c", TWIN_CASES)
def test_twin(pkg, clutter, kernel, c):
    reg, tgt, src, Rt, tt, tree = clutter
    reg.set_icp_options(0, 16)
    reg.set_icp_robust(kernel, c)
    try:
        _against_twin(reg, tgt, src, tree, kernel, c, None)
    finally:
        reg.set_icp_robust(0)


@pytest.mark.parametrize("kernel,c", PLANE_TWIN_CASES)
def test_twin_point_to_plane(pkg, clutter, kernel, c):
    reg, tgt, src, Rt, tt, tree = clutter
    reg.set_icp_options(1, 16)
    reg.set_icp_robust(kernel, c)
    try:
        _against_twin(reg, tgt, src, tree, kernel, c, reg.target_normals())
    finally:
        reg.set_icp_robust(0)
        reg.set_icp_options(0, 16)


# ----------------------------------------------------------------------------------------------
# 3. robustness, 4. a too-small scale
# ----------------------------------------------------------------------------------------------
def test_robust_to_clutter(pkg, clutter):
    reg, tgt, src, Rt, tt, tree = clutter
    reg.set_icp_options(0, 16)
    reg.set_icp_robust(0)
    R0, t0, _, it0 = _run(reg)
    ang0, d0 = rot_angle(R0, Rt), float(np.linalg.norm(t0 - tt))
    print("plain: %.3e rad / %.3e from the truth, %d iterations" % (ang0, d0, it0))
    try:
        for kernel, c in TABLE:
            reg.set_icp_robust(kernel, c)
            R, t, _, it = _run(reg)
            tR, tt_, _, tit, _, _ = twin_icp(tree, tgt, src, kernel, c, 10000)
            ang, d = rot_angle(R, Rt), float(np.linalg.norm(t - tt))
            tang, td = rot_angle(tR, Rt), float(np.linalg.norm(tt_ - tt))
            print("%s c %.3g: %.3e rad / %.3e from the truth, %d iterations (twin %.3e / %.3e, %d)" % (NAMES[kernel], c, ang, d, it, tang, td, tit))
            # within the twin's distance of the truth plus the converged bar (1e-3 per element: 3e-3 as a rotation's chord, sqrt(3) e-3 as a vector)
            assert ang <= tang + 3e-3 and d <= td + np.sqrt(3) * 1e-3, (kernel, c, ang, tang, d, td)
            assert ang0 >= 10 * ang and d0 >= 10 * d, (kernel, c, ang0, ang, d0, d)
    finally:
        reg.set_icp_robust(0)


def test_too_small_scale_is_reported(pkg, clutter):
    """Tukey with a scale far below the residuals at the start pose: almost no weight, the loop stops near the start -- status OK, and the
    weight sum says so (the twin: W = 1 171 of 6 676)"""
    reg, tgt, src, Rt, tt, tree = clutter
    reg.set_icp_options(0, 16)
    reg.set_icp_robust(TUKEY, 0.02)
    try:
        R, t, err, it = _run(reg)                                    # status GOICP_OK (asserted in _run)
        cost, W = _stats(reg)
        tW = twin_icp(tree, tgt, src, TUKEY, 0.02, 10000)[4]
        print("tukey 0.02: %d iterations, W %.1f of %d (twin %.1f), cost %.6g, err %.6g" % (it, W, len(src), tW, cost, err))
        assert it <= 10
        assert 0 < float(W) < 0.25 * len(src)
    finally:
        reg.set_icp_robust(0)


# ----------------------------------------------------------------------------------------------
# 5. batch
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_batch_equals_single_runs(pkg, clutter, metric):
    reg = clutter[0]
    rng = np.random.default_rng(5)
    R0 = np.array([_rodrigues(rng.normal(size=3) * (0.12 if k < 4 else 0.9)) for k in range(8)], np.float32)
    t0 = np.array([rng.uniform(-1, 1, 3) * (0.04 if k < 4 else 0.3) for k in range(8)], np.float32)
    R0[0], t0[0] = np.eye(3), 0
    reg.set_icp_options(metric, 16)
    reg.set_icp_robust(CAUCHY, 0.05)
    try:
        R, t, err, it = reg.icp_run_batch(R0, t0, 200, 1e-7)
        bc, bw = reg.icp_robust_stats(8)
        with pytest.raises(pkg.GoicpError):
            reg.icp_robust_stats(7)                                  # K must be the last run's
        for k in range(8):
            sR, st, se, si = _run(reg, R0[k], t0[k], 200, 1e-7)
            assert np.array_equal(R[k], sR) and np.array_equal(t[k], st) and err[k] == se and it[k] == si, (metric, k)
            sc, sw = _stats(reg)
            assert sc.tobytes() == bc[k].tobytes() and sw.tobytes() == bw[k].tobytes(), (metric, k, sc, bc[k], sw, bw[k])
        print("batch metric %d: W %s iters %s" % (metric, np.round(bw, 1).tolist(), it.tolist()))
        assert len(set(bw.tolist())) > 1                             # starts that end in different places are among them
    finally:
        reg.set_icp_robust(0)
        reg.set_icp_options(0, 16)


# ----------------------------------------------------------------------------------------------
# 6. reproducibility
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_reproducible(pkg, clutter, metric):
    reg = clutter[0]
    reg.set_icp_options(metric, 16)
    try:
        for kernel, c in TWIN_CASES:
            outs = []
            for _ in range(2):
                reg.set_icp_robust(kernel, c)
                outs.append(_run(reg, max_iter=300) + _stats(reg))
            assert _same(outs[0], outs[1]), (metric, kernel, c, [o[2:] for o in outs])
    finally:
        reg.set_icp_robust(0)
        reg.set_icp_options(0, 16)


def test_million_points_reproducible(pkg):
    """S2 (N = M = 1 M: the neighbour pass, a three-level tree): the same robust run twice, bit-equal, both metrics"""
    from cuda_go_icp_amd import synth
    model, data, Rgt, tgt = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"])
    reg = pkg.Registration(model, data, 1e-3, dt_size=synth.S2["V"])
    try:
        R0, t0 = _rodrigues([0.02, -0.03, 0.01]) @ Rgt, tgt + np.array([0.01, -0.02, 0.015])
        for metric in (0, 1):
            reg.set_icp_options(metric, 16)
            for kernel, c in ((CAUCHY, 0.03), (TUKEY, 0.05)):
                reg.set_icp_robust(kernel, c)
                outs = [_run(reg, R0, t0, max_iter=4) + _stats(reg) for _ in range(2)]
                print("1 M points metric %d %s: err %.7g W %.1f of %d" % (metric, NAMES[kernel], outs[0][2], outs[0][5], len(data)))
                assert _same(outs[0], outs[1]), (metric, kernel, [o[2:] for o in outs])
                assert 0 < float(outs[0][5]) < len(data)
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 7. refusals
# ----------------------------------------------------------------------------------------------
def _set(reg, kernel, scale):
    r = reg._lib.goicp_set_icp_robust.argtypes[1]._type_(kernel, scale)
    return reg._lib.goicp_set_icp_robust(reg.handle, C.byref(r))


def test_refusals(pkg):
    model, data = cloud("model_bunny"), cloud("data_bunny", 10)
    reg = pkg.Registration(model, data, 1e-3)
    lib = reg._lib
    plain = _run(reg, max_iter=20)
    for bad in (-1, 5, 99):
        assert _set(reg, bad, 0.1) == INVALID and b"kernel" in lib.goicp_last_error()
    for bad in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert _set(reg, HUBER, bad) == INVALID and b"scale" in lib.goicp_last_error()
    assert _set(reg, 0, float("nan")) == 0                          # off: the scale is not looked at
    # a kernel and a gate, in either order
    reg.set_icp_gate(0.1)
    assert _set(reg, CAUCHY, 0.05) == INVALID and b"gate" in lib.goicp_last_error()
    reg.set_icp_gate(0.0)
    assert _set(reg, CAUCHY, 0.05) == 0
    with pytest.raises(pkg.GoicpError) as e:
        reg.set_icp_gate(0.1)
    assert e.value.code == INVALID and "robust" in str(e.value)
    # the stats belong to the last run
    _run(reg, max_iter=2)
    f = np.zeros(4, np.float32)
    fp = f.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.goicp_icp_robust_stats(reg.handle, 2, fp, fp) == INVALID and b"K must be" in lib.goicp_last_error()
    assert lib.goicp_icp_robust_stats(reg.handle, 1, fp, None) == 0 and f[0] > 0
    # kernel 0 restores the plain run, bit for bit
    assert not _same(_run(reg, max_iter=20), plain)
    assert _set(reg, 0, 0.0) == 0
    assert _same(_run(reg, max_iter=20), plain)
    reg.close()
    trimmed = pkg.Registration(model, data, 1e-3, trim_fraction=0.1)
    assert _set(trimmed, HUBER, 0.1) == INVALID and b"trim" in lib.goicp_last_error() and _set(trimmed, 0, 0.0) == 0
    trimmed.close()
    linear = pkg.Registration(model, data, 1e-3, dt_layout=0, dt_size=96)
    assert _set(linear, HUBER, 0.1) == INVALID and b"dt_layout" in lib.goicp_last_error()
    linear.close()
    fused = pkg.Registration(model, data, 1e-3, icp_fused=1)
    assert _set(fused, HUBER, 0.1) == INVALID and b"icp_fused" in lib.goicp_last_error()
    fused.close()
    with pytest.raises(pkg.GoicpError):
        pkg.Registration(model, data, 1e-3, trim_fraction=0.1, robust_kernel=HUBER, robust_scale=0.1)
    # during a registration: from the progress callback, on the registering thread
    eng = pkg.FastGoICP(model, data, 1e-3)
    rcs, msgs = [], []

    def during(r, u):
        rcs.append(_set(eng.registration, HUBER, 0.1))
        msgs.append(lib.goicp_last_error())
    CB = C.CFUNCTYPE(None, C.POINTER(pkg.binding.CResult), C.c_void_p)
    cb = CB(during)
    pkg.binding.check(lib.goicp_set_progress_callback(eng.registration.handle, C.cast(cb, C.c_void_p), None))
    th = threading.Thread(target=eng.run)
    th.start(); th.join()
    pkg.binding.check(lib.goicp_set_progress_callback(eng.registration.handle, None, None))
    assert rcs and all(rc == INVALID for rc in rcs) and all(b"registration runs" in m for m in msgs)
    assert _set(eng.registration, HUBER, 0.1) == 0
    eng.registration.close()


# ----------------------------------------------------------------------------------------------
# 8. registration, 9. collective loop
# ----------------------------------------------------------------------------------------------
def test_register_with_unit_weights_equals_plain(pkg):
    model, data = cloud("model_bunny"), cloud("data_bunny")
    g = golden("e2e_bunny_full")
    extent = float(max((model.max(0) - model.min(0)).max(), (data.max(0) - data.min(0)).max()))
    a = pkg.FastGoICP(model, data, g["mse_threshold"])
    b = pkg.FastGoICP(model, data, g["mse_threshold"], robust_kernel=HUBER, robust_scale=10 * extent)
    try:
        a.run(); b.run()
        ra, rb = a.registration.poll(), b.registration.poll()
        assert a.finished and b.finished
        assert bytes(ra.optR) == bytes(rb.optR) and bytes(ra.optT) == bytes(rb.optT)
        assert np.float32(ra.best_sse).tobytes() == np.float32(rb.best_sse).tobytes()
        assert bytes(ra.counters) == bytes(rb.counters)
        assert b.counters.icp_runs > 0
    finally:
        a.registration.close()
        b.registration.close()


def test_collective_robust(pkg):
    from cuda_go_icp_amd import sharded
    tgt, src, _, _ = clutter_case()
    R0, t0 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    regs = [pkg.Registration(tgt, src, 1e-3) for _ in range(2)]
    try:
        regs[0].set_icp_robust(CAUCHY, 0.05)
        out = sharded.icp_run_thread_ranks(regs, R0, t0, raise_on_error=False)      # one rank robust, one not
        assert [o[0] for o in out] == [INVALID, INVALID]
        regs[1].set_icp_robust(CAUCHY, 0.02)
        out = sharded.icp_run_thread_ranks(regs, R0, t0, raise_on_error=False)      # different scales
        assert [o[0] for o in out] == [INVALID, INVALID]
        regs[1].set_icp_robust(GM, 0.05)
        out = sharded.icp_run_thread_ranks(regs, R0, t0, raise_on_error=False)      # different kernels
        assert [o[0] for o in out] == [INVALID, INVALID]
        regs[1].set_icp_robust(CAUCHY, 0.05)
        ref = _run(regs[0], R0, t0)
        w1 = sharded.icp_run_thread_ranks(regs[:1], R0, t0)[0]
        assert w1[0] == 0 and _same((w1[2], w1[3], w1[1], w1[4]), ref)
        for rc, e, R, t, it in sharded.icp_run_thread_ranks(regs, R0, t0):
            assert rc == 0 and _same((R, t, e, it), ref)
        assert regs[0].icp_shard_stats()["sliced"] == 0                            # replicated, as point-to-plane and the gate
    finally:
        for r in regs:
            r.close()
