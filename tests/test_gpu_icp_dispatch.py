"""The opt-in ICP iteration's dispatch cells that no other test compares directly: the batch under a gate and under a robust kernel, either metric,
on both sides of the strided switch.  In every cell a batch of three starts, two of them equal, is run for 1 and for 5 iterations and must
equal three single goicp_icp_run calls bit for bit -- R, t, err, iters, and slot by slot goicp_icp_inliers and goicp_icp_robust_stats.

Case: test_gpu_small_shapes' (target of 2 000 points, dt_size 32, far points appended).  N = 5: one ragged workgroup, below point-to-plane's
floor of 6 (the gated / robust loop leaves the pose); N = 65 in input order with the far points of test_gated_pass_row_without_owner: a
wavefront whose rows have no owning lane under the capped walk; N = 40 001: neighbour addressing.  Modes: the data-chosen gate with the
capped and the full walk, Huber at the median neighbour distance, Tukey at 1.5 x it.  No tolerance: every comparison is of bits."""
import numpy as np
import pytest

import twins
from conftest import load_pkg
from test_gpu_icp_gate import _run
from test_gpu_small_shapes import M_ICP, _case, _reg
from test_icp_robust_host import HUBER, TUKEY

pytestmark = pytest.mark.gpu
MODES = ["gate_capped", "gate_full", "huber", "tukey"]


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _cell(N):
    if N == 65:
        return _case(M_ICP, 65, out_idx=(3, 20, 37, 54, 64)), {"morton_sort": 0}
    return _case(M_ICP, N), {}


def _bits(*xs):
    return tuple(np.asarray(x).tobytes() for x in xs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("N", [5, 65, 40001])
def test_batch_equals_single_runs(pkg, N, metric, mode):
    c, kw = _cell(N)
    reg = _reg(pkg, c, **kw)
    try:
        _, d2 = reg.nn_query(c["q"])
        d = np.sqrt(d2.astype(np.float64))
        reg.set_icp_options(metric, 8)
        if mode.startswith("gate"):
            g, margin = twins.pick_gate(d, c["out_idx"])
            assert margin >= 1e-4, (N, g, margin)
            reg.set_icp_gate(g, capped_walk=1 if mode == "gate_capped" else 0)
        else:
            med = np.median(d)
            reg.set_icp_robust(HUBER if mode == "huber" else TUKEY, float(np.float32(med if mode == "huber" else 1.5 * med)))
        R1 = (twins.rodrigues64([-0.03, 0.01, 0.02]) @ c["R0"].astype(np.float64)).astype(np.float32)
        t1 = (c["t0"] + np.array([-0.01, 0.015, 0.005], np.float32)).astype(np.float32)
        Rb, tb = np.stack([c["R0"], R1, c["R0"]]), np.stack([c["t0"], t1, c["t0"]])
        for iters in (1, 5):
            bR, bt, berr, bit = reg.icp_run_batch(Rb, tb, iters, 1e-7)
            bn = np.array(reg.icp_inliers(3))
            bcost, bW = (np.array(x) for x in reg.icp_robust_stats(3))
            for k in range(3):
                sR, st, se, si = _run(reg, Rb[k], tb[k], max_iter=iters)
                sn = reg.icp_inliers(1)
                scost, sW = reg.icp_robust_stats(1)
                tag = (N, metric, mode, iters, k)
                assert _bits(bR[k], bt[k], berr[k]) == _bits(sR, st, se) and int(bit[k]) == int(si), tag + (berr[k], se, int(bit[k]), si)
                assert int(bn[k]) == int(sn[0]), tag + (bn, sn)
                assert _bits(bcost[k], bW[k]) == _bits(scost[0], sW[0]), tag + (bcost, bW, scost, sW)
            assert _bits(bR[0], bt[0], berr[0], bit[0], bn[0], bcost[0], bW[0]) == _bits(bR[2], bt[2], berr[2], bit[2], bn[2], bcost[2], bW[2])
            print("N %d metric %d %s iters %d: err %s iters %s inliers %s W %s" % (N, metric, mode, iters, berr, bit, bn, bW))
    finally:
        reg.close()
