"""goicp_debug_source_order: the DEVICE ordering that goicp_set_source uses (kdbuild.hip launch_source_order: one radix sort per axis, then
level-by-level flag / scan / stable partition inside every run) equals goicp_source_order_host element for element -- same sizes and
degenerate clouds as tests/test_source_order_host.py (which holds the host function to an independent Python twin), modes 0, 1 and 2.  The
handle only lends its device and stream: one small one serves every case."""
import numpy as np
import pytest

from conftest import load_pkg
from test_source_order_host import KINDS, SIZES, make_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def reg(pkg):
    from cuda_go_icp_amd import synth
    tgt, src, _, _ = synth.make_pair(seed=11, M=300, N=40, noise=0.0)
    r = pkg.Registration(tgt, src, 1e-3, dt_size=32)
    yield r
    r.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_device_order_equals_host_order(pkg, reg, kind, n):
    xyz = make_cloud(kind, n)
    for mode in (0, 1, 2):
        dev = reg.debug_source_order(xyz, mode)
        host = pkg.source_order(xyz, mode)
        assert np.array_equal(np.sort(dev), np.arange(n)), (kind, n, mode)       # a permutation
        bad = np.flatnonzero(dev != host)
        assert bad.size == 0, (kind, n, mode, bad[:8], dev[bad[:8]], host[bad[:8]])


def test_handle_untouched_and_refusals(pkg, reg):
    """the test hook changes nothing on the handle; a bad mode, a NaN, n = 0 are refused"""
    import ctypes as C
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    before = reg.transform_source(I, z).copy()
    reg.debug_source_order(make_cloud("random", 1000), 2)
    assert np.array_equal(reg.transform_source(I, z), before) and reg.ns == 40
    lib = pkg.load_library()
    xyz = make_cloud("random", 16)
    perm = np.full(16, -7, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    x, p = xyz.ctypes.data_as(fp), perm.ctypes.data_as(ip)
    assert lib.goicp_debug_source_order(reg.handle, x, 16, 3, p) == -1
    assert lib.goicp_debug_source_order(reg.handle, x, 0, 2, p) == -1
    bad = xyz.copy(); bad[5, 1] = np.nan
    assert lib.goicp_debug_source_order(reg.handle, bad.ctypes.data_as(fp), 16, 2, p) == -1
    assert np.all(perm == -7)
