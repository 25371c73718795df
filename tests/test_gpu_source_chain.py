"""The staged source swap (Engine::set_source_staged) behind its four entry points, over every set of stages.

goicp_set_source_voxel, _filtered, _pipeline and _clustered fill one record of stages (voxel grid, statistical filter, radius filter,
cluster selection; a size of 0 switches a stage off) and run one chain.  The first stage that runs takes its frame from the host's walk
over the raw cloud, every later one from the bounds of its input on the device, so each of the 16 subsets takes a path of its own: all
of them are held here against goicp_set_source of the composition of the host functions, through every entry point that can express
them, on one live handle (growing and shrinking swaps in turn).  The three subsets that start behind the voxel grid and end in the
cluster stage get the full fingerprint of tests/test_gpu_voxel_downsample.py, and what only an intermediate cloud can show is refused
when that cloud exists, the handle left as it was: as a handle of the same history that never saw the refused call."""
import ctypes as C
import functools

import numpy as np
import pytest

import cluster_twin as CT
from conftest import load_pkg
from test_gpu_cluster import CLUSTER, scan_with_blob
from test_gpu_voxel_downsample import _make, assert_same, fingerprint

pytestmark = pytest.mark.gpu
INVALID = -1
VOXEL, STAT, RADIUS = 0.03, (8, 2.0), (0.1, 3)                   # the sizes tests/test_gpu_cluster.py chains
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def raw():
    return scan_with_blob(3000, 300)


@functools.lru_cache(maxsize=None)
def host(mask):
    """the composition of the host functions for the stages of mask (voxel 1, statistical 2, radius 4, cluster 8) and the size of the
    input of its last stage: computed once, shared, never changed"""
    pkg = load_pkg()
    d, before = raw(), None
    for bit, fn in ((1, lambda x: pkg.voxel_downsample(x, VOXEL)[0]), (2, lambda x: pkg.statistical_outlier_removal(x, *STAT)[0]),
                    (4, lambda x: pkg.radius_outlier_removal(x, *RADIUS)[0]), (8, lambda x: pkg.cluster_filter(x, *CLUSTER)[0])):
        if mask & bit:
            before, d = len(d), fn(d)
    d = np.ascontiguousarray(d, np.float32)
    d.setflags(write=False)
    return d, before


def _structs(mask, stat=STAT, radius=RADIUS):
    from cuda_go_icp_amd import binding as B
    k, alpha = stat if mask & 2 else (0, 0.0)
    r, mn = radius if mask & 4 else (0.0, 0)
    return B.CSourcePipeline(VOXEL if mask & 1 else 0.0, k, alpha, r, mn), B.CClusterSelect(*(CLUSTER if mask & 8 else (0.0, 0, 0, 0)))


def swap_clustered(lib, reg, mask, kept=None, **kw):
    p, s = _structs(mask, **kw)
    return lib.goicp_set_source_clustered(reg.handle, raw().ctypes.data_as(FP), len(raw()), C.byref(p), C.byref(s), None if kept is None else C.byref(kept))


def swap_pipeline(lib, reg, mask, kept=None, **kw):
    p, _ = _structs(mask, **kw)
    return lib.goicp_set_source_pipeline(reg.handle, raw().ctypes.data_as(FP), len(raw()), C.byref(p), None if kept is None else C.byref(kept))


def swap_filtered(lib, reg, mask, kept):
    from cuda_go_icp_amd import binding as B
    p, _ = _structs(mask)
    f = B.CSourceFilter(p.voxel, p.radius, p.min_neighbors)
    return lib.goicp_set_source_filtered(reg.handle, raw().ctypes.data_as(FP), len(raw()), C.byref(f), C.byref(kept))


def swap_voxel(lib, reg, mask, kept):
    return lib.goicp_set_source_voxel(reg.handle, raw().ctypes.data_as(FP), len(raw()), VOXEL, C.byref(kept))


def swap_plain(lib, reg, mask, kept):
    kept.value = len(raw())                                      # goicp_set_source reports no count: it keeps every point
    return lib.goicp_set_source(reg.handle, raw().ctypes.data_as(FP), len(raw()))


def test_every_stage_set_through_every_entry_point(pkg):
    """mask order on one handle: 3 300 -> 2 241 -> 3 181 -> ... -> 1 374 points, so the swaps grow and shrink; every stage removes
    something wherever it stands, so no subset passes by doing nothing"""
    lib = pkg.load_library()
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    a = _make(pkg, 500, "default")
    try:
        for mask in range(16):
            D, before = host(mask)
            assert before is None or 100 < len(D) < before, (mask, len(D), before)
            ways = [swap_clustered]
            if not mask & 8:
                ways.append(swap_pipeline)
            if not mask & 10:
                ways.append(swap_filtered)
            if mask == 1:
                ways.append(swap_voxel)
            if mask == 0:
                ways.append(swap_plain)
            for way in ways:
                kept = C.c_size_t(0)
                assert way(lib, a, mask, kept) == 0, (mask, way.__name__, lib.goicp_last_error())
                assert kept.value == len(D), (mask, way.__name__, kept.value, len(D))
                a.ns, a.pcs = len(D), D
                assert CT.same_bits(a.transform_source(I, z) + np.float32(0), D + np.float32(0)), (mask, way.__name__)
    finally:
        a.close()


@pytest.mark.parametrize("mask", (10, 12, 14))
def test_chains_that_start_behind_the_grid_and_end_in_the_cluster_stage(pkg, mask):
    """statistical + cluster, radius + cluster, statistical + radius + cluster: the first stage is not the voxel grid, the last is the
    cluster selection"""
    lib = pkg.load_library()
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        fingerprint(pkg, a, register=False); fingerprint(pkg, b, register=False)
        D, before = host(mask)
        assert 100 < len(D) < before
        kept = C.c_size_t(0)
        assert swap_clustered(lib, a, mask, kept) == 0, lib.goicp_last_error()
        assert kept.value == len(D)
        a.ns, a.pcs = len(D), D
        b.set_source(D)
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), mask)
    finally:
        a.close(); b.close()


def test_refusals_that_only_an_intermediate_cloud_shows(pkg):
    """each refused after device stages have run and before the swap: INVALID, and the handle answers as its twin b does, which has the
    same history without the refused calls (a fingerprint moves the handle's step pose, so it is taken on both each time)"""
    lib = pkg.load_library()
    a, b = _make(pkg, 500, "default"), _make(pkg, 500, "default")
    try:
        assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), "before")

        def refused(what, rc, text):
            assert rc == INVALID and text in lib.goicp_last_error(), (what, rc, lib.goicp_last_error())
            assert_same(fingerprint(pkg, a, register=False), fingerprint(pkg, b, register=False), what)
        # k above the reduced cloud's size minus one.  k is at most 64, so the grid has to leave at most 64 cells for the reduced count to
        # decide: k in range and equal to that count.  Behind the grid of the other tests (2 241 cells) a k of the reduced count is
        # refused up front by its range
        coarse = len(pkg.voxel_downsample(raw(), 0.3)[0])
        assert 1 < coarse <= 64
        from cuda_go_icp_amd import binding as B
        p = B.CSourcePipeline(0.3, coarse, 2.0, 0.0, 0)
        refused("voxel + stat, k = reduced count", lib.goicp_set_source_pipeline(a.handle, raw().ctypes.data_as(FP), len(raw()), C.byref(p), None), b"n - 1")
        refused("voxel 0.03 + stat, k = reduced count", swap_pipeline(lib, a, 3, stat=(len(host(1)[0]), 2.0)), b"1..64")
        # a radius stage that keeps nothing, behind the statistical stage and in front of the cluster stage
        refused("stat + radius", swap_pipeline(lib, a, 6, radius=(0.05, 2000)), b"keeps no point")
        refused("radius + cluster", swap_clustered(lib, a, 12, radius=(0.05, 2000)), b"keeps no point")
        kept = C.c_size_t(0)
        assert swap_clustered(lib, a, 14, kept) == 0 and kept.value == len(host(14)[0])     # and a good swap still works
    finally:
        a.close(); b.close()
