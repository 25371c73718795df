"""goicp_segment_plane_host / goicp_plane_filter_host: RANSAC plane segmentation on the host (no handle, no GPU) against the numpy twin of
its definition (tests/plane_twin.py) -- labels, plane records (every field, as bytes), kept cloud and indices bit for bit over the shared
cases -- and what the definition promises on named cases: the exact plane (every non-degenerate hypothesis ties, the smallest one wins,
the normal is exactly (0, 0, 1)), the points at the distance and one ulp beyond, degenerate clouds, floor + wall + object, min_inliers, the
object on a floor.  Also here: the boundary (ABI version, struct sizes, the new symbols) and every refusal that needs no device.

The object-on-floor property (at least 95 % of the floor and at most 2 % of the object labelled 0) is asserted on the TWIN's output for the
seeds 0, 1, 2 and 12345; the library is then held to the twin bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plane_twin as PT
from conftest import ROOT, load_pkg

INVALID = -1
NEW = {"goicp_plane_select_default", "goicp_segment_plane_host", "goicp_segment_plane", "goicp_plane_filter_host", "goicp_plane_filter",
       "goicp_set_source_segmented"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def assert_equal(got, want, what):
    """(labels, planes) or (cloud, indices, planes) of the library against the twin's, as bytes"""
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, g[:4], w[:4])


@pytest.mark.parametrize("name", list(PT.cases()))
def test_library_equals_twin(pkg, name):
    xyz, kw = PT.cases()[name]
    label, planes, kept, idx = PT.twin_of(name)
    assert planes.dtype == pkg.fgoicp.PLANE_DTYPE and planes.dtype.itemsize == 40
    assert_equal(pkg.segment_plane(xyz, **kw), (label, planes), name)
    assert_equal(pkg.plane_filter(xyz, **kw), (kept, idx, planes), name)
    # the properties, on the twin's output: the labels count the planes' inliers, the kept points are the unlabelled ones
    assert np.array_equal(np.bincount(label[label >= 0], minlength=len(planes)), planes["inliers"])
    assert np.array_equal(idx, np.flatnonzero(label < 0)) and PT.same_bits(kept, xyz[idx])


@pytest.mark.parametrize("refine", [0, 1])
def test_exact_plane_ties_go_to_the_smallest_hypothesis(pkg, refine):
    xyz, kw = PT.cases()["exact_plane_r%d" % refine]
    label, planes = pkg.segment_plane(xyz, **kw)
    assert len(planes) == 1 and not label.any()
    assert planes[0]["inliers"] == len(xyz) and planes[0]["hypothesis"] == PT.first_valid_hypothesis(xyz, kw["iterations"], 0)
    assert planes[0]["normal"].tobytes() == np.array([0, 0, 1], np.float32).tobytes() and planes[0]["d"] == 0
    assert planes[0]["refined"] == refine


def test_points_at_the_distance_and_one_ulp_beyond(pkg):
    xyz, kw = PT.cases()["boundary_r0"]
    label, planes = pkg.segment_plane(xyz, **kw)
    assert len(planes) == 1 and planes[0]["normal"].tolist() == [0, 0, 1] and planes[0]["inliers"] == 205
    assert not label[:205].any() and np.all(label[205:] == -1)


def test_degenerate_clouds_have_no_plane(pkg):
    for name in ("duplicates", "collinear"):
        xyz, kw = PT.cases()[name]
        label, planes = pkg.segment_plane(xyz, **kw)
        assert len(planes) == 0 and np.all(label == -1), name
        kept, idx, _ = pkg.plane_filter(xyz, **kw)
        assert PT.same_bits(kept, xyz) and np.array_equal(idx, np.arange(len(xyz)))       # zero planes, m == n
    three = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    kept, idx, planes = pkg.plane_filter(three, 0.1, 1)
    assert len(planes) == 1 and kept.shape == (0, 3) and len(idx) == 0                     # m == 0


def test_floor_wall_object(pkg):
    xyz = PT.cases()["floor_wall_object_P2"][0]
    one = pkg.segment_plane(xyz, **PT.cases()["floor_wall_object_P1"][1])
    two = pkg.segment_plane(xyz, **PT.cases()["floor_wall_object_P2"][1])
    stop = pkg.segment_plane(xyz, **PT.cases()["floor_wall_object_min_inliers"][1])
    assert len(one[1]) == 1 and len(two[1]) == 2 and len(stop[1]) == 1
    assert 480 <= two[1][0]["inliers"] <= 520 and 290 <= two[1][1]["inliers"] < 400         # the floor, then the wall: below min_inliers = 400
    assert abs(two[1][0]["normal"][2]) > 0.999 and abs(two[1][1]["normal"][0]) > 0.999
    assert one[0].tobytes() == stop[0].tobytes() and np.array_equal(one[0] == 0, two[0] == 0)


@pytest.mark.parametrize("seed", PT.OBJECT_SEEDS)
def test_object_on_floor_property_of_the_twin(seed):
    xyz, is_floor = PT.object_on_floor()
    label = PT.segment_plane(xyz, seed=seed, **PT.OBJECT_ON_FLOOR)[0]
    floor_share, object_share = np.mean(label[is_floor] == 0), np.mean(label[~is_floor] == 0)
    print("seed %d: floor %.4f object %.4f" % (seed, floor_share, object_share))
    assert floor_share >= 0.95 and object_share <= 0.02, (seed, floor_share, object_share)


def test_refusals_write_nothing(pkg):
    lib = pkg.load_library()
    from cuda_go_icp_amd import binding as B
    fp, ip, pp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(B.CPlane)
    good = PT.slab(257)
    g, n = good.ctypes.data_as(fp), len(good)
    lab, out, idx = np.full(n, -7, np.int32), np.full((n, 3), -7, np.float32), np.full(n, -7, np.int32)
    planes = np.full(8 * 10, -7, np.int32)
    c, m = C.c_size_t(99), C.c_size_t(99)
    L, O, X, P = lab.ctypes.data_as(ip), out.ctypes.data_as(fp), idx.ctypes.data_as(ip), planes.ctypes.data_as(pp)

    def sel(distance=0.01, iterations=8, refine=1, max_planes=1, min_inliers=0, seed=0):
        return C.byref(B.CPlaneSelect(distance, iterations, refine, max_planes, min_inliers, seed))

    def plain(x, n_, **kw):
        return lib.goicp_segment_plane_host(x, n_, sel(**kw), L, P, C.byref(c))

    def filt(x, n_, **kw):
        return lib.goicp_plane_filter_host(x, n_, sel(**kw), O, X, P, C.byref(c), C.byref(m))

    for call in (plain, filt):
        for bad_value in (np.nan, np.inf):
            bad = np.array(good)
            bad[100, 1] = bad_value
            assert call(bad.ctypes.data_as(fp), n) == INVALID and b"non-finite" in lib.goicp_last_error()
        assert call(g, 0) == INVALID and call(None, n) == INVALID
        assert call(g, (2 ** 31 - 1) // 8 + 1) == INVALID
        for d in (0.0, -0.1, float("nan"), float("inf")):
            assert call(g, n, distance=d) == INVALID and b"distance" in lib.goicp_last_error(), d
        for kw, word in ((dict(iterations=-1), b"iterations"), (dict(iterations=B.PLANE_MAX_ITERATIONS + 1), b"iterations"), (dict(max_planes=-1), b"max_planes"),
                         (dict(max_planes=B.PLANE_MAX_PLANES + 1), b"max_planes"), (dict(min_inliers=-1), b"min_inliers"), (dict(refine=2), b"refine"),
                         (dict(refine=-1), b"refine")):
            assert call(g, n, **kw) == INVALID and word in lib.goicp_last_error(), kw
    assert lib.goicp_segment_plane_host(g, n, None, L, P, C.byref(c)) == INVALID
    assert lib.goicp_segment_plane_host(g, n, sel(), None, P, C.byref(c)) == INVALID
    assert lib.goicp_segment_plane_host(g, n, sel(), L, None, C.byref(c)) == INVALID
    assert lib.goicp_segment_plane_host(g, n, sel(), L, P, None) == INVALID
    assert lib.goicp_plane_filter_host(g, n, None, O, X, P, C.byref(c), C.byref(m)) == INVALID
    assert lib.goicp_plane_filter_host(g, n, sel(), None, X, P, C.byref(c), C.byref(m)) == INVALID
    assert lib.goicp_plane_filter_host(g, n, sel(), O, X, P, C.byref(c), None) == INVALID
    assert np.all(lab == -7) and np.all(out == -7) and np.all(idx == -7) and np.all(planes == -7) and c.value == 99 and m.value == 99
    # the defaults (iterations 0 = 1000, max_planes 0 = 1), a min_inliers above n (no plane), and the optional outputs
    want = pkg.plane_filter(good, 0.012, 1000, 1, 1, 0, 5)
    assert lib.goicp_plane_filter_host(g, n, sel(0.012, 0, 1, 0, 0, 5), O, None, None, None, C.byref(m)) == 0
    assert m.value == len(want[0]) and PT.same_bits(out[:m.value], want[0]) and np.all(idx == -7) and np.all(planes == -7)
    assert plain(g, n, min_inliers=n + 1) == 0 and c.value == 0 and np.all(lab == -1)


def test_shim_call_sites_compile():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_plane.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_boundary(pkg):
    from cuda_go_icp_amd import binding as B
    lib = pkg.load_library()
    assert lib.goicp_abi_version() == 4
    assert C.sizeof(B.CPlaneSelect) == 32 and C.sizeof(B.CPlane) == 40 and B.CPlaneSelect.seed.offset == 24
    assert NEW <= set(B.SYMBOLS) and all(hasattr(lib, name) for name in NEW)
    with open(os.path.join(ROOT, "include", "goicp_mi355.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NEW) and "GOICP_PLANE_MAX_ITERATIONS 65536" in header and "GOICP_PLANE_MAX_PLANES 8" in header
    s = B.CPlaneSelect(1.0, 2, 1, 4, 5, 6)
    lib.goicp_plane_select_default(C.byref(s))
    assert (s.distance, s.iterations, s.refine, s.max_planes, s.min_inliers, s.seed) == (0.0, 0, 0, 0, 0, 0)
    lib.goicp_plane_select_default(None)
    assert callable(pkg.segment_plane) and callable(pkg.plane_filter) and callable(pkg.Registration.segment_plane) and callable(pkg.Registration.plane_filter)
