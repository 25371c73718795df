"""Bricked DT (layout 1) bounds against the linear layout (layout 0), bit for bit.

The lean sibling path reads, for x siblings less than 4 voxels apart, one 16-B x row of a brick per (y, z) pair and takes both x
values from it (a masked dword load for the lanes whose second x lies in the next row).  Only load widths change: every value,
the per-thread point order and the summation order stay, so every bound must keep its bits.  Checked on the bench batch, sibling
expansions of every depth (child spacings from far above to below one voxel), the generic batch, and points outside the grid and
on its faces, against layout 0; the LDS tile kernel and an ICP run (which sum in other orders than the linear layout's paths)
against bits recorded from the parent commit on MI355X (tests/golden/dt_sector_tile_icp.npz).
"""
import ctypes as C

import numpy as np
import pytest


pytestmark = pytest.mark.gpu

V = 300


@pytest.fixture(scope="module")
def pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def regs(pkg, bunny_model, bunny_data):
    """The bench's engine (DT 300^3, k-d source order) in both layouts."""
    r = {lay: pkg.Registration(bunny_model, bunny_data, 1e-3, dt_size=V, dt_layout=lay, morton_sort=2) for lay in (0, 1)}
    yield r
    for x in r.values():
        x.close()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _batch(pkg, reg, rots, recs):
    B = pkg.binding
    n = len(recs)
    ub, lb = np.empty(n, np.float32), np.empty(n, np.float32)
    B.check(reg._lib.goicp_eval_bounds_batch(reg.handle, _fp(np.ascontiguousarray(rots, np.float32)), len(rots),
                                             np.ascontiguousarray(recs).ctypes.data_as(C.POINTER(B.CCube)), n, _fp(ub), _fp(lb)))
    return ub, lb


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _children(parents):
    """the 8 children (centre xyz + width) of each parent (corner xyz + width), in the engine's order and float operations"""
    out = []
    for px, py, pz, pw in parents.astype(np.float32):
        w = pw / np.float32(2)
        for j in range(8):
            c = [px + np.float32(j & 1) * w, py + np.float32(j >> 1 & 1) * w, pz + np.float32(j >> 2 & 1) * w]
            out.append([c[0] + w / np.float32(2), c[1] + w / np.float32(2), c[2] + w / np.float32(2), w])
    return np.array(out, np.float32)


def _parents(rng, n, depth, lo=-0.5, hi=0.5):
    w = np.float32(1.0) / np.float32(1 << depth)
    k = rng.integers(0, 1 << depth, (n, 3)).astype(np.float32)
    corner = np.float32(-0.5) + k * w
    corner = np.clip(corner, lo, hi).astype(np.float32)
    return np.concatenate([corner, np.full((n, 1), w, np.float32)], 1)


def test_bench_batch_bit_identical(pkg, regs):
    """bench.make_batch(8192, 8, seed=1234): the headline launch (lean sibling path, merged x-row loads at depths 4 and 5)."""
    import bench
    rots, recs, _ = bench.make_batch(pkg, regs[1], 8192, 8, seed=1234)
    ub1, lb1 = _batch(pkg, regs[1], rots, recs)
    ub0, lb0 = _batch(pkg, regs[0], rots, recs)
    assert _same_bits(ub1, ub0) and _same_bits(lb1, lb0)
    assert (lb1 <= ub1).all()


@pytest.mark.parametrize("depth", list(range(0, 9)))
def test_sibling_expansions_every_depth(pkg, regs, depth):
    """Expansions of depths 0..8 (child spacing 150 voxels down to 0.6 voxel) under three rotations, with and without the
    rotation radii (both passes of the lean path)."""
    rng = np.random.default_rng(100 + depth)
    kids = _children(_parents(rng, 24, depth))
    for v in ([0.3, -0.2, 0.9], [-2.1, 0.4, 1.1], [0.0, 0.0, 0.0]):
        R = pkg.fgoicp.rodrigues(v)
        for level in (-1, 3, 6):
            ub1, lb1 = regs[1].eval_bounds(R, kids, level)
            ub0, lb0 = regs[0].eval_bounds(R, kids, level)
            assert _same_bits(ub1, ub0) and _same_bits(lb1, lb0), (depth, v, level)


def test_generic_batch_bit_identical(pkg, regs):
    import bench
    rots, recs, _ = bench.make_generic_batch(pkg, regs[1], 4096, 8, seed=4321)
    ub1, lb1 = _batch(pkg, regs[1], rots, recs)
    ub0, lb0 = _batch(pkg, regs[0], rots, recs)
    assert _same_bits(ub1, ub0) and _same_bits(lb1, lb0)


def test_points_outside_and_on_faces(pkg, bunny_model):
    """A source cloud laid on the grid's six faces (voxel 0 and V-1, exactly and half a voxel beyond) and outside it: lookups that
    clamp to the faces and add the overshoot, wavefronts with some lanes inside and some outside, near and far siblings."""
    probe = pkg.Registration(bunny_model, bunny_model[:16], 1e-3, dt_size=V, dt_layout=1)
    Vg, scale, org = probe.dt_info()
    probe.close()
    lo = np.array(org, np.float64)
    hi = lo + (Vg - 1) / scale
    rng = np.random.default_rng(7)
    pts = []
    for axis in range(3):
        for face in (lo[axis], hi[axis], lo[axis] - 0.5 / scale, hi[axis] + 0.5 / scale, lo[axis] - 3.0 / scale, hi[axis] + 7.0 / scale):
            p = rng.uniform(lo, hi, (700, 3))
            p[:, axis] = face
            pts.append(p)
    pts.append(rng.uniform(lo - 0.3, hi + 0.3, (3000, 3)))
    src = np.ascontiguousarray(np.concatenate(pts).astype(np.float32))
    r = {lay: pkg.Registration(bunny_model, src, 1e-3, dt_size=V, dt_layout=lay) for lay in (0, 1)}
    try:
        for depth in (0, 3, 5, 7, 9):
            kids = _children(_parents(np.random.default_rng(depth), 8, depth))
            for v in ([0.0, 0.0, 0.0], [0.02, -0.01, 0.03]):
                R = pkg.fgoicp.rodrigues(v)
                for level in (-1, 5):
                    ub1, lb1 = r[1].eval_bounds(R, kids, level)
                    ub0, lb0 = r[0].eval_bounds(R, kids, level)
                    assert _same_bits(ub1, ub0) and _same_bits(lb1, lb0), (depth, v, level)
    finally:
        for x in r.values():
            x.close()


GOLDEN_TILE_ICP = "dt_sector_tile_icp.npz"


def tile_outputs(pkg, reg):
    """goicp_debug_bounds_tile on 32 expansions of depths 4-7, two rotations, levels -1 and 5: the tile kernel's ub, lb and the direct
    kernel's ub, lb on the same parents, stacked (16, 4, 256)."""
    B = pkg.binding
    rng = np.random.default_rng(5)
    out_all = []
    for depth in (4, 5, 6, 7):
        par = _parents(rng, 32, depth)
        m = len(par)
        for v in ([0.3, -0.2, 0.9], [-2.1, 0.4, 1.1]):
            R = pkg.fgoicp.rodrigues(v)
            for level in (-1, 5):
                out = [np.zeros(8 * m, np.float32) for _ in range(4)]
                ms, st = (C.c_float * 2)(), (C.c_uint32 * 2)()
                B.check(reg._lib.goicp_debug_bounds_tile(reg.handle, _fp(np.ascontiguousarray(R.reshape(-1).astype(np.float32))),
                                                         _fp(np.ascontiguousarray(par.reshape(-1))), 1, m, level, 4,
                                                         _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), ms, st))
                out_all.append(np.stack(out))
    return np.stack(out_all)


def icp_result(pkg, bunny_model, bunny_data10, layout=1):
    """ICP from a perturbed pose on the bunny (DT 300^3): error, R (9), t (3), iterations as one float32 row of 14."""
    reg = pkg.Registration(bunny_model, bunny_data10, 1e-3, dt_size=V, dt_layout=layout)
    try:
        icp = pkg.IterativeClosestPoint3D(reg, 50, 1e-9, pkg.fgoicp.rodrigues([0.05, -0.03, 0.04]), np.array([0.02, -0.01, 0.015], np.float32))
        err, R, t = icp.run()
        return np.concatenate([[err], R.reshape(-1), t, [icp.iters]]).astype(np.float32)
    finally:
        reg.close()


def _golden():
    import os
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, GOLDEN_TILE_ICP))


def test_tile_kernel_bit_identical(pkg, regs):
    """The tile kernel (LDS boxes staged from the bricked grid, its own summation order) and the direct kernel on the same
    parents: the recorded bits."""
    got = tile_outputs(pkg, regs[1])
    assert _same_bits(got, _golden()["tile"])


def test_icp_run_same_pose_bits(pkg, bunny_model, bunny_data10):
    """ICP on the bricked grid (fixed-point sums, nearest-point table in the grid's layout): error, pose and iteration count with the
    recorded bits.  The linear layout sums in another form, so it is not the reference here."""
    got = icp_result(pkg, bunny_model, bunny_data10)
    assert _same_bits(got, _golden()["icp"])
