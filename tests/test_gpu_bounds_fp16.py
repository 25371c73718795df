"""The half-precision bound path (Params::bounds_fp16: dt_to_half_kernel, half_fetch, the layout-2 branches of dt_fetch and
sibling_residuals_rotated, bounds_kernel<2>, bounds_kernel<2, false, true>, bounds_queue_kernel<2>, bounds_queue_kernel<2, false, true>)
against an exact round-toward-zero twin: the engine's own fp32 grid (goicp_dt_download) through half_twin.half_rtz, wrapped as an oracle
distance transform (half_twin.half_dt); oracle.cube_terms on it gives the per-point residuals, twins.bound_ref their float64 sums.
  (a) every voxel of the half grid, read one by one through the lookup, bit for bit -- V = 32, 33 (a ragged ninth brick), 50 -- and
      queries beyond every face, edge and corner;
  (b) the same on targets scaled by 2^-15 (half subnormals) and 2^16 (values above 65504, which must end AT 65504);
  (c) every kernel form against the per-point terms at TOL = 2e-6 (the project's bar for this summation: only the grid's element type
      differs from the fp32 path), plain and truncated, N = 1 bitwise;
  (d) one round of the device queues, twin fusion on and off, plain and truncated;
  (e) every switch that must fall back to the fp32 grid, bit for bit against the fp32 engine; layout 2 after a source swap;
  (f) validity as a property: no pose inside a cube pair scores below the pair's lower bound;
  (g) two converged registrations.
Data: test_gpu_small_shapes' (its 2 000-point target, its make_pair sources, ROTS, LEVEL, _bounds_case's launches).

Measured on MI355X, worst relative deviation from the twin (floor max(ref, 1e-3)) against TOL = 2e-6:
  bounds_kernel<2>, N = 1, 7, 257, 8 193:         unrelated cubes 2.3e-7, siblings 2.1e-7, three rotations / both passes 1.4e-7, far parents 2.4e-7
  bounds_kernel<2, false, true> (g = 0.05):       unrelated cubes 2.4e-7, siblings 1.8e-7, three rotations / both passes 1.6e-7, far parents 1.6e-7
  bounds_queue_kernel<2>, N = 257 / 8 193:        1.9e-7 / 2.2e-7, the same with twin fusion on and off
  bounds_queue_kernel<2, false, true>:            1.8e-7 / 2.0e-7, the same with twin fusion on and off
  after set_source 257 -> 513:                    plain 1.5e-7, truncated 2.1e-7
Every voxel and every outside query of (a) and (b) is bit-equal.  Voxels changed by the conversion: 0.980 (V = 32), 0.981 (33), 0.991 (50);
target x 2^-15: every nonzero voxel a half subnormal, none below 2^-24; target x 2^16: 0.275 (V = 33) and 0.279 (50) of the voxels above 65504.
The queue round against eval_bounds of the children: all 1 344 values bit-equal at N = 257 (2 chunks); at N = 8 193 (16 chunks, partials added
in chunk order) 780 differ plain and 850 truncated, all inside TOL of the twin.  (f): 41 of 48 pairs with lb > 0.  (g): SSE equal to the
reference's to 7 digits, rotation nodes 1 730 / 1 259 against 1 609 / 1 201.

Teeth (once, on scratch copies of device.hip, on MI355X; both edits only change which in-bounds value is read or stored):
  half_fetch picks the opposite half of the pair:    17 of the 22 tests here fail -- all of (a), (b), (c), (d), the pose re-score's "strictly
                                                     lower", the order / pair launch, the source swap and (f); test_bounds_fp16_optin fails too
  __float2half instead of __float2half_rz:           the same 17, and test_bounds_fp16_optin
  (passing under both: the layout-0, trimmed and tiny-registration tests, which either never read the half grid or hold only the optimum.)
Wall time on MI355X: this file 2.1 s, the slowest test 0.44 s.
"""
import ctypes as C

import numpy as np
import pytest

import twins
from conftest import golden, load_pkg, tiny_problem
from half_twin import half_dt, half_rtz
from test_gpu_bounds_order_pairs import _Hip, _expansions, _path
from test_gpu_scale_parity import TOL, _rel
from test_gpu_search_trunc import _children, _parents
from test_gpu_small_shapes import LEVEL, ROTS, V_BOUNDS, _bounds_case, _bounds_target

pytestmark = pytest.mark.gpu
FP16 = dict(bounds_fp16=1, dt_layout=1)
G = 0.05
FAR = np.array([[0.75, -0.25, 0.0, 0.5], [-1.5, 0.5, 0.25, 0.5], [2.0, 2.0, -2.0, 1.0]], np.float32)      # children straddle / leave the grid
ORIGIN_POINT = np.zeros((1, 3), np.float32)


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def hip():
    h = _Hip()
    yield h
    h.free_all()


def _source(N):
    return _bounds_case(N)[0]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dt16(pkg, oracle_mod):
    """the twin's grid at V = 64: the engine's fp32 grid -- the oracle's own, bit for bit -- rounded toward zero to half"""
    target, dt = _bounds_target()
    reg = pkg.Registration(target, ORIGIN_POINT, 1e-3, dt_size=V_BOUNDS, **FP16)
    try:
        assert np.array_equal(_bits(reg.dt_download()), _bits(dt.grid()))
        return half_dt(reg, oracle_mod)
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# (a), (b): every voxel through the lookup
# ----------------------------------------------------------------------------------------------
def _voxel_queries(V, scale, origin):
    """one query per voxel centre, float32(origin + idx / scale), in grid order (z, y, x); each maps to its own voxel under the lookup's index
    expression int((double(q) - min) * scale + 0.5)"""
    z, y, x = np.meshgrid(np.arange(V), np.arange(V), np.arange(V), indexing="ij")
    idx = np.stack([x, y, z], -1).reshape(-1, 3)
    q = (np.array(origin) + idx / scale).astype(np.float32)
    back = np.floor((q.astype(np.float64) - np.array(origin)) * scale + 0.5).astype(np.int64)
    assert np.array_equal(back, idx)
    return q


def _outside_queries(V, scale, origin, rng, per=16):
    """`per` queries 1-3 voxels beyond each of the 6 faces, 12 edges and 8 corners of the grid"""
    out = []
    for s in np.ndindex(3, 3, 3):
        if s == (1, 1, 1):
            continue
        idx = np.empty((per, 3))
        for k in range(3):
            idx[:, k] = (-rng.integers(1, 4, per), rng.integers(0, V, per), V - 1 + rng.integers(1, 4, per))[s[k]]
        out.append(idx)
    return (np.array(origin) + np.concatenate(out) / scale).astype(np.float32)


def _lookup(reg, q):
    """a one-point source at the origin, the identity, cubes of width 0: ub = lb = (the looked-up value)^2, one float product"""
    return reg.eval_bounds(np.eye(3, dtype=np.float32), np.concatenate([q, np.zeros((len(q), 1), np.float32)], 1), -1)


def _every_voxel(pkg, oracle_mod, V, factor):
    target = (_bounds_target()[0] * np.float32(factor)).astype(np.float32)           # a power of two: exact
    a = pkg.Registration(target, ORIGIN_POINT, 1e-3, dt_size=V, dt_layout=1)
    b = pkg.Registration(target, ORIGIN_POINT, 1e-3, dt_size=V, **FP16)
    try:
        grid = b.dt_download()
        assert grid.shape == (V, V, V) and np.array_equal(_bits(grid), _bits(a.dt_download())) and np.all(grid >= 0) and np.isfinite(grid).all()
        _, scale, origin = b.dt_info()
        h = half_rtz(grid)
        hf = h.astype(np.float32)
        want = (hf * hf).reshape(-1)
        q = _voxel_queries(V, scale, origin)
        ub, lb = _lookup(b, q)
        bad = np.flatnonzero(_bits(ub) != _bits(want))
        assert len(bad) == 0, ("V %d x %g: %d of %d voxels differ from the twin, first (x, y, z) %s: device %r twin %r (fp32 grid %r)"
                               % (V, factor, len(bad), V ** 3, np.unravel_index(bad[0], (V, V, V))[::-1], ub[bad[0]], want[bad[0]], grid.reshape(-1)[bad[0]]))
        assert np.array_equal(_bits(lb), _bits(ub))
        changed = float(np.mean(hf != grid))
        ua, _ = _lookup(a, q)
        assert np.array_equal(_bits(ua), _bits((grid * grid).reshape(-1)))            # the fp32 engine on the same queries: its own grid
        dt = half_dt(b, oracle_mod)
        qo = _outside_queries(V, scale, origin, np.random.default_rng(V))
        d = dt.distance(qo.astype(np.float64))
        uo, lo = _lookup(b, qo)
        assert len(qo) >= 400 and np.array_equal(_bits(uo), _bits(d * d)) and np.array_equal(_bits(lo), _bits(uo)), (V, factor)
        nz = grid > 0
        hb = h.view(np.uint16)
        stats = dict(changed=changed, subnormal=float(np.mean((hb[nz] > 0) & (hb[nz] < 0x0400))), saturated=float(np.mean(grid > 65504)),
                     flushed=float(np.mean(grid[nz] < 2.0 ** -24)))
        print("every voxel V %d target x %g: %d voxels + %d outside queries bit-equal to the twin; changed by the conversion %.4f, half subnormals "
              "among nonzero %.4f, above 65504 %.4f, nonzero below 2^-24 %.4f" % (V, factor, V ** 3, len(qo), changed, stats["subnormal"], stats["saturated"], stats["flushed"]))
        return stats
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("V", [32, 33, 50])
def test_every_voxel_bit_for_bit(pkg, oracle_mod, V):
    """33: nine bricks per axis, the last one ragged; 50: no multiple of 4.  Equality with the fp32 grid cannot pass: the conversion changes
    98-99 % of the voxels (asserted >= 0.9)."""
    s = _every_voxel(pkg, oracle_mod, V, 1.0)
    assert s["changed"] >= 0.9


@pytest.mark.parametrize("V", [33, 50])
@pytest.mark.parametrize("factor,what,share", [(2.0 ** -15, "subnormal", 0.9), (2.0 ** 16, "saturated", 0.2)], ids=["subnormal", "saturated"])
def test_subnormal_and_saturated_halves(pkg, oracle_mod, V, factor, what, share):
    """The twin is IEEE: half subnormals are kept (target x 2^-15: 98-99 % of the nonzero voxels), overflow gives 65504 (target x 2^16: 27-28 %
    of the voxels)."""
    s = _every_voxel(pkg, oracle_mod, V, factor)
    assert s[what] >= share, s
    assert s["flushed"] == 0.0, s


# ----------------------------------------------------------------------------------------------
# (c): every kernel form against per-point terms on the half grid
# ----------------------------------------------------------------------------------------------
_HALF_CASES = {}


def _half_case(N, dt16):
    """_bounds_case(N)'s launches with the terms of every cube taken on the half grid, plus the children of the three far parents at both
    levels: [(name, kind, argument, level or None, [(terms, child width, delta)])]"""
    if N in _HALF_CASES:
        return _HALF_CASES[N]
    import oracle as O
    lib = load_pkg().load_library()
    source, rots, calls = _bounds_case(N)
    _, rho = O.rot_radii(source)
    prots = [O.rotate(R, source) for R in rots]
    delta = lambda w: np.float32(lib.goicp_trans_delta(float(w)))
    names = iter(["unrelated"] * 6 + ["siblings", "mixed"])
    out = []
    for kind, arg, level, terms in calls:
        if kind == "eval":
            new = [(O.cube_terms(dt16, prots[0], rho[level] if level >= 0 else None, c[:3], c[3]), c[3], delta(c[3])) for c in arg]
        else:
            new = [(O.cube_terms(dt16, prots[r[5]], rho[LEVEL] if r[4] > 0 else None, np.array(r[:3], np.float32), w), w, np.float32(r[3]))
                   for r, (_, w) in zip(arg, terms)]
        out.append((next(names), kind, arg, level, new))
    kids = np.concatenate([_children(p) for p in FAR])
    for level in (-1, LEVEL):
        out.append(("far", "eval", kids, level, [(O.cube_terms(dt16, prots[0], rho[level] if level >= 0 else None, c[:3], c[3]), c[3], delta(c[3])) for c in kids]))
    _HALF_CASES[N] = (source, rots, out)
    return _HALF_CASES[N]


def _single_point_bits(m, delta, trunc):
    """N = 1: the kernel's own float operations on the one term"""
    m, g = np.float32(m), np.float32(trunc)
    dis = np.float32(max(m - delta, np.float32(0)))
    if trunc > 0:
        m, dis = min(m, g), min(dis, g)
    return np.float32(m * m), np.float32(dis * dis)


def _run_calls(reg, rots, calls, tag, trunc=0.0, worst=None, names=None):
    """every launch on reg against twins.bound_ref of its terms -> the launches' raw outputs; worst[name] collects the deviations"""
    outs = []
    worst = {} if worst is None else worst
    for name, kind, arg, level, terms in calls:
        if names is not None and name not in names:
            continue
        ub, lb = reg.eval_bounds(rots[0], arg, level) if kind == "eval" else reg.eval_bounds_batch(rots, arg)
        assert len(ub) == len(terms)
        outs.append((ub, lb))
        for i, (m, w, delta) in enumerate(terms):
            fu, fl = twins.bound_ref(m, w, trunc)
            d = max(_rel(ub[i], fu), _rel(lb[i], fl))
            worst[name] = max(worst.get(name, 0.0), d)
            assert d <= TOL and lb[i] <= ub[i], (tag, name, level, i, ub[i], fu, lb[i], fl)
            if len(m) == 1:
                su, sl = _single_point_bits(m[0], delta, trunc)
                assert ub[i].tobytes() == su.tobytes() and lb[i].tobytes() == sl.tobytes(), (tag, name, level, i, ub[i], su, lb[i], sl)
    return outs


def _fmt(worst):
    return ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))


@pytest.mark.parametrize("N", [1, 7, 257, 8193])
def test_every_kernel_form_vs_half_terms(pkg, dt16, N):
    """bounds_kernel<2> and bounds_kernel<2, false, true>: unrelated cubes of n = 1, 8, 77 at levels -1 and LEVEL, the 8 children of two
    parents (one per pass), 13 cubes over three rotations and both passes, the children of three parents that straddle or leave the grid;
    truncation off again brings the plain bits back."""
    target, _ = _bounds_target()
    source, rots, calls = _half_case(N, dt16)
    reg = pkg.Registration(target, source, 1e-3, dt_size=V_BOUNDS, **FP16)
    a, b = {}, {}
    try:
        plain = _run_calls(reg, rots, calls, "N %d" % N, worst=a)
        reg.set_search_truncation(G)
        _run_calls(reg, rots, calls, "N %d truncated" % N, trunc=G, worst=b)
        reg.set_search_truncation(0.0)
        again = _run_calls(reg, rots, calls, "N %d plain again" % N)
        for (u0, l0), (u1, l1) in zip(plain, again):
            assert np.array_equal(_bits(u0), _bits(u1)) and np.array_equal(_bits(l0), _bits(l1))
        print("fp16 bounds N %d: worst rel deviation plain [%s]; truncated [%s]" % (N, _fmt(a), _fmt(b)))
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# (d): one round of the device queues
# ----------------------------------------------------------------------------------------------
def _queue_round(pkg, reg, R, parents, level):
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    n = len(parents)
    out = [np.zeros(8 * n, np.float32) for _ in range(4)]
    info = (C.c_int32 * 2)()
    pkg.binding.check(reg._lib.goicp_debug_queue_expand(reg.handle, fp(np.ascontiguousarray(R.reshape(-1).astype(np.float32))), level,
                                                        fp(np.ascontiguousarray(parents.reshape(-1))), n, fp(out[0]), fp(out[1]), fp(out[2]), fp(out[3]), info))
    return out, tuple(info)


@pytest.mark.parametrize("N", [257, 8193])
def test_device_queue_round_vs_half_terms(pkg, oracle_mod, dt16, N):
    """bounds_queue_kernel<2> and <2, false, true>: 39 parents of depths 0-4 and the three far ones, both passes listed, twin fusion on and
    off.  All four output arrays against the twin at TOL, as test_sibling_expansion_all_sixteen_vs_oracle's `check` holds them to the oracle
    (that test asks no bit equality between the queue round and eval_bounds -- the round adds chunk partials in its own order -- so none is
    asked here; the number of differing values is printed)."""
    target, _ = _bounds_target()
    source = _source(N)
    R = pkg.fgoicp.rodrigues(ROTS[0])
    prot = oracle_mod.rotate(R, source)
    _, rho = oracle_mod.rot_radii(source)
    parents = np.concatenate([_parents(np.random.default_rng(N), 10, range(0, 5)), FAR])
    n = len(parents)
    assert 40 <= n <= 44
    kids = np.concatenate([_children(p) for p in parents])
    terms = {ps: [oracle_mod.cube_terms(dt16, prot, r, k[:3], k[3]) for k in kids] for ps, r in ((0, None), (1, rho[LEVEL]))}
    worst, differ = {}, {}
    for tw in (1, 0):
        reg = pkg.Registration(target, source, 1e-3, dt_size=V_BOUNDS, twin_fusion=tw, **FP16)
        try:
            for g in (0.0, G):
                reg.set_search_truncation(g)
                per_cube = {0: reg.eval_bounds(R, kids, -1), 1: reg.eval_bounds(R, kids, LEVEL)}
                out, info = _queue_round(pkg, reg, R, parents, LEVEL)
                assert info[1] == tw
                tag = "twin=%d %s chunks=%d" % (tw, "truncated" if g else "plain", info[0])
                for ps, (qu, ql) in enumerate(((out[0], out[1]), (out[2], out[3]))):
                    for i, k in enumerate(kids):
                        fu, fl = twins.bound_ref(terms[ps][i], k[3], g)
                        d = max(_rel(qu[i], fu), _rel(ql[i], fl))
                        worst[tag] = max(worst.get(tag, 0.0), d)
                        assert d <= TOL and ql[i] <= qu[i], (tag, ps, i, qu[i], fu, ql[i], fl)
                        e = max(_rel(per_cube[ps][0][i], fu), _rel(per_cube[ps][1][i], fl))
                        assert e <= TOL, (tag, "eval_bounds", ps, i)
                    differ[tag] = differ.get(tag, 0) + int(np.sum(_bits(qu) != _bits(per_cube[ps][0]))) + int(np.sum(_bits(ql) != _bits(per_cube[ps][1])))
        finally:
            reg.close()
    print("fp16 queue round N %d: worst rel deviation [%s]; values differing from eval_bounds of the children, of %d: %s" % (N, _fmt(worst), 32 * n, differ))


# ----------------------------------------------------------------------------------------------
# (e): the fall-backs to the fp32 grid, and layout 2 across a source swap
# ----------------------------------------------------------------------------------------------
def _same_bits_on_every_launch(a, b, N, dt16):
    _, rots, calls = _half_case(N, dt16)
    for name, kind, arg, level, _ in calls:
        ua, la = a.eval_bounds(rots[0], arg, level) if kind == "eval" else a.eval_bounds_batch(rots, arg)
        ub, lb = b.eval_bounds(rots[0], arg, level) if kind == "eval" else b.eval_bounds_batch(rots, arg)
        assert np.array_equal(_bits(ua), _bits(ub)) and np.array_equal(_bits(la), _bits(lb)), (name, level)


@pytest.mark.parametrize("N", [7, 257])
def test_linear_layout_ignores_the_flag(pkg, dt16, N):
    """bounds_fp16 = 1 with dt_layout = 0: no half copy is made, the bounds are the fp32 layout-0 engine's (documented so in goicp_mi355.h)"""
    target, _ = _bounds_target()
    a = pkg.Registration(target, _source(N), 1e-3, dt_size=V_BOUNDS, dt_layout=0)
    b = pkg.Registration(target, _source(N), 1e-3, dt_size=V_BOUNDS, dt_layout=0, bounds_fp16=1)
    try:
        for g in (0.0, G):
            a.set_search_truncation(g); b.set_search_truncation(g)
            _same_bits_on_every_launch(a, b, N, dt16)
    finally:
        a.close(); b.close()


def test_trimmed_bounds_keep_the_fp32_grid(pkg, dt16):
    target, _ = _bounds_target()
    a = pkg.Registration(target, _source(257), 1e-3, dt_size=V_BOUNDS, dt_layout=1, trim_fraction=0.1)
    b = pkg.Registration(target, _source(257), 1e-3, dt_size=V_BOUNDS, trim_fraction=0.1, **FP16)
    try:
        assert a.inliers == b.inliers < 257
        _same_bits_on_every_launch(a, b, 257, dt16)
    finally:
        a.close(); b.close()


def test_pose_rescore_keeps_the_fp32_grid(pkg):
    target, _ = _bounds_target()
    a = pkg.Registration(target, _source(257), 1e-3, dt_size=V_BOUNDS, dt_layout=1)
    b = pkg.Registration(target, _source(257), 1e-3, dt_size=V_BOUNDS, **FP16)
    rng = np.random.default_rng(16)
    try:
        for _ in range(16):
            R = pkg.fgoicp.rodrigues(rng.uniform(-1.5, 1.5, 3).astype(np.float32))
            t = rng.uniform(-0.4, 0.4, 3).astype(np.float32)
            ea, eb = a.compute_sse_error(R, t), b.compute_sse_error(R, t)
            assert ea.tobytes() == eb.tobytes() and ea > 0
            u16 = b.eval_bounds(R, np.array([[t[0], t[1], t[2], 0.0]], np.float32), -1)[0][0]
            assert u16 < eb                                      # the same pose through the bound path: the half grid, strictly lower here
    finally:
        a.close(); b.close()


def test_footprint_order_and_pairs_fall_back_to_the_plain_form(pkg, hip):
    """bounds_order 0, 1, 2 with bounds_order_min_groups = 1 on fp16 handles, 512 expansions of 4 rotations through goicp_time_bounds_device:
    the ordered and paired kernels exist for the fp32 bricked grid only, so all three launch the plain form (goicp_debug_bounds_order) on the
    half grid -- the same bits, and not the fp32 engine's."""
    target, _ = _bounds_target()
    source = _source(257)
    rng = np.random.default_rng(4096)
    rots = np.stack([pkg.fgoicp.rodrigues(v) for v in list(ROTS) + [[0.1, 0.2, -0.3]]]).astype(np.float32)
    recs = _expansions(pkg, rng, np.repeat(np.arange(4, dtype=np.int32), 128))
    n = len(recs)
    assert n == 4096
    got = {}
    for key, kw in ((0, dict(bounds_order=0, **FP16)), (1, dict(bounds_order=1, **FP16)), (2, dict(bounds_order=2, **FP16)), ("fp32", dict(bounds_order=0, dt_layout=1))):
        reg = pkg.Registration(target, source, 1e-3, dt_size=V_BOUNDS, bounds_order_min_groups=1, **kw)
        try:
            d_rots, d_cubes = hip.upload(rots.reshape(-1)), hip.upload(np.ascontiguousarray(recs).view(np.uint8))
            d_ub, d_lb = hip.alloc(4 * n), hip.alloc(4 * n)
            ms = C.c_float()
            pkg.binding.check(reg._lib.goicp_time_bounds_device(reg.handle, d_rots, d_cubes, n, d_ub, d_lb, 1, C.byref(ms)))
            got[key] = (hip.download(d_ub, n, np.uint32), hip.download(d_lb, n, np.uint32))
            assert _path(reg)[0] == 0, (key, _path(reg))
        finally:
            hip.free_all()
            reg.close()
    for o in (1, 2):
        assert np.array_equal(got[o][0], got[0][0]) and np.array_equal(got[o][1], got[0][1]), o
    ub16, ub32 = got[0][0].view(np.float32), got["fp32"][0].view(np.float32)
    assert np.isfinite(ub16).all() and np.all(ub16 <= ub32 * (1 + 1e-6)) and not np.array_equal(got[0][0], got["fp32"][0])


def test_layout_2_survives_a_source_swap(pkg, dt16):
    """set_source of another cloud (257 -> 513 points) on an fp16 handle: the launches of (c) against terms of the NEW cloud on the half grid,
    plain and truncated (dt16_.trunc follows the handle's truncation)"""
    target, _ = _bounds_target()
    reg = pkg.Registration(target, _source(257), 1e-3, dt_size=V_BOUNDS, **FP16)
    try:
        source, rots, calls = _half_case(513, dt16)
        reg.set_source(source)
        assert reg.ns == 513
        a, b = {}, {}
        _run_calls(reg, rots, calls, "after set_source", worst=a)
        reg.set_search_truncation(G)
        _run_calls(reg, rots, calls, "after set_source, truncated", trunc=G, worst=b)
        print("fp16 bounds after set_source 257 -> 513: worst rel deviation plain [%s]; truncated [%s]" % (_fmt(a), _fmt(b)))
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# (f): validity as a property
# ----------------------------------------------------------------------------------------------
def test_lower_bound_holds_for_poses_inside_the_cubes(pkg):
    """test_gpu_search_trunc.test_lower_bound_holds_for_poses_inside_the_cubes' construction on an fp16 handle (V = 64, N = 257): 48 rotation
    cube x translation cube pairs, 32 poses inside each.  E16(pose), the pose's score on the half grid (eval_bounds at width 0 without a
    rotation radius), is >= the pair's lower bound; E32(pose), compute_sse_error on the fp32 grid, is >= E16(pose): no half exceeds its
    float.  Bar 1e-5 relative, that test's own (two float sums of at most N terms)."""
    target, _ = _bounds_target()
    reg = pkg.Registration(target, _source(257), 1e-3, dt_size=V_BOUNDS, **FP16)
    rng = np.random.default_rng(41)
    pairs = positive = 0
    worst, worst32 = np.inf, np.inf
    try:
        for _ in range(48):
            lr = int(rng.integers(3, 9))
            wr = 2 * np.pi / (1 << lr)
            while True:
                r0 = rng.uniform(-np.pi, np.pi, 3)
                if np.linalg.norm(r0) <= np.pi:
                    break
            lt = int(rng.integers(1, 7))
            wt = np.float32(1.0 / (1 << lt))
            tc = (rng.uniform(-0.5, 0.5, 3) * (1 - wt)).astype(np.float32)
            R0 = pkg.fgoicp.rodrigues(r0.astype(np.float32))
            cube = np.array([[tc[0], tc[1], tc[2], wt]], np.float32)
            _, lb = reg.eval_bounds(R0, cube, lr)
            ub0, lb0 = reg.eval_bounds(R0, cube, -1)
            assert lb[0] <= lb0[0] <= ub0[0]
            pairs += 1
            positive += lb[0] > 0
            for _ in range(32):
                r = np.float32(r0) + rng.uniform(-0.5, 0.5, 3).astype(np.float32) * np.float32(wr)
                t = tc + rng.uniform(-0.5, 0.5, 3).astype(np.float32) * wt
                R = pkg.fgoicp.rodrigues(r)
                e16 = float(reg.eval_bounds(R, np.array([[t[0], t[1], t[2], 0.0]], np.float32), -1)[0][0])
                e32 = float(reg.compute_sse_error(R, t))
                worst, worst32 = min(worst, e16 - float(lb[0])), min(worst32, e32 - e16)
                assert e16 >= float(lb[0]) * (1 - 1e-5), (lr, lt, e16, float(lb[0]))
                assert e32 >= e16 * (1 - 1e-5), (lr, lt, e32, e16)
        print("fp16 validity: %d pairs, %d with lb > 0, smallest E16(pose) - lb %.3e, smallest E32(pose) - E16(pose) %.3e" % (pairs, positive, worst, worst32))
        assert positive * 4 >= pairs                                        # not vacuous: at least a quarter
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# (g): a converged search
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 3])
def test_tiny_registration_converges(pkg, seed):
    """conftest.tiny_problem with bounds_fp16 = 1 and the default search: SSEThresh lies under the optimum's cost, so the search ends only when
    every cube whose lower bound is SSEThresh under the incumbent is refuted.  The half grid's objective never exceeds the fp32 one, and
    best_sse is re-scored on the fp32 grid: both this run's SSE and the reference's lie within SSEThresh above the global optimum, hence
    within SSEThresh of each other."""
    tgt, src = tiny_problem(seed)
    g = golden("e2e_tiny%d" % seed)
    eng = pkg.FastGoICP(tgt, src, g["mse_threshold"], bounds_fp16=1)
    try:
        eng.run()
        sse = float(eng.get_best_error())
        print("e2e tiny%d bounds_fp16: sse %.7g (reference %.7g, SSEThresh %.3g), rotation nodes %d (reference %d)"
              % (seed, sse, g["sse"], g["sse_threshold"], eng.counters.rot_pops, g["rNodeCount"]))
        assert eng.finished
        assert abs(float(eng.sse_threshold) - g["sse_threshold"]) <= 1e-6 * g["sse_threshold"]
        assert abs(sse - g["sse"]) <= g["sse_threshold"], (sse, g["sse"], g["sse_threshold"])
    finally:
        eng.registration.close()
