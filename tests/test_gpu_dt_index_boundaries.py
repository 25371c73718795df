"""The float voxel-index fast path at voxel boundaries, through every lookup site of csrc/device.hip.  The reference's index is
int((double(q) - min) * scale + 0.5); the kernels truncate F = fma(q - min_f, scale_f, 0.5f) and recompute in double only when F lies within
eps(F) = c1 + c2 |F| of an integer (engine.cpp: c1 = 1.05 x 2^-24 (scale max|min| + 8), c2 = 1.05 x 2^-24 x 4).  The sites and their thresholds:
  S1 dt_distance / voxel_fast          per axis c1 + c2 |F|                   unrelated cubes, ragged groups, the grouped launch, out-of-grid fallbacks
  S2 sibling_residuals_rotated         per axis, one `risky` for six indices  sibling sets on the linear and the half grid, lean wavefronts that leave
                                                                              the grid, the trimmed kernel's sibling form, the tile kernel's fallback
  S3 lean_points (NP 1: LAST_ZERO on / off; NP 2: twin-fused)   eps_grid = c1 + c2 (V + 1) on the smallest of six margins
  S4 lean_index (the pair kernel)      the same eps_grid
  S5 bounds_tile_kernel, staged path   eps_box = c1 + c2 V
Lookups are placed ON the rounding boundaries: per axis b = min + (k - 0.5) / scale for k in {-1, 0, 1, 2, V-2, V-1, V, V+1} and up to 40 of
3 .. V-3, moved by 0 and +-2^-10 .. 2^-33 voxel and then by -4 .. +4 float32 ulps, on one, two or all three axes (boundary_coords, _queries:
from dt_info() alone).  The expected index is the double expression in numpy; the expected distance is oracle.DistanceTransform.distance
(half_twin.half_dt for the half grid).  Targets: A = test_gpu_small_shapes._bounds_target (origin-centred), B = A + (37.25, -11.5, 5.125)
in float32 -- c1 is 17 to 20 times larger there, the only regime in which the min_f term counts; grids 32 and 64; bricked, linear and half grid.

Every case prints and asserts two preconditions on the CPU before it touches the device (preconditions): at least 20 of its lookups get
ANOTHER index from the truncated float F than from the double expression (emulated_F: the float32 difference, product and sum exact, one
rounding -- no c1, no c2, and it supplies no expected value), and for at least 85 % of its adversarial coordinates the grid holds another
value across the boundary (k = 0 is counted although int() truncates toward zero and both sides are voxel 0).
  (a) test_one_query_per_cube     source (0, 0, 0), R = I, w = 0: ub == lb == Distance(q)^2 bit for bit; 251 cubes (S1) and the grouped launch
  (b) test_sibling_sets*          the 8 children of the nodes whose child (0,0,0) / (1,1,1) looks up q, one-point source at the origin (level -1)
                                  and at P_OFF (level -1 and 12: rho > 0): ub = fl(m^2), lb = fl(max(fl(m - delta), 0)^2), m = max(d - rho, 0), bit
                                  for bit -- eval_bounds (S3, S2, S4 by configuration), the trimmed kernel, goicp_debug_bounds_tile with its
                                  counters (inner queries all staged: S5; k in {-1, V, V+1} all fallen back), goicp_debug_queue_expand (NP = 2)
  (c) test_full_wavefronts        N = 64, 257, 513 source points that are the queries, risky and safe lanes interleaved, some beyond the grid:
                                  float64 sums of oracle.cube_terms (twins.bound_ref) at TOL; plain, truncated, trimmed; eval_bounds, pair kernel,
                                  tile + direct kernel, queue round.  Precondition: some child's sum moves by >= 50 TOL under the emulated index
  (d) test_off_origin_*           target B: nn_query == oracle.nn_brute in indices and distance bits; first-pass error within ERR_REL
The file has no tolerance of its own: (a), (b) and (d)'s neighbours are bit equality, (c) TOL = 2e-6, (d)'s error ERR_REL = 5e-6, both imported.

No defect was found: every case passed on MI355X as first run.  Measured there:
  preconditions  (a) 11 540 .. 23 724 lookups per case, float index wrong for 2 364 .. 2 984, 97.4 .. 98.5 % sharp; the 251-cube batch: 120 wrong, >= 97.8 %
                 (b) 15 568 .. 15 952 lookups, wrong 4 928 .. 5 928, 97.1 .. 98.9 % sharp; tile classes 3 760 .. 10 160, wrong 666 .. 3 702, >= 98.2 %;
                     queue rounds 4 096, wrong 2 264 .. 2 416, >= 97.7 %
                 (c) the largest move of a child's upper bound under the emulated index: 3.7e-2 .. 2.2e-1 relative (18 600 .. 109 000 x TOL)
  (c) worst deviation over all twelve cases: 2.25e-7 (truncated, target B, grid 32, N = 513); plain 1.68e-7, trimmed 1.83e-7, tile 1.84e-7
Teeth (once, on scratch copies of device.hip / engine.cpp, each built into its own library and loaded through GOICP_LIBRARY; this file, the
bounds tests of test_gpu_parity (10), test_gpu_small_shapes and test_gpu_bounds_* (631); every mutant reads valid memory only):
  A  voxel_fast never sets `risky`                18 of the 641 earlier tests fail, 56 of the 57 here (28 | 28 on target A | B)
  B  eps_grid = 0 in lean_points and lean_index    2 of the 641 earlier (test_segment_geometry at N = 8 193, grid 64), 26 here (12 | 14): test_sibling_sets
                                                  bricked and pairs, the tile test's direct kernel, the queue round, 10 of (c)
  C  eps_box = 0 in the tile kernel                the same 2 of the 641 earlier, 14 here (6 | 8): test_sibling_sets_tile on both targets, 10 of (c)
  D  c1 without its scale |min| term               0 of the 641 earlier, 28 here, ALL on target B (every test of B); none on target A
None of the required counts was zero: A, B and C each fail a case of (a) or (b) on both targets, D fails on target B.
Wall time on MI355X: this file 3.1 s (57 tests, the slowest 0.3 s); the GPU suite with it 301 s (1 317 tests)."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import half_twin
import twins
from conftest import load_pkg
from test_gpu_icp_gate import _run, _transform_f32
from test_gpu_scale_parity import TOL, _rel, _trim_reg
from test_gpu_search_trunc import _children
from test_gpu_small_shapes import ERR_REL, M_ICP, _bounds_target, _case, _knn_queries

pytestmark = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32
SHIFT = np.array([37.25, -11.5, 5.125], f32)
TARGETS = ("A", "B")
GRIDS = (32, 64)
VARIANTS = {"bricked": dict(dt_layout=1, bounds_order=0), "linear": dict(dt_layout=0), "fp16": dict(dt_layout=1, bounds_fp16=1)}
PAIRS = dict(dt_layout=1, bounds_order=2, bounds_order_min_groups=1)
W = f32(1.0 / 64)                                   # child width of every expansion here: 0.28 (dt_size 32) and 0.57 (64) of a voxel
LEVEL = 12                                          # rotation level of the lower-bound passes: the radius is 1.3e-3 |p|, below the distances off the origin too
P_OFF = np.array([0.125, -0.0625, 0.03125], f32)    # the one-point source of nonzero norm: powers of two, so q - p and p + (q - p) are exact
FAR = np.array([-500.0, 500.0, -500.0], f32)        # the point a trimmed engine drops
TRUNC_G = 0.05
NEAR = 2.0 ** -9                                    # a lookup is adversarial when its exact F lies this close to an integer (offsets <= 2^-10 voxel + 4 ulps)
EYE = np.eye(3, dtype=f32)


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ----------------------------------------------------------------------------------------------
# geometry, the exact index, the emulated float index (no error model in it), the oracle's lookup on an index
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _target(tgt):
    a = _bounds_target()[0]
    t = a if tgt == "A" else (a + SHIFT).astype(f32)
    t = np.ascontiguousarray(t)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _oracle_dt(tgt, V):
    import oracle
    if tgt == "A" and V == 64:
        return _bounds_target()[1]
    return oracle.DistanceTransform(_target(tgt), V, 2.0)


def _info(tgt, V):
    """what Registration.dt_info() returns for this geometry (every test asserts that it does)"""
    dt = _oracle_dt(tgt, V)
    return dt.V, dt.scale, tuple(dt.origin)


def exact_F(info, pos):
    """the reference's expression, (double(q) - min) * scale + 0.5: three IEEE operations in float64"""
    _, scale, org = info
    return (pos.astype(f64) - np.array(org, f64)) * scale + 0.5


def exact_index(info, pos):
    return np.trunc(exact_F(info, pos)).astype(np.int64)


def _f32_of_fraction(x):
    """a Fraction rounded to the nearest float32, ties to even (normal range)"""
    if x == 0:
        return f32(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length() - 24
    while a / Fraction(2) ** e >= 1 << 24:
        e += 1
    while a / Fraction(2) ** e < 1 << 23:
        e -= 1
    y = a / Fraction(2) ** e
    n = y.numerator // y.denominator
    r = y - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return f32(s * float(n) * 2.0 ** e)


def emulated_F(info, pos):
    """The kernels' float F = fma(q - min_f, scale_f, 0.5f): the difference rounded to float32, the product and the sum exact, ONE rounding to
    float32.  The product of two float32 is exact in float64; where adding 0.5 to it is not (TwoSum says so), the element is redone in rationals."""
    _, scale, org = info
    out = np.empty(pos.shape, f32)
    for a in range(3):
        d = pos[:, a].astype(f32) - f32(org[a])
        p = d.astype(f64) * f64(f32(scale))
        t = p + 0.5
        bb = t - p
        err = (p - (t - bb)) + (0.5 - bb)
        F = t.astype(f32)
        for i in np.flatnonzero(err != 0):
            F[i] = _f32_of_fraction(Fraction(float(d[i])) * Fraction(float(f32(scale))) + Fraction(1, 2))
        out[:, a] = F
    return out


def emulated_index(info, pos):
    return np.trunc(emulated_F(info, pos)).astype(np.int64)


def dt_value(grid, info, idx):
    """DT3D::Distance on a voxel index (x, y, z): the grid's value, or outside the grid the face value plus the overshoot -- the oracle's operations"""
    V, scale, _ = info
    a = np.where(idx < 0, idx, np.where(idx >= V, idx - V + 1, 0)).astype(f32)
    c = np.clip(idx, 0, V - 1)
    g = grid[c[:, 2], c[:, 1], c[:, 0]].astype(f32)
    s = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    out = g.copy()
    o = ((idx < 0) | (idx >= V)).any(1)
    out[o] = (np.sqrt(s[o]).astype(f64) / scale + g[o].astype(f64)).astype(f32)
    return out


def analyse(info, grid, pos, d):
    """Per lookup position: the exact and the emulated index; which of its coordinates are adversarial (exact F within NEAR of an integer k) and,
    for those, whether the grid holds another value in the voxel across that boundary.  The boundary of int(F) at k: voxels k - 1 | k for k >= 1,
    -1 | 0 at k = -1 (truncation toward zero); at k = 0 both sides are voxel 0 -- an adversarial lookup that cannot be sharp.
    Asserts that dt_value on the exact index is `d` (the oracle's distance of the position), bit for bit."""
    F, ex, k, adv, sharp, v0 = sharpness(info, grid, pos)
    em = emulated_index(info, pos)
    assert np.array_equal(v0.view(u32), np.asarray(d, f32).view(u32)), "dt_value is not the oracle's distance"
    return dict(F=F, ex=ex, em=em, k=k, adv=adv, sharp=sharp, wrong=(ex != em).any(1))


def sharpness(info, grid, pos):
    """-> exact F, exact index, nearest integer k of F, adversarial mask, sharp mask (all (n, 3)), the grid's value at the exact index"""
    F = exact_F(info, pos)
    ex = np.trunc(F).astype(np.int64)
    k = np.rint(F)
    adv = np.abs(F - k) <= NEAR
    lo, hi = np.trunc(k - 0.25).astype(np.int64), np.trunc(k + 0.25).astype(np.int64)
    across = np.where(ex == hi, lo, hi)
    v0 = dt_value(grid, info, ex)
    sharp = np.zeros(adv.shape, bool)
    for a in range(3):
        other = ex.copy()
        other[:, a] = across[:, a]
        sharp[:, a] = dt_value(grid, info, other) != v0
    return F, ex, k.astype(np.int64), adv, sharp, v0


def preconditions(tag, an, sel=None):
    """the two preconditions of a case, printed and asserted: >= 20 lookups whose truncated float F gives another index than the exact
    expression, and >= 85 % of the adversarial lookups with another grid value across their boundary"""
    sel = slice(None) if sel is None else sel
    n_wrong, adv = int(an["wrong"][sel].sum()), an["adv"][sel]
    frac = float(an["sharp"][sel][adv].mean())
    print("%s: %d lookups, float index wrong for %d, %d adversarial coordinates, %.1f %% sharp" % (tag, len(an["wrong"][sel]), n_wrong, int(adv.sum()), 100 * frac))
    assert n_wrong >= 20, (tag, n_wrong)
    assert frac >= 0.85, (tag, frac)


def describe(info, an, pos, i):
    """what the test knows about lookup i, for a failure message"""
    Fe = emulated_F(info, pos[i:i + 1])[0]
    return dict(lookup=int(i), q=pos[i].tolist(), exact_F=an["F"][i].tolist(), float_F=Fe.tolist(), exact_index=an["ex"][i].tolist(), float_index=an["em"][i].tolist(),
                adversarial_axes=np.flatnonzero(an["adv"][i]).tolist(), k=an["k"][i].tolist())


def same_bits(got, want, what, info, an, pos, owner=None):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    bad = np.flatnonzero(got.view(u32) != want.view(u32))
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s: %d of %d differ; first %d: got %r want %r; %r" % (what, len(bad), len(got), i, float(got[i]), float(want[i]),
                                                                                   describe(info, an, pos, i if owner is None else int(owner[i]))))


# ----------------------------------------------------------------------------------------------
# the adversarial queries, from dt_info() alone
# ----------------------------------------------------------------------------------------------
def boundary_coords(info, axis, rng):
    """float32 coordinates on and around the rounding boundaries of one axis: k in {-1, 0, 1, 2, V-2 .. V+1} and up to 40 of 3 .. V-3;
    b = min + (k - 0.5) / scale; fl(b + o) for o in {0} and +-2^-e / scale, e = 10 .. 33, each stepped by -4 .. +4 ulps; without duplicates"""
    V, scale, org = info
    inner = np.arange(3, V - 2)
    ks = np.concatenate([[-1, 0, 1, 2, V - 2, V - 1, V, V + 1], rng.choice(inner, min(40, len(inner)), replace=False)])
    o = np.concatenate([[0.0], [s * 2.0 ** -e / scale for e in range(10, 34) for s in (1, -1)]])
    b = org[axis] + (ks.astype(f64) - 0.5) / scale
    c = (b[:, None] + o[None, :]).astype(f32).reshape(-1)
    out, up, dn = [c], c, c
    for _ in range(4):
        up, dn = np.nextafter(up, f32(np.inf)), np.nextafter(dn, f32(-np.inf))
        out += [up, dn]
    return np.unique(np.concatenate(out))


@functools.lru_cache(maxsize=None)
def _queries(tgt, V):
    """the lookups of case (a): every boundary coordinate of every axis on its own (the other two axes mid-voxel), and 1 500 queries each with
    two and with three adversarial coordinates, half of those drawn from the coordinates whose float index is wrong.  The mid-voxel places
    (voxels 2 .. V-3) are drawn so that the lookup is sharp where that can be had (settle).  Read-only, with the oracle's distances and the
    analysis on the oracle's grid."""
    info = _info(tgt, V)
    _, scale, org = info
    rng = np.random.default_rng(1000 * V + (tgt == "B"))
    coords = [boundary_coords(info, a, rng) for a in range(3)]

    def mid(n, a):
        return (org[a] + rng.integers(2, V - 2, n) / scale).astype(f32)            # F = j + 0.5

    def wrong_pool(a):
        q = np.stack([mid(len(coords[a]), b) for b in range(3)], 1)
        q[:, a] = coords[a]
        w = coords[a][(exact_index(info, q) != emulated_index(info, q))[:, a]]
        return w if len(w) else coords[a]

    pools = [wrong_pool(a) for a in range(3)]
    grid = _oracle_dt(tgt, V).grid()

    def settle(make, n):
        """n queries from make(rows); a query with an adversarial coordinate across whose boundary the grid holds the same value on both sides
        (a wrong index there would not show) is drawn again, up to 8 times: the mid-voxel places and the combinations are the test's to choose"""
        q = make(np.arange(n))
        for _ in range(8):
            _, _, k, adv, sharp, _ = sharpness(info, grid, q)
            bad = np.flatnonzero((adv & ~sharp & (k != 0)).any(1))
            if not len(bad):
                break
            q[bad] = make(bad)
        return q

    def single(a):
        def make(rows):
            q = np.stack([mid(len(rows), b) for b in range(3)], 1)
            q[:, a] = coords[a][rows]
            return q
        return make

    def several(naxes):
        def make(rows):
            n = len(rows)
            q = np.stack([mid(n, b) for b in range(3)], 1)
            skip = rng.integers(0, 3, n) if naxes == 2 else np.full(n, -1)
            for a in range(3):
                c = np.where(rng.random(n) < 0.5, rng.choice(pools[a], n), rng.choice(coords[a], n))
                q[:, a] = np.where(skip == a, q[:, a], c)
            return q
        return make

    parts = [settle(single(a), len(coords[a])) for a in range(3)] + [settle(several(naxes), 1500) for naxes in (2, 3)]
    pos = np.ascontiguousarray(np.concatenate(parts).astype(f32))
    d = _oracle_dt(tgt, V).distance(pos)
    an = analyse(info, _oracle_dt(tgt, V).grid(), pos, d)
    for x in [pos, d] + list(an.values()):
        x.setflags(write=False)
    return pos, d, an


def small_batch(an, n=251, seed=5):
    """n < 256 lookups, up to 120 of them with a wrong float index, shuffled: groups of eight unrelated cubes and a ragged last one"""
    rng = np.random.default_rng(seed)
    w, r = np.flatnonzero(an["wrong"]), np.flatnonzero(~an["wrong"])
    w = rng.permutation(w)[:120]
    return rng.permutation(np.concatenate([w, rng.choice(r, n - len(w), replace=False)]))


# ----------------------------------------------------------------------------------------------
# engines: one per (target, grid, configuration, source), made on first use, closed with the module
# ----------------------------------------------------------------------------------------------
class Regs:
    def __init__(self, pkg):
        self.pkg, self.regs = pkg, {}

    def get(self, tgt, V, source, tag, inliers=None, **kw):
        key = (tgt, V, tag, inliers) + tuple(sorted(kw.items()))
        if key not in self.regs:
            if inliers is None:
                r = self.pkg.Registration(_target(tgt), source, 1e-3, dt_size=V, **kw)
            else:
                r = _trim_reg(self.pkg, _target(tgt), source, inliers, dt_size=V, **kw)
            got, want = r.dt_info(), _info(tgt, V)
            assert got[0] == want[0] and got[1] == want[1] and tuple(got[2]) == want[2], ("the engine's grid geometry is not the oracle's", got, want)
            self.regs[key] = r
        return self.regs[key]

    def close(self):
        for r in self.regs.values():
            r.close()
        self.regs.clear()


@pytest.fixture(scope="module")
def regs(pkg):
    r = Regs(pkg)
    yield r
    r.close()


def _grid_of(reg, variant, tgt, V, oracle_mod):
    """the distance transform a variant looks up: the oracle's, or for the half grid the oracle's lookup over what that grid must hold"""
    return half_twin.half_dt(reg, oracle_mod) if variant == "fp16" else _oracle_dt(tgt, V)


# ----------------------------------------------------------------------------------------------
# (a) one query per cube: the generic per-cube path (S1), below 256 cubes and through the grouped launch
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("V", GRIDS)
@pytest.mark.parametrize("tgt", TARGETS)
def test_one_query_per_cube(pkg, regs, oracle_mod, tgt, V, variant):
    """source = the point (0, 0, 0), R = I, w = 0: goicp_eval_bounds returns Distance(q)^2 of the cube centre q, for both bounds"""
    info = _info(tgt, V)
    pos, d, an = _queries(tgt, V)
    reg = regs.get(tgt, V, np.zeros((1, 3), f32), "origin", **VARIANTS[variant])
    if variant == "fp16":
        dt = _grid_of(reg, variant, tgt, V, oracle_mod)
        d = dt.distance(pos)
        an = analyse(info, dt.grid(), pos, d)
    for name, sel in (("S1, 251 cubes", small_batch(an)), ("S1, grouped launch", np.arange(len(pos)))):
        tag = "(a) target %s grid %d %s %s" % (tgt, V, variant, name)
        preconditions(tag, an, sel)
        cubes = np.concatenate([pos[sel], np.zeros((len(sel), 1), f32)], 1)
        ub, lb = reg.eval_bounds(EYE, cubes, -1)
        same_bits(ub, d[sel] * d[sel], tag + " ub", info, an, pos, owner=sel)
        same_bits(lb, ub, tag + " lb == ub", info, an, pos, owner=sel)


# ----------------------------------------------------------------------------------------------
# (b) sibling sets over a one-point source
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sibling_case(tgt, V, src):
    """For a selection of case (a)'s queries q (every one with a wrong float index up to 500, 300 others, up to 200 on the grid's ends) and the
    source point p (`src`: "origin" or "offset" = P_OFF): the two translation nodes whose child (0, 0, 0) resp. (1, 1, 1) has its centre at
    q - p, so that the child looks up fl(p + (q - p)) = q.  Every child's own lookup position is formed with the engine's float operations
    (_children, then p + t), and everything expected or counted is taken from those positions.
    -> parents (2 n, 4), kids (16 n, 4), look (16 n, 3), oracle distances, analysis, class of each node for the tile counters (0 inner, 1 edge, 2 outer)"""
    info = _info(tgt, V)
    pos, _, an = _queries(tgt, V)
    rng = np.random.default_rng(77 + V)
    p = np.zeros(3, f32) if src == "origin" else P_OFF
    half = W / f32(2)
    t0 = (pos - p).astype(f32)
    c0, c7 = t0 - half, (t0 - W) - half                                   # the two nodes' corners
    hits = ((p + (c0 + half) == pos) & (p + ((c7 + W) + half) == pos)).all(1)      # the float operations land on q again (q - p is not always a float)
    ends = (an["adv"] & np.isin(an["k"], [-1, V, V + 1])).any(1)
    w_, o_, e_ = np.flatnonzero(an["wrong"] & hits), np.flatnonzero(~an["wrong"] & ~ends & hits), np.flatnonzero(ends & hits)
    pick = np.unique(np.concatenate([rng.permutation(w_)[:500], rng.choice(o_, 300, replace=False), rng.permutation(e_)[:200]]))
    q = pos[pick]
    par = np.empty((2 * len(q), 4), f32)
    par[0::2, :3] = c0[pick]
    par[1::2, :3] = c7[pick]
    par[:, 3] = f32(2) * W
    kids = np.concatenate([_children(x) for x in par])
    look = np.ascontiguousarray((p[None, :] + kids[:, :3]).astype(f32))
    assert (look[0::16] == q).all() and (look[15::16] == q).all(), "the construction misses its queries"
    cls = np.where(ends[pick], 2, np.where(((an["ex"][pick] >= 3) & (an["ex"][pick] <= V - 4)).all(1), 0, 1))
    d = _oracle_dt(tgt, V).distance(look)
    an2 = analyse(info, _oracle_dt(tgt, V).grid(), look, d)
    for x in [par, kids, look, d, cls] + list(an2.values()):
        x.setflags(write=False)
    return par, kids, look, d, an2, np.repeat(cls, 2)


def expected_terms(d, rho, delta):
    """(ub, lb) of one point's lookup d, all in float32: m = max(d - rho, 0), ub = m^2, lb = max(m - delta, 0)^2"""
    m = np.maximum(np.asarray(d, f32) - f32(rho), f32(0))
    dis = np.maximum(m - f32(delta), f32(0))
    return m * m, dis * dis


def _rho(oracle_mod, src, level):
    if level < 0:
        return f32(0)
    return f32(oracle_mod.rot_radii(np.zeros((1, 3), f32) if src == "origin" else P_OFF[None, :])[1][level][0])


def _source_of(src):
    return np.zeros((1, 3), f32) if src == "origin" else np.ascontiguousarray(P_OFF[None, :])


SIB_ROUTES = [("origin", -1), ("offset", -1), ("offset", LEVEL)]


@pytest.mark.parametrize("variant", sorted(VARIANTS) + ["pairs"])
@pytest.mark.parametrize("V", GRIDS)
@pytest.mark.parametrize("tgt", TARGETS)
def test_sibling_sets(pkg, regs, oracle_mod, tgt, V, variant):
    """goicp_eval_bounds on the 8 children of every node: bricked -> lean_points (S3; level -1: LAST_ZERO, level 12 with |p| > 0: not),
    linear and fp16 -> sibling_residuals_rotated (S2), pairs (bounds_order 2) -> lean_index (S4), asserted from goicp_debug_bounds_order"""
    info = _info(tgt, V)
    lib = pkg.load_library()
    delta = lib.goicp_trans_delta(float(W))
    kw = PAIRS if variant == "pairs" else VARIANTS[variant]
    for src, level in SIB_ROUTES:
        par, kids, look, d, an, _ = _sibling_case(tgt, V, src)
        reg = regs.get(tgt, V, _source_of(src), src, **kw)
        if variant == "fp16":
            dt = _grid_of(reg, variant, tgt, V, oracle_mod)
            d = dt.distance(look)
            an = analyse(info, dt.grid(), look, d)
        tag = "(b) target %s grid %d %s source %s level %d" % (tgt, V, variant, src, level)
        preconditions(tag, an)
        if level >= 0:
            assert reg.rot_coeff(level) == oracle_mod.rot_coeff(level)
        rho = _rho(oracle_mod, src, level)
        assert level < 0 or rho > 0
        ub, lb = reg.eval_bounds(EYE, kids, level)
        if variant == "pairs":
            form = (C.c_int32 * 3)()
            assert lib.goicp_debug_bounds_order(reg.handle, form) == 0
            assert tuple(form) == (2, 1, len(par) // 2), tuple(form)
        wu, wl = expected_terms(d, rho, delta)
        same_bits(ub, wu, tag + " ub", info, an, look)
        same_bits(lb, wl, tag + " lb", info, an, look)


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("V", GRIDS)
@pytest.mark.parametrize("tgt", TARGETS)
def test_sibling_sets_trimmed(pkg, regs, oracle_mod, tgt, V, layout):
    """the trimmed kernel's sibling form: a two-point source, inliers 1; the far point has the larger residual under every cube and is dropped"""
    info = _info(tgt, V)
    delta = pkg.load_library().goicp_trans_delta(float(W))
    for src, level in SIB_ROUTES:
        par, kids, look, d, an, _ = _sibling_case(tgt, V, src)
        reg = regs.get(tgt, V, np.ascontiguousarray(np.stack([_source_of(src)[0], FAR])), src + "+far", inliers=1, dt_layout=layout)
        assert reg.inliers == 1
        tag = "(b) trimmed target %s grid %d layout %d source %s level %d" % (tgt, V, layout, src, level)
        preconditions(tag, an)
        assert d.max() < 100                                              # the far point's residual is several hundred under every cube
        ub, lb = reg.eval_bounds(EYE, kids, level)
        wu, wl = expected_terms(d, _rho(oracle_mod, src, level), delta)
        same_bits(ub, wu, tag + " ub", info, an, look)
        same_bits(lb, wl, tag + " lb", info, an, look)


def _tile_call(pkg, reg, par, nseg, n, level):
    """goicp_debug_bounds_tile, every segment under the identity -> (ub tile, lb tile, ub direct, lb direct), (staged, not staged)"""
    out = [np.full(8 * nseg * n, np.nan, f32) for _ in range(4)]
    ms = (C.c_float * 2)()
    st = (C.c_uint32 * 2)()
    rots = np.ascontiguousarray(np.tile(EYE.reshape(-1), nseg))
    pkg.binding.check(reg._lib.goicp_debug_bounds_tile(reg.handle, _fp(rots), _fp(np.ascontiguousarray(par.reshape(-1))), nseg, n, level, 1,
                                                        _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), ms, st))
    return out, (int(st[0]), int(st[1]))


@pytest.mark.parametrize("V", GRIDS)
@pytest.mark.parametrize("tgt", TARGETS)
def test_sibling_sets_tile(pkg, regs, oracle_mod, tgt, V):
    """goicp_debug_bounds_tile: a segment = the two nodes of one query, one 1-point sub-patch.  The tile kernel (S5 when staged, else S2) and the
    direct kernel of the same call (S3), bit for bit.  Queries wholly inside voxels 3 .. V-4 are all staged (the box: their lookups, a child
    width < a voxel and a voxel of margin each way); queries on the boundaries k in {-1, V, V+1} all fall back (the box reaches over the face)."""
    info = _info(tgt, V)
    delta = pkg.load_library().goicp_trans_delta(float(W))
    for src, level in SIB_ROUTES:
        par, kids, look, d, an, cls = _sibling_case(tgt, V, src)
        reg = regs.get(tgt, V, _source_of(src), src, **VARIANTS["bricked"])
        wu, wl = expected_terms(d, _rho(oracle_mod, src, level), delta)
        for c, name in ((0, "inner"), (1, "edge"), (2, "outer")):
            nodes = np.flatnonzero(cls == c)
            kid_sel = (nodes[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
            nseg = len(nodes) // 2
            tag = "(b) tile target %s grid %d source %s level %d, %s" % (tgt, V, src, level, name)
            if c != 1:
                preconditions(tag, an, kid_sel)
            out, st = _tile_call(pkg, reg, par[nodes], nseg, 2, level)
            print("%s: %d segments, staged %d, fallen back %d" % (tag, nseg, st[0], st[1]))
            assert st[0] + st[1] == nseg
            if c == 0:
                assert st == (nseg, 0), (tag, st)
            if c == 2:
                assert st == (0, nseg), (tag, st)
            for got, want, what in ((out[0], wu, "tile ub"), (out[1], wl, "tile lb"), (out[2], wu, "direct ub"), (out[3], wl, "direct lb")):
                same_bits(got, want[kid_sel], tag + " " + what, info, an, look, owner=kid_sel)


@pytest.mark.parametrize("V", GRIDS)
@pytest.mark.parametrize("tgt", TARGETS)
def test_sibling_sets_queue_round(pkg, regs, oracle_mod, tgt, V):
    """goicp_debug_queue_expand: both searches list every node, twin fusion on -> lean_points with NP = 2; both passes bit for bit.  The nodes
    with a wrong float index in a child's lookup first, 512 nodes in rounds of 128."""
    info = _info(tgt, V)
    delta = pkg.load_library().goicp_trans_delta(float(W))
    for src in ("origin", "offset"):
        par, kids, look, d, an, _ = _sibling_case(tgt, V, src)
        reg = regs.get(tgt, V, _source_of(src), src, **VARIANTS["bricked"])
        node_wrong = an["wrong"].reshape(-1, 8).any(1)
        nodes = np.concatenate([np.flatnonzero(node_wrong), np.flatnonzero(~node_wrong)])[:512]
        kid_sel = (nodes[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
        tag = "(b) queue round target %s grid %d source %s" % (tgt, V, src)
        preconditions(tag, an, kid_sel)
        want = (expected_terms(d, f32(0), delta), expected_terms(d, _rho(oracle_mod, src, LEVEL), delta))
        for s0 in range(0, len(nodes), 128):
            nd = nodes[s0:s0 + 128]
            ks = (nd[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
            out = [np.full(8 * len(nd), np.nan, f32) for _ in range(4)]
            qi = (C.c_int32 * 2)()
            pkg.binding.check(reg._lib.goicp_debug_queue_expand(reg.handle, _fp(np.ascontiguousarray(EYE.reshape(-1))), LEVEL, _fp(np.ascontiguousarray(par[nd].reshape(-1))),
                                                                len(nd), _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), qi))
            assert qi[1] == 1, "twin fusion is off"
            for ps in range(2):
                same_bits(out[2 * ps], want[ps][0][ks], "%s pass %d ub" % (tag, ps), info, an, look, owner=ks)
                same_bits(out[2 * ps + 1], want[ps][1][ks], "%s pass %d lb" % (tag, ps), info, an, look, owner=ks)


# ----------------------------------------------------------------------------------------------
# (c) full wavefronts: the source points are the queries
# ----------------------------------------------------------------------------------------------
C_NODES = np.array([[-W / 2, -W / 2, -W / 2, 2 * W], [-3 * W / 2, -3 * W / 2, -3 * W / 2, 2 * W], [-W / 2, -3 * W / 2, -W / 2, 2 * W]], f32)   # child 0, child 7, child 2 at t = 0


@functools.lru_cache(maxsize=None)
def _wave_case(tgt, V, N):
    """N source points inside a window of 14 voxels per axis at the grid's centre (so that a 64-point sub-patch of the tile kernel fits its
    LDS box and is staged): the even places hold points with three adversarial coordinates (case (a)'s, 70 % of them drawn from those whose
    float index is wrong), the odd places mid-voxel points; at N = 257 three and at N = 513 six places hold queries beyond the grid's faces
    (their wavefronts fail the lean loop's all-inside test, their sub-patches fall back whole, their pair members are given up).  The engine's order is
    k-d order unless that unmixes the wavefronts (then input order).  -> source, morton_sort, the points in the engine's order, per node and child
    the oracle's terms at level -1 and LEVEL (float32, in input order), the largest move of a child's sum under the emulated index"""
    import oracle as O
    pkg = load_pkg()
    info = _info(tgt, V)
    _, scale, org = info
    dt = _oracle_dt(tgt, V)
    pos, _, an = _queries(tgt, V)
    rng = np.random.default_rng(N + V)
    lo = V // 2 - 7                                                     # the window: voxels lo .. lo + 13 on every axis
    n_adv = (N + 1) // 2
    src = np.stack([(org[a] + rng.integers(lo, lo + 14, N) / scale).astype(f32) for a in range(3)], 1)
    for a in range(3):
        one = pos[an["adv"][:, a] & (an["adv"].sum(1) == 1) & (an["ex"][:, a] >= lo) & (an["ex"][:, a] <= lo + 13)]
        bad = (exact_index(info, one) != emulated_index(info, one))[:, a]
        pool_w, pool = one[bad, a] if bad.any() else one[:, a], one[:, a]       # (off the origin an axis of coarse floats has few wrong ones)
        src[0::2, a] = np.where(rng.random(n_adv) < 0.7, rng.choice(pool_w, n_adv), rng.choice(pool, n_adv))
    is_adv = np.zeros(N, bool)
    is_adv[0::2] = True
    n_out = 0
    if N > 64:
        ends = np.flatnonzero((an["adv"] & np.isin(an["k"], [-1, V, V + 1])).any(1) & ((an["ex"] < 0) | (an["ex"] >= V)).any(1))
        where = np.array([1, 65, 129] if N == 257 else [1, 65, 67, 129, 193, 255])
        src[where] = pos[rng.choice(ends, len(where), replace=False)]
        n_out = len(where)
    src = np.ascontiguousarray(src)
    morton = 2
    order = pkg.fgoicp.source_order(src, 2)
    mixed = lambda o: all(0 < is_adv[o[s:s + 64]].sum() < len(o[s:s + 64]) for s in range(0, N - 1, 64))
    if not mixed(order):
        morton, order = 0, np.arange(N)
    assert mixed(order)
    _, rho = O.rot_radii(src)
    terms, move = {}, 0.0
    for level in (-1, LEVEL):
        r = rho[level] if level >= 0 else None
        for ni, node in enumerate(C_NODES):
            for c, kid in enumerate(_children(node)):
                m = O.cube_terms(dt, src, r, kid[:3], kid[3])
                terms[(level, ni, c)] = m
                look = (src + kid[None, :3]).astype(f32)
                v = dt_value(dt.grid(), info, emulated_index(info, look))
                m_em = np.maximum(v - (r if r is not None else f32(0)), f32(0))
                a, b = twins.bound_ref(m, kid[3])[0], twins.bound_ref(m_em, kid[3])[0]
                if level < 0:
                    move = max(move, abs(a - b) / max(a, 1e-3))
    src.setflags(write=False)
    return src, morton, n_out, terms, move


def _check_children(got_ub, got_lb, terms, level, nodes, trunc, inliers, tag):
    worst = 0.0
    for j, ni in enumerate(nodes):
        for c in range(8):
            fu, fl = twins.bound_ref(terms[(level, ni, c)], W, trunc, inliers)
            u, l = got_ub[8 * j + c], got_lb[8 * j + c]
            dev = max(_rel(u, fu), _rel(l, fl))
            worst = max(worst, dev)
            assert dev <= TOL and l <= u, (tag, level, ni, c, float(u), fu, float(l), fl, dev)
    return worst


@pytest.mark.parametrize("N", [64, 257, 513])
@pytest.mark.parametrize("V", GRIDS)
@pytest.mark.parametrize("tgt", TARGETS)
def test_full_wavefronts(pkg, regs, oracle_mod, tgt, V, N):
    """Risky and safe lanes in the same wavefronts, against the float64 sums of the oracle's terms at TOL: eval_bounds on sibling cubes (plain,
    truncated, trimmed), the pair kernel, the tile kernel with the direct kernel, and the queue round (plain and truncated)."""
    lib = pkg.load_library()
    src, morton, n_out, terms, move = _wave_case(tgt, V, N)
    tag = "(c) target %s grid %d N %d" % (tgt, V, N)
    print("%s: morton_sort %d, %d points beyond the grid; the largest move of a child's upper bound under the truncated float index: %.2e (%.0f x TOL)"
          % (tag, morton, n_out, move, move / TOL))
    assert move >= 50 * TOL, (tag, move)
    kids = np.concatenate([_children(x) for x in C_NODES])
    nodes = range(len(C_NODES))
    worst = {}
    reg = regs.get(tgt, V, src, "wave%d" % N, morton_sort=morton, **VARIANTS["bricked"])
    preg = regs.get(tgt, V, src, "wave%d" % N, morton_sort=morton, **PAIRS)
    treg = regs.get(tgt, V, src, "wave%d" % N, inliers=N - 1, morton_sort=morton, dt_layout=1)
    for trunc in (0.0, TRUNC_G):
        name = "truncated" if trunc else "plain"
        for r in (reg, preg):
            r.set_search_truncation(trunc)
        try:
            for level in (-1, LEVEL):
                ub, lb = reg.eval_bounds(EYE, kids, level)
                worst[name + " eval"] = max(worst.get(name + " eval", 0), _check_children(ub, lb, terms, level, nodes, trunc, None, tag + " eval " + name))
                ub, lb = preg.eval_bounds(EYE, kids, level)
                form = (C.c_int32 * 3)()
                assert lib.goicp_debug_bounds_order(preg.handle, form) == 0 and tuple(form) == (2, 1, 2), tuple(form)
                worst[name + " pairs"] = max(worst.get(name + " pairs", 0), _check_children(ub, lb, terms, level, nodes, trunc, None, tag + " pairs " + name))
                out, st = _tile_call(pkg, reg, C_NODES, 1, len(C_NODES), level)
                worst[name + " tile"] = max(worst.get(name + " tile", 0), _check_children(out[0], out[1], terms, level, nodes, trunc, None, tag + " tile " + name))
                worst[name + " direct"] = max(worst.get(name + " direct", 0), _check_children(out[2], out[3], terms, level, nodes, trunc, None, tag + " direct " + name))
                assert st == (1, 0) if N == 64 else (st[0] > 0 and st[1] > 0), (tag, st)   # staged; with points beyond the grid: some sub-patches of each kind
            out = [np.full(8 * len(C_NODES), np.nan, f32) for _ in range(4)]
            qi = (C.c_int32 * 2)()
            pkg.binding.check(lib.goicp_debug_queue_expand(reg.handle, _fp(np.ascontiguousarray(EYE.reshape(-1))), LEVEL, _fp(np.ascontiguousarray(C_NODES.reshape(-1))),
                                                           len(C_NODES), _fp(out[0]), _fp(out[1]), _fp(out[2]), _fp(out[3]), qi))
            assert qi[1] == 1
            w0 = _check_children(out[0], out[1], terms, -1, nodes, trunc, None, tag + " queue upper-bound pass " + name)
            w1 = _check_children(out[2], out[3], terms, LEVEL, nodes, trunc, None, tag + " queue lower-bound pass " + name)
            worst[name + " queue"] = max(w0, w1)
        finally:
            for r in (reg, preg):
                r.set_search_truncation(0.0)
    for level in (-1, LEVEL):
        ub, lb = treg.eval_bounds(EYE, kids, level)
        worst["trimmed eval"] = max(worst.get("trimmed eval", 0), _check_children(ub, lb, terms, level, nodes, 0.0, N - 1, tag + " trimmed"))
    print("%s: worst rel deviation %s" % (tag, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


# ----------------------------------------------------------------------------------------------
# (d) the off-origin target elsewhere: bit-exact bars and the first pass's error
# ----------------------------------------------------------------------------------------------
def test_off_origin_nn_query_and_first_pass(pkg, oracle_mod):
    """target B: nn_query of 800 queries (on the target, near it, around the cloud, outside the grid) == oracle.nn_brute in indices and distance
    bits; the first plain ICP pass's error within ERR_REL of the float64 sum of the brute-force distances.  No pose is held."""
    c = _case(M_ICP, 257, outliers=False)
    target = np.ascontiguousarray((c["target"] + SHIFT).astype(f32))
    t0 = (c["t0"] + SHIFT).astype(f32)
    reg = pkg.Registration(target, c["source"], 1e-3, dt_size=32)
    try:
        q = _knn_queries(target, 800, 41)
        bi, bd = oracle_mod.nn_brute(target, q)
        idx, d2 = reg.nn_query(q)
        assert np.array_equal(idx, bi), int(np.sum(idx != bi))
        assert np.array_equal(d2.view(u32), bd.view(u32)), int(np.sum(d2.view(u32) != bd.view(u32)))
        moved = _transform_f32(c["R0"], t0, c["source"])
        mi, md = oracle_mod.nn_brute(target, moved)
        idx, d2 = reg.nn_query(moved)
        assert np.array_equal(idx, mi) and np.array_equal(d2.view(u32), md.view(u32))
        _, _, err, _ = _run(reg, c["R0"], t0, max_iter=1)
        ref = float(np.sum(md.astype(f64)))
        e_rel = abs(float(err) - ref) / ref
        print("(d) target B: 800 + 257 neighbours bit-equal; first-pass error rel %.2e" % e_rel)
        assert e_rel <= ERR_REL, (float(err), ref)
    finally:
        reg.close()
