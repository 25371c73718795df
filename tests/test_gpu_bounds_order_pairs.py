"""Footprint-ordered and paired bound launches (Params::bounds_order 1 and 2) against the plain launch (0): the raw float bits of every
upper and lower bound must be equal -- the order only changes which workgroup evaluates a group when, a pair only shares the point
load and the rotation between two groups, and every group writes its own rows.  Every comparison also reads back which form was launched
and what the device pre-pass decided (goicp_debug_bounds_order), so a gate that always fell back to the plain launch would fail it.

Tiny synthetic clouds (N = 257, 1 000, 5 003: partial last wavefronts, one to twenty point chunks, both chunk-to-XCD mappings) on a
64^3 bricked grid; bounds_order_min_groups is lowered so that batches of a few groups reach the ordered and the paired code, and
bounds_order_max_runs = 4 so that a batch of five rotation runs takes the bypass; bounds_order_reprobe = 0 (every batch runs the pre-pass)
except in the test of that hint.  The grid spans [-2, 2]^3 at 16 voxels per unit:
child spacing 8 voxels for parent width 1 (two dword gathers per x-sibling pair), 1 voxel for width 1/8 (merged x rows).
"""
import ctypes as C

import numpy as np
import pytest


pytestmark = pytest.mark.gpu

SIZES = (257, 1000, 5003)
CUBE = np.dtype([("tx", "<f4"), ("ty", "<f4"), ("tz", "<f4"), ("delta", "<f4"), ("coeff", "<f4"), ("rot", "<i4")])
N_ROT = 6
MAX_RUNS = 4
THRESHOLD = 5


@pytest.fixture(scope="module")
def pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()          # fails loudly if the HIP extension is missing
    return m


class _Hip:
    """Device buffers for the device-pointer entry point, from the runtime the library itself links against."""

    def __init__(self):
        h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes, h.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h, self.live = h, []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.h.hipMalloc(C.byref(p), max(int(nbytes), 4)) == 0
        self.live.append(p)
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.h.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return p

    def download(self, p, n, dtype):
        assert self.h.hipDeviceSynchronize() == 0              # the entry point queues on the engine's stream
        out = np.empty(n, dtype)
        assert self.h.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, out.nbytes, 2) == 0
        return out

    def free_all(self):
        for p in self.live:
            self.h.hipFree(p)
        self.live = []


@pytest.fixture(scope="module")
def hip():
    h = _Hip()
    yield h
    h.free_all()


def _clouds(n):
    """a bumpy unit-box shell: target 2 000 points, source n points of the same surface"""
    rng = np.random.default_rng(n)

    def shell(m):
        d = rng.normal(size=(m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = 0.6 + 0.25 * np.sin(3.0 * d[:, 0]) * np.cos(2.0 * d[:, 1])
        return (d * r[:, None] * np.array([1.0, 0.8, 0.6])).astype(np.float32)

    target = shell(2000)
    target[0], target[1] = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)      # pins the grid to [-2, 2]^3
    return target, shell(n)


class _Regs:
    """the three forms of one engine configuration, created when first asked for and kept for the module"""

    def __init__(self, pkg):
        self.pkg, self.regs, self.clouds = pkg, {}, {}

    def get(self, n, order, min_groups=1, trunc=None, fresh=False, reprobe=0):
        key = (n, order, min_groups, trunc, reprobe)
        if fresh or key not in self.regs:
            if n not in self.clouds:
                self.clouds[n] = _clouds(n)
            t, s = self.clouds[n]
            r = self.pkg.Registration(t, s, 1e-3, dt_size=64, trunc_dist=trunc, bounds_order=order, bounds_order_min_groups=min_groups,
                                      bounds_order_max_runs=MAX_RUNS, bounds_order_reprobe=reprobe)
            if fresh:
                return r
            self.regs[key] = r
        return self.regs[key]

    def close(self):
        for r in self.regs.values():
            r.close()


@pytest.fixture(scope="module")
def regs(pkg):
    r = _Regs(pkg)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rots(pkg):
    rng = np.random.default_rng(7)
    return np.stack([pkg.fgoicp.rodrigues(rng.uniform(-2.0, 2.0, 3)) for _ in range(N_ROT)]).astype(np.float32)


def _expansions(pkg, rng, rot, level=None, coeff=None, centre=None):
    """one sibling set per entry of `rot`, built as the search builds them (corner + bit * w + w / 2); level = log2 of 1 / parent width"""
    lib = pkg.binding.load_library()
    g = len(rot)
    level = rng.integers(0, 4, g) if level is None else np.broadcast_to(level, g)
    coeff = np.where(np.arange(g) % 2 == 1, rng.uniform(0.02, 0.3, g), 0.0) if coeff is None else np.broadcast_to(coeff, g)
    pw = (1.0 / (1 << np.asarray(level))).astype(np.float32)
    centre = rng.uniform(-0.5, 0.5, (g, 3)) if centre is None else np.broadcast_to(centre, (g, 3))
    corner = (np.asarray(centre, np.float64) - pw[:, None] / 2).astype(np.float32)
    w = pw / np.float32(2)
    j = np.arange(8)
    off = np.stack([j & 1, (j >> 1) & 1, (j >> 2) & 1], 1).astype(np.float32)
    c = corner[:, None, :] + off[None] * w[:, None, None] + (w / np.float32(2))[:, None, None]
    recs = np.zeros(8 * g, CUBE)
    recs["tx"], recs["ty"], recs["tz"] = c[..., 0].ravel(), c[..., 1].ravel(), c[..., 2].ravel()
    recs["delta"] = np.repeat(np.array([lib.goicp_trans_delta(float(x)) for x in w], np.float32), 8)
    recs["coeff"] = np.repeat(np.asarray(coeff, np.float32), 8)
    recs["rot"] = np.repeat(np.asarray(rot, np.int32), 8)
    return recs


def _eval(pkg, hip, reg, rots, recs):
    n = len(recs)
    d_rots, d_cubes = hip.upload(rots.reshape(-1)), hip.upload(np.ascontiguousarray(recs).view(np.uint8))
    d_ub, d_lb = hip.alloc(4 * n), hip.alloc(4 * n)
    pkg.binding.check(reg._lib.goicp_eval_bounds_device(reg.handle, d_rots, d_cubes, n, d_ub, d_lb, None))
    out = hip.download(d_ub, n, np.uint32), hip.download(d_lb, n, np.uint32)
    hip.free_all()
    return out


def _path(reg):
    """(form launched, 1 = the pre-pass built an order, items of the pair list) of the handle's last launch: goicp_debug_bounds_order"""
    info = (C.c_int32 * 3)()
    assert reg._lib.goicp_debug_bounds_order(reg.handle, info) == 0
    return tuple(info)


def _expected_path(recs, order, min_groups):
    """what the launch must have done: the plain form below the threshold; above it an order unless the batch has more runs of equal rotation
    (by each group's first record, in arrival order) than the cap; the pair list holds every run's pairs and its leftover"""
    rot = recs["rot"][0::8]
    if order == 0 or len(rot) < min_groups:
        return (0, 0, 0)
    starts = np.flatnonzero(np.concatenate([[True], rot[1:] != rot[:-1]]))
    if len(starts) > MAX_RUNS:
        return (order, 0, 0)
    lengths = np.diff(np.concatenate([starts, [len(rot)]]))
    return (order, 1, int(((lengths + 1) // 2).sum()))


def _same_bits(pkg, hip, regs, rots, recs, n, what, **kw):
    ref = _eval(pkg, hip, regs.get(n, 0, **kw), rots, recs)
    assert _path(regs.get(n, 0, **kw)) == (0, 0, 0), what
    assert np.isfinite(ref[0].view(np.float32)).all() and (ref[1].view(np.float32) <= ref[0].view(np.float32)).all(), what
    for order in (2, 1):
        got = _eval(pkg, hip, regs.get(n, order, **kw), rots, recs)
        assert _path(regs.get(n, order, **kw)) == _expected_path(recs, order, kw.get("min_groups", 1)), what
        for name, a, b in (("ub", got[0], ref[0]), ("lb", got[1], ref[1])):
            assert np.array_equal(a, b), "%s: bounds_order %d changed %d of %d %s (first at %d)" % (what, order, int((a != b).sum()), len(a), name, int(np.argmax(a != b)))


def _mixed(pkg, rng, g):
    """g groups over two rotation runs, random depths and passes"""
    return _expansions(pkg, rng, np.where(np.arange(g) < (g + 1) // 2, 1, 4))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("groups", (1, 2, 3, 9, 128))
def test_group_counts(pkg, hip, regs, rots, n, groups):
    """1, 2, 3, 9 groups (a single, a pair, a pair and a leftover, several) and 128 (eight point chunks at N = 5 003: the chunk-per-XCD mapping);
    each also with a partial last group -- B no multiple of 8 -- which is a pair member for an even count and a leftover for an odd one"""
    rng = np.random.default_rng(100 + groups)
    recs = _expansions(pkg, rng, np.zeros(groups, np.int32))
    _same_bits(pkg, hip, regs, rots, recs, n, "%d groups" % groups)
    _same_bits(pkg, hip, regs, rots, recs[:-3], n, "%d groups, partial last" % groups)


@pytest.mark.parametrize("groups", (THRESHOLD - 1, THRESHOLD, THRESHOLD + 1))
def test_threshold(pkg, hip, regs, rots, groups):
    rng = np.random.default_rng(200 + groups)
    _same_bits(pkg, hip, regs, rots, _mixed(pkg, rng, groups), 1000, "threshold %d, %d groups" % (THRESHOLD, groups), min_groups=THRESHOLD)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("runs", ((0, 0, 0, 1, 1, 1, 1), (0, 0, 1, 1, 1, 2, 2, 2, 2), (3, 3, 3, 5, 5, 3, 3, 3), (0, 1, 0, 1, 0, 1, 0, 1, 0, 1)),
                         ids=("two_runs", "three_runs", "recurring_rotation", "more_runs_than_cap"))
def test_rotation_runs(pkg, hip, regs, rots, n, runs):
    rng = np.random.default_rng(300 + len(runs))
    _same_bits(pkg, hip, regs, rots, _expansions(pkg, rng, np.array(runs, np.int32)), n, "runs %s" % (runs,))


def _pair_cases(pkg):
    rng = np.random.default_rng(400)
    r2 = np.array([2, 2], np.int32)
    cases = {}
    cases["pass"] = _expansions(pkg, rng, r2, level=1, coeff=[0.0, 0.17])
    cases["both_lower_bound"] = _expansions(pkg, rng, r2, level=1, coeff=[0.05, 0.17])
    cases["both_upper_bound"] = _expansions(pkg, rng, r2, level=2, coeff=[0.0, 0.0])
    cases["depth"] = _expansions(pkg, rng, r2, level=[0, 3], coeff=[0.0, 0.1])          # child spacing 8 voxels against 1: merged rows for one member only
    cases["deep_both"] = _expansions(pkg, rng, r2, level=[3, 3], coeff=[0.1, 0.0])
    d = _expansions(pkg, rng, r2, level=2, coeff=0.1)
    d["delta"][8:] *= np.float32(1.5)
    cases["delta"] = d
    one = _expansions(pkg, rng, r2[:1], level=2, coeff=0.1)
    cases["identical"] = np.concatenate([one, one])
    p = _expansions(pkg, rng, r2, level=1)
    p["tx"][11] += np.float32(0.01)
    cases["not_siblings"] = p
    f = _expansions(pkg, rng, r2, level=1)
    f["rot"][13] = 4
    cases["foreign_rotation"] = f
    g = np.zeros(64, CUBE)
    c = rng.uniform(-0.5, 0.5, (64, 3)).astype(np.float32)
    g["tx"], g["ty"], g["tz"] = c[:, 0], c[:, 1], c[:, 2]
    g["delta"], g["coeff"], g["rot"] = np.float32(0.03), np.where(np.arange(64) % 2, np.float32(0.1), np.float32(0)), rng.integers(0, N_ROT, 64)
    cases["generic"] = g
    g1 = g.copy()
    g1["rot"] = 1
    cases["generic_one_rotation"] = g1
    # part of the cloud (radius 0.2 .. 0.85) leaves the grid faces at +-2 under a translation of 1.7: the checked branch for one member, for both
    cases["outside_one"] = _expansions(pkg, rng, r2, level=2, coeff=[0.0, 0.1], centre=[[0.1, 0.0, -0.1], [1.7, 0.2, 0.0]])
    cases["outside_one_first"] = _expansions(pkg, rng, r2, level=2, coeff=[0.0, 0.1], centre=[[0.1, 0.0, -1.7], [0.3, 0.2, 0.0]])
    cases["outside_both"] = _expansions(pkg, rng, r2, level=2, coeff=[0.1, 0.0], centre=[[0.1, -1.7, -0.1], [1.7, 0.2, 0.0]])
    cases["outside_far"] = _expansions(pkg, rng, r2, level=1, coeff=[0.1, 0.0], centre=[[3.5, 0.0, 0.0], [0.0, 0.1, 0.0]])
    return cases


PAIR_CASES = ("pass", "both_lower_bound", "both_upper_bound", "depth", "deep_both", "delta", "identical", "not_siblings", "foreign_rotation", "generic",
              "generic_one_rotation", "outside_one", "outside_one_first", "outside_both", "outside_far")


@pytest.fixture(scope="module")
def pair_cases(pkg):
    return _pair_cases(pkg)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", PAIR_CASES)
def test_pair_members(pkg, hip, regs, rots, pair_cases, n, case):
    _same_bits(pkg, hip, regs, rots, pair_cases[case], n, case)


@pytest.mark.parametrize("n", SIZES)
def test_truncated_objective(pkg, hip, regs, rots, pair_cases, n):
    """trunc_dist > 0 (the TRUNC instantiations): every pair case in one batch per case, and a mixed batch of three rotation runs"""
    for case in PAIR_CASES:
        _same_bits(pkg, hip, regs, rots, pair_cases[case], n, "truncated " + case, trunc=0.3)
    rng = np.random.default_rng(500)
    _same_bits(pkg, hip, regs, rots, _expansions(pkg, rng, np.repeat([0, 5, 2], 7)), n, "truncated three runs", trunc=0.3)


@pytest.mark.parametrize("order", (1, 2))
def test_second_call_regrows_buffers(pkg, hip, regs, rots, order):
    """a handle that has served a small batch serves a larger one (its order and pair buffers grow) with the bits of a fresh handle"""
    rng = np.random.default_rng(600)
    small, large = _mixed(pkg, rng, 3), _mixed(pkg, rng, 41)[:-5]
    used = regs.get(1000, order, fresh=True)
    fresh = regs.get(1000, order, fresh=True)
    try:
        _eval(pkg, hip, used, rots, small)
        a = _eval(pkg, hip, used, rots, large)
        b = _eval(pkg, hip, fresh, rots, large)
        ref = _eval(pkg, hip, regs.get(1000, 0), rots, large)
        c = _eval(pkg, hip, used, rots, small)
        ref_small = _eval(pkg, hip, regs.get(1000, 0), rots, small)
    finally:
        used.close()
        fresh.close()
    for k in (0, 1):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], ref[k]) and np.array_equal(c[k], ref_small[k])


@pytest.mark.parametrize("order", (1, 2))
def test_left_alone_batches_skip_the_pre_pass(pkg, hip, regs, rots, pair_cases, order):
    """bounds_order_reprobe = 3: once the pre-pass has left a batch alone (more runs than the cap), batches of the same size take the plain
    launch, every third of them runs the pre-pass again, and a batch of another size runs it at once; the bits never change"""
    rng = np.random.default_rng(700)
    many = _expansions(pkg, rng, np.arange(10, dtype=np.int32) % 2)              # ten runs
    few = _expansions(pkg, rng, np.zeros(10, np.int32))                           # same size, one run
    other = _expansions(pkg, rng, np.zeros(7, np.int32))
    ref = {k: _eval(pkg, hip, regs.get(1000, 0), rots, v) for k, v in (("many", many), ("few", few), ("other", other))}
    reg = regs.get(1000, order, fresh=True, reprobe=3)
    try:
        seen = []
        for name, recs in (("many", many), ("many", many), ("few", few), ("many", many), ("many", many), ("other", other), ("few", few), ("few", few)):
            got = _eval(pkg, hip, reg, rots, recs)                                # the download waits for the launch: the note is there for the next call
            seen.append(_path(reg))
            assert np.array_equal(got[0], ref[name][0]) and np.array_equal(got[1], ref[name][1]), (name, seen)
    finally:
        reg.close()
    # pre-pass, left alone | skipped | skipped | third since: pre-pass again, left alone | skipped | another size: ordered | ordered | ordered
    assert seen == [(order, 0, 0), (0, 0, 0), (0, 0, 0), (order, 0, 0), (0, 0, 0), (order, 1, 4), (order, 1, 5), (order, 1, 5)], seen
