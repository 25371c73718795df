"""Coincident members of a pair item (Params::bounds_order 2, bounds_pair_kernel): two sibling sets of one rotation whose six translations and
delta are equal bit for bit are evaluated with one index set and one set of gathers per point -- the NP = 2 loop of the queue twins when
their coefficients differ (twin form), one plain evaluation stored to both groups' rows when those are equal too (identical form).  Anything
short of bit equality keeps the pair form.

Every case compares the raw bits of ub and lb with bounds_order = 0, reads back which form was launched and what the pre-pass decided
(goicp_debug_bounds_order) and how many items took the twin and the identical form (goicp_debug_bounds_twins) -- a kernel that never took
either would fail the tally, one that took them wrongly the bits.  Helpers, clouds (N = 257: one chunk, bounds written directly; 1 000;
5 003: partials and bounds_finalize; 64^3 bricked grid), bounds_order_max_runs = 4, bounds_order_min_groups = 1 and bounds_order_reprobe = 0
of test_gpu_bounds_order_pairs.py.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_bounds_order_pairs as P
from test_gpu_bounds_order_pairs import pkg, hip, regs, rots  # noqa: F401  (fixtures)


pytestmark = pytest.mark.gpu

SIZES = P.SIZES
CENTRE = (0.13, -0.07, 0.21)
R2 = np.array([2, 2], np.int32)


def _tally(reg):
    """(items in twin form, items in identical form) of the handle's last launch"""
    info = (C.c_int32 * 2)()
    assert reg._lib.goicp_debug_bounds_twins(reg.handle, info) == 0
    return tuple(info)


def _check(pkg, hip, regs, rots, recs, n, what, tally=None, least=None, reg=None, **kw):
    """bits against the plain launch, the pre-pass's decision, and the tally: `tally` exactly, or at least `least` items in both forms together"""
    ref_reg = regs.get(n, 0, **kw)
    ref = P._eval(pkg, hip, ref_reg, rots, recs)
    assert P._path(ref_reg) == (0, 0, 0) and _tally(ref_reg) == (0, 0), what
    assert np.isfinite(ref[0].view(np.float32)).all() and (ref[1].view(np.float32) <= ref[0].view(np.float32)).all(), what
    reg = regs.get(n, 2, **kw) if reg is None else reg
    got = P._eval(pkg, hip, reg, rots, recs)
    assert P._path(reg) == P._expected_path(recs, 2, 1), what
    seen = _tally(reg)
    for name, a, b in (("ub", got[0], ref[0]), ("lb", got[1], ref[1])):
        assert np.array_equal(a, b), "%s (tally %s): changed %d of %d %s (first at %d)" % (what, seen, int((a != b).sum()), len(a), name, int(np.argmax(a != b)))
    if tally is not None:
        assert seen == tally, (what, seen, tally)
    if least is not None:
        assert seen[0] + seen[1] >= least and min(seen) >= 0, (what, seen, least)
    return seen


def _copies(pkg, coeff, level=1, centre=CENTRE, rot=None):
    """len(coeff) expansions of one parent cube (same centre, same width), as the searches of a rotation child list them"""
    g = len(coeff)
    rot = np.full(g, 2, np.int32) if rot is None else np.asarray(rot, np.int32)
    return P._expansions(pkg, np.random.default_rng(0), rot, level=level, coeff=np.asarray(coeff, np.float32), centre=np.asarray(centre))


COINCIDENT = {
    # name: (coefficients, (twin form, identical form))
    "ub_lb": ([0.0, 0.17], (1, 0)),
    "lb_ub": ([0.17, 0.0], (1, 0)),
    "lb_lb_other": ([0.05, 0.17], (1, 0)),
    "ub_ub": ([0.0, 0.0], (0, 1)),
    "lb_lb_same": ([0.1, 0.1], (0, 1)),
    "zero_signs": ([0.0, -0.0], (0, 1)),
    "negative_zero_first": ([-0.0, 0.17], (1, 0)),
    "negative_zero_last": ([0.17, -0.0], (1, 0)),
    "negative_zero_twice": ([-0.0, -0.0], (0, 1)),
}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("level", (1, 3), ids=("dword_gathers", "merged_rows"))
@pytest.mark.parametrize("case", sorted(COINCIDENT))
def test_coincident_pair(pkg, hip, regs, rots, n, level, case):
    coeff, tally = COINCIDENT[case]
    _check(pkg, hip, regs, rots, _copies(pkg, coeff, level=level), n, case, tally=tally)


def _next(a):
    return np.nextafter(a, np.float32(np.inf), dtype=np.float32)


def _near_misses(pkg):
    cases = {}
    cases["other_width"] = _copies(pkg, [0.0, 0.17], level=[1, 2])
    for axis in ("tx", "ty", "tz"):
        bit = {"tx": 1, "ty": 2, "tz": 4}[axis]
        for side in (0, 1):
            r = _copies(pkg, [0.0, 0.17], level=2)
            sel = 8 + np.flatnonzero(((np.arange(8) & bit) != 0) == bool(side))          # the second group's children on one side: still a sibling set
            r[axis][sel] = _next(r[axis][sel])
            cases["%s%d_ulp" % (axis, side)] = r
    r = _copies(pkg, [0.1, 0.1], level=2)
    r["delta"][8:] = _next(r["delta"][8:])
    cases["delta_ulp"] = r
    r = _copies(pkg, [0.0, 0.0], level=2)
    r["tx"][:8] = 0.0
    r["tx"][8:] = -0.0                                         # equal as floats, not as bits: no children along x, +0 against -0
    cases["translation_zero_signs"] = r
    cases["partial_last_group"] = _copies(pkg, [0.0, 0.17])[:-3]
    r = _copies(pkg, [0.0, 0.17])
    r["rot"][13] = 4
    cases["foreign_rotation"] = r
    r = _copies(pkg, [0.0, 0.17])
    r["coeff"][11] = 0.2
    cases["not_siblings"] = r
    cases["two_rotation_runs"] = _copies(pkg, [0.0, 0.17], rot=[1, 4])
    cases["two_rotation_runs_of_two"] = _copies(pkg, [0.0, 0.17, 0.17, 0.0], rot=[1, 4, 4, 1])       # three runs: 1 | 4 4 | 1
    return cases


NEAR_MISSES = ("other_width", "tx0_ulp", "tx1_ulp", "ty0_ulp", "ty1_ulp", "tz0_ulp", "tz1_ulp", "delta_ulp", "translation_zero_signs", "partial_last_group",
               "foreign_rotation", "not_siblings", "two_rotation_runs")


@pytest.fixture(scope="module")
def near_misses(pkg):
    return _near_misses(pkg)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", NEAR_MISSES)
def test_not_twins(pkg, hip, regs, rots, near_misses, n, case):
    """the pair form (or the plain path, or two runs) for everything short of bit equality: tally 0"""
    _check(pkg, hip, regs, rots, near_misses[case], n, case, tally=(0, 0))


@pytest.mark.parametrize("n", SIZES)
def test_same_translation_in_neighbouring_runs(pkg, hip, regs, rots, near_misses, n):
    """runs 1 | 4 4 | 1 of one parent cube: only the two groups of the middle run meet in an item"""
    _check(pkg, hip, regs, rots, near_misses["two_rotation_runs_of_two"], n, "runs 1 | 4 4 | 1", tally=(0, 1))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", (7, 8))
def test_family_alone_in_a_run(pkg, hip, regs, rots, n, family):
    """all copies share a cell, so whatever order the pre-pass gives, neighbours are copies: floor(family / 2) items, and a leftover single for 7"""
    recs = _copies(pkg, np.full(family, 0.1))
    assert P._expected_path(recs, 2, 1) == (2, 1, 4)
    _check(pkg, hip, regs, rots, recs, n, "family of %d" % family, tally=(0, family // 2))
    mixed = _copies(pkg, np.where(np.arange(family) % 2, 0.17, 0.0))              # both searches' listings: each item is a twin or an identical pair
    seen = _check(pkg, hip, regs, rots, mixed, n, "mixed family of %d" % family, least=family // 2)
    assert seen[0] + seen[1] == family // 2, seen


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", (7, 8))
def test_family_with_strangers_in_its_cell(pkg, hip, regs, rots, n, family):
    """two other expansions a sixth of a voxel away (the smallest cell is a voxel): each breaks at most one pair of copies"""
    fam = _copies(pkg, np.full(family, 0.0))
    s1 = _copies(pkg, [0.1], level=2, centre=np.add(CENTRE, 0.01))
    s2 = _copies(pkg, [0.0], level=1, centre=np.add(CENTRE, (0.01, 0.0, 0.01)))
    recs = np.concatenate([fam[:24], s1, fam[24:40], s2, fam[40:]])
    seen = _check(pkg, hip, regs, rots, recs, n, "family of %d, two strangers" % family, least=family // 2 - 2)
    assert seen[0] == 0 and seen[1] <= family // 2, seen


OUTSIDE = {"partly": ((1.7, 0.2, 0.0), 2), "partly_low_z": ((0.1, 0.0, -1.7), 2), "wholly": ((3.5, 0.0, 0.0), 1)}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", sorted(OUTSIDE))
def test_coincident_pair_outside_the_grid(pkg, hip, regs, rots, n, where):
    """part of the cloud (radius 0.2 .. 0.85, grid to +-2) leaves a face under a translation of 1.7, all of it under 3.5: wavefronts of the
    twin and the identical form take the loop's checked branch"""
    centre, level = OUTSIDE[where]
    for coeff, tally in (([0.0, 0.1], (1, 0)), ([0.05, 0.1], (1, 0)), ([0.1, 0.1], (0, 1)), ([0.0, 0.0], (0, 1))):
        _check(pkg, hip, regs, rots, _copies(pkg, coeff, level=level, centre=centre), n, "%s outside, coefficients %s" % (where, coeff), tally=tally)


@pytest.mark.parametrize("n", SIZES)
def test_truncated_objective(pkg, hip, regs, rots, near_misses, n):
    """trunc_dist > 0 (the TRUNC instantiations): every coincident form inside and outside the grid, and the near misses"""
    for case in sorted(COINCIDENT):
        coeff, tally = COINCIDENT[case]
        for level in (1, 3):
            _check(pkg, hip, regs, rots, _copies(pkg, coeff, level=level), n, "truncated " + case, tally=tally, trunc=0.3)
    for where in sorted(OUTSIDE):
        centre, level = OUTSIDE[where]
        for coeff, tally in (([0.0, 0.1], (1, 0)), ([0.05, 0.1], (1, 0)), ([0.1, 0.1], (0, 1))):
            _check(pkg, hip, regs, rots, _copies(pkg, coeff, level=level, centre=centre), n, "truncated %s outside %s" % (where, coeff), tally=tally, trunc=0.3)
    for case in NEAR_MISSES:
        _check(pkg, hip, regs, rots, near_misses[case], n, "truncated " + case, tally=(0, 0), trunc=0.3)
    _check(pkg, hip, regs, rots, _copies(pkg, np.where(np.arange(7) % 2, 0.17, 0.0)), n, "truncated mixed family", least=3, trunc=0.3)


@pytest.mark.parametrize("n", SIZES)
def test_search_shaped_batch(pkg, hip, regs, rots, n):
    """two rotation runs, each the root listed by six searches among nine deeper expansions, partial last group.  The deeper centres lie 0.3
    to 0.5 (4.8 to 8 voxels) from the root's on every axis and a cell is 4 voxels, so the six copies have a cell to themselves: three
    coincident items per run, or two when an odd number of groups comes before that cell"""
    rng = np.random.default_rng(900)
    parts = []
    for rot in (1, 4):
        root = _copies(pkg, [0.0, 0.2, 0.0, 0.2, 0.2, 0.0], level=0, centre=(0.0, 0.0, 0.0), rot=np.full(6, rot))
        centre = rng.uniform(0.3, 0.5, (9, 3)) * rng.choice([-1.0, 1.0], (9, 3))
        deep = P._expansions(pkg, rng, np.full(9, rot, np.int32), level=rng.integers(1, 4, 9), centre=centre)
        parts.append(np.concatenate([root[:24], deep[:32], root[24:], deep[32:]]))     # the partial last group is a deeper one
    recs = np.concatenate(parts)[:-5]
    seen = _check(pkg, hip, regs, rots, recs, n, "search-shaped batch", least=4)
    assert seen[0] + seen[1] <= 6, seen


def test_batch_over_the_run_cap_afterwards(pkg, hip, regs, rots):
    """a handle that has just counted twins serves a batch of more runs than the cap: left alone, tally back at 0, bits equal"""
    reg = regs.get(1000, 2, fresh=True)
    try:
        _check(pkg, hip, regs, rots, _copies(pkg, [0.0, 0.17, 0.17, 0.17]), 1000, "before", least=2, reg=reg)
        many = _copies(pkg, np.where(np.arange(10) % 2, 0.17, 0.0), rot=np.arange(10) % 2)            # ten runs of one coincident group each
        assert P._expected_path(many, 2, 1) == (2, 0, 0)
        _check(pkg, hip, regs, rots, many, 1000, "over the run cap", tally=(0, 0), reg=reg)
        _check(pkg, hip, regs, rots, _copies(pkg, [0.0, 0.17]), 1000, "after", tally=(1, 0), reg=reg)
    finally:
        reg.close()
