"""Expansions that a rotation run lists more than once (goicp_params::bounds_dedup; device.hip bounds_order_kernel's alias table,
BoundsOrder::alias): in the pair launch over several point chunks a group whose eight records repeat another group of its run, all 48 words
as raw bits, is not evaluated -- bounds_finalize sums its bounds from the rows of the group evaluated in its place (the owner).  Anything
short of bit equality, another run, a partial last group, one point chunk and a batch the pre-pass left alone keep every listing evaluated.

Every case compares the raw bits of ub and lb with bounds_order = 0 and with bounds_dedup = 0, the copies count (goicp_debug_bounds_copies)
with a numpy recount -- full groups minus distinct full groups per run, a group taken as its 192 bytes -- and goicp_debug_bounds_order and
goicp_debug_bounds_twins with those of the bounds_dedup = 0 handle: the pair list and the tallies of the forms do not change.

Helpers and fixtures of test_gpu_bounds_order_pairs.py / test_gpu_bounds_twin_pairs.py (64^3 bricked grid over [-2, 2]^3,
bounds_order_max_runs = 4, bounds_order_min_groups = 1, bounds_order_reprobe = 0).  N = 257 (two chunks up to 1 023 groups, ONE from 1 024
groups on: bounds written directly, count 0), 1 000 and 5 003 (partials and bounds_finalize), 7 937 and 9 001 (the 8-chunk shape and its
balanced cuts up to 128 groups).  chunks_of restates bounds_shape.

The probe bound (device.hpp kBoundsAliasProbes = 32): a group that finds 32 slots of its probe sequence taken by groups that differ from
it stays its own owner, so only a crowd of more than 32 DISTINCT groups with equal children 0 and 7 (one hash) can make the count fall
short of the recount; test_more_distinct_groups_of_one_hash_than_the_probe_bound asserts count <= recount there, every other case equality.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_bounds_order_pairs as P
import test_gpu_bounds_twin_pairs as T
from test_gpu_bounds_order_pairs import pkg, hip, rots  # noqa: F401  (fixtures)


pytestmark = pytest.mark.gpu

SIZES = (257, 1000, 5003, 7937, 9001)
PROBES = 32


def chunks_of(b, n):
    """device.hip bounds_shape: the point chunks of a launch of b cubes over n points"""
    g, max_chunks = -(-b // 8), -(-n // 256)
    c, sets = -(-1024 // g), max_chunks >= 32
    if sets:
        c = -(-c // 8) * 8
    if c > max_chunks:
        c = max_chunks // 8 * 8 if sets else max_chunks
    c = max(c, 1)
    cp = -(-(-(-n // c)) // 256) * 256
    c2 = -(-n // cp)
    return c if sets and c % 8 == 0 and c2 != c else c2


def recount(recs, n):
    """groups the launch need not evaluate: per run of equal rotation (each group's first record, arrival order) the full groups minus the
    distinct ones; 0 over one point chunk and for a batch of more runs than the cap"""
    path = P._expected_path(recs, 2, 1)
    if chunks_of(len(recs), n) == 1 or not path[1]:
        return 0
    full = len(recs) // 8
    raw = np.ascontiguousarray(recs[:8 * full]).view(np.uint8).reshape(full, 192)
    rot = recs["rot"][0:8 * full:8]
    run = np.cumsum(np.concatenate([[0], rot[1:] != rot[:-1]]))
    return sum(int((run == r).sum()) - len({row.tobytes() for row in raw[run == r]}) for r in np.unique(run))


class _Regs:
    """(bounds_order 0, bounds_order 2 without dedup, bounds_order 2 with dedup) per cloud size and objective, kept for the module"""

    def __init__(self, pkg):
        self.pkg, self.regs = pkg, {}

    def make(self, n, trunc=None):
        t, s = P._clouds(n)
        kw = dict(dt_size=64, trunc_dist=trunc, bounds_order_min_groups=1, bounds_order_max_runs=P.MAX_RUNS, bounds_order_reprobe=0)
        return [self.pkg.Registration(t, s, 1e-3, bounds_order=0, **kw), self.pkg.Registration(t, s, 1e-3, bounds_order=2, bounds_dedup=0, **kw),
                self.pkg.Registration(t, s, 1e-3, bounds_order=2, bounds_dedup=1, **kw)]

    def get(self, n, trunc=None):
        if (n, trunc) not in self.regs:
            self.regs[(n, trunc)] = self.make(n, trunc)
        return self.regs[(n, trunc)]

    def close(self):
        for three in self.regs.values():
            for r in three:
                r.close()


@pytest.fixture(scope="module")
def regs(pkg):
    r = _Regs(pkg)
    yield r
    r.close()


def _copies_count(reg):
    info = (C.c_int32 * 1)()
    assert reg._lib.goicp_debug_bounds_copies(reg.handle, info) == 0
    return int(info[0])


def check(pkg, hip, regs, rots, recs, n, what, trunc=None, three=None, exact=True, want=None, stable=True):
    """stable: the tallies of the forms are a function of the batch -- every Morton cell holds copies of one expansion only (any order of
    them pairs alike), or the batch has at most 64 groups (one wavefront of the pre-pass places them all, in lane order).  Otherwise two
    launches of ONE handle may pair a cell's groups differently; the tallies are then held to what every order gives, their bound"""
    ref_reg, off_reg, on_reg = regs.get(n, trunc) if three is None else three
    ref = P._eval(pkg, hip, ref_reg, rots, recs)
    assert P._path(ref_reg) == (0, 0, 0) and _copies_count(ref_reg) == 0, what
    assert np.isfinite(ref[0].view(np.float32)).all(), what
    off = P._eval(pkg, hip, off_reg, rots, recs)
    path, twins = P._path(off_reg), T._tally(off_reg)
    assert path == P._expected_path(recs, 2, 1) and _copies_count(off_reg) == 0, what
    on = P._eval(pkg, hip, on_reg, rots, recs)
    assert P._path(on_reg) == path, (what, P._path(on_reg), path)
    if stable:
        assert T._tally(on_reg) == twins, (what, T._tally(on_reg), twins)
    else:
        assert min(T._tally(on_reg)) >= 0 and sum(T._tally(on_reg)) <= path[2] and sum(twins) <= path[2], (what, T._tally(on_reg), twins, path)
    count, expect = _copies_count(on_reg), recount(recs, n)
    for name, g, e, r in (("ub", on[0], off[0], ref[0]), ("lb", on[1], off[1], ref[1])):
        assert np.array_equal(e, r), "%s: bounds_dedup 0 changed %d of %d %s" % (what, int((e != r).sum()), len(r), name)
        assert np.array_equal(g, r), "%s (%d copies): bounds_dedup 1 changed %d of %d %s (first at %d)" % (what, count, int((g != r).sum()), len(r), name, int(np.argmax(g != r)))
    if want is not None:
        assert expect == (want if chunks_of(len(recs), n) > 1 else 0), (what, expect, want)
    assert count == expect if exact else 0 <= count <= expect, (what, count, expect)
    return count


def strangers(pkg):
    """two other expansions a sixth of a voxel from the families' centre: in their Morton cell whatever the run's extent"""
    return (T._copies(pkg, [0.1], level=2, centre=np.add(T.CENTRE, 0.01)), T._copies(pkg, [0.0], level=1, centre=np.add(T.CENTRE, (0.01, 0.0, 0.01))))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", (1, 2, 3, 7, 8, 64))
def test_family(pkg, hip, regs, rots, n, family):
    """identical listings alone in a run, and among strangers in their cell: all but one are copies"""
    fam = T._copies(pkg, np.full(family, 0.1))
    check(pkg, hip, regs, rots, fam, n, "family of %d" % family, want=family - 1)
    s1, s2 = strangers(pkg)
    cut = 8 * (family // 2)
    check(pkg, hip, regs, rots, np.concatenate([fam[:cut], s1, fam[cut:], s2]), n, "family of %d, two strangers" % family, want=family - 1, stable=family + 2 <= 64)


@pytest.mark.parametrize("n", SIZES)
def test_mixed_families(pkg, hip, regs, rots, n):
    """one node listed by the upper-bound search and by lower-bound searches of two coefficients, interleaved: three families"""
    for family in (3, 7, 8, 64):
        coeff = np.array([0.0, 0.17, 0.05], np.float32)[np.arange(family) % 3]
        check(pkg, hip, regs, rots, T._copies(pkg, coeff), n, "mixed family of %d" % family, want=family - min(family, 3))
        s1, s2 = strangers(pkg)
        fam = T._copies(pkg, coeff, level=2)
        check(pkg, hip, regs, rots, np.concatenate([s2, fam[:16], s1, fam[16:]]), n, "mixed family of %d, two strangers" % family, want=family - min(family, 3),
              stable=family + 2 <= 64)


def search_shaped(pkg):
    """the batch of test_gpu_bounds_twin_pairs.py test_search_shaped_batch: two runs, each the root listed by six searches (three without,
    three with one coefficient) among nine deeper expansions, partial last group"""
    rng = np.random.default_rng(900)
    parts = []
    for rot in (1, 4):
        root = T._copies(pkg, [0.0, 0.2, 0.0, 0.2, 0.2, 0.0], level=0, centre=(0.0, 0.0, 0.0), rot=np.full(6, rot))
        centre = rng.uniform(0.3, 0.5, (9, 3)) * rng.choice([-1.0, 1.0], (9, 3))
        deep = P._expansions(pkg, rng, np.full(9, rot, np.int32), level=rng.integers(1, 4, 9), centre=centre)
        parts.append(np.concatenate([root[:24], deep[:32], root[24:], deep[32:]]))
    return np.concatenate(parts)[:-5]


@pytest.mark.parametrize("n", SIZES)
def test_search_shaped_batch(pkg, hip, regs, rots, n):
    """per run the family of six is two families of three: four copies a run"""
    check(pkg, hip, regs, rots, search_shaped(pkg), n, "search-shaped batch", want=8)
    check(pkg, hip, regs, rots, search_shaped(pkg), n, "truncated search-shaped batch", trunc=0.3, want=8)


def _next(a):
    return np.nextafter(a, np.float32(np.inf), dtype=np.float32)


def near_misses(pkg):
    """two listings of one node with one coefficient, and what keeps the second from being a copy"""
    cases = {}
    for axis in ("tx", "ty", "tz"):
        r = T._copies(pkg, [0.1, 0.1], level=2)
        sel = 8 + np.flatnonzero((np.arange(8) & {"tx": 1, "ty": 2, "tz": 4}[axis]) != 0)       # one side of the second group: still a sibling set
        r[axis][sel] = _next(r[axis][sel])
        cases[axis + "_ulp"] = r
    r = T._copies(pkg, [0.1, 0.1], level=2)
    r["tx"][8] = _next(r["tx"][8])                            # child 0 alone: no sibling set any more
    cases["child0_ulp"] = r
    r = T._copies(pkg, [0.1, 0.1], level=2)
    r["delta"][8:] = _next(r["delta"][8:])
    cases["delta_ulp"] = r
    r = T._copies(pkg, [0.1, 0.1], level=2)
    r["coeff"][8:] = _next(r["coeff"][8:])
    cases["coeff_ulp"] = r
    r = T._copies(pkg, [0.1, 0.1], level=2)
    r["tx"][:8], r["tx"][8:] = 0.0, -0.0
    cases["translation_zero_signs"] = r
    cases["coeff_zero_signs"] = T._copies(pkg, [0.0, -0.0])  # the identical form (equal as floats) and no copy (not as bits)
    cases["two_runs"] = T._copies(pkg, [0.1, 0.1], rot=[1, 4])
    cases["recurring_rotation"] = T._copies(pkg, [0.1, 0.1, 0.1], rot=[1, 4, 1])       # runs 1 | 4 | 1: the third group is in another run than the first
    return cases


@pytest.mark.parametrize("n", SIZES)
def test_near_misses(pkg, hip, regs, rots, n):
    check(pkg, hip, regs, rots, T._copies(pkg, [0.1, 0.1], level=2), n, "the pair the near misses are made from", want=1)
    for name, recs in sorted(near_misses(pkg).items()):
        check(pkg, hip, regs, rots, recs, n, name, want=0)
        check(pkg, hip, regs, rots, recs, n, "truncated " + name, trunc=0.3, want=0)
    r = T._copies(pkg, [0.1, 0.1, 0.1, 0.1], rot=[1, 4, 4, 1])
    check(pkg, hip, regs, rots, r, n, "runs 1 | 4 4 | 1", want=1)


def generic(seed, rot=1):
    """eight unrelated cubes of one rotation: no sibling set"""
    rng = np.random.default_rng(seed)
    g = np.zeros(8, P.CUBE)
    c = rng.uniform(-0.5, 0.5, (8, 3)).astype(np.float32)
    g["tx"], g["ty"], g["tz"] = c[:, 0], c[:, 1], c[:, 2]
    g["delta"], g["coeff"], g["rot"] = np.float32(0.03), np.where(np.arange(8) % 2, np.float32(0.1), np.float32(0)), rot
    return g


@pytest.mark.parametrize("n", SIZES)
def test_generic_and_partial_groups(pkg, hip, regs, rots, n):
    a, b = generic(1), generic(2)
    check(pkg, hip, regs, rots, np.concatenate([a, b, a, a, b]), n, "identical generic groups", want=3)
    check(pkg, hip, regs, rots, np.concatenate([a, b, a, a, b]), n, "truncated identical generic groups", trunc=0.3, want=3)
    check(pkg, hip, regs, rots, np.concatenate([a, a, a])[:-3], n, "the partial last group repeats the full ones", want=1)
    check(pkg, hip, regs, rots, np.concatenate([b, a])[:-1], n, "a partial last group after a stranger", want=0)
    sib = T._copies(pkg, [0.1, 0.1, 0.1])
    check(pkg, hip, regs, rots, sib[:-3], n, "sibling sets, the partial last one a copy but for its length", want=1)
    # children 0 and 7 equal (one hash, one slot), child 3 not: the full comparison tells them apart
    a3 = a.copy()
    a3["ty"][3] = _next(a3["ty"][3])
    check(pkg, hip, regs, rots, np.concatenate([a, a3]), n, "equal but for child 3", want=0)
    check(pkg, hip, regs, rots, np.concatenate([a, a3, a3, b, a]), n, "two families of one hash", want=2)
    s3 = T._copies(pkg, [0.1, 0.1, 0.1], level=2)
    s3["coeff"][8 + 3] = _next(s3["coeff"][8 + 3])
    check(pkg, hip, regs, rots, s3, n, "sibling sets equal but for child 3 of one", want=1)


@pytest.mark.parametrize("n", SIZES)
def test_outside_the_grid(pkg, hip, regs, rots, n):
    """families partly and wholly outside the grid: the owner's checked branch serves the copies"""
    for where in sorted(T.OUTSIDE):
        centre, level = T.OUTSIDE[where]
        for trunc in (None, 0.3):
            check(pkg, hip, regs, rots, T._copies(pkg, np.full(3, 0.1), level=level, centre=centre), n, "%s outside, family of 3" % where, trunc=trunc, want=2)
            check(pkg, hip, regs, rots, T._copies(pkg, [0.0, 0.1, 0.0, 0.0, 0.1], level=level, centre=centre), n, "%s outside, mixed family" % where, trunc=trunc, want=3)


def crowd(pkg, groups, seed):
    """one run of `groups` random expansions with centres in [-0.5, 0.5]^3 in which families of 2, 3, 5, 9, 33 and 64 listings replace
    random places but the last.  Each family sits at a corner (+-0.9, +-0.9, +-0.9) of its own: a cell is 0.25 wide, so it has its cell to
    itself and the tallies of the forms do not depend on the order inside a cell (no two of the random expansions coincide)"""
    rng = np.random.default_rng(seed)
    recs = P._expansions(pkg, rng, np.zeros(groups, np.int32))
    place = rng.permutation(groups - 1)
    at = 0
    for k, size in enumerate((2, 3, 5, 9, 33, 64)):
        corner = 0.9 * np.array([1.0 if k & 1 else -1.0, 1.0 if k & 2 else -1.0, 1.0 if k & 4 else -1.0])
        one = T._copies(pkg, [0.1 if k % 2 else 0.0], level=1 + k % 3, centre=corner, rot=[0])
        for g in place[at:at + size]:
            recs[8 * g:8 * g + 8] = one
        at += size
    return recs, at - 6


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("groups", (1023, 1024, 1025, 4097))
def test_long_runs(pkg, hip, regs, rots, n, groups):
    """one group per thread of the pre-pass, one more, and runs past what a thread holds in registers: the table under load"""
    recs, want = crowd(pkg, groups, groups)
    check(pkg, hip, regs, rots, recs, n, "run of %d groups" % groups, want=want)
    check(pkg, hip, regs, rots, recs[:-3], n, "run of %d groups, partial last" % groups)


@pytest.mark.parametrize("n", (1000, 9001))
def test_more_distinct_groups_of_one_hash_than_the_probe_bound(pkg, hip, regs, rots, n):
    """40 distinct groups that differ in child 3 only -- one hash, one probe sequence -- each listed twice: a listing that finds PROBES slots
    taken by strangers before it meets its double is evaluated itself.  The occupant of the first slot is always found by its double"""
    a = generic(3)
    parts = []
    for k in range(PROBES + 8):
        v = a.copy()
        for _ in range(k):
            v["tz"][3] = _next(v["tz"][3])
        parts += [v, v]
    recs = np.concatenate(parts)
    assert recount(recs, n) == PROBES + 8
    assert check(pkg, hip, regs, rots, recs, n, "a crowd of one hash", exact=False) >= 1


def test_handle_life(pkg, hip, regs, rots):
    """one handle of each form: copies, a batch over the run cap (left alone: count 0), copies again, a larger batch (the buffers regrow, alias[]
    and ctl[] move), goicp_set_source to another N with the 8-chunk shape and to one without"""
    three = regs.make(9001)
    try:
        fam = np.concatenate([T._copies(pkg, np.full(7, 0.1)), search_shaped(pkg)])
        first = check(pkg, hip, regs, rots, fam, 9001, "before", three=three)
        assert first == 6 + 8
        many = T._copies(pkg, np.full(10, 0.1), rot=np.arange(10) % 2)
        assert P._expected_path(many, 2, 1) == (2, 0, 0)
        check(pkg, hip, regs, rots, many, 9001, "over the run cap", three=three, want=0)
        assert check(pkg, hip, regs, rots, fam, 9001, "after", three=three) == first
        recs, want = crowd(pkg, 2049, 5)
        check(pkg, hip, regs, rots, recs, 9001, "regrown", three=three, want=want)
        assert check(pkg, hip, regs, rots, fam, 9001, "small again", three=three) == first
        for m in (7937, 1000, 257):
            other = P._clouds(m)[1][::-1].copy()
            for r in three:
                r.set_source(other)
            assert check(pkg, hip, regs, rots, fam, m, "after set_source to %d points" % m, three=three) == first
        check(pkg, hip, regs, rots, recs, 257, "one chunk after set_source", three=three, want=0)
    finally:
        for r in three:
            r.close()
