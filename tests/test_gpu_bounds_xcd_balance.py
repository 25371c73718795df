"""The cost-balanced mapping of the pair launch's 8-chunk shape (goicp_params::bounds_balance; device.hip bounds_chunk_cost_kernel,
device.hpp bounds_cuts, bounds_pair_kernel): block label x = blockIdx & 7 evaluates the units cut[x] .. cut[x + 1] - 1 of the chunk-major
list u = chunk * items + item instead of chunk x under every item.  Scheduling only: the chunk partition and the order of every sum stay.

Every case compares the raw bits of ub and lb with bounds_order = 0 and with bounds_balance = 0, and reads the mapping back
(goicp_debug_bounds_balance): cut[0] = 0, cut[8] = 8 items, non-decreasing, no piece above ceil(1.25 items), cut[] equal to the integer
formula restated here and fed with the returned lines and waves, lines[] and waves[] equal to a numpy recount over the ordered cloud, the
twin / identical tallies (goicp_debug_bounds_twins) those of the equal split.

64^3 bricked grid over [-2, 2]^3 (the target of test_gpu_bounds_order_pairs.py), bounds_order_min_groups = 1, bounds_order_reprobe = 0,
bounds_order_max_runs = 4.  N = 7 937 (chunks of 1 024 points, the last 769), 8 193 (1 280, chunk 7 EMPTY), 9 001; groups 128, 129, 255
(eight chunks from 128 groups on); 127 groups are 16 chunks: mapping unused.  Clouds: half a tight blob and half a thin shell (raw weights
beyond the clamp, pieces straddling chunks), and an even sphere.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_bounds_order_pairs as P
from test_gpu_bounds_order_pairs import pkg, hip, rots  # noqa: F401  (fixtures)


pytestmark = pytest.mark.gpu

SIZES = (7937, 8193, 9001)
DEFAULT_A = 18.0
# device.hip kCostRots: the identity and three fixed rotations, as float32 literals
COST_ROTS = np.array([
    [1, 0, 0, 0, 1, 0, 0, 0, 1],
    [0.84567982, -0.449964464, -0.286980212, 0.0414698496, 0.591505408, -0.805233896, 0.532076955, 0.669069052, 0.518884122],
    [0.219921082, -0.74321264, 0.631877899, 0.372148067, 0.662668586, 0.649904728, -0.901743054, 0.0922243893, 0.422319949],
    [0.122044131, 0.98462534, 0.124972485, -0.646330416, 0.174399301, -0.742860556, -0.753234506, 0.00988825131, 0.65767777]], np.float32)


def uneven(n):
    """half the points in a blob a voxel wide, half on a thin shell: a wavefront of the blob gathers a line or two, one of the shell dozens"""
    rng = np.random.default_rng(n)
    blob = np.array([0.3, 0.2, -0.1]) + rng.normal(size=(n // 2, 3)) * 0.01
    d = rng.normal(size=(n - n // 2, 3))
    shell = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.8 + 0.002 * rng.normal(size=(len(d), 1)))
    return rng.permutation(np.concatenate([blob, shell]).astype(np.float32))


def even(n):
    """a Fibonacci lattice on a sphere of radius 0.7: even density"""
    i = np.arange(n) + 0.5
    phi, z = i * np.pi * (3.0 - np.sqrt(5.0)), 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    return (0.7 * np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)).astype(np.float32)


class _Regs:
    def __init__(self, pkg):
        self.pkg, self.regs, self.target = pkg, {}, P._clouds(1000)[0]

    def make(self, src, order, balance=1, a=0.0, trunc=None):
        return self.pkg.Registration(self.target, src, 1e-3, dt_size=64, trunc_dist=trunc, bounds_order=order, bounds_order_min_groups=1,
                                     bounds_order_max_runs=P.MAX_RUNS, bounds_order_reprobe=0, bounds_balance=balance, bounds_balance_a=a)

    def get(self, cloud, n, order, balance=1, a=0.0, trunc=None):
        key = (cloud.__name__, n, order, balance, a, trunc)
        if key not in self.regs:
            self.regs[key] = self.make(cloud(n), order, balance, a, trunc)
        return self.regs[key]

    def close(self):
        for r in self.regs.values():
            r.close()


@pytest.fixture(scope="module")
def regs(pkg):
    r = _Regs(pkg)
    yield r
    r.close()


def _balance(reg):
    info = (C.c_int32 * 26)()
    assert reg._lib.goicp_debug_bounds_balance(reg.handle, info) == 0
    return list(info[0:9]), list(info[9:17]), list(info[17:25]), int(info[25])


def _twins(reg):
    info = (C.c_int32 * 2)()
    assert reg._lib.goicp_debug_bounds_twins(reg.handle, info) == 0
    return tuple(info)


def formula(lines, waves, a, items):
    """device.hpp bounds_cuts, restated: W_k = a waves_k + lines_k in 1/256, over the mean and clamped to [0.8, 1.25] at a scale of 2^20;
    cut[x] = the first unit at which the weighted prefix reaches x / 8 of the total; no piece above ceil(1.25 items)"""
    a_q8 = int(min(np.float32(a) * np.float32(256) + np.float32(0.5), np.float32(16777216)))
    w = [a_q8 * int(waves[k]) + 256 * int(lines[k]) for k in range(8)]
    s = sum(w)
    if s <= 0:
        return [x * items for x in range(9)]
    while s >= 1 << 39:
        w = [v >> 1 for v in w]
        s = sum(w)
    w = [min(max((v << 23) // s, 838861), 1310720) for v in w]
    total, cut, k, before = sum(w), [0] * 8 + [8 * items], 0, 0
    for x in range(1, 8):
        want = x * total * items
        while k < 7 and 8 * (before + w[k]) * items <= want:
            before += w[k]
            k += 1
        cut[x] = k * items + min((want - 8 * before * items + 8 * w[k] - 1) // (8 * w[k]), items)
    cap = (items * 5 + 3) // 4
    for x in range(1, 8):
        cut[x] = min(cut[x], cut[x - 1] + cap)
    for x in range(7, 0, -1):
        cut[x] = max(cut[x], cut[x + 1] - cap)
    return cut


def recount(pkg, reg, src):
    """lines[8], waves[8] of bounds_chunk_cost_kernel in numpy: the cloud in the engine's order, float32 operation for operation"""
    s = src[pkg.source_order(src, 2)]
    n = len(s)
    if -(-n // 256) < 32:
        return [0] * 8, [0] * 8
    V, scale, origin = reg.dt_info()
    sc, mn, VB = np.float32(scale), [np.float32(o) for o in origin], (V + 3) // 4
    chunk_pts = -(-(-(-n // 8)) // 256) * 256
    wave_chunk = (np.arange(-(-n // 64)) * 64) // chunk_pts
    lines = np.zeros(8, np.int64)
    for R in COST_ROTS:
        idx = []
        for k in range(3):
            r = (R[3 * k] * s[:, 0] + R[3 * k + 1] * s[:, 1]) + R[3 * k + 2] * s[:, 2]
            idx.append((((r - mn[k]) * sc) + np.float32(0.5)).astype(np.int32))
        x, y, z = idx
        ok = (x >= 0) & (x < V) & (y >= 0) & (y < V) & (z >= 0) & (z < V)
        line = np.where(ok, ((((z >> 2).astype(np.int64) * VB + (y >> 2)) * VB + (x >> 2)) << 1) | ((z >> 1) & 1), -1)
        srt = np.sort(np.pad(line, (0, (-n) % 64), constant_values=-1).reshape(-1, 64), 1)
        per_wave = ((srt[:, 1:] != srt[:, :-1]) & (srt[:, 1:] >= 0)).sum(1) + (srt[:, 0] >= 0)
        lines += np.bincount(wave_chunk, weights=per_wave, minlength=8).astype(np.int64)
    return lines.tolist(), (4 * np.bincount(wave_chunk, minlength=8)).tolist()


def batch(pkg, groups, runs=1, seed=0, family=8):
    """`groups` sibling sets over `runs` rotation runs, random depths and passes, centres in [-0.5, 0.5]^3; the first `family` groups of
    run 0 are copies of one expansion with one coefficient at (0.9, 0.9, 0.9): alone in their Morton cell (a cell is 0.25 wide), so their
    items take the identical form, floor(family / 2) of them or one fewer by the parity of the groups before the cell -- the same on every
    launch, whatever order the pre-pass's atomics give inside a cell"""
    rng = np.random.default_rng(1000 * groups + runs + seed)
    rot = np.sort(np.arange(groups) * runs // groups).astype(np.int32) + 1
    recs = P._expansions(pkg, rng, rot)
    if family:
        fam = P._expansions(pkg, rng, np.full(family, rot[0], np.int32), level=1, coeff=np.float32(0.1), centre=np.array([0.9, 0.9, 0.9]))
        recs[:8 * family] = fam
    return recs


def check(pkg, hip, regs, rots, cloud, n, recs, what, a=0.0, trunc=None, reg=None, src=None, used=1):
    ref_reg = regs.get(cloud, n, 0, trunc=trunc) if reg is None else reg[0]
    ref = P._eval(pkg, hip, ref_reg, rots, recs)
    assert P._path(ref_reg) == (0, 0, 0), what
    assert np.isfinite(ref[0].view(np.float32)).all(), what
    eq_reg = regs.get(cloud, n, 2, balance=0, trunc=trunc) if reg is None else reg[1]
    eq = P._eval(pkg, hip, eq_reg, rots, recs)
    path = P._expected_path(recs, 2, 1)
    assert P._path(eq_reg) == path, what
    items = path[2] if path[1] else (len(recs) // 8 + (1 if len(recs) % 8 else 0) + 1) // 2
    ecut, elines, ewaves, eused = _balance(eq_reg)
    assert ecut == [x * items for x in range(9)] and eused == 0, (what, ecut)
    etw = _twins(eq_reg)
    bal_reg = regs.get(cloud, n, 2, balance=1, a=a, trunc=trunc) if reg is None else reg[2]
    got = P._eval(pkg, hip, bal_reg, rots, recs)
    assert P._path(bal_reg) == path, what
    for name, g, e, r in (("ub", got[0], eq[0], ref[0]), ("lb", got[1], eq[1], ref[1])):
        assert np.array_equal(e, r), "%s: bounds_balance 0 changed %d of %d %s" % (what, int((e != r).sum()), len(r), name)
        assert np.array_equal(g, r), "%s: bounds_balance 1 changed %d of %d %s (first at %d)" % (what, int((g != r).sum()), len(r), name, int(np.argmax(g != r)))
    cut, lines, waves, was_used = _balance(bal_reg)
    assert was_used == used, what
    assert cut[0] == 0 and cut[8] == 8 * items, (what, cut, items)
    d = np.diff(cut)
    assert (d >= 0).all() and d.max() <= (5 * items + 3) // 4, (what, cut, items)
    exp_lines, exp_waves = recount(pkg, bal_reg, cloud(n) if src is None else src)
    assert lines == exp_lines and waves == exp_waves and elines == exp_lines and ewaves == exp_waves, (what, lines, exp_lines, waves, exp_waves)
    assert cut == (formula(lines, waves, a if a > 0 else DEFAULT_A, items) if used else [x * items for x in range(9)]), (what, cut)
    tw = _twins(bal_reg)
    assert tw == etw and (tw[1] >= 3 if path[1] else tw == (0, 0)), (what, tw, etw)      # the family of eight: four items, or three and two halves
    return cut, lines, waves, items


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("groups", (128, 129, 255))
def test_uneven_cloud(pkg, hip, regs, rots, n, groups):
    """blob chunks weigh a fraction of shell chunks: the raw weights leave [0.8, 1.25] and the pieces straddle chunk boundaries"""
    cut, lines, waves, items = check(pkg, hip, regs, rots, uneven, n, batch(pkg, groups), "uneven %d x %d" % (n, groups))
    w = np.array(lines, float) + DEFAULT_A * np.array(waves, float)
    assert w.max() > 1.25 * w.mean() or w.min() < 0.8 * w.mean(), (lines, waves)
    assert any(c % items for c in cut[1:8]), cut
    partial = batch(pkg, groups)[:-3]                      # a partial last group
    check(pkg, hip, regs, rots, uneven, n, partial, "uneven %d x %d, partial last group" % (n, groups))


def test_empty_last_chunk(pkg, hip, regs, rots):
    """N = 8 193: chunk 7 has no point, no wavefront and no line; it keeps 0.8 of the mean weight"""
    cut, lines, waves, items = check(pkg, hip, regs, rots, uneven, 8193, batch(pkg, 128), "chunk 7 empty")
    assert lines[7] == 0 and waves[7] == 0 and min(waves[:7]) > 0
    assert 8 * items - cut[7] > 0


@pytest.mark.parametrize("groups", (128, 255))
def test_even_cloud(pkg, hip, regs, rots, groups):
    """N = 8 192: eight full chunks of an even sphere: every cut within a few units of x items -- items / 16, i.e. 4 units at the 64 items of
    128 groups, a sixteenth of a piece (the chunks differ only by how their patch faces the 4 x 4 x 2-voxel lines, which four poses average
    to a few percent).  Besides, with r the largest relative deviation of a chunk's weight from the mean, a prefix of x items' worth of weight
    is reached between x items (1 - r) / (1 + r) and x items (1 + r) / (1 - r), plus one unit of rounding"""
    cut, lines, waves, items = check(pkg, hip, regs, rots, even, 8192, batch(pkg, groups), "even sphere x %d" % groups)
    assert waves == [64] * 8
    for x in range(9):
        assert abs(cut[x] - x * items) <= items // 16, (x, cut, items, lines)
    w = np.array(lines, float) + DEFAULT_A * np.array(waves, float)
    r = float(np.abs(w / w.mean() - 1).max())
    for x in range(1, 8):
        assert x * items * (1 - r) / (1 + r) - 1 <= cut[x] <= x * items * (1 + r) / (1 - r) + 1, (x, cut, items, r)


def test_sixteen_chunks_leave_the_mapping_unused(pkg, hip, regs, rots):
    """127 groups: sixteen chunks, two per label as ever; the mapping is reported unused and the cuts as the equal split of the items"""
    check(pkg, hip, regs, rots, uneven, 7937, batch(pkg, 127), "127 groups", used=0)


@pytest.mark.parametrize("runs", (2, 3, 5))
def test_rotation_runs(pkg, hip, regs, rots, runs):
    """two and three runs (a leftover single per odd run); five runs are over the cap: the pre-pass leaves the batch alone and the cuts are
    taken over items = (groups + 1) / 2"""
    check(pkg, hip, regs, rots, uneven, 9001, batch(pkg, 131, runs=runs), "%d runs" % runs)


def test_truncated_objective(pkg, hip, regs, rots):
    check(pkg, hip, regs, rots, uneven, 7937, batch(pkg, 129, runs=2), "truncated", trunc=0.3)


def test_weight_of_a_wavefront(pkg, hip, regs, rots):
    """bounds_balance_a very large: the cuts follow the wavefronts, i.e. the points only (chunk 7 of N = 7 937 has 13 of the others' 16)"""
    cut, lines, waves, items = check(pkg, hip, regs, rots, uneven, 7937, batch(pkg, 128), "a = 65 536", a=65536.0)
    assert waves == [64] * 7 + [52]
    by_points = formula([0] * 8, waves, 1.0, items)        # the lines weigh 2^-16 of a wavefront each: at most a unit of difference
    assert max(abs(np.subtract(cut, by_points))) <= 1 and by_points != [x * items for x in range(9)], (cut, by_points)


def test_regrown_buffers_and_another_source(pkg, hip, regs, rots):
    """one handle of each form: a batch, an eight times larger batch (the order buffers regrow and ctl[] moves), then goicp_set_source to
    another N and cloud: the cost is counted again, the cuts change, the bits hold"""
    three = [regs.make(uneven(7937), 0), regs.make(uneven(7937), 2, balance=0), regs.make(uneven(7937), 2, balance=1)]
    try:
        first = check(pkg, hip, regs, rots, uneven, 7937, batch(pkg, 128), "before", reg=three)
        check(pkg, hip, regs, rots, uneven, 7937, batch(pkg, 1024, runs=3), "regrown", reg=three)
        again = check(pkg, hip, regs, rots, uneven, 7937, batch(pkg, 128), "after", reg=three)
        assert again == first
        other = uneven(9001)[::-1].copy()
        for r in three:
            r.set_source(other)
        swapped = check(pkg, hip, regs, rots, uneven, 9001, batch(pkg, 128), "after set_source", reg=three, src=other)
        assert swapped[1] != first[1] and swapped[0] != first[0]
        small = even(5003)                                 # no 8-chunk shape: the cost is cleared
        for r in three:
            r.set_source(small)
        check(pkg, hip, regs, rots, even, 5003, batch(pkg, 128), "after set_source to 5 003 points", reg=three, src=small, used=0)
    finally:
        for r in three:
            r.close()
