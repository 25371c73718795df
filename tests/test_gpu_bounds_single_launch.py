"""The pair form (Params::bounds_order 2) as ONE evaluation launch, and the edges of its device pre-pass.

A batch the pre-pass leaves alone (more runs of equal rotation than bounds_order_max_runs) is evaluated by the pair launch itself, item i taking
groups 2 i and 2 i + 1 as they came on the plain path; no second launch follows.  The pre-pass finds the run starts with one comparison per
group (thread t looks at groups t, t + 1 024, ...), keeps the centres of a thread's first four groups of a run in registers (runs of more
than 4 096 groups load the rest again) and writes order[] and the pair list from the slots of its counting sort.

Every case compares the raw bits of ub and lb with bounds_order = 0 and reads back which form was launched and what the pre-pass decided
(goicp_debug_bounds_order) against what the batch implies -- the helpers, clouds (N = 257 / 1 000, 64^3 bricked grid), bounds_order_max_runs = 4,
bounds_order_min_groups = 1 and bounds_order_reprobe = 0 of test_gpu_bounds_order_pairs.py.  _same_bits runs the ordered form (1) beside the
pair form (2): the pre-pass is theirs in common.
"""
import numpy as np
import pytest

import test_gpu_bounds_order_pairs as P
from test_gpu_bounds_order_pairs import pkg, hip, regs, rots, pair_cases  # noqa: F401  (fixtures)


pytestmark = pytest.mark.gpu

SIZES = (257, 1000)
HELD = 4096          # device.hip kOrderHeld * 1 024: the longest run whose centres stay in registers


def _alternating(groups):
    """every group a run of its own: more runs than the cap from five groups on"""
    return (np.arange(groups) % 2).astype(np.int32)


# ----------------------------------------------------------------------------------------------
# batches the pre-pass leaves alone
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("groups", (10, 11, 128, 129))
def test_left_alone_group_counts(pkg, hip, regs, rots, n, groups):
    """an even and an odd number of groups (the last item a single), each also with a partial last group"""
    rng = np.random.default_rng(1100 + groups)
    recs = P._expansions(pkg, rng, _alternating(groups))
    assert P._expected_path(recs, 2, 1) == (2, 0, 0)
    P._same_bits(pkg, hip, regs, rots, recs, n, "left alone, %d groups" % groups)
    P._same_bits(pkg, hip, regs, rots, recs[:-3], n, "left alone, %d groups, partial last" % groups)


@pytest.mark.parametrize("n", SIZES)
def test_left_alone_generic_groups(pkg, hip, regs, rots, pair_cases, n):
    """generic (non-sibling) groups between sibling sets, as a pair item's first member, its second, and both"""
    rng = np.random.default_rng(1200)
    sib = P._expansions(pkg, rng, _alternating(9))
    gen = pair_cases["generic"]                                   # eight groups of unrelated cubes, a rotation each
    recs = np.concatenate([sib[:8], gen[:8], sib[8:32], gen[8:24], sib[32:], gen[24:]])
    assert P._expected_path(recs, 2, 1) == (2, 0, 0)
    P._same_bits(pkg, hip, regs, rots, recs, n, "left alone, generic groups")
    P._same_bits(pkg, hip, regs, rots, recs[:-5], n, "left alone, generic groups, partial last")


@pytest.mark.parametrize("n", SIZES)
def test_left_alone_outside_the_grid(pkg, hip, regs, rots, n):
    """members partly (translation 1.7 of a cloud of radius 0.2 .. 0.85 in a grid to +-2) and wholly (3.5) outside the grid"""
    rng = np.random.default_rng(1300)
    centre = np.array([[0.1, 0.0, -0.1], [1.7, 0.2, 0.0], [0.1, 0.0, -1.7], [0.3, 0.2, 0.0], [0.1, -1.7, -0.1], [1.7, 0.2, 0.0], [3.5, 0.0, 0.0]])
    recs = P._expansions(pkg, rng, _alternating(7), level=2, centre=centre)
    assert P._expected_path(recs, 2, 1) == (2, 0, 0)
    P._same_bits(pkg, hip, regs, rots, recs, n, "left alone, outside the grid")


@pytest.mark.parametrize("n", SIZES)
def test_left_alone_truncated_then_ordered(pkg, hip, regs, rots, pair_cases, n):
    """the truncated objective (the TRUNC instantiation) on a batch left alone, then an ordered batch on the same handles, then the first again"""
    rng = np.random.default_rng(1400)
    many = np.concatenate([P._expansions(pkg, rng, _alternating(11)), pair_cases["generic"][:16]])[:-3]
    few = P._expansions(pkg, rng, np.repeat([0, 5, 2], 7))
    assert P._expected_path(many, 2, 1) == (2, 0, 0) and P._expected_path(few, 2, 1) == (2, 1, 12)
    for trunc in (0.3, None):
        for what, recs in (("left alone", many), ("ordered after it", few), ("left alone again", many)):
            P._same_bits(pkg, hip, regs, rots, recs, n, "%s, trunc %s" % (what, trunc), trunc=trunc)


# ----------------------------------------------------------------------------------------------
# pre-pass edges
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", (1023, 1024, 1025, 2049))
def test_group_counts_at_the_thread_stride(pkg, hip, regs, rots, groups):
    """one run of G groups: a thread's last group missing, present, and one group into the next stride"""
    rng = np.random.default_rng(2000 + groups)
    recs = P._expansions(pkg, rng, np.zeros(groups, np.int32))
    P._same_bits(pkg, hip, regs, rots, recs, 257, "%d groups" % groups)
    P._same_bits(pkg, hip, regs, rots, recs[:-3], 257, "%d groups, partial last" % groups)


@pytest.mark.parametrize("start", (1, 1023, 1024, 1025))
def test_run_start_at_the_thread_stride(pkg, hip, regs, rots, start):
    """2 049 groups in two runs, the second starting at a seam of the run detection's stride of 1 024 threads"""
    rng = np.random.default_rng(2100 + start)
    rot = np.where(np.arange(2049) < start, 3, 1).astype(np.int32)
    recs = P._expansions(pkg, rng, rot)
    assert P._expected_path(recs, 2, 1) == (2, 1, (start + 1) // 2 + (2049 - start + 1) // 2)
    P._same_bits(pkg, hip, regs, rots, recs, 257, "run start %d" % start)


@pytest.mark.parametrize("runs", ((1, 2, 3, 1030), (1030, 3, 2, 1), (1, 1, 1, 1), (2, 2, 1025, 2), (1, 2, 3, 1030, 1), (1, 1, 1, 1, 1), (300, 300, 300, 300, 300)),
                         ids=("short_runs_first", "short_runs_last", "four_singles", "exactly_the_cap", "one_over_the_cap", "five_singles", "five_long_runs"))
def test_run_lengths_and_the_cap(pkg, hip, regs, rots, runs):
    """runs of length 1, 2 and 3 beside a long one; exactly bounds_order_max_runs = 4 runs are ordered, five are left alone"""
    rng = np.random.default_rng(2200 + len(runs) + runs[0])
    rot = np.repeat(np.arange(len(runs)) % P.N_ROT, runs).astype(np.int32)
    recs = P._expansions(pkg, rng, rot)
    want = (2, 1, sum((r + 1) // 2 for r in runs)) if len(runs) <= P.MAX_RUNS else (2, 0, 0)
    assert P._expected_path(recs, 2, 1) == want
    P._same_bits(pkg, hip, regs, rots, recs, 257, "runs %s" % (runs,))


def test_recurring_rotation(pkg, hip, regs, rots):
    """a rotation that comes back starts a new run: 3 x 700, 5 x 2, 3 x 700, 5 x 1"""
    rng = np.random.default_rng(2300)
    rot = np.repeat([3, 5, 3, 5], [700, 2, 700, 1]).astype(np.int32)
    recs = P._expansions(pkg, rng, rot)
    assert P._expected_path(recs, 2, 1) == (2, 1, 350 + 1 + 350 + 1)
    P._same_bits(pkg, hip, regs, rots, recs, 257, "recurring rotation")


@pytest.mark.parametrize("runs", ((HELD - 1,), (HELD,), (HELD + 1,), (3, HELD + 4, 1030)), ids=("below", "at", "above", "above_between_runs"))
def test_run_length_beyond_the_held_groups(pkg, hip, regs, rots, runs):
    """both sides of the run length up to which a thread keeps its groups' centres in registers (4 per thread, 4 096 per run)"""
    rng = np.random.default_rng(2400 + runs[0])
    rot = np.repeat(np.arange(len(runs)), runs).astype(np.int32)
    recs = P._expansions(pkg, rng, rot)
    assert P._expected_path(recs, 2, 1) == (2, 1, sum((r + 1) // 2 for r in runs))
    P._same_bits(pkg, hip, regs, rots, recs, 257, "runs %s" % (runs,))


def test_identical_centres(pkg, hip, regs, rots):
    """every group of a run in one Morton cell (equal centres): one counter hands out all the slots"""
    rng = np.random.default_rng(2500)
    recs = P._expansions(pkg, rng, np.zeros(1500, np.int32), level=2, coeff=0.1, centre=[0.2, -0.1, 0.05])
    P._same_bits(pkg, hip, regs, rots, recs, 257, "identical centres")
