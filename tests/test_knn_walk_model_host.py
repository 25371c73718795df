"""The k-NN walk's control flow, stepped on the CPU (tests/knn_walk_twin.py) over the hierarchies the device build makes of the clouds of
tests/test_gpu_kd_device_build.py.  Three statements:

  1. with the "group exhausted" test the kernel has (an all-taken group is exhausted whatever the bound) every walk ends within the cap
     and returns the brute-force list -- with the seed entry and without it;
  2. the GPU file's clouds and queries really hold what the kernel used to get wrong: a bottom-level group with fewer than k points whose
     child 3 is an empty leaf, reached by one of the very queries the GPU test sends while that query's list is still short.  Otherwise the
     GPU tests could pass without walking through it;
  3. with the test the kernel had (only "the key lies above the bound") the model hits the cap on such a shape.  A statement about the
     model: the unfixed walk is never run on a device.

The cap: a walk that leaves emptied groups takes every child of every group at most once, and every step but the last takes one that was
not taken before, so groups + leaves + 1 steps bound it (K = 2: 4 162).  Every statement uses that bound as its cap."""
import functools

import numpy as np
import pytest

import knn_walk_twin as T
from conftest import load_pkg
from test_gpu_small_shapes import _knn_queries


@functools.lru_cache(maxsize=None)
def _cell(kind, M):
    load_pkg()
    from cuda_go_icp_amd import synth
    target = T.device_build_case(synth, kind, M)["target"]
    return target, T.Hierarchy(target), _knn_queries(target, T.N_QUERIES, T.query_seed(M))


def _cap(h):
    return sum(64 ** l for l in range(h.K + 1)) + 1


def _nearest_slot(h, target, q):
    return int(h.slot_of[T.brute_keys(target, q, 1)[0] & 0xFFFFFFFF])


def _pick(n, count):
    """`count` of n query places, spread over the four quarters (on, near, around, far outside)"""
    return [int(i) for i in np.linspace(0, n - 1, count).round()]


@pytest.mark.parametrize("kind,M", T.CELLS, ids=lambda v: str(v))
def test_walk_with_the_all_taken_test_is_exact(kind, M):
    """every k of the GPU file, 12 of its queries at one and two box levels and 4 at three; seeded from the nearest point's slot, from the
    last point's slot (any point is a valid seed) and unseeded"""
    target, h, qs = _cell(kind, M)
    assert h.K == (1 if M <= 1024 else 2 if M <= 65536 else 3)
    worst = 0
    for i in _pick(len(qs), 12 if h.K < 3 else 4):
        q = qs[i]
        for k in T.ks_of(M) if h.K < 3 else (T.ks_of(M)[-1],):
            want = T.brute_keys(target, q, k)
            for seed in (None, _nearest_slot(h, target, q), int(h.slot_of[M - 1])):
                r = T.walk(h, q, k, T.EXHAUSTED_ALL_TAKEN, seed, _cap(h))
                assert r["ended"], (kind, M, k, i, seed, r["steps"])
                assert r["keys"] == want, (kind, M, k, i, seed)
                worst = max(worst, r["steps"])
    print("%s M %d (K %d): longest walk %d steps of at most %d" % (kind, M, h.K, worst, _cap(h)))


@pytest.mark.parametrize("kind,M,k", T.BAND_CELLS, ids=lambda v: str(v))
def test_gpu_shapes_hold_the_trigger(kind, M, k):
    """the hierarchy has trigger groups, and a walk the GPU tests start runs out of one with a short list: one of knn_query's own queries
    (the first 64 are looked at at two levels, the first 24 and 8 spread ones at three), and one of the normals' rows -- a point of such a group, seeded
    with itself.  At 31.98 points per group (M = 2 047, 131 071) a single group is one point short, few queries start in it, and only
    the normals are sure to: there the queries are looked at but not asked to hit"""
    target, h, qs = _cell(kind, M)
    groups = h.trigger_groups(k)
    assert len(groups), (kind, M, k, float(h.group_count().mean()))

    def hits(q, seed):
        r = T.walk(h, q, k, T.EXHAUSTED_ALL_TAKEN, seed, _cap(h))
        assert r["ended"]
        return any(empty for _, empty in r["short_exhausts"])

    hit_q = sum(hits(qs[i], _nearest_slot(h, target, qs[i])) for i in (range(64) if h.K < 3 else list(range(24)) + _pick(len(qs), 8)))
    g = int(groups[0])
    slots = [s for s in range(g * 64 * T.LEAF_SLOTS, (g + 1) * 64 * T.LEAF_SLOTS) if h.ids[s] != T.INT_MAX][:4]
    hit_n = sum(hits(h.pts[s], s) for s in slots)
    assert hit_n, (kind, M, k)
    assert hit_q or M in (2047, 131071), (kind, M, k)
    print("%s M %d k %d: %d of %d bottom-level groups are triggers; %d of the queries and %d of the %d normal rows looked at leave one with a short list"
          % (kind, M, k, len(groups), len(h.group_count()), hit_q, hit_n, len(slots)))


def test_walk_with_the_bound_only_test_hits_the_cap():
    """uniform cube, M = 1 500, k = 32: of the GPU test's first 24 queries some never end (they rescan a child 3 that is empty, or that holds
    nothing but the seed's slot, which the scans skip), and one that does end returns a list with a point in it twice -- or, by luck, the
    exact list"""
    target, h, qs = _cell("uniform", 1500)
    capped = dup = exact = 0
    for q in qs[:24]:
        r = T.walk(h, q, 32, T.EXHAUSTED_BOUND_ONLY, _nearest_slot(h, target, q), _cap(h))
        if not r["ended"]:
            capped += 1
            assert r["short_exhausts"] and len(r["keys"]) < 32       # stuck in an emptied group, the list still short
        elif len(set(r["keys"])) < len(r["keys"]):
            dup += 1
        else:
            exact += r["keys"] == T.brute_keys(target, q, 32)
    print("bound-only test, uniform M 1500 k 32: %d of 24 walks hit the cap of %d steps, %d hold a point twice, %d exact" % (capped, _cap(h), dup, exact))
    assert capped >= 1
    # outside the band nothing distinguishes the two tests: M = 2 048, 32 points in every group
    target, h, qs = _cell("synth", 2048)
    for q in qs[:24:3]:
        r = T.walk(h, q, 32, T.EXHAUSTED_BOUND_ONLY, None, _cap(h))
        assert r["ended"] and r["keys"] == T.brute_keys(target, q, 32)
