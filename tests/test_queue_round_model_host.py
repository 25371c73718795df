"""The model of a queue round (tests/queue_round_twin.py) held to something simpler than itself, before the kernel is held to the model
(tests/test_gpu_queue_round.py):

  brute force    on a few thousand random small states the model's selection and removal equal a pure-Python reading of the rules -- pick the
                 smallest (key, position) K times by linear scan, no sort -- and its removal satisfies the multiset identity;
  whole search   the model's round, iterated over a synthetic bound function with lb <= true <= ub on every cube, finds what a plain heapq
                 best-first search of jly_goicp.cpp:227-340's shape finds, within SSEThresh, attains its best node's bound and expands no node
                 twice -- for every round width, stale_widen and with Morton-order selection: the model is a valid BnB;
  seeded defects four logic defects applied to the MODEL are each caught by check_properties, the order-free statement the GPU test asserts
                 before its byte comparison.
"""
import heapq
import struct

import numpy as np
import pytest

import queue_round_twin as T
from queue_round_twin import F, Round, Search

ROOT = (-0.5, -0.5, -0.5, 1.0)


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def brute(q, best, thr, K, rp, compact):
    """(done, listed rows, queue rows after) of the selection on queue q, in plain Python"""
    n = len(q)
    if n == 0:
        return True, [], []
    rw = (fbits(rp.root[3]) >> 23) & 0xff
    fails = [bool(F(best) - F(r[5]) < F(thr)) for r in q]
    keys = []
    for r, f in zip(q, fails):
        if compact:
            if f:
                keys.append(0xfffffffe)
                continue
            g = [min(max(int((F(r[a]) - F(rp.root[a])) * (F(1024.0) / F(rp.root[3]))), 0), 1023) for a in range(3)]
            keys.append(sum(((g[a] >> b) & 1) << (3 * b + a) for a in range(3) for b in range(10)))
        else:
            keys.append((fbits(r[5]) & 0xffffffe0) | min(max(rw - ((fbits(r[3]) >> 23) & 0xff), 0), 31))
    first = min(range(n), key=lambda i: (keys[i], i))
    if (all(fails) if compact else fails[first]):
        return True, [], [list(r) for r in q]
    picked = set()
    for _ in range(min(K, n)):
        bi = None
        for i in range(n):
            if i not in picked and (bi is None or keys[i] < keys[bi]):
                bi = i
        picked.add(bi)
    sel = [i in picked and not fails[i] for i in range(n)]
    if not any(sel):
        return True, [], [list(r) for r in q]
    m = n - sum(sel)
    tail = [i for i in range(m, n) if not sel[i]]
    after = []
    for p in range(m):
        after.append(list(q[p]) if not sel[p] else list(q[tail.pop(0)]))
    return False, [list(q[i][:4]) for i in range(n) if sel[i]], after


def random_state(rng):
    n = int(rng.integers(0, 25))
    cells = rng.permutation(4096)[:n]
    depth = rng.integers(1, 13, n)
    w = (2.0 ** -depth).astype(F)
    xyz = np.stack([cells & 15, (cells >> 4) & 15, cells >> 8], 1).astype(F) / F(16) + F(-0.5)
    lbs = np.array([1.0, 1.0 + 2 ** -20, 1.0 + 2 ** -19, 1.0 + 2 ** -18, 1.5, 2.0, 2.0 + 2 ** -21, 3.0], F)
    lb = lbs[rng.integers(0, len(lbs), n)]
    return np.concatenate([xyz, w[:, None], (lb + F(1))[:, None], lb[:, None]], 1).astype(F)


def test_selection_and_removal_equal_brute_force():
    rng = np.random.default_rng(11)
    seen = {"done": 0, "listed": 0, "cut": 0, "compact": 0}
    for _ in range(3000):
        q = random_state(rng)
        K = int(rng.integers(1, 9))
        best = float(F(rng.choice([1.0, 1.5, 2.0, 2.5, 3.5])))
        thr = float(F(rng.choice([0.0, 2 ** -20, 0.5])))
        sc = int(rng.choice([0, 0, 4]))
        stale = int(rng.integers(0, 2))
        rp = Round(thr=thr, K=K, root=ROOT, stale_compact=sc)
        S = Search(queue=q, best=best, stale=stale)
        out = T.one_round(S, rp)
        compact = sc > 0 and stale >= 1 and len(q) >= sc
        done, listed, after = brute(q, best, thr, K, rp, compact)
        assert bool(out.search.done) == done
        assert np.array_equal(np.asarray(listed, F).reshape(-1, 4), out.listed)
        assert np.array_equal(np.asarray(after, F).reshape(-1, 6), out.search.queue)
        assert out.search.pops == (1 if done and len(q) else 0)
        if not done:
            T.check_properties(S, rp, out, out.search.queue, out.listed, out.search.best)
            seen["listed"] += 1
            seen["cut"] += len(listed) < min(K, len(q))
            seen["compact"] += compact
        else:
            seen["done"] += 1
    assert min(seen.values()) > 50, seen                             # every branch was exercised


# ---- whole search ------------------------------------------------------------------------------------------------------------------
_PTS = np.random.default_rng(5).uniform(-0.45, 0.45, (6, 3)).astype(F)
_OFF = np.array([0.30, 0.10, 0.22, 0.10 + 2 ** -6, 0.4, 0.15], F)


def bounds(c4):
    """(ub, lb) of cubes (n, 4) for f(t) = min_p |t - p|^2 + off_p: ub = f at the centre, lb = the same with the distance from the cube"""
    c4 = np.asarray(c4, F).reshape(-1, 4)
    lo, hi = c4[:, None, :3], c4[:, None, :3] + c4[:, None, 3:4]
    d = np.maximum(np.maximum(lo - _PTS[None], _PTS[None] - hi), F(0))
    lb = ((d * d).sum(2, dtype=F) + _OFF[None]).min(1)
    cen = c4[:, None, :3] + c4[:, None, 3:4] / F(2) - _PTS[None]
    ub = ((cen * cen).sum(2, dtype=F) + _OFF[None]).min(1)
    return ub.astype(F), lb.astype(F)


def heap_search(thr):
    """GoICP::InnerBnB's shape: pop the smallest lb, stop when best - lb < thr, bound the 8 children, push those with lb < best"""
    best = F(1e30)
    heap = [(F(0), 0, ROOT)]
    tick = 1
    while heap:
        lb, _, node = heapq.heappop(heap)
        if best - lb < F(thr):
            break
        ch = T.children([node])
        ub, lbs = bounds(ch)
        for c, u, l in zip(ch, ub, lbs):
            if u < best:
                best = u
            if l < best:
                heapq.heappush(heap, (l, tick, tuple(c)))
                tick += 1
    return float(best)


THR = 1e-3


@pytest.mark.parametrize("compact", [0, 64])
@pytest.mark.parametrize("widen", [0, 1, 2, 3])
@pytest.mark.parametrize("K", [1, 8, 32, 128])
def test_iterated_rounds_are_a_valid_bnb(K, widen, compact):
    rp = Round(thr=THR, K=K, kmax=512, root=ROOT, stale_widen=widen, stale_compact=compact)
    S = Search(queue=np.array([[*ROOT, 0, 0]], F), best=1e30)
    prev4 = ub = lb = None
    expanded = set()
    best_ub_seen = np.inf
    for _ in range(20000):
        out = T.one_round(S, rp, prev4, ub, lb)
        S = out.search
        if S.done:
            break
        assert len(out.listed) == S.n_parents > 0
        for r in out.listed:
            k = r.tobytes()
            assert k not in expanded, "a node was expanded twice"
            expanded.add(k)
        prev4 = out.listed
        ub, lb = bounds(T.children(prev4))
        best_ub_seen = min(best_ub_seen, float(ub.min()))
    assert S.done == 1
    ref = heap_search(THR)
    assert abs(S.best - ref) <= THR, (S.best, ref)
    assert S.best >= float(_OFF.min()) and S.best - float(_OFF.min()) <= 2 * THR        # within thr of the true optimum, never below it
    # the best node's bound is attained: the record names a cube whose ub is the value, and it is the smallest ub any child had
    u, _ = bounds([S.bnode])
    assert S.improved == 1 and float(u[0]) == S.best == S.min_ub == best_ub_seen
    assert S.pops == len(expanded) + 1 or S.pops == len(expanded)       # + the node popped and rejected, unless the queue ran empty
    assert S.cubes == 8 * len(expanded)


# ---- seeded defects ----------------------------------------------------------------------------------------------------------------
def _nodes(lbs, depth=4):
    n = len(lbs)
    i = np.arange(n)
    w = F(2.0 ** -depth)
    xyz = np.stack([i & 15, (i >> 4) & 15, i >> 8], 1).astype(F) * w + F(-0.5)
    lbs = np.asarray(lbs, F)
    return np.concatenate([xyz, np.full((n, 1), w, F), (lbs + F(1))[:, None], lbs[:, None]], 1).astype(F)


def _caught(S, rp, defect, prev4=None, ub=None, lb=None):
    good = T.one_round(S, rp, prev4, ub, lb)
    T.check_properties(S, rp, good, good.search.queue, good.listed, good.search.best)         # the model itself passes
    bad = T.one_round(S, rp, prev4, ub, lb, defect=defect)
    with pytest.raises(AssertionError) as e:
        T.check_properties(S, rp, good, bad.search.queue, bad.listed, bad.search.best)
    return str(e.value)


def test_seeded_defects_of_the_model_are_caught():
    # rank <= rem: a tie group straddles the K-th place -> one node too many
    S = Search(queue=_nodes([1, 2, 2, 2, 2, 3]), best=10.0)
    assert "width" in _caught(S, Round(thr=0.5, K=3, root=ROOT), "rank_le")
    # the stop rule with <=: a node with best - lb == thr exactly is one of the K smallest and passes the rule, so it must be listed
    S = Search(queue=_nodes([2.0, 1.0, 3.0]), best=2.5)
    assert "complete" in _caught(S, Round(thr=0.5, K=2, root=ROOT), "stop_le")
    # fillers in reverse order: two holes in the head, two fillers in the tail
    S = Search(queue=_nodes([1, 5, 1, 6, 7, 8]), best=10.0)
    assert "removal" in _caught(S, Round(thr=0.5, K=2, root=ROOT), "fill_reverse")
    # the second digest pass ignored: 129 expansions, the last one's children are never pushed
    prev4 = _nodes(np.zeros(129), depth=3)[:, :4]
    lb = np.full(8 * 129, 2.0, F)
    ub = np.full(8 * 129, 20.0, F)
    S = Search(queue=_nodes([1, 2], depth=5), best=10.0, n_parents=129)
    assert "identity" in _caught(S, Round(thr=0.5, K=1, root=ROOT), "skip_pass2", prev4, ub, lb)
