"""A model of ONE round of the device BnB queue kernel (bnb_queue_kernel, csrc/bnbqueue.hip) as data operations in numpy: what a round
computes, written from the rules in that file's header, in device.hpp (cube_in_range) and in GoICP::InnerBnB (jly_goicp.cpp:227-340) -- a
sort and a few list operations, no ballots, no ranks, no barriers.  tests/test_queue_round_model_host.py holds the model itself to a brute-force
reading of the rules and to a plain heap search; tests/test_gpu_queue_round.py holds the kernel to the model byte for byte.

Floats are float32 wherever the kernel compares or forms them (w / 2, corner + bit * w / 2, best - lb, the Morton scaling, the spread).  The
chunk partials of a digest are added here in chunk order: the callers keep them small integers, so every order gives the same float.

The model is exact where the rules decide the outcome.  They do not decide WHICH of several nodes with the same smallest truncated key is held
to the stop rule before the selection: the kernel's reduction keeps whichever a tie leaves in place (thread-major over a thread's slots, a
butterfly over the lanes -- a fixed choice, but not the first in queue order, at any queue length).  The model asks the first in queue order.
The two agree when all nodes of the smallest key give one verdict, and also when the first of them fails and the round takes one node: asked
or not, that node is then the one selected, it fails the rule per node, nothing is listed and the search is done with one pop either way.
Every other state with a split verdict is flagged `ambiguous`; the callers build none.

What a search that stops leaves behind is part of the model too: it stores its incumbent and count, but not `stale`, `deep` or `parent_off`
(they go with a listing); one that overflows its slab or the list stores none of them and its queue is not defined afterwards (the host re-runs
such a search from its original incumbent).
"""
import copy
from dataclasses import dataclass, field

import numpy as np

F = np.float32
QCAP, MAXPOP, ROUNDPOP, THREADS = 8192, 512, 128, 1024
# one_round(defect=...): "rank_le", "stop_le", "fill_reverse", "skip_pass2" seed a defect into the model itself (test_queue_round_model_host.py)


@dataclass
class Round:
    thr: float = 0.0
    K: int = 32
    kmax: int = 512
    cap: int = QCAP
    list_cap: int = 4096
    soft_overflow: int = 0
    root: tuple = (-0.5, -0.5, -0.5, 1.0)
    boxed: int = 0
    depth: int = 0
    lo: tuple = (0.0, 0.0, 0.0)
    hi: tuple = (0.0, 0.0, 0.0)
    stale_widen: int = 0
    stale_compact: int = 0
    tile_spread: float = 0.0
    tile_min: int = 0


@dataclass
class Search:
    queue: np.ndarray = field(default_factory=lambda: np.zeros((0, 6), F))     # rows x, y, z, w, ub, lb
    best: float = 1e30
    coeff: float = 0.0
    rot: int = 0
    done: int = 0
    improved: int = 0
    n_parents: int = 0
    parent_off: int = 0
    pops: int = 0
    cubes: int = 0
    bnode: tuple = (0.0, 0.0, 0.0, 0.0)
    tile: int = 0
    min_ub: float = np.inf
    deep: int = 0
    stale: int = 0
    twin: int = -1


@dataclass
class Outcome:
    search: Search                      # the record afterwards (parent_off: as it came; the caller knows where the list put the search)
    listed: np.ndarray                  # (n_sel, 4) corner + width, queue order
    queue_defined: bool = True
    overflow: int = 0                   # raised QCtl::overflow
    tile_hint: int = 0                  # added to QCtl::tile_hint
    active: int = 0                     # added to QCtl::n_active
    claimed: int = 0                    # slots taken from QCtl::n_groups (the selection's size, also when the list then had no room)
    ambiguous: bool = False             # the state lies outside the model's scope (module docstring): no expectation
    pushed: np.ndarray = None           # (., 6) what the digest appended
    purged: np.ndarray = None           # (., 6) what the full slab threw out


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def depth_of(root_w, w):
    """levels below the root: the exponent difference of the two widths (w = root_w 2^-depth exactly)"""
    return ((bits(root_w) >> 23) & 0xff).astype(np.int64) - ((bits(w) >> 23) & 0xff).astype(np.int64)


def lb_keys(rp, q):
    return (bits(q[:, 5]) & ~np.uint32(31)).astype(np.int64) | np.clip(depth_of(F(rp.root[3]), q[:, 3]), 0, 31)


def morton_keys(rp, q):
    """30-bit Morton code of the corner on the 1 024^3 grid of the root, x in the lowest bit"""
    sc = F(1024.0) / F(rp.root[3])
    key = np.zeros(len(q), np.int64)
    for axis in range(3):
        g = np.clip(np.trunc((q[:, axis] - F(rp.root[axis])) * sc).astype(np.int64), 0, 1023)
        for b in range(10):
            key |= ((g >> b) & 1) << (3 * b + axis)
    return key


def in_range(rp, x, y, z, w):
    """cube_in_range (device.hpp): the half-open cube against the closed range"""
    lo, hi = np.asarray(rp.lo, F), np.asarray(rp.hi, F)
    return (x + w > lo[0]) & (x <= hi[0]) & (y + w > lo[1]) & (y <= hi[1]) & (z + w > lo[2]) & (z <= hi[2])


def children(prev4):
    """(n_prev, 4) expansions -> (8 n_prev, 4) children, expansion order then child order (jly_goicp.cpp:262-273)"""
    prev4 = np.asarray(prev4, F).reshape(-1, 4)
    c = np.arange(8)
    cw = np.repeat(prev4[:, 3] / F(2), 8)
    out = np.empty((8 * len(prev4), 4), F)
    for axis in range(3):
        out[:, axis] = np.repeat(prev4[:, axis], 8) + np.tile((c >> axis) & 1, len(prev4)).astype(F) * cw
    out[:, 3] = cw
    return out


def sum_partials(scratch, chunks):
    """[expansion][chunk][ub 8 | lb 8] -> (ub, lb) of the 8 n children, added in chunk order in float32"""
    s = np.asarray(scratch, F).reshape(-1, chunks, 2, 8)
    acc = np.zeros((len(s), 2, 8), F)
    for j in range(chunks):
        acc = acc + s[:, j]
    return acc[:, 0].reshape(-1).copy(), acc[:, 1].reshape(-1).copy()


def fails_stop(best, lb, thr, defect=None):
    """jly_goicp.cpp:257: a node that can no longer close the gap"""
    gap = F(best) - np.asarray(lb, F)
    return gap <= F(thr) if defect == "stop_le" else gap < F(thr)


def round_width(rp, stale, n):
    K = rp.K
    if rp.stale_widen == 1:
        K = min(4 * rp.K, MAXPOP) if stale >= 3 else (min(2 * rp.K, MAXPOP) if stale >= 1 else rp.K)
    elif rp.stale_widen == 2:
        K = min(4 * rp.K, MAXPOP) if stale >= 1 else rp.K
    elif rp.stale_widen == 3:
        K = min(4 * rp.K, MAXPOP) if stale >= 1 else min(2 * rp.K, MAXPOP)
    K = min(K, rp.kmax)
    if K > ROUNDPOP:
        K = max(ROUNDPOP, min(K, (rp.cap - n) // 8))
    return K


def one_round(S, rp, prev4=None, ub=None, lb=None, off=None, defect=None):
    """One round of one search.  prev4: the previous list's records of THIS search ((n_parents, 4) corner + width), ub / lb: its 8 n_parents
    children's bounds.  off: where the round's list would put the search's expansions (None: there is room)."""
    S = copy.deepcopy(S)
    empty4, empty6 = np.zeros((0, 4), F), np.zeros((0, 6), F)
    out = Outcome(S, empty4, pushed=empty6, purged=empty6)
    if S.done:
        return out
    q = np.asarray(S.queue, F).reshape(-1, 6).copy()
    best, stale = F(S.best), S.stale
    n_prev = S.n_parents
    if n_prev > 0:
        ch = children(prev4)
        ub, lb = np.asarray(ub, F), np.asarray(lb, F)
        assert len(ch) == 8 * n_prev == len(ub) == len(lb)
        valid = in_range(rp, ch[:, 0], ch[:, 1], ch[:, 2], ch[:, 3]) if rp.boxed else np.ones(len(ch), bool)
        shallow = depth_of(F(rp.root[3]), ch[:, 3]) < rp.depth if rp.depth > 0 else np.ones(len(ch), bool)
        improved_any = False
        pushed, purged = [], []
        for p0 in range(0, len(ch), THREADS):
            if defect == "skip_pass2" and p0 == THREADS:
                continue
            sl = slice(p0, min(p0 + THREADS, len(ch)))
            vub = np.where(valid[sl], ub[sl], F(np.inf))
            i = int(np.argmin(vub))                                      # the first of equal minima
            if vub[i] < F(S.min_ub):
                S.min_ub = float(vub[i])
            if vub[i] < best:
                best, improved_any = vub[i], True
                S.bnode, S.improved = tuple(float(v) for v in ch[p0 + i]), 1
            push = valid[sl] & (lb[sl] < best) & shallow[sl]
            new = np.concatenate([ch[sl][push], ub[sl][push, None], lb[sl][push, None]], axis=1)
            if len(q) + len(new) > rp.cap:
                dead = fails_stop(best, q[:, 5], rp.thr)
                purged.append(q[dead])
                q = q[~dead]
            if len(q) + len(new) > rp.cap:
                S.done = 2 if rp.soft_overflow else 1
                S.n_parents = 0
                out.overflow = 0 if rp.soft_overflow else 1
                out.queue_defined = False
                return out
            pushed.append(new)
            q = np.concatenate([q, new])
        out.pushed = np.concatenate(pushed) if pushed else empty6
        out.purged = np.concatenate(purged) if purged else empty6
        stale = 0 if improved_any else stale + 1
        S.pops += n_prev
        S.cubes += 8 * n_prev
    n = len(q)
    K = round_width(rp, stale, n)
    compact = rp.stale_compact > 0 and stale >= 1 and n >= rp.stale_compact
    stopped = n == 0
    if n > 0:
        fails = fails_stop(best, q[:, 5], rp.thr, defect)
        pos = np.arange(n)
        if compact:
            key = np.where(fails, np.int64(0xfffffffe), morton_keys(rp, q))
            stopped = bool(fails.all())
        else:
            key = lb_keys(rp, q)
            first = np.lexsort((pos, key))[0]
            stopped = bool(fails[first])
            # outside the model: the nodes of the smallest key disagree on the stop rule, and which of them is asked would matter
            ties = fails[key == key[first]]
            out.ambiguous = bool(ties.any() and not ties.all()) and not (stopped and min(K, n) == 1)
    if not stopped:
        order = np.lexsort((pos, key))
        take = min(K, n)
        if defect == "rank_le" and n > K:                                # one tie too many
            take += int(key[order[K]] == key[order[K - 1]])
        sel = np.zeros(n, bool)
        sel[order[:take]] = True
        sel &= ~fails
        stopped = not sel.any()
    if stopped:
        S.best, S.queue, S.n_parents, S.done = float(best), q, 0, 1
        S.pops += 1 if n > 0 else 0
        return out
    n_sel = int(sel.sum())
    out.listed = q[sel][:, :4].copy()
    # the spread decision: the extent of the selected corners, per axis, plus the widest selected cube
    deep = 0
    if rp.tile_spread > 0:
        c = out.listed
        spread = F(0)
        for axis in range(3):
            spread = max(spread, F(c[:, axis].max() - c[:, axis].min()))
        spread = F(spread + c[:, 3].max())
        deep = int(spread <= F(rp.tile_spread))
        out.tile_hint = deep
    out.active, out.claimed = 1, n_sel
    if off is not None and off + n_sel > rp.list_cap:
        # the list has no room: the batch goes back to the host, nothing of the selection is stored
        S.done, S.n_parents = 1, 0
        out.overflow, out.queue_defined, out.listed = 1, False, empty4
        return out
    # removal: the holes among the first m positions take the unselected nodes of the tail, in order
    m = n - n_sel
    fillers = [p for p in range(m, n) if not sel[p]]
    if defect == "fill_reverse":
        fillers = fillers[::-1]
    after = q[:m].copy()
    after[sel[:m]] = q[fillers]
    S.best, S.queue, S.n_parents, S.tile, S.stale, S.deep = float(best), after, n_sel, 0, stale, deep
    return out


# ---- the same thing without an order: what a failure is a failure OF ------------------------------------------------------------

def rows(a):
    """multiset of node rows, by their bits"""
    a = np.ascontiguousarray(np.asarray(a, F))
    out = {}
    for r in a:
        k = r.tobytes()
        out[k] = out.get(k, 0) + 1
    return out


def _add(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


def check_properties(before, rp, expect, queue_after, listed4, best_after):
    """Order-free (and one order-light) statement of a listing round; raises AssertionError naming the property.  before: the Search the round
    started from; expect: the model's Outcome (its pushed / purged sets and width only); queue_after, listed4, best_after: what was observed."""
    qb = np.asarray(before.queue, F).reshape(-1, 6)
    qa = np.asarray(queue_after, F).reshape(-1, 6)
    listed4 = np.asarray(listed4, F).reshape(-1, 4)
    pool = np.concatenate([qb, expect.pushed])
    if len(expect.purged):
        dead = rows(expect.purged)
        keep = []
        for r in pool:
            k = r.tobytes()
            if dead.get(k, 0) > 0:
                dead[k] -= 1
            else:
                keep.append(r)
        pool = np.array(keep, F).reshape(-1, 6)
    # the listed records carry no bounds: find their nodes in the pool by corner + width (the callers keep those unique)
    by4 = {}
    for r in pool:
        by4.setdefault(r[:4].tobytes(), []).append(r)
    lnodes = []
    for r in listed4:
        cand = by4.get(r.tobytes())
        assert cand, "identity: a listed record is no node of queue_before + pushed - purged"
        lnodes.append(cand.pop())
    lnodes = np.array(lnodes, F).reshape(-1, 6)
    assert _add(rows(qa), rows(lnodes)) == rows(pool), "identity: queue_before + pushed != queue_after + listed + purged (a node lost or doubled)"
    assert not set(rows(qa[:, :4])) & set(rows(listed4)), "disjoint: a listed node is still queued"
    assert not fails_stop(best_after, lnodes[:, 5], rp.thr).any(), "stop rule: a listed node has best - lb < thr"
    stale = expect.search.stale
    K = round_width(rp, stale, len(pool))
    assert len(listed4) <= K, "width: more nodes listed than the round's K"
    compact = rp.stale_compact > 0 and stale >= 1 and len(pool) >= rp.stale_compact
    passing = qa[~fails_stop(best_after, qa[:, 5], rp.thr)]
    kf = morton_keys if compact else lb_keys
    if len(passing) and len(lnodes):
        assert kf(rp, lnodes).max() <= kf(rp, passing).min(), "order: a queued node that passes the stop rule has a smaller key than a listed one"
    if len(passing) and len(listed4) < min(K, len(pool)):
        # fewer than K listed: every node that is surely among the K smallest keys and is still queued fails the stop rule
        kp = np.where(fails_stop(best_after, pool[:, 5], rp.thr), np.int64(0xfffffffe), kf(rp, pool)) if compact else kf(rp, pool)
        kth = np.sort(kp)[min(K, len(pool)) - 1]
        surely = kth + 1 if (kp <= kth).sum() == min(K, len(pool)) else kth
        assert not (kf(rp, passing) < surely).any(), "complete: a node among the K smallest keys passes the stop rule and was not listed"
    # order-light: the nodes that stay in the head stay where they were; the moved ones keep their order
    m = len(qa)
    pos_before = {}
    for i, r in enumerate(pool):
        pos_before.setdefault(r.tobytes(), []).append(i)
    moved = []
    for p, r in enumerate(qa):
        src = pos_before[r.tobytes()].pop(0)
        if src < m:
            assert src == p, "removal: a node of the head that was not selected moved"
        else:
            moved.append(src)
    assert moved == sorted(moved), "removal: the fillers from the tail are not in their order"
