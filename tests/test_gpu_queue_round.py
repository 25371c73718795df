"""One round of the device BnB queue kernel (bnb_queue_kernel, csrc/bnbqueue.hip) against the model of tests/queue_round_twin.py, byte for byte,
through goicp_debug_queue_round: one launch of at most eight workgroups on caller-given queues, previous expansions and children's bounds.

Every case runs with the 128-VGPR and the 64-VGPR build (`deep` 0 / 1); the first is held to the model -- the order-free properties
(check_properties) first, so that a failure says what kind it is, then the queue, the QSearch record, the listed records and the control words
bit for bit -- and the second to the first.  Where several searches share a launch, the ORDER of their ranges in the round's list is decided by
an atomic and is not asserted: the ranges are disjoint, cover [n_groups before, n_groups after), and each holds what the model lists.

Inputs are built so that every expectation is exact: the root width is a power of two, corners lie on the 2^-12 grid of the root, and the chunk
partials of a digest are small non-negative integers (any summation order gives the same float).  Every queue's (corner, width) pairs are
unique, so a listed record names one node.  The nodes that share a queue's smallest truncated key all pass or all fail the stop rule (the
model's scope, queue_round_twin.py; verify() refuses a case outside it), but for the one case whose outcome does not depend on which is asked.

Two shapes of the issue's list cannot occur and are replaced by their nearest neighbours: 512 nodes cannot be taken out of a queue of 8 192 (a
round wider than 128 is throttled by the slab's room, (cap - n) / 8, down to 128), so 512 are taken out of 513, 1 024 and 4 096 and 128 out of
8 192.
"""
import ctypes as C

import numpy as np
import pytest

import queue_round_twin as T
from conftest import load_pkg, tiny_problem
from queue_round_twin import F, Round, Search

pytestmark = pytest.mark.gpu

INVALID = -1
ROOT = (-0.5, -0.5, -0.5, 1.0)
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4"), ("coeff", "<f4"), ("rot", "<i4")])
INTS = ("rot", "count", "done", "improved", "n_parents", "pops", "cubes", "tile", "deep", "stale", "twin")
FIELDS = ("best", "coeff", "rot", "count", "done", "improved", "n_parents", "pops", "cubes", "bx", "by", "bz", "bw", "tile", "min_ub", "deep", "stale", "twin")


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def reg(pkg):
    tgt, src = tiny_problem(1)
    r = pkg.Registration(tgt, src, 5e-3)
    yield r
    r.close()


# ---- building states ---------------------------------------------------------------------------------------------------------------
def nodes_at(grid12, lb, depth=6):
    """queue nodes with corners ROOT + grid12 * 2^-12 (integers, (n, 3)), widths 2^-depth, ub = lb + 1"""
    lb = np.asarray(lb, F)
    n = len(lb)
    xyz = np.asarray(grid12, np.int64).reshape(n, 3).astype(F) * F(2.0 ** -12) + F(-0.5)
    w = np.ldexp(F(1), -np.broadcast_to(np.asarray(depth), (n,)).astype(np.int32)).astype(F)
    return np.concatenate([xyz, w[:, None], (lb + F(1))[:, None], lb[:, None]], 1).astype(F)


def nodes(lb, depth=6, cell0=0):
    """len(lb) queue nodes on distinct cells of the depth-5 grid of ROOT from cell0 on (32 768 cells)"""
    c = cell0 + np.arange(len(lb))
    assert len(c) == 0 or c[-1] < 32768
    return nodes_at(np.stack([c & 31, (c >> 5) & 31, c >> 10], 1) * 128, lb, depth)


def parents(n, depth=5, cell0=16384):
    """n previous expansions on distinct depth-5 cells of the upper half of ROOT (no queue node of nodes() with cell < 16 384 lies there)"""
    return nodes(np.zeros(n), depth, cell0)[:, :4]


class Case:
    def __init__(self, rp, searches, prevs=None, chunks=1, parity=0, ctl0=(0, 0, 0, 0, 0, 0), with_ps=True):
        self.rp, self.searches, self.chunks, self.parity, self.ctl0, self.with_ps = rp, searches, chunks, parity, list(ctl0), with_ps
        self.prevs = prevs if prevs is not None else [None] * len(searches)
        cursor = 1                                                    # caller-chosen offsets: a gap in front of and between the searches' ranges
        for S, p in zip(self.searches, self.prevs):
            S.n_parents = 0 if p is None else len(p[0])
            if p is not None:
                S.parent_off = cursor
                cursor += len(p[0]) + 1
        self.n_prev_list = cursor


def split(v, chunks, shift):
    """non-negative integer partials of the integers v over `chunks` chunks, (len(v), chunks)"""
    v = np.asarray(v, np.int64)
    assert (v >= 0).all() and (v < 2 ** 24).all() and (v == np.asarray(v)).all()
    j = (np.arange(chunks)[None, :] + np.asarray(shift)[:, None]) % chunks
    return (v[:, None] // chunks + (j < (v[:, None] % chunks))).astype(F)


def launch(pkg, reg, case, deep):
    B = pkg.binding
    rp, ns = case.rp, len(case.searches)
    r = B.CQueueRound(nsearch=ns, parity=case.parity, deep=deep, chunks=case.chunks, n_prev_list=case.n_prev_list, thr=rp.thr, K=rp.K, kmax=rp.kmax,
                      cap=rp.cap, list_cap=rp.list_cap, soft_overflow=rp.soft_overflow, root=(C.c_float * 4)(*rp.root), boxed=rp.boxed, depth=rp.depth,
                      lo=(C.c_float * 3)(*rp.lo), hi=(C.c_float * 3)(*rp.hi), stale_widen=rp.stale_widen, stale_compact=rp.stale_compact,
                      tile_spread=rp.tile_spread, tile_min=rp.tile_min)
    recs = (B.CQueueSearch * ns)()
    slab = np.full((ns, B.QUEUE_SLAB, 6), np.nan, F)
    npl = case.n_prev_list
    prev = np.zeros(npl, REC)
    prev.view(np.uint32)[:] = 0xffffffff
    ub, lb = np.full(8 * npl, np.nan, F), np.full(8 * npl, np.nan, F)
    scratch = np.full((npl, case.chunks, 2, 8), np.nan, F)
    for s, (S, p) in enumerate(zip(case.searches, case.prevs)):
        q = np.asarray(S.queue, F).reshape(-1, 6)
        slab[s, :len(q)] = q
        c = recs[s]
        c.best, c.coeff, c.rot, c.count, c.done, c.improved, c.n_parents, c.parent_off = S.best, S.coeff, S.rot, len(q), S.done, S.improved, S.n_parents, S.parent_off
        c.pops, c.cubes, (c.bx, c.by, c.bz, c.bw), c.tile, c.min_ub, c.deep, c.stale, c.twin = S.pops, S.cubes, S.bnode, S.tile, S.min_ub, S.deep, S.stale, S.twin
        if p is not None:
            sl = slice(S.parent_off, S.parent_off + len(p[0]))
            for k, name in enumerate("xyzw"):
                prev[name][sl] = p[0][:, k]
            prev["coeff"][sl], prev["rot"][sl] = 0.25, 7
            if case.chunks == 1:
                ub[8 * sl.start:8 * sl.stop], lb[8 * sl.start:8 * sl.stop] = p[1], p[2]
            else:
                shift = np.arange(len(p[1])) * 7 + s
                scratch[sl, :, 0, :] = split(p[1], case.chunks, shift).reshape(-1, 8, case.chunks).transpose(0, 2, 1)
                scratch[sl, :, 1, :] = split(p[2], case.chunks, shift + 3).reshape(-1, 8, case.chunks).transpose(0, 2, 1)
                su, sl_ = T.sum_partials(scratch[sl], case.chunks)
                assert su.tobytes() == np.asarray(p[1], F).tobytes() and sl_.tobytes() == np.asarray(p[2], F).tobytes()
    ctl = (C.c_int32 * 6)(*case.ctl0)
    listed = np.zeros(rp.list_cap, REC)
    psearch = np.zeros(rp.list_cap, np.int32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = reg._lib.goicp_debug_queue_round(reg.handle, C.byref(r), recs, fp(slab), prev.ctypes.data_as(C.c_void_p), fp(ub), fp(lb), fp(scratch), ctl,
                                          listed.ctypes.data_as(C.c_void_p), psearch.ctypes.data_as(C.POINTER(C.c_int32)) if case.with_ps else None)
    if rc != 0:
        return rc
    out = []
    for s in range(ns):
        c = recs[s]
        S = Search(queue=slab[s, :c.count].copy(), best=c.best, coeff=c.coeff, rot=c.rot, done=c.done, improved=c.improved, n_parents=c.n_parents,
                   parent_off=c.parent_off, pops=c.pops, cubes=c.cubes, bnode=(c.bx, c.by, c.bz, c.bw), tile=c.tile, min_ub=c.min_ub, deep=c.deep,
                   stale=c.stale, twin=c.twin)
        S.count = c.count
        out.append(S)
    return out, listed, (psearch if case.with_ps else None), list(ctl)


def record_bytes(S, count):
    v = dict(best=S.best, coeff=S.coeff, rot=S.rot, count=count, done=S.done, improved=S.improved, n_parents=S.n_parents, pops=S.pops, cubes=S.cubes,
             bx=S.bnode[0], by=S.bnode[1], bz=S.bnode[2], bw=S.bnode[3], tile=S.tile, min_ub=S.min_ub, deep=S.deep, stale=S.stale, twin=S.twin)
    return {k: (np.int32(v[k]) if k in INTS else F(v[k])).tobytes() for k in FIELDS}


def normalised(case, obs):
    """what must not depend on the build or on the order the searches reached the list's counter"""
    got, listed, psearch, ctl = obs
    per = [(record_bytes(S, S.count), S.queue.tobytes(), listed[S.parent_off:S.parent_off + S.n_parents].tobytes()) for S in got]
    return per, ctl


def verify(case, obs):
    rp = case.rp
    got, listed, psearch, ctl = obs
    ns = len(case.searches)
    exp = []
    for s, (S0, p, G) in enumerate(zip(case.searches, case.prevs, got)):
        before = Search(**{**S0.__dict__})
        pv = (None, None, None) if p is None else p
        off = case.ctl0[case.parity] if ns == 1 else None
        e = T.one_round(before, rp, pv[0], pv[1], pv[2], off=off)
        exp.append(e)
        assert not e.ambiguous, "search %d: the case lies outside the model's scope (split stop verdict on the smallest key)" % s
        E = e.search
        listing = E.n_parents > 0
        if listing:
            assert G.n_parents > 0 and not G.done, "search %d: the model lists %d nodes, the kernel stopped (done %d)" % (s, E.n_parents, G.done)
            glist = listed[G.parent_off:G.parent_off + G.n_parents]
            g4 = np.stack([glist["x"], glist["y"], glist["z"], glist["w"]], 1)
            T.check_properties(before, rp, e, G.queue, g4, G.best)
            assert g4.tobytes() == e.listed.tobytes(), "search %d: listed records" % s
            assert (glist["coeff"] == F(S0.coeff)).all() and (glist["rot"] == S0.rot).all(), "search %d: coeff / rot of the listed records" % s
            if psearch is not None:
                assert (psearch[G.parent_off:G.parent_off + G.n_parents] == s).all(), "search %d: parent_search" % s
        else:
            assert G.n_parents == 0, "search %d: the model lists nothing (done %d), the kernel %d nodes" % (s, E.done, G.n_parents)
            assert G.parent_off == S0.parent_off
        want = record_bytes(E, len(np.asarray(E.queue).reshape(-1, 6)))              # (a search that overflowed keeps the count it came with)
        have = record_bytes(G, G.count)
        diff = [k for k in FIELDS if want[k] != have[k]]
        show = lambda rec: [np.frombuffer(rec[k], np.int32 if k in INTS else F)[0] for k in diff]
        assert not diff, "search %d: QSearch fields %s: kernel %s, model %s" % (s, diff, show(have), show(want))
        if e.queue_defined:
            assert G.queue.tobytes() == np.asarray(E.queue, F).tobytes(), "search %d: queue" % s
    # the ranges: disjoint, and together exactly [n_groups before, n_groups after)
    par = case.parity
    assert ctl[par] == case.ctl0[par] + sum(e.claimed for e in exp), "n_groups"
    spans = sorted((G.parent_off, G.parent_off + G.n_parents) for G in got if G.n_parents)
    covered = case.ctl0[par]
    for a, b in spans:
        assert a >= covered and b <= ctl[par], "the searches' ranges overlap or leave [n_groups before, n_groups after)"
        covered = b
    if all(e.claimed == e.search.n_parents for e in exp):          # (a search that found no room in the list had taken its range already)
        assert sum(b - a for a, b in spans) == ctl[par] - case.ctl0[par], "the searches' ranges leave a gap"
    written = np.zeros(rp.list_cap, bool)
    for a, b in spans:
        written[a:b] = True
    raw = listed.view(np.uint32).reshape(-1, 6)
    assert (raw[~written] == 0xffffffff).all(), "a record outside every search's range was written"
    if psearch is not None:
        assert (psearch[~written] == -1).all(), "parent_search outside every search's range was written"
    assert ctl[par ^ 1] == 0 and ctl[2 + (par ^ 1)] == 0, "the other parity's counters are zeroed by workgroup 0"
    assert ctl[2 + par] == case.ctl0[2 + par] + sum(e.active for e in exp), "n_active"
    assert ctl[4] == max([case.ctl0[4]] + [e.overflow for e in exp]), "overflow"
    assert ctl[5] == case.ctl0[5] + sum(e.tile_hint for e in exp), "tile_hint"
    return exp


def run(pkg, reg, case):
    o0 = launch(pkg, reg, case, 0)
    if isinstance(o0, int):
        pkg.binding.check(o0)
    exp = verify(case, o0)
    o1 = launch(pkg, reg, case, 1)
    if isinstance(o1, int):
        pkg.binding.check(o1)
    assert normalised(case, o0) == normalised(case, o1), "the <4> and the <8> build differ"
    return exp, o0


# ---- digest ------------------------------------------------------------------------------------------------------------------------
def int_bounds(rng, n_children, lo=10, hi=900):
    ub = rng.integers(lo, hi, n_children).astype(F)
    lb = np.floor(ub * rng.uniform(0, 1, n_children)).astype(F)
    return ub, lb


@pytest.mark.parametrize("chunks", [1, 2, 5, 118])
@pytest.mark.parametrize("n_prev", [1, 16, 128, 129, 256, 512])
def test_digest_shapes(pkg, reg, n_prev, chunks):
    """one to four passes, the bounds given or summed from chunk partials, into an empty queue and into queues on both sides of the switch
    between the one-slot and the eight-slot form (count + 8 n_prev <= 1 024); each pass prunes with the incumbent so far"""
    rng = np.random.default_rng(1000 * n_prev + chunks)
    counts = [0] + ([1024 - 8 * n_prev, 1024 - 8 * n_prev + 1] if 8 * n_prev <= 1024 else [57])
    searches, prevs = [], []
    for k, c0 in enumerate(counts):
        ub, lb = int_bounds(rng, 8 * n_prev)
        if n_prev >= 129:                                              # the incumbent falls again in the last pass
            ub[-3] = 5
        q = nodes(rng.integers(0, 700, c0).astype(F), depth=rng.integers(5, 9, c0))
        searches.append(Search(queue=q, best=600.0, coeff=0.5 * k, rot=k, stale=k, pops=3, cubes=24))
        prevs.append((parents(n_prev, cell0=16384 + 600 * k), ub, lb))
    exp, _ = run(pkg, reg, Case(Round(thr=2.0, K=32, root=ROOT, stale_widen=1), searches, prevs, chunks=chunks))
    assert all(e.search.improved and e.search.stale == 0 and e.search.n_parents > 0 for e in exp)
    assert any(len(e.pushed) < 8 * n_prev for e in exp)                      # something was pruned


def test_digest_ties_and_edges(pkg, reg):
    """equal minimum ub in two lanes of a wavefront, in two wavefronts and in two passes (the first child wins, a later pass does not replace
    it); a child with lb == incumbent is not pushed; no improvement -> stale + 1 and min_ub still falls; n_prev = 0 -> stale stays"""
    def tie(n_prev, i, j, best=600.0):
        ub = np.full(8 * n_prev, 300, F)
        lb = np.full(8 * n_prev, 10, F)
        ub[i] = ub[j] = 50
        lb[i + 1] = 50                                                 # lb == the incumbent: not pushed
        lb[i + 2] = 49
        return Search(queue=nodes([10, 20, 30]), best=best, stale=1), (parents(n_prev), ub, lb)
    cases = [tie(16, 3, 40), tie(128, 10, 700), tie(129, 5, 1024 + 5), tie(256, 1500, 2047), tie(16, 3, 40, best=40.0)]
    searches, prevs = [c[0] for c in cases], [c[1] for c in cases]
    searches.append(Search(queue=nodes([10, 20, 30]), best=600.0, stale=2))
    prevs.append(None)
    exp, (got, *_) = run(pkg, reg, Case(Round(thr=2.0, K=2, root=ROOT), searches, prevs))
    ch = [T.children(p[0]) for p in prevs[:5]]
    assert got[0].bnode == tuple(ch[0][3]) and got[1].bnode == tuple(ch[1][10]) and got[2].bnode == tuple(ch[2][5]) and got[3].bnode == tuple(ch[3][1500])
    assert [g.stale for g in got] == [0, 0, 0, 0, 2, 2] and got[4].min_ub == 50 and got[4].best == 40 and not got[4].improved
    assert len(exp[0].pushed) == 8 * 16 - 1                                  # all but the lb == incumbent child


def test_digest_range_and_depth(pkg, reg):
    """the translation-range cull with faces on split planes (the cube that only ends at the low face is out, the one that starts at the high
    face is in), a range no child lies in, and the depth limit at, below and above the children's depth"""
    W = 0.5
    root = (-W / 2, -W / 2, -W / 2, W)
    # the 64 depth-2 cubes of the root: their children (depth 3, width W / 8) have faces on the planes z = +-W / 8
    g = np.arange(64)
    p4 = np.stack([g & 3, (g >> 2) & 3, g >> 4], 1).astype(F) * F(W / 4) + F(-W / 2)
    p4 = np.concatenate([p4, np.full((64, 1), W / 4, F)], 1)
    rng = np.random.default_rng(3)
    box = dict(boxed=1, lo=(-W / 2, -W / 2, -W / 8), hi=(W / 2, W / 2, W / 8))
    low = lambda: (rng.integers(10, 900, 512).astype(F), rng.integers(0, 9, 512).astype(F))      # every lb under every ub: all valid children are pushed
    for depth in (0, 2, 3, 4):
        searches = [Search(queue=np.zeros((0, 6), F), best=5000.0) for _ in range(2)]
        prevs = [(p4, *low()), (p4[::-1].copy(), *low())]
        exp, _ = run(pkg, reg, Case(Round(thr=1.0, K=8, root=root, depth=depth, **box), searches, prevs))
        z = exp[0].pushed[:, 2]
        if depth in (0, 4):
            # the slabs [-W/8, 0), [0, W/8) and [W/8, W/4) of 64 cubes each: the last starts on the high face, [-W/4, -W/8) only ends on the low one
            assert len(z) == 192 and sorted(set(z.tolist())) == [-W / 8, 0.0, W / 8]
        else:
            assert len(z) == 0 and exp[0].search.done == 1                            # depth 3 children are leaves at a limit of 2 or 3
    nothing = dict(boxed=1, lo=(2.0, 2.0, 2.0), hi=(3.0, 3.0, 3.0))
    S = Search(queue=nodes([10, 20]), best=5000.0, stale=4, min_ub=777.0)
    exp, (got, *_) = run(pkg, reg, Case(Round(thr=1.0, K=1, root=ROOT, **nothing), [S], [(parents(20), *int_bounds(rng, 160))]))
    assert got[0].stale == 5 and got[0].min_ub == 777.0 and got[0].best == 5000.0 and got[0].cubes == 160 and len(exp[0].pushed) == 0


# ---- slab --------------------------------------------------------------------------------------------------------------------------
def slab_search(rng, c0, n_prev, n_push, n_dead, best=500.0, thr=2.0, second_pass_best=None):
    """a queue of c0 nodes of which n_dead fail the stop rule against the incumbent AFTER the digest (400), spread over the whole queue, and a
    digest that pushes n_push of its 8 n_prev children"""
    lbq = rng.integers(0, 300, c0).astype(F)
    if n_dead:
        lbq[np.linspace(0, c0 - 1, n_dead).astype(int)] = rng.integers(399, 450, n_dead)
    ub = np.full(8 * n_prev, 450, F)
    ub[-2 if second_pass_best else 4] = 400
    lb = np.full(8 * n_prev, 401, F)
    lb[rng.permutation(8 * n_prev)[:n_push]] = rng.integers(0, 390, n_push)
    return Search(queue=nodes(lbq, depth=rng.integers(5, 9, c0)), best=best, stale=1), (parents(n_prev), ub, lb)


@pytest.mark.parametrize("cap,n_prev,over,n_dead", [(64, 4, 33, 5), (1000, 16, 873, 37), (8192, 12, 8100, 300)])
def test_slab_fit_purge_overflow(pkg, reg, cap, n_prev, over, n_dead):
    """`over` queued nodes and cap - over + 1 children to push: one node too many.  An exact fit (over - 1 nodes, with and without dead ones:
    no purge); one over with dead nodes (the purge makes room, the survivors keep their order); one over without, and still one over after
    the purge (done = 2 under soft overflow, done = 1 and QCtl::overflow otherwise, while the launch's other searches go on).  cap 8 192: a
    queue of 8 100 nodes whose dead ones lie in all eight slots of many wavefronts"""
    rng = np.random.default_rng(cap)
    n_push = cap - over + 1
    for soft in (1, 0):
        built = [slab_search(rng, over - 1, n_prev, n_push, 0), slab_search(rng, over - 1, n_prev, n_push, n_dead), slab_search(rng, over, n_prev, n_push, n_dead),
                 slab_search(rng, over, n_prev, n_push, 0), slab_search(rng, over + n_push // 2, n_prev, n_push, n_push // 2)]
        rp = Round(thr=2.0, K=8, cap=cap, soft_overflow=soft, root=ROOT)
        exp, (got, _, _, ctl) = run(pkg, reg, Case(rp, [b[0] for b in built], [b[1] for b in built]))
        assert [len(e.purged) for e in exp[:3]] == [0, 0, n_dead] and [len(e.pushed) for e in exp[:3]] == [n_push] * 3
        assert [g.done for g in got] == [0, 0, 0, 2 if soft else 1, 2 if soft else 1] and ctl[4] == 1 - soft
        assert got[0].count + got[0].n_parents == cap and got[2].count + got[2].n_parents == cap + 1 - n_dead


def test_slab_purge_in_the_second_pass(pkg, reg):
    """129 expansions: the first pass of 1 024 children fits, the second (8 children) does not; the incumbent that makes the dead nodes dead is
    found in that second pass"""
    rng = np.random.default_rng(8)
    S, p = slab_search(rng, 70, 129, 1032, 20, second_pass_best=True)
    p[2][-1] = 401                                                    # 1 031 pushed: 70 + 1 024 fit into 1 100, the second pass's 7 more do not
    exp, (got, *_) = run(pkg, reg, Case(Round(thr=2.0, K=8, cap=1100, root=ROOT), [S], [p]))
    assert len(exp[0].purged) == 20 and len(exp[0].pushed) == 1031 and got[0].best == 400 and got[0].count + got[0].n_parents == 70 + 1031 - 20


def test_list_without_room(pkg, reg):
    """a round's list that cannot take the selection: overflow, nothing written"""
    S = Search(queue=nodes([1, 2, 3]), best=100.0)
    exp, (got, _, _, ctl) = run(pkg, reg, Case(Round(thr=1.0, K=2, list_cap=16, root=ROOT), [S], ctl0=(15, 0, 0, 0, 0, 0)))
    assert got[0].done == 1 and ctl[4] == 1 and ctl[0] == 17


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def from_bits(b):
    return np.asarray(b, np.uint32).view(F)


def key_patterns(rng, n, K):
    """(lb, depth) per pattern"""
    one = 0x3f800000
    out = {}
    out["distinct"] = (F(1) + rng.permutation(n).astype(F) * F(2.0 ** -13), 6)
    out["equal"] = (np.full(n, 2, F), 6)
    lb = np.full(n, 3, F)
    lb[:K // 2] = 1
    lb[K // 2:K // 2 + max(2, (n - K // 2) // 2)] = 2
    out["straddle"] = (rng.permutation(lb), 6)                               # the K-th place falls inside the group of 2s
    out["low5"] = (from_bits(0x40000000 + rng.integers(0, 32, n)), 6)        # one key: queue order decides, not lb
    out["depth"] = (np.full(n, 2, F), rng.integers(5, 13, n))                # equal lb: the wider cube first
    out["top11"] = (from_bits(((0x1fc + rng.integers(0, 40, n)) << 21) | 0x12345), 6)
    out["mid11"] = (from_bits(one | (rng.integers(0, 2048, n) << 10) | 0x155), 6)
    out["low10"] = (from_bits(one | (rng.integers(0, 32, n) << 5) | 0x1f), rng.integers(5, 13, n))
    return out


PAIRS = [(1, 1), (1, 2), (1, 1024), (1, 8192), (8, 8), (8, 9), (8, 1023), (8, 4097), (32, 32), (32, 33), (32, 1025), (32, 8192),
         (128, 128), (128, 129), (128, 1024), (128, 4097), (512, 512), (512, 513), (512, 1023), (512, 1025), (512, 8192)]


@pytest.mark.parametrize("K,n", PAIRS)
def test_select_key_patterns(pkg, reg, K, n):
    """the radix select over three digits and its tie ranks: eight key patterns, one search each, in one launch"""
    rng = np.random.default_rng(100 * K + n)
    pats = key_patterns(rng, n, K)
    searches = [Search(queue=nodes(lb, depth=d), best=1e30, coeff=0.125 * k, rot=k) for k, (lb, d) in enumerate(pats.values())]
    exp, (got, *_) = run(pkg, reg, Case(Round(thr=1.0, K=K, kmax=512, root=ROOT), searches))
    width = T.round_width(Round(K=K, kmax=512), 0, n)
    assert all(g.n_parents == min(width, n) for g in got), (width, [g.n_parents for g in got])


def test_select_stop_rule(pkg, reg):
    """selected nodes that fail the stop rule stay queued; all but the first fail; the smallest key fails (done, one pop); an empty queue (done,
    no pop); and nodes sharing the smallest truncated key of which the first misses the rule by one ulp, K = 1 (done, one pop)"""
    rng = np.random.default_rng(21)
    ulp = F(2.0 ** -22)
    def q(n, n_pass):
        lb = rng.uniform(9.5, 30, n).astype(F)
        lb[rng.permutation(n)[:n_pass]] = rng.uniform(1, 8, n_pass).astype(F)
        return nodes(lb, depth=rng.integers(5, 9, n))
    searches = [Search(queue=q(300, 20), best=10.0), Search(queue=q(2000, 20), best=10.0), Search(queue=q(300, 1), best=10.0),
                Search(queue=q(2000, 1), best=10.0), Search(queue=q(300, 0), best=10.0, pops=5), Search(queue=q(2000, 0), best=10.0, pops=5),
                Search(queue=np.zeros((0, 6), F), best=10.0, pops=5)]
    exp, (got, *_) = run(pkg, reg, Case(Round(thr=1.0, K=32, root=ROOT), searches))
    assert [g.n_parents for g in got] == [20, 20, 1, 1, 0, 0, 0] and [g.done for g in got] == [0, 0, 0, 0, 1, 1, 1]
    assert [g.pops for g in got] == [0, 0, 0, 0, 6, 6, 5] and [g.count for g in got] == [280, 1980, 299, 1999, 300, 2000, 0]
    a, b = F(2) + ulp, F(2)                                           # best 3, thr 1: 3 - a = 1 - ulp < 1 fails, 3 - b = 1 passes; one key
    assert F(3) - a < F(1) and not F(3) - b < F(1) and T.lb_keys(Round(root=ROOT), nodes([a, b]))[0] == T.lb_keys(Round(root=ROOT), nodes([a, b]))[1]
    # K = 1 and the first of the two fails: done whichever of them the kernel asks (asked b, it selects a, which fails the rule per node).  With the
    # order reversed, or K = 2, the outcome depends on the one asked -- a fixed choice of the kernel's reduction, not the first in queue order
    # (here it asks the later one and stops a search whose first node passes by that one ulp): outside the model, not asserted
    searches = [Search(queue=nodes([5, a, b, 7]), best=3.0, pops=1), Search(queue=nodes([5, 7, 9, a, 6, b]), best=3.0, pops=1),
                Search(queue=nodes([5, a, a, b]), best=3.0, pops=1)]
    exp, (got, *_) = run(pkg, reg, Case(Round(thr=1.0, K=1, root=ROOT), searches))
    assert [(g.done, g.pops, g.count, g.n_parents) for g in got] == [(1, 2, 4, 0), (1, 2, 6, 0), (1, 2, 4, 0)]
    assert T.one_round(Search(queue=nodes([5, b, a, 7]), best=3.0), Round(thr=1.0, K=1, root=ROOT)).ambiguous
    assert T.one_round(Search(queue=nodes([5, a, b, 7]), best=3.0), Round(thr=1.0, K=2, root=ROOT)).ambiguous


# ---- width -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmax", [128, 512])
@pytest.mark.parametrize("K", [32, 128, 512])
@pytest.mark.parametrize("widen", [0, 1, 2, 3])
def test_round_width(pkg, reg, widen, K, kmax):
    """K from qp.K, stale_widen and the search's stale, clamped by kmax and -- above 128 -- by the slab's room (cap - n) / 8, never below 128.
    cap 2 048: room 243 (n 100), 218 (n 300), 200 (n 448), 106 (n 1 200).  The last two searches get their stale from a digest."""
    rng = np.random.default_rng(widen * 100 + K + kmax)
    shapes = [(0, 100), (1, 100), (2, 300), (3, 300), (5, 300), (1, 1200), (3, 1200), (5, 448)]
    searches = [Search(queue=nodes(F(1) + rng.permutation(n).astype(F) * F(2.0 ** -13)), best=1e30, stale=st) for st, n in shapes]
    rp = Round(thr=1.0, K=K, kmax=kmax, cap=2048, root=ROOT, stale_widen=widen)
    exp, (got, *_) = run(pkg, reg, Case(rp, searches))
    assert [g.n_parents for g in got] == [min(T.round_width(rp, st, n), n) for st, n in shapes]
    assert [g.stale for g in got] == [st for st, _ in shapes]
    # stale 2 -> 3 by a digest that does not improve, and 2 -> 0 by one that does: the width follows the new value
    s2 = [Search(queue=nodes(F(1) + rng.permutation(300).astype(F) * F(2.0 ** -13)), best=50.0, stale=2) for _ in range(2)]
    ub = np.full(8, 60, F)
    lb = np.full(8, 20, F)
    ub2 = ub.copy()
    ub2[6] = 40
    exp, (got, *_) = run(pkg, reg, Case(rp, s2, [(parents(1), ub, lb), (parents(1), ub2, lb)]))
    assert [g.stale for g in got] == [3, 0] and [g.n_parents for g in got] == [min(T.round_width(rp, 3, 308), 308), min(T.round_width(rp, 0, 308), 308)]


# ---- compact -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", [0, 200, 201])
def test_compact_selection(pkg, reg, sc):
    """Morton-order selection: on for stale >= 1 and n >= stale_compact only; nodes that fail the stop rule have the smallest Morton codes and
    take no slot; nodes deeper than 10 levels share a Morton cell and go in queue order"""
    rng = np.random.default_rng(sc)
    def q(n):
        # 12 nodes that fail the stop rule (best 10, thr 1) in the cells (0..11, 0, 0) of the 2^-10 grid: the smallest codes of all
        fail = nodes_at([[4 * k, 0, 0] for k in range(12)], rng.uniform(9.5, 20, 12), depth=11)
        # six nodes of depth 12 in the one cell (16, 0, 0): the next code
        deep = nodes_at(np.array([[0, 0, 0], [1, 0, 0], [2, 1, 0], [3, 3, 3], [0, 2, 1], [1, 1, 1]]) + [64, 0, 0], rng.uniform(1, 8, 6), depth=12)
        # the rest on depth-5 cells with y >= 2: larger codes
        c = rng.permutation(4000)[:n - 18] + 64
        rest = nodes_at(np.stack([c & 31, (c >> 5) & 31, c >> 10], 1) * 128, rng.uniform(1, 8, n - 18), depth=rng.integers(5, 9, n - 18))
        return np.concatenate([fail, deep, rest])[rng.permutation(n)]
    searches = [Search(queue=q(200), best=10.0, stale=0), Search(queue=q(200), best=10.0, stale=1), Search(queue=q(1500), best=10.0, stale=1),
                Search(queue=q(200), best=10.0, stale=3)]
    rp = Round(thr=1.0, K=16, root=ROOT, stale_compact=sc)
    exp, (got, *_) = run(pkg, reg, Case(rp, searches))
    assert all(g.n_parents == 16 for g in got)
    if sc == 200:                                                      # Morton order and lb order pick different nodes
        by_lb = T.one_round(searches[1], Round(thr=1.0, K=16, root=ROOT))
        assert by_lb.listed.tobytes() != exp[1].listed.tobytes()


# ---- removal -----------------------------------------------------------------------------------------------------------------------
def removal_queue(n, picked):
    lb = np.full(n, 50, F) + np.arange(n).astype(F) * F(2.0 ** -8)
    lb[picked] = F(1) + np.arange(len(picked)).astype(F) * F(2.0 ** -8)
    return nodes(lb)


def test_removal_patterns(pkg, reg):
    """the selected nodes all in the tail, all at the head, every second node, one block across m = n - n_sel"""
    k = 128
    for n in (600, 1100, 3000):                                       # the one-slot form, the eight-slot form with two and with three slots in use
        pats = [np.arange(n - k, n), np.arange(k), np.arange(0, 2 * k, 2), np.arange(n - k - 40, n - 40), np.arange(n - 2 * k, n, 2),
                np.arange(n - k - 127, n - 127), np.arange(n - k - 1, n - 1), np.concatenate([np.arange(k // 2), np.arange(n - k // 2, n)])]
        searches = [Search(queue=removal_queue(n, p), best=1e30) for p in pats]
        exp, (got, *_) = run(pkg, reg, Case(Round(thr=1.0, K=k, root=ROOT), searches))
        assert all(g.n_parents == k and g.count == n - k for g in got)


@pytest.mark.parametrize("n,k", [(513, 512), (1024, 512), (4096, 512), (8192, 128)])
def test_removal_of_the_most(pkg, reg, n, k):
    """512 holes (the most a round can make; 128 at a full slab, whose room throttles the round)"""
    rng = np.random.default_rng(n)
    b0 = max(0, n - k - k // 2)
    pats = [np.sort(rng.permutation(n)[:k]), np.arange(n - k, n), np.arange(k), np.arange(b0, b0 + k)]
    searches = [Search(queue=removal_queue(n, p), best=1e30) for p in pats]
    exp, (got, *_) = run(pkg, reg, Case(Round(thr=1.0, K=512, kmax=512, root=ROOT), searches))
    assert all(g.n_parents == k and g.count == n - k for g in got)


# ---- launch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("with_ps", [True, False])
def test_launch_of_eight_searches(pkg, reg, parity, with_ps):
    """eight searches of different sizes in one launch, one of them already done (it comes back untouched), with and without a parent_search
    array, both parities; the other parity's counters were left non-zero and are zeroed"""
    rng = np.random.default_rng(parity)
    sizes = [5, 700, 1500, 64, 0, 3000, 33, 1024]
    searches = [Search(queue=nodes(F(1) + rng.permutation(n).astype(F) * F(2.0 ** -13), depth=rng.integers(5, 9, n)), best=1e30, coeff=0.1 * s, rot=10 + s,
                       twin=s ^ 1) for s, n in enumerate(sizes)]
    searches[3].done, searches[3].stale, searches[3].parent_off = 1, 4, 9
    ctl0 = [0, 0, 0, 0, 0, 3]
    ctl0[parity ^ 1], ctl0[2 + (parity ^ 1)] = 77, 5
    exp, (got, _, _, ctl) = run(pkg, reg, Case(Round(thr=1.0, K=32, root=ROOT), searches, parity=parity, ctl0=ctl0, with_ps=with_ps))
    assert ctl[parity] == 5 + 32 * 5 and ctl[2 + parity] == 6 and got[3].count == 64 and got[3].done == 1 and got[4].done == 1


def test_tile_spread_decision(pkg, reg):
    """QSearch::deep and QCtl::tile_hint on either side of tile_spread: the extent of the selected corners plus the widest selected cube"""
    def q(extent_cells, depth):
        # two selected nodes extent_cells depth-5 cells apart along y, and unselected ones far away
        lb = np.array([1, 60, 2, 70, 80], F)
        qn = nodes(lb, depth=depth)
        qn[2, :3] = qn[0, :3] + np.array([0, extent_cells / 32, 0], F)
        qn[1, :3] += F(0.25)
        return qn
    spread = 3 / 32 + 2.0 ** -6                                      # extent 3 cells + width 2^-6
    searches = [Search(queue=q(3, 6), best=1e30, deep=1), Search(queue=q(3, 5), best=1e30, deep=1), Search(queue=q(4, 6), best=1e30),
                Search(queue=q(2, 6), best=1e30), Search(queue=q(3, [6, 5, 7, 5, 5]), best=1e30)]
    exp, (got, _, _, ctl) = run(pkg, reg, Case(Round(thr=1.0, K=2, root=ROOT, tile_spread=spread, tile_min=1), searches, ctl0=(0, 0, 0, 0, 0, 10)))
    assert [g.deep for g in got] == [1, 0, 0, 1, 1] and ctl[5] == 13 and all(g.tile == 0 for g in got)
    exp, (got, _, _, ctl) = run(pkg, reg, Case(Round(thr=1.0, K=2, root=ROOT, tile_spread=0.0), searches, ctl0=(0, 0, 0, 0, 0, 10)))
    assert [g.deep for g in got] == [0] * 5 and ctl[5] == 10


# ---- the hook itself ---------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, reg):
    """arguments outside the documented ranges: GOICP_ERR_INVALID, no launch"""
    def call(case):
        out = launch(pkg, reg, case, 0)
        return out if isinstance(out, int) else 0
    ok = Case(Round(thr=1.0, K=2, root=ROOT), [Search(queue=nodes([1, 2, 3]), best=100.0)])
    assert call(ok) == 0
    for bad in (dict(K=0), dict(K=513), dict(cap=8193), dict(cap=0), dict(cap=2), dict(kmax=0), dict(list_cap=0), dict(stale_widen=4), dict(stale_compact=-1),
                dict(depth=-1), dict(root=(0, 0, 0, 0.0))):
        rp = Round(**{**dict(thr=1.0, K=2, root=ROOT), **bad})
        assert call(Case(rp, [Search(queue=nodes([1, 2, 3]), best=100.0)])) == INVALID, bad
    p = (parents(4), np.zeros(32, F), np.zeros(32, F))
    c = Case(Round(thr=1.0, K=2, list_cap=5, root=ROOT), [Search(queue=nodes([1]), best=100.0)], [p])      # 1 + 4 + 1 records > list_cap
    assert c.n_prev_list == 6 and call(c) == INVALID
    for n_parents, parent_off in ((4, 0), (1, 1), (1, -1), (513, 0)):   # the search's range leaves the previous list of one record
        c = Case(Round(thr=1.0, K=2, root=ROOT), [Search(queue=nodes([1]), best=100.0)])
        c.searches[0].n_parents, c.searches[0].parent_off = n_parents, parent_off
        assert c.n_prev_list == 1 and call(c) == INVALID
    for field, v in (("tile", 1), ("done", 3), ("stale", -1)):
        S = Search(queue=nodes([1]), best=100.0)
        setattr(S, field, v)
        assert call(Case(Round(thr=1.0, K=2, root=ROOT), [S])) == INVALID, field
    assert call(Case(Round(thr=1.0, K=2, root=ROOT), [Search(queue=nodes([1]), best=100.0)], chunks=0)) == INVALID
    assert call(Case(Round(thr=1.0, K=2, root=ROOT), [Search(queue=nodes([1]), best=100.0)], parity=2)) == INVALID
    assert call(Case(Round(thr=1.0, K=2, root=ROOT), [Search(queue=nodes([1]), best=100.0) for _ in range(9)])) == INVALID
    assert call(Case(Round(thr=1.0, K=2, list_cap=8, root=ROOT), [Search(queue=nodes([1]), best=100.0)], ctl0=(9, 0, 0, 0, 0, 0))) == INVALID


def test_hook_leaves_the_handle_alone(pkg):
    """a tiny registration after several hook calls on its handle gives the bytes a fresh handle gives"""
    from test_gpu_search_paths import fingerprint
    tgt, src = tiny_problem(1)
    prints = []
    for calls in (0, 3):
        e = pkg.FastGoICP(tgt, src, 5e-3)
        try:
            rng = np.random.default_rng(1)
            for k in range(calls):
                S = Search(queue=nodes(rng.uniform(1, 50, 2000).astype(F)), best=100.0, stale=k)
                p = (parents(200), *int_bounds(rng, 1600))
                out = launch(pkg, e.registration, Case(Round(thr=1.0, K=128, root=ROOT, stale_widen=1), [S, Search(queue=nodes([1, 2]), best=9.0)], [p, None],
                                                       chunks=1 + k, parity=k & 1), k & 1)
                assert not isinstance(out, int)
            e.run()
            assert e.finished
            prints.append(fingerprint(e))
        finally:
            e.registration.close()
    assert prints[0] == prints[1]
