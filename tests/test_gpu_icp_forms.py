"""The forms of the plain point-to-point ICP iteration that launch_icp_iteration can take besides the default one, each with and without the
neighbour cache.  test_gpu_small_shapes holds the default (`acc`: dt_layout 1, icp_fused 0, fixed-point sums); here:
  rows    dt_layout 0              icp_pass_kernel<K,0,false,CACHE> (float partial rows, `wv*4+row` addressing at every N) + icp_finalize_update,
                                   above 4 096 workgroups also icp_partials_reduce
  fused1  icp_fused 1              icp_pass_kernel<K,1,true,CACHE,2>: write-through rows, a ticket, the last workgroup runs the finalize
  fused0  icp_fused 1, dt_layout 0 the same on the linear grid
What is held to what:
  1  test_plain_pass_forms         every (form, cache) cell, N ragged around the wavefront / workgroup sizes, check_plain of test_gpu_small_shapes:
                                   nn_query == oracle.nn_brute bit for bit, first-pass error against the float64 sum (ERR_REL), one iteration against the
                                   float64 Kabsch step (TOL_ICP, the Kabsch condition asserted).  Cached cells twice on one handle; between the two a
                                   repeated pass at the pose must answer at least half its queries from the cache and none that the host cannot
                                   prove (goicp_debug_cache_hits), asserted
  2  test_hierarchy_depth_forms    the same for K = 1, 2, 3 box levels (M = 16, 1 025, 65 537)
  3  test_finalize_row_counts      the same at 4 096 rows (single-level finalize), 4 097 (two-level, a last reduce block of one row) and 4 098 rows
  4  test_cache_is_exact[_with_ties], test_layout_does_not_matter, test_fused_equals_standalone, test_converged_against_default
                                   whole runs (two start poses, max_iter 1, 2, 7, 10 000): cache on == cache off in the bytes of R, t, err and the
                                   iteration count within every form, also on a target with 500 duplicated points; fused0 == fused1; fused0 == rows,
                                   also at 65 536 points (4 096 rows); at 4 097 rows test_fused_against_two_level_standalone: within TOL_ICP;
                                   rows, fused1, fused0 converged against acc at test_gpu_parity's converged bars (error 1e-3 rel, R and t 2e-4)
  5  test_ticket_and_drained_launches   three runs back to back on one fused handle, each == the same run on a fresh handle
  6  test_cache_in_the_tail        icp_nn_cache = 2 == icp_nn_cache = 0 in bytes over 96 unstoppable iterations, with the proof, replayed on the host from
                                   the cache-off run's chunk errors, that Engine::icp_run switched the cache on early enough for the cached kernel to run
  7  test_plane_on_the_linear_grid check_plane (point-to-plane against the float64 Gauss-Newton twin, PLANE_COND asserted) on dt_layout 0

Fused against stand-alone (4).  The fused kernel sums the rows with finalize_reduce<256>, the stand-alone finalize with finalize_reduce<1024>: a
thread adds rows r, r + T/4, ... in double, so the two do NOT add in the same order.  A double sum of n floats is exact -- hence order-free --
while the terms' exponents span at most 29 - log2(n) bits, and the finalize rounds sums and H to float again; above 4 096 workgroups the
stand-alone form also rounds 1 024-row subtotals to float, which the fused form never does.  So equality is an observation, not a property of
the code; the sources and DESIGN 3 now say so.  Observed on MI355X (test_fused_equals_standalone): fused0 and rows agree in every byte of all
32 runs compared -- N = 257, 1 025, 4 099 and 65 536, i.e. 17, 65, 257 and 4 096 rows; two poses; max_iter 1, 2, 7, 10 000; the converged runs
take 20 .. 125 iterations.  Row counts between 257 and 4 096 were not compared.  At 65 537 points (4 097 rows, the two-level sum) the bytes DO
differ after one iteration -- |dR| 1.5e-8, |dt| 1.5e-8, err rel 9.8e-8 -- and test_fused_against_two_level_standalone holds the two forms to
each other at TOL_ICP / ERR_REL there.

Measured on MI355X, the worst deviation over every case of a test (every test prints its own):
                                      err rel (ERR_REL 5e-6)   |dR| (TOL_ICP 1e-6)   |dt| (TOL_ICP 1e-6)
  acc (test_gpu_small_shapes)         8.1e-8                   8.4e-8                2.6e-8
  1  rows, fused1, fused0             1.0e-7                   8.2e-8                5.0e-8     (cache 0 and 1, first and cached second pass: the same figures)
  2  rows, fused1, fused0             3.8e-8                   4.2e-8                1.9e-8
  3  rows / fused1                    5.0e-8 / 4.8e-8          6.6e-8                2.3e-8
  1  cache hits of the repeated pass: all N queries at every N but 1 025 (1 022; the host finds all 1 025 provable: the walk's best2 is a lower bound)
  4  cache, ties, layout, fused / stand-alone: 0 runs of 8 differ, every N and form; queries on duplicated target points at the start pose are
     asserted (>= N / 8); converged against acc: err rel <= 4.9e-7, |dR| <= 2.4e-7,
     |dt| <= 6.0e-8, the same iteration counts
  6  the rule fires at chunk 2 in all six cases (the cache runs from iteration 49 of 96)
  7  point-to-plane on the linear grid: |dR| <= 1.2e-6, |dt| <= 2.6e-7 (PLANE_POSE 1e-5), error against the plain pass's <= 1.6e-7 (PLANE_ERR_REL 1e-6;
     not 0 as on the bricked grid: the plain pass here adds float rows, the plane pass fixed point)

Teeth (done once on scratch copies of device.hip, on MI355X, one run of this file per mutant; every mutant reads valid memory only and terminates):
  (the file had 156 tests then; test_fused_equals_standalone[65536] and test_fused_against_two_level_standalone came later and saw no mutant)
  A  the fused finalize sums gridDim.x - 1 rows:                                                  76 of the 156 tests fail
  B  the stand-alone finalize behind icp_partials_reduce reads nb2 - 1 reduced rows:              2 (test_finalize_row_counts[rows-65537], [rows-65553])
  C  the cache's skip test with 0.9f in the place of 1.00001f:                                    30 (all 24 cache-on / off identities, 6 cached cells of test 1;
     test_cache_in_the_tail passes: by iteration 49 the pose no longer moves and every hit is a true one)
  D  icp_pass_body's `valid` without `i < N`, surplus rows counting the last point again:         87 (66 of test 1, all of 2, 6 of 3, 6 of 7)
Wall time on MI355X: this file 5.3 s (158 tests, the slowest 0.3 s); the suite without it 311 s.

Clouds: test_gpu_small_shapes._case (synth.make_pair(SEED, M, N, noise 0.002), far points appended unless outliers = False), dt_size 32.
"""
import contextlib
import ctypes as C
import io
import re

import numpy as np
import pytest

import twins
from conftest import load_pkg
from test_gpu_icp_gate import _run, _same
from test_gpu_scale_parity import TOL_ICP
from test_gpu_small_shapes import ERR_REL, M_ICP, _case, _frozen, _is_rotation, _reg, check_plain, check_plane

pytestmark = pytest.mark.gpu

FORMS = {"acc": dict(), "rows": dict(dt_layout=0), "fused1": dict(icp_fused=1), "fused0": dict(icp_fused=1, dt_layout=0)}
UNDER_TEST = ("rows", "fused1", "fused0")
N_FORMS = [1, 2, 3, 4, 5, 15, 16, 17, 33, 63, 64, 65, 257, 1025]
M_DEPTH = [16, 1025, 65537]
N_ROWS = [65535, 65536, 65537, 65553]
N_RUNS = [257, 1025, 4099]
N_FULL_ROWS = 65536                                      # 4 096 partial rows: the largest single-level finalize
MAX_ITERS = (1, 2, 7, 10000)
CONVERGED_ERR_REL, CONVERGED_POSE = 1e-3, 2e-4           # test_gpu_parity's bars for converged runs against the oracle
CHUNK, CACHE_REL = 16, np.float32(0.02)                  # EngineParams::icp_chunk, Engine::kIcpCacheRel


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _kw(form, cache=0):
    return dict(FORMS[form], icp_nn_cache=cache)


# ----------------------------------------------------------------------------------------------
# check_plain with its figures collected per form
# ----------------------------------------------------------------------------------------------
_WORST = {}
_FIGURES = re.compile(r"err rel (\S+), \|dR\| (\S+) \|dt\| (\S+) ")


def _plain(reg, c, tag, pose=True):
    """check_plain; what it printed is printed again, and the worst err rel, |dR|, |dt| of `tag` so far after it"""
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            check_plain(reg, c, pose=pose)
    finally:
        print(buf.getvalue(), end="")
    m = _FIGURES.search(buf.getvalue())
    assert m, buf.getvalue()
    w = _WORST.setdefault(tag, [0.0, 0.0, 0.0])
    for k, s in enumerate(m.groups()):
        v = float(s.rstrip(","))
        if np.isfinite(v):
            w[k] = max(w[k], v)
    print("worst so far, %s: err rel %.2e |dR| %.2e |dt| %.2e" % (tag, w[0], w[1], w[2]))


def _cache_hits(pkg, reg, R, t):
    hits = C.c_int64()
    fp = C.POINTER(C.c_float)
    Rf, tf = np.ascontiguousarray(R, np.float32).reshape(9), np.ascontiguousarray(t, np.float32)
    pkg.binding.check(pkg.load_library().goicp_debug_cache_hits(reg.handle, Rf.ctypes.data_as(fp), tf.ctypes.data_as(fp), C.byref(hits)))
    return int(hits.value)


def _provable_hits(c):
    """how many queries of c["q"] can pass the cache's skip test at an unchanged pose at all: d1 * 1.00001 + 1e-7 < d2 * 0.99999 with d1, d2 the
    distances to the nearest and second-nearest target point (float64), loosened by 1e-5"""
    q, m = c["q"].astype(np.float64), c["target"].astype(np.float64)
    if len(m) < 2:
        return 0
    d2 = ((q[:, None, :] - m[None, :, :]) ** 2).sum(2)
    two = np.sqrt(np.partition(d2, 1, axis=1)[:, :2])
    return int(np.sum(two[:, 0] * 1.00001 * (1 - 1e-5) < two[:, 1] * 0.99999 * (1 + 1e-5)))


def _plain_cell(pkg, c, form, cache, tag, pose=True):
    reg = _reg(pkg, c, **_kw(form, cache))
    try:
        _plain(reg, c, tag, pose=pose)
        if cache:
            # goicp_debug_cache_hits runs two frozen passes of its own at this pose and counts the hits of the second.  What it shows: this form's
            # cached kernel answers a repeated pose from its entries, and the check below starts from entries filled at this very pose (by
            # whichever pass came first -- it does not show that check_plain's own pass above wrote them).  The bars: no more hits than queries
            # whose neighbour is provably nearest on the host (the second-nearest point farther by the test's own 1.00001 / 0.99999, with 1e-5
            # either way for the float32 roots); at least half of N, because the walk's best2 is only a lower bound on the second distance (the DT
            # seed takes part as a pseudo-candidate), so no host count is a firm lower bound -- half is what "the second check runs on cached
            # answers" needs to mean something, whatever the seed
            hits = _cache_hits(pkg, reg, c["R0"], c["t0"])
            provable = _provable_hits(c)
            print("cache hits of a repeated pass: %d of %d (provable on the host: at most %d)" % (hits, c["N"], provable))
            assert 2 * hits >= c["N"] and hits <= provable, (form, c["N"], hits, provable)
            _plain(reg, c, tag, pose=pose)
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 1. every form against the plain reference, ragged N
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", N_FORMS)
@pytest.mark.parametrize("cache", [0, 1])
@pytest.mark.parametrize("form", UNDER_TEST)
def test_plain_pass_forms(pkg, form, cache, N):
    """N <= 16: one workgroup (fused: the first ticket is the last); 17: two.  The clouds are test_plain_pass_ragged's."""
    _plain_cell(pkg, _case(M_ICP, N), form, cache, "%s cache %d" % (form, cache))


# ----------------------------------------------------------------------------------------------
# 2. box-hierarchy depth, 3. the finalize's row counts
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", M_DEPTH)
@pytest.mark.parametrize("form", UNDER_TEST)
def test_hierarchy_depth_forms(pkg, form, M):
    """N = 257 against targets of one, two and three box levels (with_k's K = 1, 2, 3); sixteen target points leave the pose step ill-posed"""
    _plain_cell(pkg, _case(M, 257, outliers=False), form, 0, "%s depth" % form, pose=M >= 17)


@pytest.mark.parametrize("N", N_ROWS)
@pytest.mark.parametrize("form", ["rows", "fused1"])
def test_finalize_row_counts(pkg, form, N):
    """nb = ceil(N / 16) rows: 4 096 twice (the largest single-level finalize), 4 097 (nb2 = 5, the last reduce block one row) and 4 098 (two rows);
    the fused finalize_reduce<256> walks them in nine sweeps"""
    _plain_cell(pkg, _case(M_ICP, N, outliers=False), form, 0, "%s rows" % form)


# ----------------------------------------------------------------------------------------------
# 4. identities between forms, over whole runs
# ----------------------------------------------------------------------------------------------
def _poses(c):
    R1 = (twins.rodrigues64([0.2, -0.1, 0.15]) @ c["R0"].astype(np.float64)).astype(np.float32)     # a second, larger turn on top of the first
    t1 = (c["t0"] + np.array([0.05, 0.02, -0.03], np.float32)).astype(np.float32)
    return ((c["R0"], c["t0"]), (R1, t1))


def _ties_case(N):
    """_case(M_ICP, N) with the target's first 500 points appended again: a query next to one of them has a second neighbour at the same
    distance, its cache entry holds sqrt(best2_ref) = 0 and must walk in every pass"""
    single = _case(M_ICP, N)
    c = {k: v for k, v in single.items() if k not in ("bi", "bd2")}                # the neighbours of the single target are not this one's
    c["target"] = np.ascontiguousarray(np.concatenate([c["target"], c["target"][:500]]))
    c["M"] = len(c["target"])
    # the tied path is exercised only if queries do land on duplicated points: a quarter of the target is, so about a quarter of the
    # queries should; an eighth is asserted, at the start pose, where every run begins (oracle.nn_brute's neighbours on the single target)
    c["tied_queries"] = int(np.sum(single["bi"] < 500))
    assert c["tied_queries"] >= N // 8, (N, c["tied_queries"])
    return _frozen(c)


def _runs_case(N):
    """the clouds of the whole runs: test_plain_pass_ragged's family; at N_FULL_ROWS test_finalize_row_counts' (no far points), already built"""
    return _case(M_ICP, N, outliers=False) if N >= N_FULL_ROWS else _case(M_ICP, N)


_RUNS = {}


def _runs(pkg, N, form, cache, ties=False):
    """{(pose, max_iter): (R, t, err, iters)} of one handle, computed once"""
    key = (N, form, cache, ties)
    if key not in _RUNS:
        c = _ties_case(N) if ties else _runs_case(N)
        reg = _reg(pkg, c, **_kw(form, cache))
        try:
            out = {}
            for p, (R, t) in enumerate(_poses(c)):
                for max_iter in MAX_ITERS:
                    out[p, max_iter] = _run(reg, R, t, max_iter=max_iter, err_diff=1e-7)
                    assert _is_rotation(out[p, max_iter][0], out[p, max_iter][1]), (key, p, max_iter)
                assert out[p, 1][3] == 1 and out[p, 2][3] == 2 and 2 < out[p, 10000][3] < 10000, (key, p, [o[3] for o in out.values()])
            _RUNS[key] = out
        finally:
            reg.close()
    return _RUNS[key]


def _equal_runs(a, b, tag):
    bad = [(k, a[k][2:], b[k][2:]) for k in a if not _same(a[k], b[k])]
    worst = max(max(float(np.abs(a[k][0] - b[k][0]).max()), float(np.abs(a[k][1] - b[k][1]).max())) for k in a)
    print("%s: %d of %d runs differ in bytes, worst |dR|, |dt| %.2e; iterations to converge %s" % (tag, len(bad), len(a), worst, [a[p, 10000][3] for p in (0, 1)]))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("N", N_RUNS)
@pytest.mark.parametrize("form", list(FORMS))
def test_cache_is_exact(pkg, form, N):
    _equal_runs(_runs(pkg, N, form, 1), _runs(pkg, N, form, 0), "%s N %d cache on / off" % (form, N))


@pytest.mark.parametrize("N", N_RUNS)
@pytest.mark.parametrize("form", list(FORMS))
def test_cache_is_exact_with_ties(pkg, form, N):
    c = _ties_case(N)
    assert np.array_equal(c["target"][2000:], c["target"][:500]) and c["M"] == 2500
    _equal_runs(_runs(pkg, N, form, 1, ties=True), _runs(pkg, N, form, 0, ties=True), "%s N %d cache on / off, tied target" % (form, N))


@pytest.mark.parametrize("N", N_RUNS)
def test_layout_does_not_matter(pkg, N):
    """the walk is exact and the seed table is the same table permuted: the linear grid and the bricked one give the fused iteration the same bits"""
    _equal_runs(_runs(pkg, N, "fused0", 0), _runs(pkg, N, "fused1", 0), "N %d fused0 / fused1" % N)


@pytest.mark.parametrize("N", N_RUNS + [N_FULL_ROWS])
def test_fused_equals_standalone(pkg, N):
    """finalize_reduce<256> inside the pass against finalize_reduce<1024> behind it, on the same float rows (see the module's docstring); 65 536
    points are 4 096 rows, the most the stand-alone finalize adds in one level"""
    _equal_runs(_runs(pkg, N, "fused0", 0), _runs(pkg, N, "rows", 0), "N %d fused0 / rows" % N)


def test_fused_against_two_level_standalone(pkg):
    """4 097 rows: the stand-alone form rounds five subtotals to float (icp_partials_reduce), the fused form adds all rows in double, so bytes are
    not asked for: R and t after each of the first iterations within TOL_ICP of each other, the error within ERR_REL (the bars either form is
    held to against the float64 step; one iteration's rounding, not a trajectory's); whether the bytes agree is printed"""
    c = _case(M_ICP, 65537, outliers=False)
    outs = {}
    for form in ("fused0", "rows"):
        reg = _reg(pkg, c, **_kw(form))
        try:
            outs[form] = [_run(reg, R, t, max_iter=1, err_diff=1e-7) for R, t in _poses(c)]
        finally:
            reg.close()
    for p, (a, b) in enumerate(zip(outs["fused0"], outs["rows"])):
        dR, dt, de = float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()), abs(float(a[2]) - float(b[2])) / float(b[2])
        print("N 65537 pose %d fused0 / rows after one iteration: bytes %s, |dR| %.2e |dt| %.2e err rel %.2e" % (p, "equal" if _same(a, b) else "differ", dR, dt, de))
        assert a[3] == b[3] == 1 and dR <= TOL_ICP and dt <= TOL_ICP and de <= ERR_REL, (p, dR, dt, de)


@pytest.mark.parametrize("N", N_RUNS)
@pytest.mark.parametrize("form", UNDER_TEST)
def test_converged_against_default(pkg, form, N):
    ref, out = _runs(pkg, N, "acc", 0), _runs(pkg, N, form, 0)
    for p in (0, 1):
        (aR, at, ae, ai), (R, t, e, it) = ref[p, 10000], out[p, 10000]
        de, dR, dt = abs(float(e) - float(ae)) / float(ae), float(np.abs(R - aR).max()), float(np.abs(t - at).max())
        print("%s N %d pose %d converged against acc: err rel %.2e |dR| %.2e |dt| %.2e, iterations %d / %d" % (form, N, p, de, dR, dt, it, ai))
        assert de <= CONVERGED_ERR_REL and dR <= CONVERGED_POSE and dt <= CONVERGED_POSE, (form, N, p, de, dR, dt, it, ai)


# ----------------------------------------------------------------------------------------------
# 5. ticket and drained launches
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,N", [("fused1", 16), ("fused1", 1025), ("fused0", 1025)])
def test_ticket_and_drained_launches(pkg, form, N):
    """A converged run leaves queued launches behind that return at the flag; the runs after it must find the ticket at zero.  A ticket left
    above zero would leave them without a finalize: the start pose, unchanged, iters == 0 (max_iter = 64 bounds such a failure)."""
    c = _case(M_ICP, N)
    (Ra, ta), (Rb, tb) = _poses(c)
    plan = ((Ra, ta, 10000), (Rb, tb, 64), (Ra, ta, 64))
    reg = _reg(pkg, c, **_kw(form))
    try:
        outs = [_run(reg, R, t, max_iter=k, err_diff=1e-7) for R, t, k in plan]
    finally:
        reg.close()
    assert 0 < outs[0][3] < 10000 - 2 * CHUNK, outs[0][3]                # it converged with launches still queued
    for (R, t, k), out in zip(plan, outs):
        fresh = _reg(pkg, c, **_kw(form))
        try:
            want = _run(fresh, R, t, max_iter=k, err_diff=1e-7)
        finally:
            fresh.close()
        assert want[3] > 0 and not np.array_equal(want[0], R), (form, N, k, want[3])
        assert _same(out, want), (form, N, k, out[2:], want[2:])
    print("%s N %d: iterations %s" % (form, N, [o[3] for o in outs]))


# ----------------------------------------------------------------------------------------------
# 6. icp_nn_cache = 2: the cache switched on in the tail of a run
# ----------------------------------------------------------------------------------------------
def _tail_rule(errs):
    """Engine::icp_run's rule on the errors at the ends of the chunks 1, 2, ...: the first examined chunk j whose error fell by less than
    kIcpCacheRel of itself against chunk j - 1's (float arithmetic, as the engine's); None if there is none"""
    prev = np.float32(-1.0)
    for j, e in enumerate(errs, 1):
        e = np.float32(e)
        if prev > 0 and e > 0 and np.float32(prev - e) < np.float32(CACHE_REL * e):
            return j
        prev = e
    return None


@pytest.mark.parametrize("N", [257, 4099])
@pytest.mark.parametrize("form", ["acc", "rows", "fused1"])
def test_cache_in_the_tail(pkg, form, N):
    """err_diff = -1e30: a run never stops, so its states after 16 j iterations are those of the chunk ends of the 96-iteration run, and the
    returned error is IcpState::err.  The chunk after the examined one is already queued when the rule fires at j*: the cached kernel runs
    from iteration 16 (j* + 1) + 1 on, fills its entries there and can answer from them one iteration later."""
    c = _case(M_ICP, N)
    R0, t0 = c["R0"], c["t0"]
    off = _reg(pkg, c, **_kw(form, 0))
    try:
        ends = [_run(off, R0, t0, max_iter=CHUNK * j, err_diff=-1e30) for j in range(1, 7)]
        stopping = _run(off, R0, t0, max_iter=10000, err_diff=1e-7)
    finally:
        off.close()
    assert [o[3] for o in ends] == [CHUNK * j for j in range(1, 7)], [o[3] for o in ends]          # no run stopped early
    errs = [o[2] for o in ends]
    j = _tail_rule(errs)
    print("%s N %d: chunk-end errors %s, the rule fires at chunk %s" % (form, N, ["%.9g" % e for e in errs], j))
    assert j is not None and CHUNK * (j + 1) + 2 <= 96, (form, N, j, errs)
    tail = _reg(pkg, c, **_kw(form, 2))
    try:
        out = _run(tail, R0, t0, max_iter=96, err_diff=-1e30)
        assert _same(out, ends[5]), (form, N, out[2:], ends[5][2:])
        out = _run(tail, R0, t0, max_iter=10000, err_diff=1e-7)
        assert _same(out, stopping), (form, N, out[2:], stopping[2:])
    finally:
        tail.close()


# ----------------------------------------------------------------------------------------------
# 7. point-to-plane on the linear grid
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 15, 16, 17, 65, 257, 1025])
def test_plane_on_the_linear_grid(pkg, N):
    """icp_opt_pass_kernel<..., LAYOUT 0>: one point-to-plane iteration against the float64 twin, as test_plane_pass_ragged on the bricked grid"""
    c = _case(M_ICP, N)
    reg = _reg(pkg, c, dt_layout=0)
    try:
        check_plane(reg, c)
    finally:
        reg.close()
