"""GPU parity at production sizes: the trimmed-selection kernels (register and streaming form), the trimmed cube bounds and ICP at
full cloud size, the batch min-reduction, and the launches the headline times -- each against a plain reference of the same
operation: exact numpy answers for selections and reductions, float64 sums of the oracle's per-point terms
(oracle.cube_bound_f64) for bounds.  The oracle's own float sums in point order drift by ~6e-4 relative at 1 M points, so they
are not the reference here.

Tolerances: the kernels' per-point terms are the oracle's, so only the order of the float sums differs from the float64
reference.  Measured on MI355X, worst per group: 2.9e-7 at N <= 40 000, 5.4e-7 at N = 1 M (printed per group, quoted in each
docstring); the bars are ten times that -- rel 2e-6 and 5e-6, floor max(ref, 1e-3) -- far below what one dropped or doubled
point (1 / N) or a wrong k-th residual would cost.  Selection flags and reduce-min results are exact.
"""
import ctypes as C

import numpy as np
import pytest


pytestmark = pytest.mark.gpu

TOL = 2e-6          # N <= 40 000 (measured worst 2.9e-7)
TOL_1M = 5e-6       # N = 1 M (measured worst 5.4e-7)
TOL_ICP = 1e-6      # one trimmed ICP iteration: error rel, R and t abs (measured worst 5.5e-8)
GOICP_ERR_INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()          # fails loudly if the HIP extension is missing
    return m


@pytest.fixture(scope="module")
def s1(pkg):
    from cuda_go_icp_amd import synth
    return synth.make_pair(**{k: synth.S1[k] for k in ("seed", "M", "N")})


@pytest.fixture(scope="module")
def s1_dt(oracle_mod, s1):
    return oracle_mod.DistanceTransform(s1[0], 300, 2.0)


@pytest.fixture(scope="module")
def reg_small(pkg, bunny_model, bunny_data10):
    r = pkg.Registration(bunny_model, bunny_data10, 1e-3)
    yield r
    r.close()


class _Hip:
    """Device buffers for the device-pointer entry points, from the runtime the library itself links against."""

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
        assert self.h.hipDeviceSynchronize() == 0              # the entry points queue on the engine's stream
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


def _rel(a, ref):
    return abs(float(a) - ref) / max(ref, 1e-3)


# ----------------------------------------------------------------------------------------------
# trimmed selection: register kernel (N <= 32 768) and streaming kernel, exact flags
# ----------------------------------------------------------------------------------------------
def _select_values(kind, n, rng):
    u32 = np.uint32
    if kind == "uniform":
        return rng.random(n, dtype=np.float32)
    if kind == "three":                                      # heavy ties
        return rng.choice(np.array([0.25, 0.5, 2.0], np.float32), n)
    if kind == "equal":
        return np.full(n, 0.375, np.float32)
    if kind == "low9":                                       # top 23 bits shared: only the third digit (bits 0..8) separates
        base = np.float32(0.7).view(u32) & u32(0xfffffe00)
        return (base | rng.integers(0, 1 << 9, n).astype(u32)).view(np.float32)
    if kind == "low20":                                      # sign + first digit shared: the second and third digits separate
        base = np.float32(0.7).view(u32) & u32(0xfff00000)
        return (base | rng.integers(0, 1 << 20, n).astype(u32)).view(np.float32)
    if kind == "extremes":                                   # zeros, subnormals and values near 1e30
        sub = rng.integers(1, 1 << 23, n).astype(u32).view(np.float32)
        big = (np.float32(1e30) * (1 + rng.random(n, dtype=np.float32) * np.float32(1e-3))).astype(np.float32)
        return np.choose(rng.integers(0, 3, n), [np.zeros(n, np.float32), sub, big]).astype(np.float32)
    raise ValueError(kind)


def _select_nums(v):
    n = len(v)
    nums = {1, 2, n // 2, n - 1, n}
    s = np.sort(v)
    brk = np.flatnonzero(np.diff(s.view(np.uint32)) != 0) + 1
    starts, ends = np.concatenate([[0], brk]), np.concatenate([brk, [n]])
    j = int(np.argmax(ends - starts))
    if ends[j] - starts[j] >= 2:                             # a count that ends inside the longest run of ties
        nums.add(int(starts[j] + (ends[j] - starts[j]) // 2))
    return sorted(x for x in nums if 1 <= x <= n)


def _select(reg, d2, num, kernel):
    d2 = np.ascontiguousarray(d2, np.float32)
    inc = np.full(len(d2), 7, np.uint8)
    rc = reg._lib.goicp_debug_select(reg.handle, d2.ctypes.data_as(C.POINTER(C.c_float)), len(d2), int(num), int(kernel),
                                     inc.ctypes.data_as(C.POINTER(C.c_uint8)))
    return rc, inc


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 32767, 32768, 32769, 100003, 1000000])
def test_select_kernels_exact(pkg, reg_small, n):
    """goicp_debug_select: the `num` smallest squared distances flagged, the ties at the threshold given to the points that come first
    (the trimmed ICP's documented rule) -- exactly numpy's stable argsort prefix, for both kernels wherever the register kernel
    applies (n <= 32 768) and the streaming kernel everywhere, on uniform values, three values, one value, values that only the
    second / third radix digit separates, and zeros + subnormals + values near 1e30."""
    rng = np.random.default_rng(n)
    kernels = (1, 2) if n <= 32768 else (2,)
    cases = 0
    for kind in ("uniform", "three", "equal", "low9", "low20", "extremes"):
        v = _select_values(kind, n, rng)
        order = np.argsort(v, kind="stable")
        for num in _select_nums(v):
            want = np.zeros(n, np.uint8)
            want[order[:num]] = 1
            for k in kernels:
                rc, got = _select(reg_small, v, num, k)
                assert rc == 0, pkg.binding.load_library().goicp_last_error()
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (kind, num, k, bad[:8], got[bad[:8]], v[bad[:8]])
                cases += 1
    print("select n=%d: %d exact cases (kernels %s)" % (n, cases, kernels))


def test_select_dispatch_and_refusals(pkg, reg_small):
    """kernel 0 (the iteration's own choice) agrees with the exact answer on both sides of the 32 768 switch; the register kernel
    refuses n > 32 768, and num outside 1..n is refused, without a launch."""
    rng = np.random.default_rng(3)
    for n in (32768, 32769):
        v = rng.choice(np.array([0.5, 1.5], np.float32), n)
        order = np.argsort(v, kind="stable")
        num = int(np.count_nonzero(v == np.float32(0.5))) + 17
        want = np.zeros(n, np.uint8)
        want[order[:num]] = 1
        rc, got = _select(reg_small, v, num, 0)
        assert rc == 0 and np.array_equal(got, want), n
    v = rng.random(32769, dtype=np.float32)
    for num, k in ((5, 1), (0, 2), (32770, 2), (5, 3)):
        rc, got = _select(reg_small, v, num, k)
        assert rc == GOICP_ERR_INVALID and (got == 7).all(), (num, k)


# ----------------------------------------------------------------------------------------------
# goicp_reduce_min_device: exact (min, first argmin)
# ----------------------------------------------------------------------------------------------
def _reduce(reg, hip, v, with_idx=True):
    lib, h = reg._lib, reg.handle
    d_v = hip.upload(np.ascontiguousarray(v, np.float32))
    d_min, d_idx = hip.upload(np.full(1, np.nan, np.float32)), hip.upload(np.full(1, -7, np.int32))
    rc = lib.goicp_reduce_min_device(h, d_v, len(v), d_min, d_idx if with_idx else None, None)
    assert rc == 0, lib.goicp_last_error()
    out = hip.download(d_min, 1, np.float32)[0], int(hip.download(d_idx, 1, np.int32)[0])
    hip.free_all()
    return out


def _reduce_cases(n, rng):
    base = rng.uniform(1.0, 2.0, n).astype(np.float32)
    lo = np.float32(0.25)
    cases = {}

    def at(name, pos, vals=None):
        v = (base if vals is None else vals).copy()
        v[np.asarray(pos, dtype=np.int64)] = lo
        cases[name] = v

    at("first", [0])
    at("last", [n - 1])
    if n % 4:
        at("scalar_tail", [n // 4 * 4 + (n % 4) // 2])
    last_thread = ((n - 4093) // 4096) * 4096 + 4092 if n > 4092 else (n - 1) // 4 * 4    # thread 1023's (or the last active thread's) last float4
    at("last_thread", [min(last_thread + 1, n - 1)])
    at("repeated", sorted(set(rng.choice(n, min(n, 5), replace=False).tolist())))
    at("repeated_across_threads", sorted({p for p in (3, 4, 4096 + 1, n // 2, n - 1) if p < n}))
    at("repeated_in_float4", sorted({p for p in (n // 8 * 4 + 2, n // 8 * 4 + 3, n - 1) if p < n}))
    infs = base.copy()
    infs[rng.random(n) < 0.3] = np.inf
    at("inf_mixed", [n // 3], infs)
    one = np.full(n, np.inf, np.float32)
    at("inf_but_one", [(2 * n) // 3], one)
    cases["all_inf"] = np.full(n, np.inf, np.float32)
    for name, (a, b) in (("minus_zero_first", (np.float32(-0.0), np.float32(0.0))), ("plus_zero_first", (np.float32(0.0), np.float32(-0.0)))):
        v = base.copy()
        i, j = (n - 1) // 3, n - 1
        v[j] = b
        v[i] = a                                             # i <= j: at n = 1 only the first value stays
        cases[name] = v
    return cases


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 4095, 4096, 4097, 65536, 65537, (1 << 20) + 3])
def test_reduce_min_exact(pkg, reg_small, hip, n):
    """(min, first index attaining it) -- numpy's (v.min(), argmin(v)) -- with the minimum first, last, in the scalar tail, in the
    last thread's slice, repeated (the first copy wins, inside one float4 and across threads), among +inf, as -0.0 beside +0.0
    (equal values: the first index), and for an all-+inf input, which must give (inf, 0)."""
    rng = np.random.default_rng(n + 11)
    for name, v in _reduce_cases(n, rng).items():
        m, i = _reduce(reg_small, hip, v)
        assert m == v.min() and i == int(np.argmin(v)), (name, m, i, v.min(), int(np.argmin(v)))
        if name == "all_inf":
            assert m == np.inf and i == 0
    m, _ = _reduce(reg_small, hip, _reduce_cases(n, rng)["last"], with_idx=False)       # d_argmin = NULL: the minimum alone
    assert m == np.float32(0.25)


def test_reduce_min_refusals(pkg, reg_small, hip):
    """n = 0 and a value pointer that is not 16-byte aligned are refused, without a launch."""
    lib, h = reg_small._lib, reg_small.handle
    d_v = hip.upload(np.arange(64, dtype=np.float32))
    d_min, d_idx = hip.upload(np.full(1, -3.0, np.float32)), hip.upload(np.full(1, -7, np.int32))
    assert lib.goicp_reduce_min_device(h, d_v, 0, d_min, d_idx, None) == GOICP_ERR_INVALID
    assert lib.goicp_reduce_min_device(h, C.c_void_p(d_v.value + 4), 16, d_min, d_idx, None) == GOICP_ERR_INVALID
    assert hip.download(d_min, 1, np.float32)[0] == np.float32(-3.0) and hip.download(d_idx, 1, np.int32)[0] == -7
    hip.free_all()


# ----------------------------------------------------------------------------------------------
# trimmed bounds at full size against the float64 reference
# ----------------------------------------------------------------------------------------------
def _sibling_cubes(rng, n_parents, pw):
    """n_parents expansions x 8 children (centre xyz + child width), children in the engine's order: the sibling path."""
    pw = np.float32(pw)
    w = pw / np.float32(2)
    corner = rng.uniform(-0.45, 0.45 - float(pw), (n_parents, 3)).astype(np.float32)
    j = np.arange(8)
    off = np.stack([(j & 1), (j >> 1) & 1, (j >> 2) & 1], 1).astype(np.float32)
    cx = (corner[:, None, :] + off[None, :, :] * w + w / np.float32(2)).astype(np.float32)
    return np.concatenate([cx.reshape(-1, 3), np.full((8 * n_parents, 1), w, np.float32)], 1)


def _trim_reg(pkg, target, source, k, **kw):
    """A trimmed engine whose inlier count is exactly k (the engine derives it from trim_fraction in float)."""
    n = len(source)
    for tf in (1.0 - (k + 0.5) / n, 1.0 - (k + 0.25) / n, 1.0 - (k + 0.75) / n):
        r = pkg.Registration(target, source, 1e-3, trim_fraction=float(np.float32(tf)), **kw)
        if r.inliers == k:
            return r
        r.close()
    raise AssertionError("no trim_fraction gives %d inliers of %d" % (k, n))


def _check_trimmed_bounds(pkg, O, dt, target, source, ks, tag, levels=(-1, 5), n_parents=2, tol=TOL, ragged=13, **kw):
    """eval_bounds (sibling path: 8 children of one expansion per workgroup) at each level and eval_bounds_batch (three rotations
    and both passes inside every group of eight, a ragged batch: the generic per-cube path) against cube_bound_f64(inliers=k)."""
    rng = np.random.default_rng(len(source))
    _, rho = O.rot_radii(source)
    rots = [pkg.fgoicp.rodrigues(v) for v in ([0.3, -0.2, 0.9], [-1.1, 0.4, 0.2], [0.05, 1.7, -0.6])]
    prots = [O.rotate(R, source) for R in rots]
    worst, ties = 0.0, 0
    for k in ks:
        reg = _trim_reg(pkg, target, source, k, **kw)
        for level in levels:
            assert level < 0 or reg.rot_coeff(level) == O.rot_coeff(level)
            cubes = _sibling_cubes(rng, n_parents, 1.0 / 8)
            ub, lb = reg.eval_bounds(rots[0], cubes, level)
            for i, c in enumerate(cubes):
                fu, fl = O.cube_bound_f64(dt, prots[0], rho[level] if level >= 0 else None, c[:3], c[3], inliers=k)
                d = max(_rel(ub[i], fu), _rel(lb[i], fl))
                worst = max(worst, d)
                assert d <= tol and lb[i] <= ub[i], (tag, "sibling", k, level, i, ub[i], fu, lb[i], fl)
                m = O.cube_terms(dt, prots[0], rho[level] if level >= 0 else None, c[:3], c[3])
                ties = max(ties, int(np.count_nonzero(m == np.partition(m, k - 1)[k - 1])))
        lv = max(levels)
        coeff = reg.rot_coeff(lv)
        cen = rng.uniform(-0.4, 0.4, (ragged, 3)).astype(np.float32)
        w = np.float32(1.0 / 16)
        delta = np.float32(reg._lib.goicp_trans_delta(float(w)))
        recs = [(cen[i, 0], cen[i, 1], cen[i, 2], delta, coeff if i % 2 else 0.0, i % 3) for i in range(ragged)]
        ub, lb = reg.eval_bounds_batch(np.stack(rots), recs)
        for i, r in enumerate(recs):
            fu, fl = O.cube_bound_f64(dt, prots[r[5]], rho[lv] if i % 2 else None, r[:3], w, inliers=k)
            d = max(_rel(ub[i], fu), _rel(lb[i], fl))
            worst = max(worst, d)
            assert d <= tol and lb[i] <= ub[i], (tag, "generic", k, i, ub[i], fu, lb[i], fl)
        reg.close()
    print("trimmed bounds %s (N = %d, inliers %s): worst rel deviation %.2e, most residuals tied at the k-th: %d" % (tag, len(source), ks, worst, ties))
    return worst, ties


def _inlier_counts(n, odd=False):
    ks = [1, n // 2, int(0.9 * n), n - 1]
    return [k + 1 if odd and k % 2 == 0 else k for k in ks]


def test_trimmed_bounds_bunny_full(pkg, oracle_mod, oracle_dt_bunny, bunny_model, bunny_data):
    """Full bunny (N = 30 379), inliers 1, N/2, 0.9 N, N - 1.  Measured worst rel deviation 2.1e-7."""
    _check_trimmed_bounds(pkg, oracle_mod, oracle_dt_bunny, bunny_model, bunny_data, _inlier_counts(len(bunny_data)), "bunny")


def test_trimmed_bounds_s1(pkg, oracle_mod, s1, s1_dt):
    """S1 (N = 40 000: the cloud size where trimmed ICP switches to the streaming selection kernel).  Measured worst 2.4e-7."""
    _check_trimmed_bounds(pkg, oracle_mod, s1_dt, s1[0], s1[1], _inlier_counts(len(s1[1])), "S1")


def test_trimmed_bounds_duplicated(pkg, oracle_mod, s1, s1_dt):
    """Every point twice (S1's first 20 000 points, N = 40 000) and odd inlier counts: the k-th smallest residual is tied with its
    twin, so the copies of the threshold that enter the sums (sel_rem) decide the bound.  Measured worst 2.3e-7."""
    src = np.concatenate([s1[1][:20000], s1[1][:20000]])
    _, ties = _check_trimmed_bounds(pkg, oracle_mod, s1_dt, s1[0], src, _inlier_counts(len(src), odd=True), "duplicated")
    assert ties >= 2


@pytest.fixture(scope="module")
def s2(pkg, oracle_mod):
    from cuda_go_icp_amd import synth
    model, data, _, _ = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"])
    return model, data, oracle_mod.DistanceTransform(model, synth.S2["V"], 2.0), synth.S2["V"]


def test_trimmed_bounds_s2(pkg, oracle_mod, s2):
    """S2 (N = 1 M, DT 512^3), half the points as inliers, one expansion (8 cubes) per pass, the lower-bound pass at rotation level 1:
    most residuals clamp to 0, so the threshold is 0 and far more than 2^16 copies of it are counted (sel_rem > 65 536).
    Measured worst 5.4e-7."""
    model, data, dt, V = s2
    n = len(data)
    _, ties = _check_trimmed_bounds(pkg, oracle_mod, dt, model, data, [n // 2], "S2", levels=(-1, 1), n_parents=1, tol=TOL_1M,
                                    ragged=5, dt_size=V)
    assert ties > (1 << 16)


def test_trimmed_sse(pkg, oracle_mod, s1, s1_dt):
    """Trimmed compute_sse_error on S1 and on the duplicated cloud: the float64 sum of the k smallest squared DT distances.
    Measured worst 1.3e-7."""
    target, source, Rgt, tgt = s1
    R = (pkg.fgoicp.rodrigues([0.02, -0.03, 0.01]) @ Rgt).astype(np.float32)
    t = (tgt + np.array([0.01, -0.02, 0.015])).astype(np.float32)
    worst = 0.0
    for tag, src, odd in (("S1", source, False), ("duplicated", np.concatenate([source[:20000], source[:20000]]), True)):
        m = oracle_mod.cube_terms(s1_dt, oracle_mod.rotate(R, src), None, t, 0.0).astype(np.float64)
        for k in _inlier_counts(len(src), odd):
            reg = _trim_reg(pkg, target, src, k)
            got = reg.compute_sse_error(R, t)
            ref = float(np.sum(np.partition(m, k - 1)[:k] ** 2))
            worst = max(worst, _rel(got, ref))
            assert _rel(got, ref) <= TOL, (tag, k, got, ref)
            reg.close()
    print("trimmed sse: worst rel deviation %.2e" % worst)


# ----------------------------------------------------------------------------------------------
# trimmed ICP: one iteration against float64, ten against the oracle
# ----------------------------------------------------------------------------------------------
def _icp_one_f64(target, q, nn_idx, nn_d2, num, R0, t0):
    """One trimmed ICP iteration in float64 from correspondences (q = the moved source, float32 as the kernel forms it): the num
    nearest (stable order: ties in point order), means, H, SVD Kabsch with the reference's reflection handling (diag(1, 1, det)
    on the smallest singular direction), then the composed pose.  -> (error at the start pose, R, t)."""
    sel = np.argsort(nn_d2, kind="stable")[:num]
    pd, pm = q[sel].astype(np.float64), target[nn_idx[sel]].astype(np.float64)
    mu_d, mu_m = pd.mean(0), pm.mean(0)
    H = (pd - mu_d).T @ (pm - mu_m)
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    d = np.linalg.det(V @ U.T)
    Rs = V @ np.diag([1.0, 1.0, d]) @ U.T
    ts = mu_m - Rs @ mu_d
    return float(np.sum(nn_d2[sel].astype(np.float64))), Rs @ np.asarray(R0, np.float64), Rs @ np.asarray(t0, np.float64) + ts


def test_trimmed_icp_scale(pkg, oracle_mod, s1):
    """Trimmed ICP (trim_fraction 0.1) on S1's source cut to 32 768 points (register selection kernel) and 32 769 (streaming kernel),
    on all 40 000, and on the duplicated cloud (odd inlier count: the threshold is tied with its twin).  One iteration from a fixed
    pose against the float64 iteration on oracle.nn_brute's correspondences; ten iterations against the oracle's own trimmed ICP at
    test_trimmed_icp_vs_oracle's bars.  Measured worst of the single iteration: error rel 2.5e-8, R 5.5e-8, t 4.7e-9."""
    target, source, Rgt, tgt = s1
    R0 = (pkg.fgoicp.rodrigues([0.02, -0.03, 0.01]) @ Rgt).astype(np.float32)
    t0 = (tgt + np.array([0.01, -0.02, 0.015])).astype(np.float32)
    x, y, z = source[:, 0], source[:, 1], source[:, 2]
    q = np.stack([R0[i, 0] * x + R0[i, 1] * y + R0[i, 2] * z + t0[i] for i in range(3)], 1).astype(np.float32)
    idx, d2 = oracle_mod.nn_brute(target, q)
    kd = oracle_mod.KdTree(target)
    dup = np.concatenate([np.arange(20000), np.arange(20000)])
    worst = [0.0, 0.0, 0.0]
    for tag, sel, k in (("32768", np.arange(32768), None), ("32769", np.arange(32769), None), ("40000", np.arange(40000), None),
                        ("duplicated", dup, 36001)):
        src = np.ascontiguousarray(source[sel])
        reg = _trim_reg(pkg, target, src, k) if k else pkg.Registration(target, src, 1e-3, trim_fraction=0.1)
        num = reg.inliers
        err, R, t = pkg.IterativeClosestPoint3D(reg, 1, 1e-9, R=R0, t=t0).run()
        ferr, fR, ft = _icp_one_f64(target, q[sel], idx[sel], d2[sel], num, R0, t0)
        dev = (_rel(err, ferr), float(np.abs(R - fR).max()), float(np.abs(t - ft).max()))
        worst = [max(a, b) for a, b in zip(worst, dev)]
        print("trimmed icp %s (num %d): one iteration, err rel %.2e, R %.2e, t %.2e" % (tag, num, *dev))
        assert dev[0] <= TOL_ICP and dev[1] <= TOL_ICP and dev[2] <= TOL_ICP, (tag, dev)
        err, R, t = pkg.IterativeClosestPoint3D(reg, 10, 1e-9, R=R0, t=t0).run()
        oerr, oR, ot, _ = kd.icp_run_trim(src, num, R0, t0, 10, 1e-9)
        assert abs(err - oerr) <= 1e-3 * oerr and np.abs(R - oR).max() <= 2e-4 and np.abs(t - ot).max() <= 2e-4, tag
        reg.close()
    print("trimmed icp, one iteration: worst err rel %.2e, R %.2e, t %.2e" % tuple(worst))


# ----------------------------------------------------------------------------------------------
# the launches the headline times
# ----------------------------------------------------------------------------------------------
def _bench():
    import bench
    return bench


def _headline_reg(pkg, model, data, **kw):
    """The engine exactly as bench.py builds it (DT 300^3, bricked layout, k-d source order)."""
    return pkg.Registration(model, data, 1e-3, dt_size=kw.pop("dt_size", 300), dt_layout=1, morton_sort=2, **kw)


def _record_refs(O, dt, data, rots, recs, idx, reg):
    """cube_bound_f64 of the records idx: rotation rots[rot], child width from delta, rotation level from coeff (0: no radii)."""
    _, rho = O.rot_radii(data)
    coeff = {float(reg.rot_coeff(l)): l for l in range(20)}
    width = {float(reg._lib.goicp_trans_delta(1.0 / (1 << j))): 1.0 / (1 << j) for j in range(12)}
    prot = {}
    out = []
    for i in idx:
        r = recs[i]
        k = int(r["rot"])
        if k not in prot:
            prot[k] = O.rotate(rots[k], data)
        lvl = coeff[float(r["coeff"])] if r["coeff"] != 0 else None
        if lvl is not None:
            assert O.rot_coeff(lvl) == r["coeff"]
        out.append(O.cube_bound_f64(dt, prot[k], None if lvl is None else rho[lvl], (r["tx"], r["ty"], r["tz"]), width[float(r["delta"])]))
    return np.array(out)


def _eval_three_ways(pkg, hip, reg, rots, recs):
    """The batch through goicp_eval_bounds_device (the timed launch), goicp_eval_bounds_batch and goicp_eval_bounds_device_grouped."""
    B = pkg.binding
    lib, h, n = reg._lib, reg.handle, len(recs)
    d_rots, d_cubes = hip.upload(rots.reshape(-1).astype(np.float32)), hip.upload(np.ascontiguousarray(recs).view(np.uint8))
    outs = [hip.alloc(4 * n) for _ in range(4)]
    B.check(lib.goicp_eval_bounds_device(h, d_rots, d_cubes, n, outs[0], outs[1], None))
    ub, lb = hip.download(outs[0], n, np.float32), hip.download(outs[1], n, np.float32)
    B.check(lib.goicp_eval_bounds_device_grouped(h, d_rots, len(rots), d_cubes, n, outs[2], outs[3], None))
    gub, glb = hip.download(outs[2], n, np.float32), hip.download(outs[3], n, np.float32)
    bub, blb = np.empty(n, np.float32), np.empty(n, np.float32)
    fp = C.POINTER(C.c_float)
    B.check(lib.goicp_eval_bounds_batch(h, np.ascontiguousarray(rots, np.float32).ctypes.data_as(fp), len(rots),
                                        np.ascontiguousarray(recs).ctypes.data_as(C.POINTER(B.CCube)), n, bub.ctypes.data_as(fp), blb.ctypes.data_as(fp)))
    return (ub, lb), (bub, blb), (gub, glb), outs[0]


def test_headline_batch_entry_points_and_min(pkg, hip, bunny_model, bunny_data):
    """bench.make_batch(8192, 8, seed=1234) on the headline engine: the device entry point the bench times, the host batch entry and
    the grouped device entry give bit-equal bounds; goicp_reduce_min_device on that ub is numpy's (min, first argmin).  (The values
    themselves are held to the float64 reference by test_bench_plain_line_and_dumped_outputs, on the bench's own dump.)"""
    bench = _bench()
    reg = _headline_reg(pkg, bunny_model, bunny_data)
    rots, recs, _ = bench.make_batch(pkg, reg, 8192, 8, seed=1234)
    (ub, lb), (bub, blb), (gub, glb), d_ub = _eval_three_ways(pkg, hip, reg, rots, recs)
    assert np.array_equal(ub, bub) and np.array_equal(lb, blb)
    assert np.array_equal(ub, gub) and np.array_equal(lb, glb)
    assert (lb <= ub).all() and (lb >= 0).all()
    d_min, d_idx = hip.alloc(4), hip.alloc(4)
    pkg.binding.check(reg._lib.goicp_reduce_min_device(reg.handle, d_ub, len(ub), d_min, d_idx, None))
    assert hip.download(d_min, 1, np.float32)[0] == ub.min() and hip.download(d_idx, 1, np.int32)[0] == int(np.argmin(ub))
    hip.free_all()
    reg.close()


def test_generic_batch_vs_f64(pkg, oracle_mod, oracle_dt_bunny, hip, bunny_model, bunny_data):
    """256 cubes of bench.make_generic_batch (unrelated cubes: the kernel's generic path) against the float64 reference, through
    all three entry points (bit-equal).  Measured worst 2.9e-7."""
    bench = _bench()
    reg = _headline_reg(pkg, bunny_model, bunny_data)
    rots, recs, _ = bench.make_generic_batch(pkg, reg, 256, 8, seed=4321)
    (ub, lb), (bub, blb), (gub, glb), _ = _eval_three_ways(pkg, hip, reg, rots, recs)
    hip.free_all()
    assert np.array_equal(ub, bub) and np.array_equal(lb, blb) and np.array_equal(ub, gub) and np.array_equal(lb, glb)
    ref = _record_refs(oracle_mod, oracle_dt_bunny, bunny_data, rots, recs, range(len(recs)), reg)
    dev = np.maximum(np.abs(ub - ref[:, 0]) / np.maximum(ref[:, 0], 1e-3), np.abs(lb - ref[:, 1]) / np.maximum(ref[:, 1], 1e-3))
    print("generic batch (256 cubes): worst rel deviation %.2e" % dev.max())
    assert dev.max() <= TOL, (int(np.argmax(dev)), dev.max())
    reg.close()


def test_s2_headline_launch_vs_f64(pkg, oracle_mod, hip, s2):
    """The S2 launch (N = M = 1 M, DT 512^3: the non-lean path): bench.make_batch(8192, 8, seed=1234) through the device entry point,
    16 of its cubes (both passes) against cube_bound_f64 on the oracle's 512^3 DT.  Measured worst 1.9e-7."""
    model, data, dt, V = s2
    bench = _bench()
    reg = _headline_reg(pkg, model, data, dt_size=V)
    rots, recs, _ = bench.make_batch(pkg, reg, 8192, 8, seed=1234)
    n = len(recs)
    d_rots, d_cubes = hip.upload(rots.reshape(-1)), hip.upload(np.ascontiguousarray(recs).view(np.uint8))
    d_ub, d_lb = hip.alloc(4 * n), hip.alloc(4 * n)
    pkg.binding.check(reg._lib.goicp_eval_bounds_device(reg.handle, d_rots, d_cubes, n, d_ub, d_lb, None))
    ub, lb = hip.download(d_ub, n, np.float32), hip.download(d_lb, n, np.float32)
    hip.free_all()
    assert (lb <= ub).all() and np.isfinite(ub).all()
    rng = np.random.default_rng(16)
    idx = np.concatenate([rng.choice(np.flatnonzero(recs["coeff"] == 0), 8, replace=False), rng.choice(np.flatnonzero(recs["coeff"] != 0), 8, replace=False)])
    ref = _record_refs(oracle_mod, dt, data, rots, recs, idx, reg)
    dev = np.maximum(np.abs(ub[idx] - ref[:, 0]) / np.maximum(ref[:, 0], 1e-3), np.abs(lb[idx] - ref[:, 1]) / np.maximum(ref[:, 1], 1e-3))
    print("S2 headline launch (16 cubes): worst rel deviation %.2e" % dev.max())
    assert dev.max() <= TOL_1M, (idx[int(np.argmax(dev))], dev.max())
    reg.close()
