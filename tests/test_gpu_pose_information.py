"""Pose information (goicp_pose_information): the Gauss-Newton normal matrix, gradient, rank and covariance at a given pose.

1. fp64 twin.  The twin restates DESIGN 15 in numpy on the library's OWN q (goicp_transform_source), neighbours and d^2
   (goicp_eval_correspondences) and normals (goicp_target_normals), so neighbour ties cannot matter; gate and robust weights are recomputed
   in np.float32, operation by operation.  The bound is a running error analysis of the device arithmetic, computed from the data:
   every float operation adds u = 2^-24 times its result (plus the propagated error of its operands: V below), a workgroup's float column
   sum of 16 rows adds 15 u times the sum of the magnitudes, and every workgroup adds one fixed-point quantum 1 / scale, with
   scale >= 4.6e18 / (2 N T^2) and T = 2 (max(Ba, E) + 1) as DESIGN 15 derives it.  Integer outputs, and W on unit weights, are exact.
   Metric 1 needs normal_k = 16 <= M target points, so the M = 2 shape runs metric 0 only.  M = 1: goicp_create itself refuses a target
   of zero extent (GOICP_ERR_INVALID, as it always has), so no handle exists to ask; the M = 1 case holds exactly that, and M = 2 -- the
   smallest target the engine accepts -- is twinned in its place.
2. batch == single, raw bytes.  3. degenerate geometry.  4. the finishing step.  5. the result surface (API + CLI).  6. refusals.
7. the handle's ICP and bounds are untouched.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, cloud, load_pkg
from test_pose_information_host import EPS, eig_tol, pinv_tol

pytestmark = pytest.mark.gpu
INVALID = -1
U = 2.0 ** -24
HUBER, TUKEY = 1, 4
f32 = np.float32


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


def _rodrigues(v):
    from cuda_go_icp_amd import synth
    return synth._rodrigues(np.asarray(v, np.float64))


POSES = {"identity": (np.eye(3, dtype=f32), np.zeros(3, f32)),
         "moved": (None, np.array([0.03, -0.02, 0.01], f32))}


def _pose(name):
    R, t = POSES[name]
    if R is None:
        R = _rodrigues([0.2, -0.1, 0.15]).astype(f32)
    return np.ascontiguousarray(R, f32), t


def _clouds(N, M, seed=0):
    from cuda_go_icp_amd import synth
    tgt, src, _, _ = synth.make_pair(seed=4200 + seed, M=max(M, 4), N=max(N, 4), noise=0.01)
    return np.ascontiguousarray(tgt[:M]), np.ascontiguousarray(src[:N])


# ----------------------------------------------------------------------------------------------
# the twin: values in fp64 with a running bound on what the float evaluation may differ by
# ----------------------------------------------------------------------------------------------
class V:
    """val: the exact-arithmetic value (fp64) of an expression of float inputs; err: bound on |its float evaluation - val|"""

    def __init__(self, val, err=None):
        self.val = np.asarray(val, np.float64)
        self.err = np.zeros_like(self.val) if err is None else err

    def _r(self, val, e):                       # one more float rounding: u * |computed| <= u (|val| + e)
        return V(val, e + U * (np.abs(val) + e))

    def __sub__(self, o):
        return self._r(self.val - o.val, self.err + o.err)

    def __add__(self, o):
        return self._r(self.val + o.val, self.err + o.err)

    def __mul__(self, o):
        return self._r(self.val * o.val, np.abs(self.val) * o.err + np.abs(o.val) * self.err + self.err * o.err)


def robust_w(kernel, c, r):
    """device.hip robust_terms' weight in np.float32, operation by operation (r = the residual, float32)"""
    c = f32(c)
    r = r.astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = r / c
        u2 = u * u
        if kernel == HUBER:
            return np.where(r <= c, f32(1), c / r).astype(f32)
        a1 = f32(1) - u2
        return np.where(r <= c, a1 * a1, f32(0)).astype(f32)


def twin(reg, tgt, normals, R, t, metric, mode, arg, pivot):
    """-> dict word name -> (value, bound): information (6, 6), gradient (6,), cost, sse, weight_sum, plus inliers (exact)"""
    N = reg.ns
    q = reg.transform_source(R, t).astype(f32)
    idx, d2, _, _ = reg.eval_correspondences(R, t, 0.0)
    m = tgt[idx]
    c = np.asarray(pivot, f32)
    Q = [V(q[:, k]) for k in range(3)]
    a = [Q[k] - V(np.full(N, c[k])) for k in range(3)]
    e = [Q[k] - V(m[:, k]) for k in range(3)]
    cross = lambda x, y: [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]
    if metric == 1:
        n32 = normals[idx].astype(f32)
        nn = [V(n32[:, k]) for k in range(3)]
        ef = (q - m).astype(f32)                                         # the residual in float, the pass's order
        res32 = (ef[:, 0] * n32[:, 0] + ef[:, 1] * n32[:, 1]).astype(f32)
        res32 = (res32 + ef[:, 2] * n32[:, 2]).astype(f32)
        resid32 = np.abs(res32)
    else:
        resid32 = np.sqrt(d2.astype(f32)).astype(f32)
    if mode == "plain":
        w32 = np.ones(N, f32)
    elif mode == "gate":
        g2 = f32(arg) * f32(arg)
        w32 = (d2 <= g2).astype(f32)
    else:
        w32 = robust_w(arg[0], arg[1], resid32)
    w = V(w32)
    D2 = V(d2)
    words = {}

    def total(name, term):
        # column sums of 16 rows in float (15 additions on partial sums below the sum of magnitudes), then one quantum per workgroup
        mag = np.abs(term.val) + term.err
        words[name] = (float(term.val.sum()), float(term.err.sum() + 15 * U * mag.sum()))

    if metric == 0:
        wa = [w * a[k] for k in range(3)]
        for k in range(3):
            total("sa%d" % k, wa[k])
        for i in range(3):
            for j in range(i, 3):
                total("aa%d%d" % (i, j), wa[i] * a[j])
        ce = cross(a, e)
        for k in range(3):
            total("b%d" % k, w * ce[k])
            total("b%d" % (3 + k), w * e[k])
        total("cost", w * D2)
    else:
        J = cross(a, nn) + nn
        res = (e[0] * nn[0] + e[1] * nn[1]) + e[2] * nn[2]
        for i in range(6):
            for j in range(i, 6):
                total("A%d%d" % (i, j), (J[i] * J[j]) * w)
            total("b%d" % i, (J[i] * res) * w)
        total("cost", (res * res) * w)
    total("sse", D2)
    total("W", w)
    return words, int((w32 > 0).sum()), w32


def quantum_bound(reg, tgt, src, R, t, pivot, default_pivot):
    """one fixed-point quantum per workgroup: scale = 2^floor(log2(4.6e18 / (N T^2))) >= 4.6e18 / (2 N T^2) (1 % on T for the
    engine's own float extents)"""
    N = len(src)
    rho = np.linalg.norm(R.astype(np.float64))
    cen = src.astype(np.float64).mean(0)
    Ba = rho * np.linalg.norm(src - cen, axis=1).max() + np.linalg.norm(np.asarray(pivot, np.float64) - default_pivot)
    E = rho * np.linalg.norm(src.astype(np.float64), axis=1).max() + np.linalg.norm(t.astype(np.float64)) + np.sqrt(3) * np.abs(tgt).max()
    T = 1.01 * 2 * (max(Ba, E) + 1)
    return (N + 15) // 16 * (2 * N * T * T / 4.6e18)


def compare(info, words, n_in, metric, quantum, n_wg, tag):
    """the library's report against the twin's words, entry by entry; returns the largest error / bound seen"""
    worst = 0.0

    def hold(name, got, val, tol):
        nonlocal worst
        tol = tol + quantum
        err = abs(got - val)
        worst = max(worst, err / tol)
        assert err <= tol, (tag, name, got, val, err, tol)

    A = info["information"]
    assert np.array_equal(A, A.T)
    if metric == 0:
        aa = {k: words["aa%d%d" % k] for k in [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]}
        diag = lambda i: (sum(aa[(k, k)][0] for k in range(3) if k != i), sum(aa[(k, k)][1] for k in range(3) if k != i) + quantum)
        for i in range(3):
            hold("Aww%d%d" % (i, i), A[i, i], *diag(i))
            for j in range(i + 1, 3):
                hold("Aww%d%d" % (i, j), A[i, j], -aa[(i, j)][0], aa[(i, j)][1])
        sa = [words["sa%d" % k] for k in range(3)]
        for (i, j, k, s) in [(0, 1, 2, -1), (0, 2, 1, 1), (1, 0, 2, 1), (1, 2, 0, -1), (2, 0, 1, -1), (2, 1, 0, 1)]:
            hold("Awt%d%d" % (i, j), A[i, 3 + j], s * sa[k][0], sa[k][1])
        for i in range(3):
            assert A[i, 3 + i] == 0.0
            for j in range(3):
                assert A[3 + i, 3 + j] == (info["weight_sum"] if i == j else 0.0)
    else:
        for i in range(6):
            for j in range(i, 6):
                hold("A%d%d" % (i, j), A[i, j], *words["A%d%d" % (i, j)])
    for i in range(6):
        hold("b%d" % i, info["gradient"][i], *words["b%d" % i])
    hold("cost", info["cost"], *words["cost"])
    hold("sse", info["sse"], *words["sse"])
    Wv, Wt = words["W"]
    assert abs(info["weight_sum"] - Wv) <= Wt + 2.0 ** -36 * n_wg, (tag, info["weight_sum"], Wv)    # W's own quantum is 2^-36 per workgroup
    assert info["inliers"] == n_in, (tag, info["inliers"], n_in)
    return worst


SHAPES = [(1, 500), (5, 500), (255, 500), (256, 500), (257, 500), (1021, 500), (257, 1), (257, 2), (257, 17), (257, 1025)]


@pytest.mark.parametrize("N,M", SHAPES)
def test_fp64_twin(pkg, N, M):
    tgt, src = _clouds(N, M)
    if M == 1:
        with pytest.raises(pkg.GoicpError) as ei:          # a one-point target has zero extent: the engine has never accepted it
            pkg.Registration(tgt, src, 1e-3, dt_size=64)
        assert ei.value.code == INVALID and "zero extent" in str(ei.value)
        return
    reg = pkg.Registration(tgt, src, 1e-3, dt_size=64)
    try:
        metrics = (0, 1) if M >= 16 else (0,)
        normals = reg.target_normals() if 1 in metrics else None
        worst = 0.0
        for pose in ("identity", "moved"):
            R, t = _pose(pose)
            _, d2, _, _ = reg.eval_correspondences(R, t, 0.0)
            ds = np.sort(d2)
            # a gate between two distinct distances: rejects some, not all (N = 1: nothing to reject)
            lo = ds[(N - 1) // 2]
            hi = ds[ds > lo].min() if (ds > lo).any() else lo * 4 + 1e-6
            gate = float(np.sqrt(f32(0.5) * (lo + hi)))
            default_pivot = (R.astype(np.float64) @ src.astype(np.float64).mean(0) + t)
            sse_plain = {}
            for mode, arg in (("plain", None), ("gate", gate), ("robust", (HUBER, gate)), ("robust", (TUKEY, 2 * gate))):
                reg.set_icp_gate(gate if mode == "gate" else 0.0)
                reg.set_icp_robust(*(arg if mode == "robust" else (0, 0.0)))
                if mode == "gate":
                    n_gate = reg.eval_correspondences(R, t, gate)[2]
                    if N > 1:
                        assert 0 < n_gate < N, (n_gate, N)
                for metric in metrics:
                    for pivot in (None, np.zeros(3)):
                        info = reg.pose_information(R, t, metric=metric, pivot=pivot)
                        tag = (N, M, pose, mode, arg, metric, pivot is None)
                        assert info["metric"] == metric
                        if pivot is None:
                            assert np.abs(info["pivot"] - default_pivot).max() <= 8 * U * (np.abs(default_pivot).max() + 1), tag
                        else:
                            assert np.array_equal(info["pivot"], pivot)
                        words, n_in, w32 = twin(reg, tgt, normals, R, t, metric, mode, arg, info["pivot"])
                        q = quantum_bound(reg, tgt, src, R, t, info["pivot"], default_pivot)
                        worst = max(worst, compare(info, words, n_in, metric, q, (N + 15) // 16, tag))
                        if mode == "gate":
                            assert info["inliers"] == n_gate, tag
                        if mode in ("plain", "gate"):
                            assert info["weight_sum"] == float(info["inliers"]), tag      # unit weights: W is an exact integer
                        if mode == "plain":
                            assert info["inliers"] == N
                            sse_plain[(metric, pivot is None)] = info["sse"]
                        # sum d^2 runs over all N points whatever the weights: the plain call's bits
                        assert info["sse"] == sse_plain[(metric, pivot is None)], tag
        print("N %d M %d: largest error / bound %.3f" % (N, M, worst))
        assert worst <= 1.0
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 2. batch
# ----------------------------------------------------------------------------------------------
def _raw_single(pkg, reg, R, t, metric):
    from cuda_go_icp_amd import binding as B
    from cuda_go_icp_amd.fgoicp import _fptr, _pose_info_options
    o, out = _pose_info_options(metric), B.CPoseInfo()
    B.check(reg._lib.goicp_pose_information(reg.handle, _fptr(R), _fptr(t), C.byref(o), C.byref(out)))
    return bytes(out)


def _raw_batch(pkg, reg, Rs, ts, metric):
    from cuda_go_icp_amd import binding as B
    from cuda_go_icp_amd.fgoicp import _fptr, _pose_info_options
    K = len(Rs)
    o, out = _pose_info_options(metric), (B.CPoseInfo * K)()
    B.check(reg._lib.goicp_pose_information_batch(reg.handle, K, _fptr(Rs), _fptr(ts), C.byref(o), out))
    return [bytes(out[k]) for k in range(K)]


@pytest.fixture(scope="module")
def shape257(pkg):
    tgt, src = _clouds(257, 500)
    reg = pkg.Registration(tgt, src, 1e-3, dt_size=64)
    yield reg, tgt, src
    reg.close()


@pytest.mark.parametrize("K", [1, 2, 65])
def test_batch_is_the_single_call_bit_for_bit(pkg, shape257, K):
    reg, tgt, src = shape257
    rng = np.random.default_rng(K)
    Rs = np.ascontiguousarray(np.stack([_rodrigues(rng.uniform(-0.3, 0.3, 3) + 1e-3) for _ in range(K)]).astype(f32).reshape(K, 9))
    ts = np.ascontiguousarray(rng.uniform(-0.05, 0.05, (K, 3)).astype(f32))
    d2 = reg.eval_correspondences(Rs[0], ts[0], 0.0)[1]
    gate = float(np.sqrt(np.median(d2)))
    try:
        for g in (0.0, gate):
            reg.set_icp_gate(g)
            for metric in (0, 1):
                got = _raw_batch(pkg, reg, Rs, ts, metric)
                for k in range(K):
                    assert got[k] == _raw_single(pkg, reg, Rs[k], ts[k], metric), (K, k, metric, g)
        d = reg.pose_information_batch(Rs.reshape(K, 3, 3), ts, metric=0)
        assert len(d) == K and d[0]["inliers"] > 0
    finally:
        reg.set_icp_gate(0.0)


# ----------------------------------------------------------------------------------------------
# 3. degenerate geometry (coordinates are multiples of 1/16: every term is exact in float)
# ----------------------------------------------------------------------------------------------
def test_plane_point_to_plane_has_rank_three(pkg):
    g = np.arange(17, dtype=f32) / f32(16)
    tgt = np.ascontiguousarray(np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2))
    tgt = np.ascontiguousarray(np.concatenate([tgt, np.zeros((len(tgt), 1), f32)], 1))
    src = np.ascontiguousarray(tgt[(np.arange(len(tgt)) * 7) % len(tgt)][:41])
    reg = pkg.Registration(tgt, src, 1e-3, dt_size=64)
    try:
        I1 = reg.pose_information(np.eye(3, dtype=f32), np.zeros(3, f32), metric=1)
        assert I1["rank"] == 3 and I1["inliers"] == len(src) and I1["sse"] == 0.0 and I1["cost"] == 0.0
        # the constrained directions are omega_x, omega_y, tau_z: the three retained eigenvectors live there
        keep = I1["eigenvectors"][3:]
        assert np.abs(keep[:, [2, 3, 4]]).max() <= 1e-6
        assert I1["eigenvalues"][2] <= 1e-6 * I1["eigenvalues"][5] and I1["eigenvalues"][3] > 1e-3 * I1["eigenvalues"][5]
        assert I1["sigma2"] == 0.0 and not I1["covariance"].any() and I1["dof_nonpositive"] == 0
        I0 = reg.pose_information(np.eye(3, dtype=f32), np.zeros(3, f32), metric=0)
        assert I0["rank"] == 6 and I0["dof_nonpositive"] == 0
    finally:
        reg.close()


def test_line_point_to_point_has_rank_five(pkg):
    tgt = np.zeros((17, 3), f32)
    tgt[:, 0] = np.arange(17, dtype=f32) / f32(16)
    src = np.ascontiguousarray(tgt[[0, 3, 7, 12, 16]])
    reg = pkg.Registration(tgt, src, 1e-3, dt_size=64)
    try:
        I = reg.pose_information(np.eye(3, dtype=f32), np.zeros(3, f32), metric=0)
        assert I["rank"] == 5
        assert I["eigenvalues"][0] == 0.0                                      # row and column omega_x are exactly zero
        assert np.array_equal(np.abs(I["eigenvectors"][0]), [1, 0, 0, 0, 0, 0])   # the null direction: rotation about x
        assert I["eigenvalues"][1] > 1e-3 * I["eigenvalues"][5]
    finally:
        reg.close()


def test_single_point(pkg):
    tgt, _ = _clouds(4, 17)
    src = np.array([[0.25, -0.5, 0.125]], f32)
    reg = pkg.Registration(tgt, src, 1e-3, dt_size=64)
    try:
        I = reg.pose_information(np.eye(3, dtype=f32), np.zeros(3, f32), metric=0)
        assert np.array_equal(I["information"], np.diag([0.0, 0, 0, 1, 1, 1]))
        assert I["rank"] == 3 and I["dof_nonpositive"] == 1 and I["sigma2"] == 0.0
        assert not I["covariance"].any()
        assert I["inliers"] == 1 and I["weight_sum"] == 1.0
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 4. the finishing step on a device-made matrix (bounds: tests/test_pose_information_host.py)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_finish(pkg, shape257, metric):
    reg, tgt, src = shape257
    R, t = _pose("moved")
    tol = 1e-6
    I = reg.pose_information(R, t, metric=metric, rank_tol=tol)
    A = I["information"]
    lam, vec = I["eigenvalues"], I["eigenvectors"]
    lam_ref = np.linalg.eigh(A)[0]
    assert np.abs(lam - lam_ref).max() <= eig_tol(A)
    assert np.linalg.norm(vec.T @ np.diag(lam) @ vec - A, 2) <= eig_tol(A)
    assert I["rank"] == int((lam_ref > tol * lam_ref.max()).sum()) == 6
    dof = (3 if metric == 0 else 1) * I["weight_sum"] - 6
    assert dof > 0 and I["dof_nonpositive"] == 0
    assert abs(I["sigma2"] - I["cost"] / dof) <= 4 * EPS * I["sigma2"]
    P_ref = np.linalg.pinv(A, rcond=tol, hermitian=True)
    err = np.linalg.norm(I["covariance"] - I["sigma2"] * P_ref, 2)
    assert err <= I["sigma2"] * pinv_tol(lam_ref, tol, P_ref), err


# ----------------------------------------------------------------------------------------------
# 5. the result surface
# ----------------------------------------------------------------------------------------------
def _toml_matrix(txt, name):
    body = txt.split("\n%s = [\n" % name)[1].split("\n]\n")[0]
    return np.array([[float(x) for x in row.strip().strip("[],").split(",")] for row in body.splitlines()])


def test_result_information_and_cli(pkg, tmp_path):
    from cuda_go_icp_amd import binding as B
    from cuda_go_icp_amd.fgoicp import _pose_info_options
    tgt, src = cloud("model_rand"), cloud("data_rand")
    go = pkg.FastGoICP(tgt, src, 1e-3)
    reg = go.registration
    try:
        with pytest.raises(pkg.GoicpError) as ei:
            go.information()
        assert ei.value.code == INVALID and "no finished registration" in str(ei.value)
        go.run()
        o, out = _pose_info_options(), B.CPoseInfo()
        B.check(reg._lib.goicp_result_information(reg.handle, C.byref(o), C.byref(out)))
        snap = reg.poll()
        R, t = np.array(snap.optR, f32), np.array(snap.optT, f32)
        assert bytes(out) == _raw_single(pkg, reg, R, t, None)
        assert go.information()["rank"] == out.rank
        # the CLI on the same clouds
        for name, pts in (("model", tgt), ("data", src)):
            with open(tmp_path / (name + ".txt"), "w") as f:
                f.write("%d\n" % len(pts))
                for p in pts:
                    f.write("%.9g %.9g %.9g\n" % tuple(p))
        exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
        texts = {}
        for flag in (False, True):
            outp = tmp_path / ("output_%d.toml" % flag)
            cfg = tmp_path / ("cfg_%d.toml" % flag)
            cfg.write_text('[info]\ndescription = "information"\n[io]\ntarget = "model.txt"\nsource = "data.txt"\noutput = "%s"\nvisualization = "%s"\n'
                           '[params]\nmode = 4\nsubsample = 1.0\nmse_threshold = 1e-3\nresize = 1.0\n' % (outp, tmp_path / "viz.ply"))
            r = subprocess.run([exe, str(cfg)] + (["--information"] if flag else []), check=True, capture_output=True, text=True, timeout=120)
            texts[flag] = outp.read_text()
            assert ("Information: rank" in r.stdout) == flag
        assert "[information]" not in texts[False] and "\n[information]\n" in texts[True]
        # without the flag the file is what the build writes when the feature is never touched: the flagged file up to its appended table
        # (dt_build_ms / register_ms are wall-clock readings and differ from run to run: masked)
        mask = lambda s: "\n".join(l for l in s.splitlines() if not l.startswith(("dt_build_ms", "register_ms")))
        assert mask(texts[False]) == mask(texts[True].split("\n[information]\n")[0])
        txt = texts[True]
        Rc = _toml_matrix(txt.split("[stats]")[0], "rotation").astype(f32).reshape(9)
        tc = np.array([float(x) for x in txt.split("translation = [")[1].split("]")[0].split(",")], f32)
        I = reg.pose_information(Rc, tc)                       # %.9g round-trips a float: the CLI's pose, bit for bit
        table = txt.split("\n[information]\n")[1]
        field = lambda k: [l for l in table.splitlines() if l.startswith(k + " =")][0].split("=")[1].strip()
        assert int(field("rank")) == I["rank"] and int(field("inliers")) == I["inliers"]
        assert float(field("sigma2")) == I["sigma2"] and float(field("weight_sum")) == I["weight_sum"]
        assert np.array_equal(np.array([float(x) for x in field("eigenvalues").strip("[]").split(",")]), I["eigenvalues"])
        assert np.array_equal(_toml_matrix("\n" + table, "information"), I["information"])
        assert np.array_equal(_toml_matrix("\n" + table, "covariance"), I["covariance"])
        bad = subprocess.run([exe, str(tmp_path / "cfg_1.toml"), "--information", "--ranks", "2"], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and "--information" in bad.stderr
    finally:
        reg.close()


# ----------------------------------------------------------------------------------------------
# 6. refusals
# ----------------------------------------------------------------------------------------------
def _refused(pkg, fn, needle):
    with pytest.raises(pkg.GoicpError) as ei:
        fn()
    assert ei.value.code == INVALID and needle in str(ei.value), (needle, str(ei.value))


def test_refusals(pkg, shape257):
    reg, tgt, src = shape257
    R, t = _pose("moved")
    run = lambda: pkg.IterativeClosestPoint3D(reg, 5, 1e-7).run()
    before = run()
    nan = f32("nan")
    Rbad, tbad = R.copy(), t.copy()
    Rbad[1, 1] = nan
    tbad[1] = f32("inf")
    _refused(pkg, lambda: reg.pose_information(R, t, metric=2), "metric")
    _refused(pkg, lambda: reg.pose_information(R, t, metric=-2), "metric")
    _refused(pkg, lambda: reg.pose_information(Rbad, t), "R has a non-finite")
    _refused(pkg, lambda: reg.pose_information(R, tbad), "t has a non-finite")
    _refused(pkg, lambda: reg.pose_information(R, t, pivot=[0, np.nan, 0]), "pivot")
    _refused(pkg, lambda: reg.pose_information(R, t, pivot=[0, np.inf, 0]), "pivot")
    _refused(pkg, lambda: reg.pose_information(R, t, pivot=[1e30, 0, 0]), "overflow")
    _refused(pkg, lambda: reg.pose_information(R, t, rank_tol=1.0), "rank_tol")
    _refused(pkg, lambda: reg.pose_information(R, t, rank_tol=-1e-9), "rank_tol")
    _refused(pkg, lambda: reg.pose_information_batch(np.zeros((0, 9), f32), np.zeros((0, 3), f32)), "K must be")
    _refused(pkg, lambda: reg.pose_information_batch(np.tile(R.reshape(1, 9), (1025, 1)), np.tile(t, (1025, 1))), "K must be")
    after = run()
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(before, after))
    # what the handle's parameters decide
    for kw, needle in (({"trim_fraction": 0.1}, "trim_fraction"), ({"dt_layout": 0}, "dt_layout"), ({"icp_fused": 1}, "icp_fused")):
        r2 = pkg.Registration(tgt, src, 1e-3, dt_size=64, **kw)
        try:
            b2 = pkg.IterativeClosestPoint3D(r2, 5, 1e-7).run()
            _refused(pkg, lambda: r2.pose_information(R, t), needle)
            _refused(pkg, lambda: r2.pose_information_batch(R.reshape(1, 9), t.reshape(1, 3)), needle)
            a2 = pkg.IterativeClosestPoint3D(r2, 5, 1e-7).run()
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(b2, a2))
        finally:
            r2.close()


def test_refused_while_a_registration_runs(pkg, shape257):
    reg, tgt, src = shape257
    R, t = _pose("identity")
    B = __import__("cuda_go_icp_amd").binding
    B.check(reg._lib.goicp_register_begin(reg.handle))
    try:
        _refused(pkg, lambda: reg.pose_information(R, t), "registration runs")
        _refused(pkg, lambda: reg.pose_information_batch(R.reshape(1, 9), t.reshape(1, 3)), "registration runs")
        _refused(pkg, lambda: reg.result_information(), "registration runs")
    finally:
        B.check(reg._lib.goicp_register_end(reg.handle))
    assert reg.pose_information(R, t)["inliers"] == len(src)


# ----------------------------------------------------------------------------------------------
# 7. defaults untouched
# ----------------------------------------------------------------------------------------------
def test_icp_and_bounds_keep_their_bits(pkg):
    tgt, src = _clouds(1021, 500, seed=1)
    reg = pkg.Registration(tgt, src, 1e-3, dt_size=64)
    try:
        R, t = _pose("moved")
        rng = np.random.default_rng(3)
        cubes = np.concatenate([rng.uniform(-0.3, 0.3, (32, 3)), np.full((32, 1), 0.125)], 1).astype(f32)

        def snapshot():
            icp = pkg.IterativeClosestPoint3D(reg, 20, 1e-7).run()
            ub, lb = reg.eval_bounds(R.reshape(3, 3), cubes, 3)
            return [np.asarray(x).tobytes() for x in icp] + [ub.tobytes(), lb.tobytes()]

        before = snapshot()
        for metric in (0, 1):
            reg.pose_information(R, t, metric=metric)
            reg.pose_information_batch(np.tile(R.reshape(1, 9), (3, 1)), np.tile(t, (3, 1)), metric=metric)
        assert snapshot() == before
    finally:
        reg.close()
