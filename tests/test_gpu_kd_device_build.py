"""Every consumer of a neighbour walk on the device-built hierarchy (kd_gpu_build = 1: Morton keys, radix sort, balanced leaf runs, bottom-up
boxes), with and without the nearest-point seed (icp_point_seed).  The walks are exact for any hierarchy, so the four handles
kd_gpu_build {0, 1} x icp_point_seed {1, 0} over the same clouds must agree BIT FOR BIT: no assertion here has a tolerance.

  against brute force   nn_query (oracle.nn_brute) and knn_query for k in {1, 16, 17, 31, 32} clipped to M (test_gpu_point_to_plane._knn_brute:
                        the leaf scan's float32 expression, ties to the lower index): indices, distance bits, ascending (d2, index);
                        256 queries of test_gpu_small_shapes._knn_queries (on target points, near them, around the cloud, far outside the grid)
  against the default   (host median splits, seeded; itself held to references by the rest of the suite) target_normals() at normal_k 8, 16, 17, 32;
                        icp_run after 1 and 8 iterations (R, t, err, iters) under metric 0, metric 1 at normal_k 32, symmetric, generalized,
                        the gate with the capped and the full walk (and its inlier count), Huber (and its W, C); icp_run_batch of three starts;
                        eval_correspondences with and without a gate; pose_information under both metrics; icp_inliers.  The pass's sums are
                        64-bit fixed point, so they do not depend on the order the hierarchy visits points in (test_icp_point_seed_is_exact
                        relies on the same).  One place is left open by the API: eval_correspondences returns index -1 beyond the gate, and the
                        distance of such a point is the walk's bound when the capped walk stopped early -- only the inliers' distances are compared.

Targets (knn_walk_twin.CELLS): the synth surface at M = 2, 17, 63, 64, 65, 1 024 (one box level; up to 65 points the root has empty leaves),
1 025, 1 500, 2 047, 2 048, 2 049 (two; 16.02 .. 32.02 points per bottom-level group) and 65 537, 100 000, 131 071, 131 073 (three); at
M = 1 500 also a uniform cube, a tight cluster with one far point (nearly all Morton keys equal: leaves are index runs with coinciding
boxes), a quarter of the points duplicated, all points but one in one place (M - 1 equal keys, boxes and distances: every tie goes to the
lower index) and points on one axis; the cube and the cluster at 100 000 too.  A target of M identical points has extent 0 and is refused
by goicp_create whatever the hierarchy (the distance transform needs a box): test_identical_target_is_refused holds that, on all four
configurations, and the coincident cloud is the nearest target a handle accepts.
The source is twins.make_case's: 225 surface points and 32 far ones, N = 257.  The full ICP matrix runs on the synth surface and the cube at
M = 1 500 and on the surface at 100 000; every other cell runs metric 0 and, from M = 32 on, metric 1 at normal_k = min(32, M).

The defect these shapes found (fixed in the same change): rows_knn left an emptied group only when its smallest key lay above the pruning
bound, and the bound is 0xffffffff while the list is short -- so a bottom-level group with fewer than k points was never left: the walk
rescanned its child 3, for ever if that leaf is empty, inserting its points again if not.  The host build cannot reach it (its bottom groups
hold >= 512 points); the device build does for M in 1 025 .. 2 047 with k > M / 64 and 65 537 .. 131 071 with k > M / 4 096.

Teeth: the unfixed walk is never run on a device.  tests/knn_walk_twin.py steps the walk's control flow on the CPU over these very
hierarchies, with this file's first queries (24 at two levels, 6 at three), seeded with the nearest point, under the OLD test and a cap of
the most steps a terminating walk can take (4 162 at two levels, 266 306 at three).  Walks that hit the cap | end with a point in the list
twice | end exact, by luck:
  synth      M   1 025 k 32   18 | 3 |  3        synth      M  65 537 k 32   3 | 0 | 3
  synth      M   1 500 k 32   14 | 2 |  8        synth      M 100 000 k 32   4 | 0 | 2
  synth      M   2 047 k 32    2 | 0 | 22        synth      M 131 071 k 32   0 | 0 | 6   (one group of 4 096 is a point short: the normals' rows reach it)
  uniform    M   1 500 k 32   19 | 0 |  5        uniform    M 100 000 k 32   3 | 0 | 3
  cluster    M   1 500 k 32   24 | 0 |  0        cluster    M 100 000 k 32   4 | 0 | 2
  duplicates M   1 500 k 32   13 | 1 | 10        synth      M   1 025 k 17  13 | 1 | 10
  coincident M   1 500 k 32    3 | 0 | 21        synth      M  65 537 k 17   0 | 0 | 6   (16 or 17 per group: only a walk seeded inside its first group)
  axis       M   1 500 k 32   12 | 9 |  3
  outside the bands (uniform M 1 500 k 16; synth M 2 048 and 2 049 k 32): 0 | 0 | 24 -- there the two tests cannot differ.
With the test the kernel has now every walk of every cell ends and returns the brute-force list, seeded and unseeded, and every band cell
holds a trigger group that a walk started here leaves with a short list (test_knn_walk_model_host.py asserts both).
"""
import functools

import numpy as np
import pytest

import knn_walk_twin as T
import twins
from conftest import load_pkg
from test_gpu_icp_gate import _run
from test_gpu_point_to_plane import _knn_brute
from test_gpu_small_shapes import _knn_queries
from test_icp_robust_host import HUBER

pytestmark = pytest.mark.gpu
CONFIGS = ((0, 1), (1, 1), (0, 0), (1, 0))              # (kd_gpu_build, icp_point_seed); the first is the default handle
NORMAL_KS = (8, 16, 17, 32)
MATRIX_CELLS = (("synth", 1500), ("uniform", 1500), ("synth", 100000))
_id = lambda v: str(v)


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@functools.lru_cache(maxsize=None)
def _case(kind, M):
    load_pkg()
    from cuda_go_icp_amd import synth
    return T.device_build_case(synth, kind, M)


@functools.lru_cache(maxsize=None)
def _brute(kind, M):
    """the queries and their brute-force neighbours, once per cell: 1-NN from the oracle, the min(32, M) nearest in (d2, index) order --
    whose first k are the k nearest"""
    import oracle
    target = _case(kind, M)["target"]
    q = _knn_queries(target, T.N_QUERIES, T.query_seed(M))
    bi, bd = oracle.nn_brute(target, q)
    ki, kd = _knn_brute(target, q, min(32, M))
    for a in (q, bi, bd, ki, kd):
        a.setflags(write=False)
    return q, bi, bd, ki, kd


class _Handles:
    """the handles of `configs` over one case; closes them all"""

    def __init__(self, pkg, c, configs=CONFIGS):
        self.regs = []
        try:
            for build, seed in configs:
                self.regs.append(pkg.Registration(c["target"], c["source"], 1e-3, dt_size=32, kd_gpu_build=build, icp_point_seed=seed))
        except Exception:
            self.close()
            raise

    def close(self):
        for r in self.regs:
            r.close()

    def __enter__(self):
        return self.regs

    def __exit__(self, *exc):
        self.close()


def _bits(x):
    """anything a handle returns -> bytes that are equal iff the bits are"""
    if isinstance(x, dict):
        return b"".join(k.encode() + _bits(v) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return b"|".join(_bits(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


def _all_equal(regs, what, fn):
    """fn(reg) on every handle; all as the default handle's, bit for bit"""
    outs = [fn(r) for r in regs]
    for cfg, o in zip(CONFIGS[1:], outs[1:]):
        assert _bits(o) == _bits(outs[0]), (what, "kd_gpu_build %d icp_point_seed %d" % cfg)
    return outs[0]


def _check_knn(reg, q, ki, kd, k, tag):
    idx, d2 = reg.knn_query(q, k)
    assert idx.shape == (len(q), k)
    assert np.array_equal(idx, ki[:, :k]), (tag, k, int(np.sum(idx != ki[:, :k])))
    assert np.array_equal(d2.view(np.uint32), kd[:, :k].view(np.uint32)), (tag, k)
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    assert np.all(key[:, 1:] > key[:, :-1]), (tag, k)              # ascending (d2, index), no point twice


# ----------------------------------------------------------------------------------------------
# 1. the walks against brute force
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M,k", T.BAND_CELLS, ids=_id)
def test_knn_band_device_built(pkg, kind, M, k):
    """the narrowest form of the defect's shapes: knn_query on the device-built hierarchy alone, one k above the points of a bottom-level group"""
    c = _case(kind, M)
    q, _, _, ki, kd = _brute(kind, M)
    with _Handles(pkg, c, ((1, 1), (1, 0))) as regs:
        for reg, seed in zip(regs, (1, 0)):
            _check_knn(reg, q, ki, kd, k, (kind, M, "seed %d" % seed))


@pytest.mark.parametrize("kind,M", T.CELLS, ids=_id)
def test_walks_against_brute_force(pkg, kind, M):
    c = _case(kind, M)
    q, bi, bd, ki, kd = _brute(kind, M)
    with _Handles(pkg, c) as regs:
        for reg, cfg in zip(regs, CONFIGS):
            tag = (kind, M) + cfg
            idx, d2 = reg.nn_query(q)
            assert np.array_equal(idx, bi), (tag, int(np.sum(idx != bi)))
            assert np.array_equal(d2.view(np.uint32), bd.view(np.uint32)), tag
            for k in T.ks_of(M):
                _check_knn(reg, q, ki, kd, k, tag)


def test_identical_target_is_refused(pkg):
    """extent 0: GOICP_ERR_INVALID from goicp_create on every configuration, before any hierarchy is built"""
    c = _case("identical", 1500)
    for build, seed in CONFIGS:
        with pytest.raises(pkg.GoicpError) as e:
            pkg.Registration(c["target"], c["source"], 1e-3, dt_size=32, kd_gpu_build=build, icp_point_seed=seed).close()
        assert e.value.code == -1, (build, seed, e.value)


# ----------------------------------------------------------------------------------------------
# 2. the target normals against the default handle
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [cell for cell in T.CELLS if cell[1] >= 3], ids=_id)
def test_target_normals_match_default(pkg, kind, M):
    """normal_build_kernel walks rows_knn once per target point, seeded with the point itself"""
    c = _case(kind, M)
    with _Handles(pkg, c) as regs:
        for nk in sorted({min(k, M) for k in NORMAL_KS}):
            def normals(reg):
                reg.set_icp_options(1, nk)
                return reg.target_normals()
            n = _all_equal(regs, ("normals", kind, M, nk), normals)
            assert np.isfinite(n).all()
            if kind in ("synth", "uniform", "duplicates") and nk >= 8:
                assert np.all(np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1) <= 1e-6)   # real normals, not the zero of a degenerate patch


# ----------------------------------------------------------------------------------------------
# 3. the ICP consumers against the default handle
# ----------------------------------------------------------------------------------------------
def _runs(c, extra=None):
    """-> fn(reg): the trajectory after 1 and after 8 iterations (and extra(reg) after each)"""
    def fn(reg):
        out = []
        for iters in (1, 8):
            out.append(_run(reg, c["R0"], c["t0"], max_iter=iters))
            if extra:
                out.append(extra(reg))
        return out
    return fn


def _check_cell(regs, c, normal_k):
    """metric 0 and, with normal_k, metric 1: run, inlier count"""
    tag = (c["kind"], c["M"])
    for r in regs:
        r.set_icp_options(0, 16)
    _all_equal(regs, tag + ("metric 0",), _runs(c, lambda r: r.icp_inliers(1)))
    if normal_k:
        for r in regs:
            r.set_icp_options(1, normal_k)
        _all_equal(regs, tag + ("metric 1", normal_k), _runs(c, lambda r: r.icp_inliers(1)))
        for r in regs:
            r.set_icp_options(0, 16)


@pytest.mark.parametrize("kind,M", [cell for cell in T.CELLS if cell not in MATRIX_CELLS], ids=_id)
def test_icp_cell_matches_default(pkg, kind, M):
    c = _case(kind, M)
    with _Handles(pkg, c) as regs:
        _check_cell(regs, c, min(32, M) if M >= 32 else 0)


@pytest.mark.parametrize("kind,M", MATRIX_CELLS, ids=_id)
def test_icp_matrix_matches_default(pkg, kind, M):
    c = _case(kind, M)
    tag = (kind, M)
    R1 = (twins.rodrigues64([-0.03, 0.01, 0.02]) @ c["R0"].astype(np.float64)).astype(np.float32)
    t1 = (c["t0"] + np.array([-0.01, 0.015, 0.005], np.float32)).astype(np.float32)
    with _Handles(pkg, c) as regs:
        _check_cell(regs, c, 32)
        # the gate and the Huber scale from the default handle's own distances at the start pose: the median, so half the points are inside
        _, d2, _, _ = regs[0].eval_correspondences(c["R0"], c["t0"])
        g = float(np.float32(np.median(np.sqrt(d2.astype(np.float64)))))
        assert 0 < int(np.sum(d2 <= np.float32(g) * np.float32(g))) < c["N"]

        def each(fn):
            for r in regs:
                fn(r)

        for metric, nk in ((0, 16), (1, 32)):
            each(lambda r: r.set_icp_options(metric, nk))
            for capped in (1, 0):
                each(lambda r: r.set_icp_gate(g, capped_walk=capped))
                out = _all_equal(regs, tag + ("gate", metric, capped), _runs(c, lambda r: r.icp_inliers(1)))
                assert 0 < int(out[1][0]) < c["N"]
            each(lambda r: r.set_icp_gate(0.0))
            each(lambda r: r.set_icp_robust(HUBER, g))
            out = _all_equal(regs, tag + ("huber", metric), _runs(c, lambda r: r.icp_robust_stats(1)))
            assert 0 < float(out[1][1][0]) < c["N"]                # W: some weights below one
            each(lambda r: r.set_icp_robust(0))
            # the batch of three starts, two of them equal
            Rb, tb = np.stack([c["R0"], R1, c["R0"]]), np.stack([c["t0"], t1, c["t0"]])
            _all_equal(regs, tag + ("batch", metric), lambda r: (r.icp_run_batch(Rb, tb, 8, 1e-7), r.icp_inliers(3)))
            _all_equal(regs, tag + ("pose_information", metric), lambda r: [r.pose_information(R, t) for R, t in ((c["R0"], c["t0"]), (R1, t1))])
        # symmetric and generalized: metric 1 over the normals of both clouds
        each(lambda r: r.set_icp_options(1, 32))
        each(lambda r: r.set_icp_symmetric(True, 16))
        _all_equal(regs, tag + ("symmetric",), _runs(c))
        each(lambda r: r.set_icp_symmetric(False, 16))
        each(lambda r: r.set_icp_generalized(True, 1e-3, 16))
        _all_equal(regs, tag + ("generalized",), _runs(c))
        each(lambda r: r.set_icp_generalized(False, 1e-3, 16))
        each(lambda r: r.set_icp_options(0, 16))

        # eval_correspondences: everything without a gate; with one, the index (-1 beyond it), the count, the sum and the inliers' distances
        _all_equal(regs, tag + ("eval_correspondences",), lambda r: r.eval_correspondences(R1, t1))

        def gated(r):
            idx, dd, n, sse = r.eval_correspondences(R1, t1, g)
            return idx, np.where(idx >= 0, dd, np.float32(0)), n, sse
        idx, _, n, _ = _all_equal(regs, tag + ("eval_correspondences", g), gated)
        assert 0 < n < c["N"] and int(np.sum(idx >= 0)) == n
