"""Pins the CPU oracle (oracle/goicp_oracle.c) to the REAL reference.

Every expected value below was produced by the reference's own CPU Go-ICP code
(src/goicp/*, compiled unmodified in the build container by oracle/Makefile and driven by
oracle/ref_harness.cpp; regenerate with `python oracle/gen_golden.py`).
Tolerances follow SURVEY.md 8(c).
"""
import numpy as np
import pytest

import os

from conftest import ROOT, cloud, golden, rot_angle


def test_dt_geometry_exact(oracle_dt_bunny):
    g = golden("dt_lookup")
    assert oracle_dt_bunny.V == g["SIZE"] == 300
    assert oracle_dt_bunny.scale == g["scale"]                      # jly_3ddt.cpp:923, double, bit-exact
    assert oracle_dt_bunny.origin == (g["xmin"], g["ymin"], g["zmin"])


def test_dt_seed_count(oracle_dt_bunny, bunny_model):
    _, n = oracle_dt_bunny.seed(bunny_model)
    assert n == 32561


def test_dt_lookup_vs_reference(oracle_dt_bunny):
    """DT3D::Distance (jly_3ddt.cpp:981-1026) incl. out-of-grid extension and int() truncation.
    Values: exact EDT vs the reference's propagated EDT -> <= 0.35 voxel, never below it."""
    g = golden("dt_lookup")
    q = np.array(g["query"]).reshape(-1, 3)
    ref = np.array(g["distance"], dtype=np.float32)
    mine = oracle_dt_bunny.distance(q)
    vox = 1.0 / g["scale"]
    assert np.all(mine <= ref + 1e-6)
    assert np.max(ref - mine) <= 0.35 * vox
    assert np.mean(mine == ref) > 0.999                             # index math exact


def test_dt_voxels_vs_reference(oracle_dt_bunny):
    g = golden("dt_lookup")
    v = np.array(g["voxel"]).reshape(-1, 3)
    ref = np.array(g["voxel_distance"], dtype=np.float32)
    mine = oracle_dt_bunny.grid()[v[:, 2], v[:, 1], v[:, 0]]
    vox = 1.0 / g["scale"]
    assert np.all(mine <= ref + 1e-7)
    assert np.max(ref - mine) <= 0.35 * vox


def test_dt_is_exact_edt_of_seed_grid(oracle_mod):
    """The oracle's DT build against scipy's exact EDT on a smaller grid."""
    from scipy import ndimage
    model = cloud("model_bunny")
    dt = oracle_mod.DistanceTransform(model, 96, 2.0)
    seed, _ = dt.seed(model)
    ref = ndimage.distance_transform_edt(seed == 0)
    expect = (np.sqrt((ref ** 2).round()).astype(np.float32).astype(np.float64) / dt.scale).astype(np.float32)
    assert np.array_equal(dt.grid(), expect)


def test_rot_radii_bit_exact(oracle_mod, bunny_data10):
    g = golden("rot_radii")
    _, rho = oracle_mod.rot_radii(bunny_data10)
    ref = np.array(g["maxRotDis"], dtype=np.float32)
    assert np.array_equal(rho[:, :64], ref)                          # jly_goicp.cpp:139-160


def test_inner_bnb_single_expansions(oracle_mod, oracle_dt_bunny, bunny_data10):
    """One expansion of GoICP::InnerBnB (jly_goicp.cpp:262-336): min ub over the 8 children and the
    arg-min child.  rel 1e-4 (float summation order: the reference permutes minDis first)."""
    g = golden("inner_bnb")
    _, rho = oracle_mod.rot_radii(bunny_data10)
    n = 0
    for case in g["cases"]:
        prot = oracle_mod.rotate(np.array(case["R"], dtype=np.float32).reshape(3, 3), bunny_data10)
        for s in case["single"]:
            r = rho[s["level"]] if s["level"] >= 0 else None
            v, best, pops, cubes = oracle_mod.inner_bnb(oracle_dt_bunny, prot, r, 1e10, 1e9, root=s["parent"])
            assert pops == s["pops"] and cubes == 8
            assert abs(v - s["min_ub"]) <= 1e-4 * max(s["min_ub"], 1e-3)
            assert np.array_equal(best, np.array(s["best"], dtype=np.float32))
            n += 1
    assert n == 384


def test_inner_bnb_full_searches(oracle_mod, oracle_dt_bunny, bunny_data10):
    """Whole InnerBnB calls: value rel 1e-3, best node identical, node pops within 1 %."""
    g = golden("inner_bnb")
    _, rho = oracle_mod.rot_radii(bunny_data10)
    for case in g["cases"]:
        prot = oracle_mod.rotate(np.array(case["R"], dtype=np.float32).reshape(3, 3), bunny_data10)
        for s in case["full"]:
            r = rho[s["level"]] if s["level"] >= 0 else None
            v, best, pops, _ = oracle_mod.inner_bnb(oracle_dt_bunny, prot, r, s["incumbent"], g["sse_threshold"])
            assert abs(v - s["value"]) <= 1e-3 * max(s["value"], 1e-3)
            assert abs(pops - s["pops"]) <= max(2, 0.01 * s["pops"])
            if s["value"] < s["incumbent"] and s["level"] < 0:
                assert np.array_equal(best, np.array(s["best"], dtype=np.float32))


def test_nn_exact(oracle_mod, bunny_model):
    g = golden("nn")
    q = np.array(g["query"], dtype=np.float32).reshape(-1, 3)
    kd = oracle_mod.KdTree(bunny_model)
    idx, d2 = kd.nn(q)
    assert np.array_equal(d2, np.array(g["dist_sq"], dtype=np.float32))   # nanoflann_goicp.hpp:1137-1184
    assert np.mean(idx == np.array(g["index"])) > 0.999                   # ties only
    bi, bd = oracle_mod.nn_brute(bunny_model, q[:256])
    assert np.array_equal(bd, d2[:256]) and np.array_equal(bi, idx[:256])


def test_kabsch_rotation(oracle_mod):
    g = golden("svd3x3")
    for c in g["cases"]:
        R = oracle_mod.kabsch_rotation(c["H"])
        assert np.abs(R - np.array(c["R"]).reshape(3, 3)).max() <= 1e-5   # jly_icp3d.hpp:268-285


def test_icp_run(oracle_mod, bunny_model, bunny_data10):
    """ICP3D<float>::Run (jly_icp3d.hpp:181-295) with forced iteration counts. 1e-4 abs on R, t
    for <= 10 iterations; the converged runs are compared at 1e-3."""
    g = golden("icp_iter")
    kd = oracle_mod.KdTree(bunny_model)
    for c in g["cases"]:
        err, R, t, it = kd.icp_run(bunny_data10, c["R0"], c["t0"], c["max_iter"], c["err_diff"])
        tol = 1e-4 if c["max_iter"] <= 10 else 1e-3
        assert np.abs(R.ravel() - np.array(c["R"])).max() <= tol
        assert np.abs(t - np.array(c["t"])).max() <= tol
        assert abs(err - c["err"]) <= 1e-3 * c["err"]
        if c["max_iter"] <= 10:
            assert it == c["max_iter"]


def test_icp_dt_score(oracle_mod, oracle_dt_bunny, bunny_data10):
    g = golden("icp_dt_score")
    sse = oracle_mod.dt_sse(oracle_dt_bunny, bunny_data10, np.array(g["R"]).reshape(3, 3), g["t"])
    assert abs(sse - g["dt_sse"]) <= 1e-4 * g["dt_sse"]                  # jly_goicp.cpp:93-132


def _check_e2e(oracle_mod, tag, model, data):
    g = golden("e2e_" + tag)
    dt = oracle_mod.DistanceTransform(model, 300, 2.0)
    r = oracle_mod.register(dt, model, data, g["mse_threshold"])
    Rg = np.array(g["R"]).reshape(3, 3)
    assert rot_angle(r["R"], Rg) <= 2e-3
    assert np.linalg.norm(r["t"] - np.array(g["t"])) <= 2e-3
    assert abs(r["sse"] - g["sse"]) <= 0.02 * g["sse"]
    assert r["sse"] < g["sse_threshold"] or g["sse"] >= g["sse_threshold"]
    return r, g


def test_e2e_rand100(oracle_mod):
    r, g = _check_e2e(oracle_mod, "rand100", cloud("model_rand"), cloud("data_rand"))
    assert r["rot_pops"] == g["rNodeCount"] and r["trans_pops"] == g["tNodeCount"]


@pytest.mark.slow
def test_e2e_bunny10(oracle_mod, bunny_model, bunny_data10):
    r, g = _check_e2e(oracle_mod, "bunny10", bunny_model, bunny_data10)
    assert r["rot_pops"] == g["rNodeCount"]
    assert abs(r["trans_pops"] - g["tNodeCount"]) <= 0.01 * g["tNodeCount"]


def _check_e2e_sub(oracle_mod, tag, model, data):
    """Strided BASELINE configs[2] / [3] (oracle/gen_golden.py --sub-configs): the optimum's DT-scored SSE can be exactly
    0 here (every strided source point lands in a seeded voxel of the dense target), so SSE is compared absolutely
    against SSEThresh rather than relatively."""
    g = golden("e2e_" + tag)
    assert len(model) == g["Nm"] and len(data) == g["Nd"]
    dt = oracle_mod.DistanceTransform(model, 300, 2.0)
    assert dt.scale == g["dt_scale"] and dt.origin == (g["dt_xmin"], g["dt_ymin"], g["dt_zmin"])
    r = oracle_mod.register(dt, model, data, g["mse_threshold"])
    assert rot_angle(r["R"], np.array(g["R"]).reshape(3, 3)) <= 2e-3
    assert np.linalg.norm(r["t"] - np.array(g["t"])) <= 2e-3
    assert abs(r["sse"] - g["sse"]) <= 0.02 * g["sse"] + 1e-3 * g["sse_threshold"]
    assert r["sse"] < g["sse_threshold"]
    assert abs(r["rot_pops"] - g["rNodeCount"]) <= max(1, 0.02 * g["rNodeCount"])
    assert abs(r["trans_pops"] - g["tNodeCount"]) <= 0.02 * g["tNodeCount"]


def test_e2e_skull_sub(oracle_mod):
    """BASELINE configs[2]: the reference's own GoICP::Register on the skull scan (98 359-point target) and every 10th
    point of the seeded known-motion source (conftest.skull_problem)."""
    from conftest import skull_problem
    target, source, Rgt, tgt = skull_problem()
    _check_e2e_sub(oracle_mod, "skull_sub", target, np.ascontiguousarray(source[::10]))
    g = golden("e2e_skull_sub")
    assert rot_angle(np.array(g["R"]).reshape(3, 3), Rgt) <= 5e-3 and np.linalg.norm(np.array(g["t"]) - tgt) <= 5e-3   # the reference recovers the motion


@pytest.mark.slow
def test_e2e_spanner_sub(oracle_mod):
    """BASELINE configs[3]: the reference's own GoICP::Register on the noisy spanner (150 000-point target) and every
    50th point of the rotated model, mse 1e-4 (92 rotation / 16 918 translation nodes)."""
    _check_e2e_sub(oracle_mod, "spanner_sub", cloud("spanner_target"), cloud("spanner_source", 50))


def test_e2e_spanner_sparse(oracle_mod):
    """BASELINE configs[3] with an SSE bar that bites: every 8th point of the noisy spanner as the target (18 750 points), every
    50th point of the rotated model, mse 3e-4.  spanner_sub's optimum scores SSE exactly 0 (so do strides 37 and 10 of the source:
    the dense noisy target seeds every voxel near the surface); here the reference's initial ICP stops in a local minimum (1.53),
    its search finds the optimum at SSE 0.10996 after 50 rotation / 3 150 translation nodes and takes the early exit."""
    g = golden("e2e_spanner_sparse")
    assert g["sse"] > 0.05                      # the point of this fixture
    _check_e2e_sub(oracle_mod, "spanner_sparse", np.ascontiguousarray(cloud("spanner_target")[::8]), cloud("spanner_source", 50))


@pytest.mark.parametrize("seed", [1, 3])
def test_e2e_tiny_proven_optimum(oracle_mod, seed):
    """The oracle on a CONVERGED search (no early exit): conftest.tiny_problem against the reference's own Register
    (tests/golden/e2e_tiny<seed>.json: 1 609 / 1 201 rotation nodes, 177 k / 108 k translation nodes) -- same optimum, node counts within 0.5 % / 1 %."""
    from conftest import tiny_problem
    tgt, src = tiny_problem(seed)
    g = golden("e2e_tiny%d" % seed)
    assert g["sse"] > g["sse_threshold"]
    dt = oracle_mod.DistanceTransform(tgt, 300, 2.0)
    assert dt.scale == g["dt_scale"]
    r = oracle_mod.register(dt, tgt, src, g["mse_threshold"])
    assert abs(r["sse"] - g["sse"]) <= 1e-5 * g["sse"]
    assert rot_angle(r["R"], np.array(g["R"]).reshape(3, 3)) <= 1e-5 and np.linalg.norm(r["t"] - np.array(g["t"])) <= 1e-5
    assert abs(r["rot_pops"] - g["rNodeCount"]) <= max(1, 0.005 * g["rNodeCount"])
    assert abs(r["trans_pops"] - g["tNodeCount"]) <= 0.01 * g["tNodeCount"]


def _second_data_set(tag):
    """(target, strided source) of the unit fixtures *_spanner.json / *_skull.json (oracle/gen_golden.py --sub-configs)."""
    if tag == "spanner":
        return cloud("spanner_target"), cloud("spanner_source", 50)
    from conftest import skull_problem
    target, source, _, _ = skull_problem()
    return target, np.ascontiguousarray(source[::10])


@pytest.mark.parametrize("tag", ["spanner", "skull"])
def test_reference_units_on_other_data_sets(oracle_mod, tag):
    """The oracle against the reference's unit fixtures on the other BASELINE data sets (the noisy spanner: 150 000 target points, every 50th
    source point; the skull scan: 98 359 target points, every 10th point of the known-motion source): DT3D::Distance samples, nanoflann
    nearest neighbours, ICP3D::Run trajectories, the DT-scored error."""
    tgt, src = _second_data_set(tag)
    dt = oracle_mod.DistanceTransform(tgt, 300, 2.0)
    g = golden("dt_lookup_" + tag)
    assert dt.scale == g["scale"] and dt.origin == (g["xmin"], g["ymin"], g["zmin"])
    q = np.array(g["query"]).reshape(-1, 3)
    ref = np.array(g["distance"], dtype=np.float32)
    mine = dt.distance(q)
    vox = 1.0 / g["scale"]
    assert np.all(mine <= ref + 1e-6) and np.max(ref - mine) <= 0.35 * vox and np.mean(mine == ref) > 0.999
    g = golden("nn_" + tag)
    kd = oracle_mod.KdTree(tgt)
    idx, d2 = kd.nn(np.array(g["query"], dtype=np.float32).reshape(-1, 3))
    assert np.array_equal(d2, np.array(g["dist_sq"], dtype=np.float32)) and np.mean(idx == np.array(g["index"])) > 0.999
    g = golden("icp_iter_" + tag)
    for c in g["cases"]:
        err, R, t, it = kd.icp_run(src, c["R0"], c["t0"], c["max_iter"], c["err_diff"])
        tol = 1e-4 if c["max_iter"] <= 10 else 1e-3
        assert np.abs(R.ravel() - np.array(c["R"])).max() <= tol and np.abs(t - np.array(c["t"])).max() <= tol
        assert abs(err - c["err"]) <= 1e-3 * c["err"]
    g = golden("icp_dt_score_" + tag)
    sse = oracle_mod.dt_sse(dt, src, np.array(g["R"]).reshape(3, 3), g["t"])
    assert abs(sse - g["dt_sse"]) <= 1e-4 * max(g["dt_sse"], 1e-3)


@pytest.mark.parametrize("tag", ["spanner", "skull"])
def test_inner_bnb_other_data_sets(oracle_mod, tag):
    """The reference's InnerBnB on the spanner DT (V = 300 over the 150 000 noisy target points, every 50th source point) and on the skull DT
    (98 359 target points, every 10th source point): single expansions (min ub + arg-min child) and full searches, as test_inner_bnb_* do on
    the bunny."""
    g = golden("inner_bnb_" + tag)
    tgt, data = _second_data_set(tag)
    assert len(data) == g["Nd"]
    dt = oracle_mod.DistanceTransform(tgt, 300, 2.0)
    _, rho = oracle_mod.rot_radii(data)
    n = 0
    for case in g["cases"]:
        prot = oracle_mod.rotate(np.array(case["R"], dtype=np.float32).reshape(3, 3), data)
        for s in case["single"]:
            r = rho[s["level"]] if s["level"] >= 0 else None
            v, best, pops, cubes = oracle_mod.inner_bnb(dt, prot, r, 1e10, 1e9, root=s["parent"])
            assert pops == s["pops"] and cubes == 8
            assert abs(v - s["min_ub"]) <= 1e-4 * max(s["min_ub"], 1e-3)
            assert np.array_equal(best, np.array(s["best"], dtype=np.float32))
            n += 1
        for s in case["full"]:
            r = rho[s["level"]] if s["level"] >= 0 else None
            v, best, pops, _ = oracle_mod.inner_bnb(dt, prot, r, s["incumbent"], g["sse_threshold"])
            assert abs(v - s["value"]) <= 1e-3 * max(s["value"], 1e-3)
            assert abs(pops - s["pops"]) <= max(2, 0.01 * s["pops"])
    assert n == 384


def test_inner_bnb_trimmed(oracle_mod, oracle_dt_bunny, bunny_data10):
    """trimFraction = 0.1 (GoICP::trimFraction set in the harness): the reference's own trimmed InnerBnB
    (jly_goicp.cpp:293-315).  Single expansions rel 1e-4 + same arg-min child; full searches: value rel
    1e-3, node pops within 1 %."""
    g = golden("inner_bnb_trim")
    k = g["inlierNum"]
    assert k == int(len(bunny_data10) * (1 - np.float32(g["trim_fraction"])))
    _, rho = oracle_mod.rot_radii(bunny_data10)
    for case in g["cases"]:
        prot = oracle_mod.rotate(np.array(case["R"], dtype=np.float32).reshape(3, 3), bunny_data10)
        for s in case["single"]:
            r = rho[s["level"]] if s["level"] >= 0 else None
            v, best, pops, cubes = oracle_mod.inner_bnb_trim(oracle_dt_bunny, prot, r, k, 1e10, 1e9, root=s["parent"])
            assert cubes == 8 and abs(v - s["min_ub"]) <= 1e-4 * max(s["min_ub"], 1e-3)
            assert np.array_equal(best, np.array(s["best"], dtype=np.float32))
        for s in case["full"]:
            r = rho[s["level"]] if s["level"] >= 0 else None
            v, best, pops, _ = oracle_mod.inner_bnb_trim(oracle_dt_bunny, prot, r, k, s["incumbent"], g["sse_threshold"])
            assert abs(v - s["value"]) <= 1e-3 * max(s["value"], 1e-3)
            assert abs(pops - s["pops"]) <= max(2, 0.01 * s["pops"])


@pytest.mark.slow
def test_oracle_trim_fixture_is_current():
    """tests/golden/e2e_bunny10_trim_oracle.json (what the GPU test of the trimmed registration compares with) is what
    the oracle computes today (~50 s of CPU)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_oracle_fixtures as G
    live, fix = G.trimmed_bunny10(), golden("e2e_bunny10_trim_oracle")
    assert np.allclose(live["R"], fix["R"], atol=1e-6) and np.allclose(live["t"], fix["t"], atol=1e-6)
    assert abs(live["sse"] - fix["sse"]) <= 1e-5 * fix["sse"]


@pytest.mark.parametrize("stride,tol", [(1, 2e-4), (10, 2e-5)])
def test_cube_bound_f64_matches_oracle(oracle_mod, oracle_dt_bunny, stride, tol):
    """oracle.cube_bound_f64 (the float64 reference of the GPU scale tests: the oracle's per-point residuals, orc_cube_terms, summed in
    float64) against the oracle's own float sums, plain and trimmed, on bunny (N = 30 379) and bunny/10: equal up to float summation
    error.  Measured worst over these 72 sums: 4.3e-5 (bunny), 4.0e-6 (bunny/10) -- the float sums in point order are the
    ones that drift."""
    data = cloud("data_bunny", stride)
    _, rho = oracle_mod.rot_radii(data)
    prot = oracle_mod.rotate(oracle_mod.rodrigues([0.3, -0.2, 0.9]), data)
    rng = np.random.default_rng(5)
    worst = 0.0
    for i in range(24):
        c = rng.uniform(-0.4, 0.4, 3).astype(np.float32)
        w = np.float32(1.0 / (1 << int(rng.integers(1, 6))))
        r = rho[(1, 5)[i % 2]] if i % 3 else None
        m = oracle_mod.cube_terms(oracle_dt_bunny, prot, r, c, w)
        assert m.shape == (len(data),) and (m >= 0).all()
        for k in (None, int(len(data) * 0.9), 1):
            fu, fl = oracle_mod.cube_bound_f64(oracle_dt_bunny, prot, r, c, w, inliers=k)
            if k is None:
                ou, ol = oracle_mod.cube_bound(oracle_dt_bunny, prot, r, c, w)
            else:
                ou, ol = oracle_mod.cube_bound_trim(oracle_dt_bunny, prot, r, c, w, k)
            dev = max(abs(ou - fu) / max(fu, 1e-3), abs(ol - fl) / max(fl, 1e-3))
            worst = max(worst, dev)
            assert dev <= tol, (i, k, ou, fu, ol, fl)
        # the k smallest: a multiset -- the first entry of the trimmed form is the smallest residual itself
        assert oracle_mod.cube_bound_f64(oracle_dt_bunny, prot, r, c, w, inliers=1)[0] == float(m.min()) ** 2
    print("cube_bound_f64 vs oracle float sums, stride %d: worst rel %.2e" % (stride, worst))
