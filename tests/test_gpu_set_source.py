"""goicp_set_source: handle A is created with (T, S0) and swapped to S1, handle B is created with (T, S1) and given the same per-handle
options -- and every answer of the C ABI must be the same BYTES: cube bounds, pose scores, the transformed source, thresholds, single and
batched ICP, correspondences, pose information, one inner search, an ICP step and a whole registration with its polled snapshot (the two
wall-clock fields masked, the counters equal).  A is used before the swap (a finished registration, ICP runs, a warm neighbour cache), so
state that survived the swap would show.  An operator that refuses (pose information on a trimmed handle) must refuse on both.

Clouds: subsamples of tests/golden/data_bunny.f32 against every 20th point of model_bunny.f32, dt_size 48: a registration takes a fraction
of a second.  Growth 37 -> 2 000, shrink 2 000 -> 5 (a stale tail of 1 995 points behind the live 5), and a swap back."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, cloud, load_pkg

pytestmark = pytest.mark.gpu
INVALID = -1
DT = 48


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@functools.lru_cache(maxsize=None)
def target():
    t = cloud("model_bunny", 20)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def source(n):
    d = cloud("data_bunny")
    s = np.ascontiguousarray(d[np.linspace(0, len(d) - 1, n).astype(np.int64)])
    s.setflags(write=False)
    return s


def _rot(v):
    load_pkg()
    from cuda_go_icp_amd import fgoicp
    return fgoicp.rodrigues(v)


@functools.lru_cache(maxsize=None)
def _cubes():
    rng = np.random.default_rng(5)
    c = np.concatenate([rng.uniform(-0.3, 0.3, (64, 3)), np.full((64, 1), 0.125)], 1).astype(np.float32)
    c.setflags(write=False)
    return c


def _try(pkg, fn):
    """the operator's answer, or the status it refused with: a refusal must be the same on both handles"""
    try:
        return fn()
    except pkg.GoicpError as e:
        return ("refused", getattr(e, "code", None) if getattr(e, "code", None) is not None else str(e)[:40])


def _poll_bytes(reg):
    r = reg.poll()
    cnt = tuple(getattr(r.counters, k) for k, _ in r.counters._fields_)
    return (bytes(bytearray(np.array(list(r.optR) + list(r.optT) + list(r.curR) + list(r.curT) + [r.best_sse], np.float32).tobytes())), int(r.finished), cnt)


def fingerprint(pkg, reg, register=True):
    """every answer the issue lists, as bytes / ints, in a fixed order of calls"""
    lib = reg._lib
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    R1, R2 = _rot([0.3, -0.2, 0.9]), _rot([-1.1, 0.4, 0.2])
    t1 = np.array([0.02, -0.03, 0.01], np.float32)
    out = {}
    thr, inl = C.c_float(), C.c_int32()
    assert lib.goicp_thresholds(reg.handle, C.byref(thr), C.byref(inl)) == 0
    out["thresholds"] = (np.float32(thr.value).tobytes(), inl.value)
    out["poll0"] = _poll_bytes(reg)
    for name, R, level in (("bounds_R1_fix", R1, -1), ("bounds_R2_fix", R2, -1), ("bounds_R1_l3", R1, 3)):
        ub, lb = reg.eval_bounds(R, _cubes(), level)
        out[name] = (ub.tobytes(), lb.tobytes())
    sse = C.c_float()
    assert lib.goicp_eval_sse(reg.handle, R1.ctypes.data_as(C.POINTER(C.c_float)), t1.ctypes.data_as(C.POINTER(C.c_float)), C.byref(sse)) == 0
    out["sse"] = np.float32(sse.value).tobytes()
    out["transform"] = reg.transform_source(R1, t1).tobytes()

    def icp():
        it = pkg.IterativeClosestPoint3D(reg, 40, 1e-7)
        err, R, t = it.run()
        return (np.float32(err).tobytes(), R.tobytes(), t.tobytes(), it.iters)
    out["icp_run"] = _try(pkg, icp)
    out["icp_inliers"] = _try(pkg, lambda: reg.icp_inliers(1).tobytes())

    def batch():
        Rs = np.stack([I, R1, _rot([0.05, 0.02, -0.04])])
        ts = np.stack([z, t1, z])
        R, t, err, it = reg.icp_run_batch(Rs, ts, 40, 1e-7)
        return (R.tobytes(), t.tobytes(), err.tobytes(), it.tobytes())
    out["icp_batch"] = _try(pkg, batch)

    def corr():
        idx, d2, n, s = reg.eval_correspondences(R1, t1, 0.05)
        return (idx.tobytes(), d2.tobytes(), n, np.float32(s).tobytes())
    out["correspondences"] = _try(pkg, corr)

    def info():
        d = reg.pose_information(I, z)
        return tuple(np.asarray(d[k]).tobytes() for k in sorted(d))
    out["pose_information"] = _try(pkg, info)

    def inner():
        v, node, cnt = reg.inner_bnb(R1, -1, 1e10)
        return (np.float32(v).tobytes(), None if node is None else node.tobytes(), cnt.trans_pops, cnt.cubes)
    out["inner_bnb"] = _try(pkg, inner)
    reg.icp_step()
    out["icp_step"] = _poll_bytes(reg)
    if register:
        assert lib.goicp_register(reg.handle) == 0, lib.goicp_last_error()
        out["register"] = _poll_bytes(reg)
        assert out["register"][1] == 1
        out["result_information"] = _try(pkg, lambda: tuple(np.asarray(v).tobytes() for _, v in sorted(reg.result_information().items())))
    return out


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], (tag, k)


VARIANTS = {
    "default": (dict(), None),
    "plane_gate": (dict(), lambda r: (r.set_icp_options(1, 8), r.set_icp_gate(0.08))),
    "trim": (dict(trim_fraction=0.1), None),
    "morton0": (dict(morton_sort=0), None),
    "morton1": (dict(morton_sort=1), None),
    "nn_cache": (dict(icp_nn_cache=1), None),
}


def _make(pkg, n, variant):
    kw, opts = VARIANTS[variant]
    r = pkg.Registration(target(), source(n), 1e-3, dt_size=DT, **kw)
    if opts:
        opts(r)
    return r


@functools.lru_cache(maxsize=None)
def fresh_fingerprint(n, variant):
    """handle B: created with (T, S_n), the variant's options applied -- computed once per (n, variant), shared, never changed"""
    pkg = load_pkg()
    b = _make(pkg, n, variant)
    try:
        return fingerprint(pkg, b)
    finally:
        b.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_swapped_handle_equals_fresh_handle(pkg, variant):
    """500 -> 2 000 points; the options were set BEFORE the swap (they persist, the normals are not rebuilt) and A was used before it"""
    a = _make(pkg, 500, variant)
    try:
        assert_same(fingerprint(pkg, a), fresh_fingerprint(500, variant), variant + " before the swap")
        a.set_source(source(2000))
        assert a.ns == 2000
        assert_same(fingerprint(pkg, a), fresh_fingerprint(2000, variant), variant + " after the swap")
    finally:
        a.close()


def test_growth_shrink_and_return(pkg):
    a = _make(pkg, 37, "default")
    try:
        fingerprint(pkg, a)
        a.set_source(source(2000))                               # growth: every N-sized buffer is reallocated
        assert_same(fingerprint(pkg, a), fresh_fingerprint(2000, "default"), "37 -> 2000")
        a.set_source(source(5))                                  # shrink: 1 995 stale points behind the live ones
        assert_same(fingerprint(pkg, a), fresh_fingerprint(5, "default"), "2000 -> 5")
        a.set_source(source(500))
        a.set_source(source(37))                                 # two swaps in a row, back to the first cloud
        assert_same(fingerprint(pkg, a), fresh_fingerprint(37, "default"), "back to 37")
    finally:
        a.close()


def test_swap_across_the_sorted_round_sizes(pkg):
    """from 12 288 points on a lane sorts the items of its large rounds by chunk centroids of the SOURCE: a swap 2 000 -> 15 000 has to build
    that set-up (and the scratch sized by it), the swap back has to drop it"""
    a = _make(pkg, 2000, "default")
    try:
        fingerprint(pkg, a)
        a.set_source(source(15000))
        assert_same(fingerprint(pkg, a), fresh_fingerprint(15000, "default"), "2000 -> 15000")
        a.set_source(source(2000))
        assert_same(fingerprint(pkg, a), fresh_fingerprint(2000, "default"), "15000 -> 2000")
    finally:
        a.close()


def test_shrink_with_trimming_and_cache(pkg):
    """the trimmed-ICP buffers and the neighbour cache across a shrink and a growth"""
    for variant in ("trim", "nn_cache"):
        a = _make(pkg, 2000, variant)
        try:
            fingerprint(pkg, a, register=False)
            a.set_source(source(37))
            a.set_source(source(500))
            assert_same(fingerprint(pkg, a), fresh_fingerprint(500, variant), variant)
        finally:
            a.close()


def test_refusals_leave_the_handle_as_it_was(pkg):
    lib = pkg.load_library()
    fp = C.POINTER(C.c_float)
    a = _make(pkg, 500, "default")
    try:
        good = source(2000)
        bad = np.array(good)
        bad[1234, 2] = np.nan
        assert lib.goicp_set_source(a.handle, bad.ctypes.data_as(fp), len(bad)) == INVALID and b"non-finite" in lib.goicp_last_error()
        bad[1234, 2] = np.inf
        assert lib.goicp_set_source(a.handle, bad.ctypes.data_as(fp), len(bad)) == INVALID
        assert lib.goicp_set_source(a.handle, good.ctypes.data_as(fp), 0) == INVALID
        assert lib.goicp_set_source(a.handle, None, 2000) == INVALID
        assert lib.goicp_set_source(a.handle, good.ctypes.data_as(fp), (2 ** 31 - 1) // 8 + 1) == INVALID     # refused before a byte is read
        # between register_begin and register_end
        assert lib.goicp_register_begin(a.handle) == 0
        assert lib.goicp_set_source(a.handle, good.ctypes.data_as(fp), len(good)) == INVALID and b"registration runs" in lib.goicp_last_error()
        assert lib.goicp_register_end(a.handle) == 0
        assert a.ns == 500
        b = _make(pkg, 500, "default")                           # the same history without the refused calls
        try:
            assert lib.goicp_register_begin(b.handle) == 0 and lib.goicp_register_end(b.handle) == 0
            assert_same(fingerprint(pkg, a), fingerprint(pkg, b), "after the refusals")
        finally:
            b.close()
        assert lib.goicp_set_source(a.handle, good.ctypes.data_as(fp), len(good)) == 0                         # and a good swap still works
        a.ns, a.pcs = len(good), good
        assert_same(fingerprint(pkg, a), fresh_fingerprint(2000, "default"), "good swap after the refusals")
    finally:
        a.close()


def test_fastgoicp_set_source(pkg):
    """FastGoICP.set_source: the mirrored fields are the fresh handle's, and the next run is the fresh engine's"""
    eng = pkg.FastGoICP(target(), source(500), 1e-3, dt_size=DT)
    ref = pkg.FastGoICP(target(), source(2000), 1e-3, dt_size=DT)
    try:
        eng.run()
        assert eng.finished
        eng.set_source(source(2000))
        assert not eng.finished and np.array_equal(eng.optR, np.eye(3, dtype=np.float32)) and eng.get_best_error() == np.float32(1e10)
        assert eng.sse_threshold == ref.sse_threshold and eng.registration.ns == 2000
        with pytest.raises(pkg.GoicpError):
            eng.information()                                    # no finished registration on the new cloud
        eng.run(); ref.run()
        assert eng.get_best_error().tobytes() == ref.get_best_error().tobytes()
        assert eng.optR.tobytes() == ref.optR.tobytes() and eng.optT.tobytes() == ref.optT.tobytes()
        assert tuple(getattr(eng.counters, k) for k, _ in eng.counters._fields_) == tuple(getattr(ref.counters, k) for k, _ in ref.counters._fields_)
    finally:
        eng.registration.close(); ref.registration.close()


def test_shim_call_site_runs(pkg, tmp_path):
    """tests/shim_set_source.cpp as a program: icp::FastGoICP::set_source between two runs ends on the bits of a fresh engine (exit status 0)"""
    libdir = os.path.dirname(pkg.library_path())
    exe = str(tmp_path / "shim_set_source")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DSHIM_SET_SOURCE_MAIN", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_set_source.cpp"),
                        "-o", exe, "-L", libdir, "-lgoicp_mi355", "-Wl,-rpath," + libdir, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "model_bunny.f32"), os.path.join(g, "data_bunny.f32")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "swapped" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_source_list(pkg, tmp_path):
    """goicp_cli --source-list: the listed cloud is swapped into the config's engine and registered; its line and its numbered outputs are
    those of a run of its own on that cloud (the swapped engine is a fresh one, bit for bit: the same %.7g error and node count)"""
    def write(name, pts):
        with open(tmp_path / (name + ".txt"), "w") as f:
            f.write("%d\n" % len(pts))
            for q in pts:
                f.write("%.9g %.9g %.9g\n" % tuple(q))
    write("model", cloud("model_rand"))
    write("scan0", cloud("data_rand")[:60])
    write("scan1", cloud("data_rand"))
    cfg = ('[info]\ndescription = "source list"\n[io]\ntarget = "model.txt"\nsource = "%s.txt"\noutput = "%s"\nvisualization = "%s"\n'
           '[params]\nmode = 4\nsubsample = 1.0\nmse_threshold = 1e-3\nresize = 1.0\n')
    (tmp_path / "cfg.toml").write_text(cfg % ("scan0", tmp_path / "out.toml", tmp_path / "viz.ply"))
    (tmp_path / "own.toml").write_text(cfg % ("scan1", tmp_path / "own_out.toml", tmp_path / "own_viz.ply"))
    (tmp_path / "scans.lst").write_text("# one more scan, beside the list\nscan1.txt\n")
    exe = os.path.join(ROOT, "cuda-go-icp_amd", "goicp_cli")
    out = subprocess.run([exe, str(tmp_path / "cfg.toml"), "--source-list", str(tmp_path / "scans.lst")], check=True, capture_output=True, text=True, timeout=120).stdout
    own = subprocess.run([exe, str(tmp_path / "own.toml")], check=True, capture_output=True, text=True, timeout=120).stdout
    line = [l for l in out.splitlines() if l.startswith("source 1 (")]
    assert len(line) == 1 and "swap " in line[0] and " ms" in line[0] and "%d points" % len(cloud("data_rand")) in line[0], out
    best_own = [l for l in own.splitlines() if l.startswith("Searching over!")][0].split("Best Error:")[1].split()[0]
    rot_own = [l for l in own.splitlines() if l.startswith("Total Rotation Nodes Searched")][0].split(":")[1].strip()
    assert "Best Error: %s," % best_own in line[0] and line[0].endswith("rotation nodes " + rot_own), (line[0], own)
    keep = lambda p: [l for l in (tmp_path / p).read_text().splitlines() if "_ms" not in l]      # the two wall-clock fields
    assert (tmp_path / "out.toml").exists() and keep("out.1.toml") == keep("own_out.toml")
    assert np.array_equal(pkg.load_cloud(tmp_path / "viz.1.ply"), pkg.load_cloud(tmp_path / "own_viz.ply"))
