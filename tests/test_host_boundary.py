"""CPU-side tests of the boundary: the C-ABI library loads and exports every symbol
include/goicp_mi355.h declares, config / cloud loading mirror the reference's behaviour, and the
product fails loudly (no CPU fallback) when no GPU is present.  No compute calls here."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_pkg


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def test_header_symbols_all_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "goicp_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(goicp_[a-z0-9_]+)\s*\(", hdr))
    from cuda_go_icp_amd import binding
    lib = pkg.load_library()
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), "symbol %s declared in the header but not exported" % name
    assert declared == set(binding.SYMBOLS), (declared ^ set(binding.SYMBOLS))
    assert lib.goicp_abi_version() == 4


def test_struct_sizes_match_abi(pkg):
    from cuda_go_icp_amd import binding as B
    import ctypes as C
    assert C.sizeof(B.CCube) == 24
    assert C.sizeof(B.CCounters) == 80
    assert C.sizeof(B.CStepStatus) == 24
    assert C.sizeof(B.CResult) == 4 * (9 + 3 + 9 + 3 + 1 + 1) + 80 + 16


CFG = """# comment
[info]
description = "Register data # not a comment"   # trailing comment

[io]
target = "../data/bunny/model_bunny.txt"
source = '../data/bunny/data_bunny.txt'
output = "output.toml"

[params]
mode = 4
trim = true
subsample = 1.7          # clamped to 1
mse_threshold = 1e-12    # clamped to 1e-10
resize = 0.01
authors = ["a",
           "b"]

[params.rotation]
xmin = -90
search_depth = 7

[visualization]
theta = 0.5
spin_after_finish = true
"""


def test_config_parse_defaults_and_clamps(pkg, tmp_path):
    p = tmp_path / "c.toml"
    p.write_text(CFG)
    c = pkg.Config(p)
    assert c.mode == 4 and c.trim is True
    assert c.subsample == 1.0                                   # src/common.cpp:63
    assert c.mse_threshold == pytest.approx(1e-10)               # src/common.cpp:64
    assert c.resize == pytest.approx(0.01)
    assert c.io.target.endswith("model_bunny.txt") and c.io.source.endswith("data_bunny.txt")
    assert c.io.output == "output.toml" and c.io.visualization == ""
    assert c.viz.theta == 0.5 and c.viz.phi == pytest.approx(0.4) and c.viz.spin_after_finish
    assert c.rotation.xmin == -90 and c.rotation.xmax == 180 and c.rotation.search_depth == 7
    assert c.description == "Register data # not a comment"


def _reference_style_toml(want):
    """A config in the layout of the reference's test/*.toml (header comment, [info] with an authors array, quoted [io] paths and
    [params] values with trailing comments, the optional [params.rotation] / [params.translation] tables, [visualization]),
    holding the values of one entry of tests/golden/reference_configs.json."""
    q = lambda s: '"%s"' % s
    b = lambda v: "true" if v else "false"
    lines = ["# Example configuration (reference layout)", "", "[info]", 'authors = ["A. Author",', '           "B. Author"]',
             'version = "0.1"', "description = %s" % q(want["description"]), "", "[io]",
             "target = %s    # target (reference) point cloud" % q(want["target"]), "source = %s     # source point cloud" % q(want["source"]),
             "output = %s                      # output file: R, t, MSE" % q(want["output"]),
             "visualization = %s                   # set to \"\" to skip" % q(want["visualization"]), "", "[params]",
             "mode = %d                                  # 0..4" % want["mode"], "trim = %s" % b(want["trim"]),
             "subsample = %r                             # subsample the source point cloud" % want["subsample"],
             "mse_threshold = %r" % want["mse_threshold"], "resize = %r" % want["resize"]]
    for key in ("rotation", "translation"):
        if want[key + "_present"]:
            r = want[key]
            lines += ["", "[params.%s]" % key] + ["%s = %r" % (k, v) for k, v in zip(("xmin", "xmax", "ymin", "ymax", "zmin", "zmax"), r[:6])]
            lines += ["search_depth = %d" % r[6]]
    lines += ["", "[visualization]", "theta = %r" % want["theta"], "phi = %r" % want["phi"], "spin_after_finish = %s" % b(want["spin_after_finish"]), ""]
    return "\n".join(lines)


def test_reference_configs_parse(pkg, tmp_path):
    """The reference's five configs (test/*.toml, e.g. test/skull_goicp.toml:16-41), restated in their layout from the committed
    expectation table (tests/golden/reference_configs.json, written from reading the files), go through goicp_config_load and
    give the table's values: [io] paths, [params] mode / trim / subsample / mse_threshold / resize, [visualization], and the
    [params.rotation] / [params.translation] / search_depth keys the reference declares but never parses (src/common.h:157-169)."""
    import json
    table = json.load(open(os.path.join(GOLDEN, "reference_configs.json")))
    assert sorted(table) == ["bunny_goicp.toml", "bunny_icp.toml", "face_goicp.toml", "skull_goicp.toml", "spanner_goicp.toml"]
    for name, want in table.items():
        (tmp_path / name).write_text(_reference_style_toml(want))
        c = pkg.Config(tmp_path / name)
        assert (c.mode, bool(c.trim), c.description) == (want["mode"], want["trim"], want["description"]), name
        for k in ("subsample", "mse_threshold", "resize"):
            assert getattr(c, k) == pytest.approx(want[k], rel=1e-6), (name, k)
        assert (c.io.target, c.io.source, c.io.output, c.io.visualization) == (want["target"], want["source"], want["output"], want["visualization"])
        assert c.viz.theta == pytest.approx(want["theta"], rel=1e-6) and c.viz.phi == pytest.approx(want["phi"], rel=1e-6)
        assert bool(c.viz.spin_after_finish) == want["spin_after_finish"]
        for sect, key in ((c.rotation, "rotation"), (c.translation, "translation")):
            assert [sect.xmin, sect.xmax, sect.ymin, sect.ymax, sect.zmin, sect.zmax, sect.search_depth] == want[key], (name, key)
            assert bool(sect.present) == want[key + "_present"], (name, key)


def test_config_errors(pkg, tmp_path):
    with pytest.raises(pkg.GoicpError) as e:
        pkg.Config(tmp_path / "missing.toml")
    assert e.value.code == -3
    p = tmp_path / "bad.toml"
    p.write_text("[info]\ndescription = \"x\"\n[params\nmode = 1\n")
    with pytest.raises(pkg.GoicpError):
        pkg.Config(p)
    p.write_text("[params]\nmode = 1\n")                       # reference: bad_optional_access on info.description
    with pytest.raises(pkg.GoicpError):
        pkg.Config(p)
    p.write_text("[info]\ndescription = \"d\"\n")              # no [params]: defaults
    c = pkg.Config(p)
    assert c.mode == 1 and c.subsample == 1.0 and c.mse_threshold == pytest.approx(1e-5) and c.resize == 1.0


def _write_ply(path, pts, binary, crlf=False, extra=False):
    nl = "\r\n" if crlf else "\n"
    hdr = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment test",
           "element vertex %d" % len(pts), "property float x", "property float y", "property float z"]
    if extra:
        hdr += ["property uchar red", "property uchar green", "property uchar blue"]
    hdr += ["element face 1", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write((nl.join(hdr) + nl).encode())
        for p in pts:
            if binary:
                f.write(np.asarray(p, "<f4").tobytes() + (bytes([1, 2, 3]) if extra else b""))
            else:
                f.write((" ".join("%.9g" % v for v in p) + (" 1 2 3" if extra else "") + "\n").encode())
        f.write(bytes([3]) + np.array([0, 1, 2], "<i4").tobytes() if binary else b"3 0 1 2\n")


@pytest.mark.parametrize("binary,crlf,extra", [(False, False, False), (True, True, True), (True, False, False), (False, True, True)])
def test_load_cloud_ply(pkg, tmp_path, binary, crlf, extra):
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(257, 3)).astype(np.float32)
    p = tmp_path / "c.PLY"                                        # extension match is case-insensitive
    _write_ply(p, pts, binary, crlf, extra)
    out = pkg.load_cloud(p, 1.0, 2.0)
    assert out.shape == (257, 3) and np.array_equal(out, np.float32(2.0) * pts)


def test_load_cloud_txt_and_subsample(pkg, tmp_path):
    pts = np.fromfile(os.path.join(GOLDEN, "data_rand.f32"), dtype="<f4").reshape(-1, 3)
    p = tmp_path / "c.txt"
    with open(p, "w") as f:
        f.write("%d\n" % len(pts))
        for q in pts:
            f.write("%.9g %.9g %.9g\n" % tuple(q))
    assert np.array_equal(pkg.load_cloud(p, 1.0, 1.0), pts)
    a = pkg.load_cloud(p, 0.5, 1.0, seed=42)
    b = pkg.load_cloud(p, 0.5, 1.0, seed=42)
    assert np.array_equal(a, b) and 0 < len(a) <= 50              # capped at floor(N*s) (src/common.cpp:167)
    assert len(pkg.load_cloud(p, 0.0, 1.0, seed=1)) == 0


def test_load_cloud_errors(pkg, tmp_path):
    for name in ("nope.ply", "nope.txt", "noext", "cloud.xyz"):
        with pytest.raises(pkg.GoicpError) as e:
            pkg.load_cloud(tmp_path / name)
        assert e.value.code == -2
    p = tmp_path / "short.txt"
    p.write_text("5\n0 0 0\n1 1 1\n")
    with pytest.raises(pkg.GoicpError):
        pkg.load_cloud(p)
    p = tmp_path / "noxyz.ply"
    p.write_text("ply\nformat ascii 1.0\nelement vertex 1\nproperty float a\nend_header\n0\n")
    with pytest.raises(pkg.GoicpError):
        pkg.load_cloud(p)


def test_no_cpu_fallback(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    pts = np.random.default_rng(0).normal(size=(50, 3)).astype(np.float32)
    with pytest.raises(pkg.GoicpError) as e:
        pkg.Registration(pts, pts)
    assert e.value.code == -4 and "no CPU fallback" in str(e.value)


def test_rodrigues_host_helper_matches_oracle(pkg, oracle_mod):
    rng = np.random.default_rng(1)
    for v in rng.uniform(-3, 3, (50, 3)):
        assert np.array_equal(pkg.fgoicp.rodrigues(v), oracle_mod.rodrigues(v))
    assert np.array_equal(pkg.fgoicp.rodrigues([0, 0, 0]), np.eye(3, dtype=np.float32))


# ----------------------------------------------------------------------------------------------
# C++ shim (include/goicp_mi355.hpp): the reference's call sites compile against it
# ----------------------------------------------------------------------------------------------
SHIM_TU = os.path.join(ROOT, "tests", "shim_callsites.cpp")


GLM_API = os.path.join(ROOT, "tests", "glm_api")     # stand-in for glm 0.9.6's vec3 / mat3 interface, used when no glm is found


def _glm_include_flags():
    """-I flags for glm: a real glm (GLM_INCLUDE_DIR, else the compiler's own search path) when `#include <glm/glm.hpp>`
    compiles with it, else the stand-in under tests/glm_api."""
    import subprocess
    extra = ["-I", os.environ["GLM_INCLUDE_DIR"]] if os.environ.get("GLM_INCLUDE_DIR") else []
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++"] + extra + ["-"], input="#include <glm/glm.hpp>\n",
                       capture_output=True, text=True)
    return extra if r.returncode == 0 else ["-I", GLM_API]


def _syntax_only(extra):
    import subprocess
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include")] + extra + [SHIM_TU],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_shim_compiles_without_glm():
    """The shim's own layout-compatible Mat3 / Vec3 (column-major, m[col][row]) carry the same call shapes."""
    _syntax_only([])


def test_shim_compiles_against_reference_glm():
    """the call shapes of src/main.cpp:94,150 (FastGoICP construction from std::vector<glm::vec3>, worker
    thread on &FastGoICP::run), src/goicp_kernel.cu:161-177 (the viewer's locked read of optR/optT/curR/curT/finished/
    get_best_error with glm::mat3 / glm::vec3 on the other side), src/icp_kernel.h:9-13 / src/goicp_kernel.h:6-10 (the
    step API) and src/fgoicp/registration.hpp:96-97, icp3d.hpp:30-35 (the operators) compile against the shim with glm types
    on the caller's side: the glm the reference vendors (0.9.6) when one is installed or named by GLM_INCLUDE_DIR, else the
    stand-in tests/glm_api with that version's vec3 / mat3 interface.  Either way the shim takes its glm branch (Mat3 / Vec3 ARE
    glm::mat3 / glm::vec3), so `prev_optR = f->optR` only compiles if that branch holds."""
    _syntax_only(["-DSHIM_WITH_GLM"] + _glm_include_flags())


def test_shim_matrix_layout_roundtrip(tmp_path):
    """to_rows / from_rows: glm-style column-major <-> the C ABI's row-major float[9] (host-only program)."""
    import subprocess
    src = tmp_path / "rt.cpp"
    src.write_text('''#include "goicp_mi355.hpp"
#include <cstdio>
using namespace goicp_mi355;
int main() {
    float r[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9}, back[9];
    Mat3 M = from_rows(r);
    if (M[1][0] != 2.f || M[0][1] != 4.f || M[2][1] != 6.f) return 1;      // m[col][row]
    to_rows(M, back);
    for (int i = 0; i < 9; i++) if (back[i] != r[i]) return 2;
    icp::RotNode n(0.f, 0.f, 0.f, 3.1415926536f / 8, 0.f, 0.f);
    if (n.level() != 3) return 3;
    std::puts("ok");
    return 0;
}''')
    exe = tmp_path / "rt"
    lib_dir = os.path.join(ROOT, "cuda-go-icp_amd")
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib_dir, "-lgoicp_mi355",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_environment_reads_are_the_allowed_ones():
    """The engine's behaviour comes from goicp_params alone: the library reads no tuning or A/B switch from the environment.
    The only reads are the roctx switch (trace.hpp), the communicator's time-out (shard.cpp) and TMPDIR (host_selftest.cpp)."""
    import glob
    csrc = os.path.join(ROOT, "cuda-go-icp_amd", "csrc")
    names = set()
    for path in sorted(glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.hpp")) + glob.glob(os.path.join(csrc, "*.hip"))):
        names |= set(re.findall(r'getenv\s*\(\s*"([^"]*)"', open(path).read()))
    assert names == {"GOICP_ROCTX", "GOICP_COMM_TIMEOUT_MS", "TMPDIR"}, sorted(names)


# ----------------------------------------------------------------------------------------------
# sanitizer builds: CPU only
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,target", [("oracle", "asan"), (os.path.join("cuda-go-icp_amd", "csrc"), "asan"),
                                          (os.path.join("cuda-go-icp_amd", "csrc"), "tsan")])
def test_sanitizer_targets(where, target):
    """`make asan` (AddressSanitizer + UBSan) on the oracle and on the library's host-only translation units (sharding
    protocol + in-process communicator, threaded k-d build, TOML/PLY/TXT IO), `make tsan` (ThreadSanitizer) on the
    latter: several ranks as host threads through csrc/shard.cpp.  Never run on the GPU box."""
    import subprocess
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, where), target], capture_output=True, text=True, timeout=900)
    if r.returncode != 0 and "unexpected memory mapping" in (r.stdout + r.stderr):
        pytest.skip("ThreadSanitizer cannot map its shadow memory in this sandbox")
    assert r.returncode == 0 and "selftest: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
