"""CPU-side checks of batched multi-start ICP (goicp_icp_run_batch): the C ABI refuses a NULL handle, the Python wrapper refuses
mismatched shapes before it reaches the library, and the C++ shim's run_batch compiles at a call site with glm types.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg

GLM_API = os.path.join(ROOT, "tests", "glm_api")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return load_pkg()


def test_null_handle_is_invalid(pkg):
    lib = pkg.load_library()
    R = np.tile(np.eye(3, dtype=np.float32).reshape(9), 2)
    t = np.zeros(6, np.float32)
    fp = C.POINTER(C.c_float)
    rc = lib.goicp_icp_run_batch(None, 2, R.ctypes.data_as(fp), t.ctypes.data_as(fp), 10, 1e-7, None, None)
    assert rc == -1                                     # GOICP_ERR_INVALID
    assert b"goicp_icp_run_batch" in lib.goicp_last_error()


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


@pytest.mark.parametrize("R, t", [
    (np.zeros((2, 3, 3)), np.zeros((3, 3))),          # K differs
    (np.zeros((2, 3, 4)), np.zeros((2, 3))),          # not a rotation shape
    (np.zeros((2, 8)), np.zeros((2, 3))),
    (np.zeros((2, 9)), np.zeros((2, 4))),
    (np.zeros((2, 9)), np.zeros(6)),
    (np.zeros((0, 9)), np.zeros((0, 3))),             # K = 0
])
def test_wrapper_rejects_shapes_before_the_library(pkg, R, t):
    reg = pkg.fgoicp.Registration.__new__(pkg.fgoicp.Registration)
    reg._lib, reg.handle = _NoLib(), None
    with pytest.raises(ValueError):
        reg.icp_run_batch(R, t)


def test_shim_run_batch_compiles_with_glm_types(tmp_path):
    """IterativeClosestPoint3D::run_batch at a call site holding std::vector<glm::mat3> / std::vector<glm::vec3>"""
    src = tmp_path / "batch_callsite.cpp"
    src.write_text('''#include <glm/glm.hpp>
#include <vector>
#include "goicp_mi355.hpp"
using namespace goicp_mi355;
float refine_all(const icp::Registration& reg, std::vector<glm::mat3>& R, std::vector<glm::vec3>& t)
{
    icp::IterativeClosestPoint3D icp(reg, 100, 1e-7f, glm::mat3(1.0f), glm::vec3(0.0f));
    std::vector<int32_t> iters;
    std::vector<float> err = icp.run_batch(R, t, &iters);
    return err.empty() ? 0.f : err[0] + (float)iters[0];
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DSHIM_WITH_GLM", "-I", os.path.join(ROOT, "include"), "-I", GLM_API, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
