"""The search drivers, bit for bit (engine.cpp: run_inner_device and its lanes, run_inner_host, the continuous flow, the fallbacks
between them, inner_bnb, debug_queue_expand).

The other search tests hold the drivers to tolerances (within SSEThresh, node counts within 1-5 %); a change to HOW the engine drives
the search -- not to what it computes -- has to leave the bits alone.  Every configuration below is deterministic by design (the
drivers' choices are counts, the sums are fixed-point or ordered), so its fingerprint is compared with a recording,
tests/golden/search_paths.json, field by field and with no tolerance:

  registrations    the bits of best_sse, the bytes of optR and optT, the ten Counters fields
  inner_bnb        the bits of the value, the best node's bytes, pops, cubes, fallbacks
  queue_expand     sha256 over the four output arrays of one device-queue round, and the chunk / twin info

A field the recording lists under a configuration's "unstable" was seen to differ between two recordings of the SAME commit; it is
left out of that configuration's comparison (and of nothing else).

Re-recording, after a DELIBERATE change to the search (another selection rule, another round width, another counter): check out the
commit the change is based on, build it, and run `python tools/record_search_paths.py OUT.json <that commit>` on the GPU with this
module's tables -- twice, in two processes -- and compare the two files; a field that differs between them goes into "unstable" by
hand, everything else must be identical.  Then describe in the commit message which fields moved and why.  The recording always comes
from the parent of the change, never from the code under test (the file carries the commit and its kernel source hash, for information).
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, cloud, golden, load_pkg, tiny_problem

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "search_paths.json")
COUNTERS = ("rot_pops", "trans_pops", "cubes", "inner_calls", "icp_runs", "icp_iters", "bounds_launches", "queue_fallbacks", "tile_expansions",
            "lane_batches")

# the range of test_search_range_bound_on_a_split_plane: both z bounds on depth-3 split planes of the root of width 0.5
_W = 0.5
SPLIT_PLANE = dict(use_trans_range=1, trans_min=[-_W / 2, -_W / 2, -_W / 8], trans_max=[_W / 2, _W / 2, _W / 8])

# name -> (problem, mse threshold, engine parameters)
REGISTRATIONS = {
    "tiny/defaults": ("tiny", 5e-3, {}),
    "tiny/lanes2": ("tiny", 5e-3, dict(lanes=2, lane_min_searches=2)),
    "tiny/lanes4": ("tiny", 5e-3, dict(lanes=4, lane_min_searches=2)),
    "tiny/host_queues": ("tiny", 5e-3, dict(device_queues=0)),
    "tiny/queue_cap48": ("tiny", 5e-3, dict(queue_cap=48)),
    "tiny/queue_cap512": ("tiny", 5e-3, dict(queue_cap=512)),        # single searches outgrow their slab and are re-run on the host
    "tiny/flow4": ("tiny", 5e-3, dict(flow=4)),
    "tiny/flow8_queue_cap48": ("tiny", 5e-3, dict(flow=8, queue_cap=48)),
    "tiny/narrow_children": ("tiny", 5e-3, dict(wide_children=0)),
    "tiny/reference_order_depth3": ("tiny", 5e-3, dict(trans_batch=1, wide_children=0, rot_search_depth=3)),
    "tiny/trim_flow8": ("tiny", 5e-3, dict(trim_fraction=0.1, flow=8)),
    "tiny/trim_lanes4": ("tiny", 5e-3, dict(trim_fraction=0.1, lanes=4, lane_min_searches=2)),
    "tiny/split_plane_range": ("tiny", 5e-3, SPLIT_PLANE),
    "bunny/defaults": ("bunny", 1e-3, {}),                             # sorted rounds, no tiles
    "bunny/mse1e-4": ("bunny", 1e-4, {}),                              # auto lanes, sticky tile batches
}
INNER_BNB = {"device_queues": dict(device_queues=1), "host_queues": dict(device_queues=0), "queue_cap48": dict(queue_cap=48)}
# name -> (source, nodes expanded)
# (257 points are two point chunks of 256 threads' worth: the evaluation leaves chunk partials; 200 points are one chunk: it writes the bounds itself)
QUEUE_EXPAND = {"src257/n1": (257, 1), "src257/n7": (257, 7), "src257/n128": (257, 128), "src200/n7": (200, 7), "bunny/n7": (0, 7)}


def _problem(name):
    if name == "tiny":
        return tiny_problem(1)
    return cloud("model_bunny"), cloud("data_bunny")


def _hex(a):
    return np.ascontiguousarray(a, np.float32).tobytes().hex()


def fingerprint(engine):
    """A finished FastGoICP -> the fields the fixture holds for a registration (one snapshot)"""
    r = engine.registration.poll()
    out = {"best_sse": _hex([r.best_sse]), "optR": _hex(list(r.optR)), "optT": _hex(list(r.optT))}
    out.update({k: int(getattr(r.counters, k)) for k in COUNTERS})
    return out


def run_registration(pkg, name):
    problem, mse, kw = REGISTRATIONS[name]
    tgt, src = _problem(problem)
    e = pkg.FastGoICP(tgt, src, mse, **kw)
    try:
        e.run()
        assert e.finished
        return fingerprint(e)
    finally:
        e.registration.close()


def run_inner_bnb(pkg, name):
    case = golden("inner_bnb")["cases"][0]
    full = case["full"][0]
    reg = pkg.Registration(cloud("model_bunny"), cloud("data_bunny", 10), 1e-3, **INNER_BNB[name])
    try:
        v, node, cnt = reg.inner_bnb(np.array(case["R"], np.float32), full["level"], full["incumbent"])
        return {"value": _hex([v]), "best_node": _hex(node), "trans_pops": int(cnt.trans_pops), "cubes": int(cnt.cubes),
                "queue_fallbacks": int(cnt.queue_fallbacks)}
    finally:
        reg.close()


def run_queue_expand(pkg, name):
    npts, n = QUEUE_EXPAND[name]
    src = cloud("data_bunny")
    if npts:
        src = np.ascontiguousarray(src[::118][:npts])
    reg = pkg.Registration(cloud("model_bunny"), src, 1e-3)
    try:
        # n distinct depth-3 cubes of the default translation root, in a seeded order
        cells = np.random.default_rng(5).permutation(512)[:n]
        par = np.array([[-0.5 + 0.125 * (c & 7), -0.5 + 0.125 * (c >> 3 & 7), -0.5 + 0.125 * (c >> 6), 0.125] for c in cells], np.float32)
        R = np.ascontiguousarray(pkg.fgoicp.rodrigues([0.3, -0.2, 0.9]).reshape(-1).astype(np.float32))
        out = [np.full(8 * n, -1, np.float32) for _ in range(4)]
        info = (C.c_int32 * 2)()
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        pkg.binding.check(reg._lib.goicp_debug_queue_expand(reg.handle, fp(R), 5, fp(np.ascontiguousarray(par.reshape(-1))), n,
                                                            fp(out[0]), fp(out[1]), fp(out[2]), fp(out[3]), info))
        res = {k: hashlib.sha256(a.tobytes()).hexdigest() for k, a in zip(("ub0", "lb0", "ub1", "lb1"), out)}
        res.update(chunks=int(info[0]), twins=int(info[1]))
        return res
    finally:
        reg.close()


RUNNERS = {"registrations": (REGISTRATIONS, run_registration), "inner_bnb": (INNER_BNB, run_inner_bnb), "queue_expand": (QUEUE_EXPAND, run_queue_expand)}


@pytest.fixture(scope="module")
def pkg():
    m = load_pkg()
    m.load_library()
    return m


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def _compare(recorded, kind, name, got):
    want = recorded[kind][name]
    unstable = set(recorded.get("unstable", {}).get(kind + "/" + name, []))
    assert set(got) == set(want), "%s %s: fields %s, recorded %s" % (kind, name, sorted(got), sorted(want))
    print(kind, name, got)
    for field in want:
        if field not in unstable:
            assert got[field] == want[field], "%s %s: field %s is %r, recorded %r" % (kind, name, field, got[field], want[field])


@pytest.mark.parametrize("name", list(REGISTRATIONS))
def test_registration_bits(pkg, recorded, name):
    """A whole registration through one driver configuration: result bits and all ten counters as recorded."""
    _compare(recorded, "registrations", name, run_registration(pkg, name))


def test_fallback_configurations_fall_back(recorded):
    """The recording itself: the configurations that stand for the fallback paths took them, the lane configurations cut batches."""
    r = recorded["registrations"]
    for name in ("tiny/queue_cap48", "tiny/queue_cap512", "tiny/flow8_queue_cap48"):
        assert r[name]["queue_fallbacks"] > 0, name
    for name in ("tiny/lanes2", "tiny/lanes4", "tiny/trim_lanes4", "bunny/mse1e-4"):
        assert r[name]["lane_batches"] > 0, name
    assert r["bunny/mse1e-4"]["tile_expansions"] > 0 and r["bunny/defaults"]["tile_expansions"] == 0
    assert recorded["inner_bnb"]["queue_cap48"]["queue_fallbacks"] > 0
    assert recorded["queue_expand"]["bunny/n7"]["chunks"] > 1 and recorded["queue_expand"]["bunny/n7"]["twins"] == 1
    assert recorded["queue_expand"]["src200/n7"]["chunks"] == 1


@pytest.mark.parametrize("name", list(INNER_BNB))
def test_inner_bnb_bits(pkg, recorded, name):
    """One inner search from the root (the first case of tests/golden/inner_bnb.json) through the device queues, the host queues and the
    fallback from one to the other."""
    _compare(recorded, "inner_bnb", name, run_inner_bnb(pkg, name))


@pytest.mark.parametrize("name", list(QUEUE_EXPAND))
def test_queue_expand_bits(pkg, recorded, name):
    """One device-queue round over given nodes, twin lists in use: one point chunk and several."""
    _compare(recorded, "queue_expand", name, run_queue_expand(pkg, name))
