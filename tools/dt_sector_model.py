#!/usr/bin/env python3
"""CPU model of the vector-cache tag lookups the headline batch makes in the lean sibling path (device.hip lean_points).

The cache looks up one tag per distinct 64-B sector that a group of lanes (a quad by default) touches in one load instruction.
This tool rebuilds the bench batch (bench.make_batch, seed 1234: rotations, corners, widths), the source cloud in the engine's
k-d order (engine.cpp, morton_sort 2) and the DT geometry (dt_expand 2, V 300), forms every voxel index the kernel forms (float
index path; lanes outside the grid are left out) and counts, per layout:
  * tags per DT gather instruction (8 dword gathers per point),
  * tags per VMEM instruction, the float4 point load (16 tags per wavefront) included,
  * with --merged: the same for 16-B x-row loads when the x siblings are less than 4 voxels apart (one row load per (y, z) pair,
    a masked dword load for the lanes whose second x lies in the next row),
  * the distinct sectors one lane's 8 sibling lookups hit, per child spacing.
Layouts: 4x4x1 / 4x2x2 / 2x2x4 / 2x4x2 (64-B sector shape, x y z, inside 4x4x4 bricks of 256 B) or linear.

  python3 tools/dt_sector_model.py [--layouts 4x4x1,4x2x2,...] [--lanes 4] [--every 16] [--merged] [--json out.json]

--lines: the 128-B LINES (two sectors of a brick) instead of the tags -- what the L1 asks the L2 for.  Distinct lines per wavefront iteration
(64 points x 8 children), per workgroup iteration (256 points: the sum over its four wavefronts and their union) and per (expansion, chunk)
item; then, for windows of consecutive expansions of one rotation run, union / sum of their line sets over the same points -- 5 expansions
over 256 points, 20 over 1 024, a PAIR over 64 and over 256 -- in the order the batch arrives in and in the order of bounds_order_kernel
(device.hip: Morton cell of the parent cube's centre, 5 bits per axis over the run's extent, cells of at least --cell voxels), and the median
distance in voxels between the centres of consecutive expansions.

  python3 tools/dt_sector_model.py --lines [--cell 4] [--every 16] [--json out.json]

--lines --keys: the same windows for other keys of the order (KEY_VARIANTS below: a cell floor of 2 voxels, 10 bits per axis over quarter-voxel
cells, the expansion's depth between a coarse and a fine Morton cell, the depth first), and the share of the order's pairs (2 i, 2 i + 1)
whose members have the same depth.

  python3 tools/dt_sector_model.py --lines --keys [--json profiles/r07_order_keys_model.json]

--twins: the COINCIDENT items of the pair launch (bounds_pair_kernel: both members of an item with the same six translations and delta,
bit for bit) when the order inside a Morton cell is random, for the bench batch and for a batch shaped like the two inner searches of a
rotation child (search_shaped_batch): items any order could give at most (floor(family / 2) per family of equal expansions in a run), the
items --trials random tie orders capture (mean, min, max), and how many two-member families share their cell with anything else.  Beside
them ("dedup", dedup_mode) the COPIES the pre-pass finds (bounds_order_kernel's alias table: a full group whose eight records repeat another
group's of its run as raw bytes): groups, distinct groups per run, and the sets of eight gathers per point chunk before and after.

  python3 tools/dt_sector_model.py --twins [--trials 200] [--json profiles/r08_twin_tie_order_model.json | profiles/r12_dedup_model.json]

--chunks: what each of the pair launch's eight point chunks costs: distinct 128-B lines per 64-lane gather and the chunk's share of the lines,
over random rotations x 12 sibling expansions; the spread of that share over the rotations; the same at the identity pose; and the device's
own per-chunk cost (bounds_chunk_cost_kernel), as goicp_debug_bounds_balance and tools/xcd_balance_probe.py report it.

  python3 tools/dt_sector_model.py --chunks [--rotations 8] [--seed 0] [--json profiles/r09_chunk_cost_model.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kd_order(src):
    """engine.cpp's k-d order (morton_sort 2): longest-axis median splits, left part a multiple of 256/64/16/4/1, down to single points"""
    perm = np.arange(len(src))
    stack = [(0, len(src))]
    while stack:
        lo, hi = stack.pop()
        n = hi - lo
        if n <= 1:
            continue
        sub = perm[lo:hi]
        pts = src[sub]
        ax = int(np.argmax(pts.max(0) - pts.min(0)))          # first axis of the largest extent, as the engine's strict '>'
        unit = 256 if n > 256 else 64 if n > 64 else 16 if n > 16 else 4 if n > 4 else 1
        nl = ((n // 2 + unit // 2) // unit) * unit
        if nl == 0:
            nl = unit
        if nl >= n:
            nl = n - (n % unit if n % unit else unit)
        order = np.lexsort((sub, pts[:, ax]))                 # (value, index): the engine's total order
        perm[lo:hi] = sub[order]
        stack.append((lo + nl, hi))
        stack.append((lo, lo + nl))
    return perm


def dt_geometry(model, V=300, expand=2.0):
    mn, mx = model.astype(np.float64).min(0), model.astype(np.float64).max(0)
    c = (mn + mx) / 2
    lo, hi = c - expand * (mx - c), c + expand * (mx - c)
    side = (hi - lo).max()
    return (c - side / 2).astype(np.float32), np.float32(V / side)


def element_index(x, y, z, V, layout):
    if layout == "linear":
        return (z.astype(np.int64) * V + y) * V + x
    sx, sy, sz = (int(t) for t in layout.split("x"))
    VB = (V + 3) // 4
    bx, by, bz = x & 3, y & 3, z & 3
    inner = (bx % sx) + sx * ((by % sy) + sy * (bz % sz))
    sector = (bx // sx) + (4 // sx) * ((by // sy) + (4 // sy) * (bz // sz))
    return (((z >> 2).astype(np.int64) * VB + (y >> 2)) * VB + (x >> 2)) * 64 + sector * 16 + inner


def tags(addr_bytes, valid, lanes):
    """distinct 64-B sectors per aligned group of `lanes` lanes, summed: addr_bytes / valid of shape (N,), N a multiple of 64"""
    s = np.where(valid, addr_bytes >> 6, -1).reshape(-1, lanes)
    s = np.sort(s, 1)
    distinct = (s[:, 1:] != s[:, :-1]) & (s[:, 1:] >= 0)
    return int(distinct.sum() + (s[:, 0] >= 0).sum())


def run_order(centres_vox, cell):
    """bounds_order_kernel's order of one rotation run (ties in arrival order)"""
    lo = centres_vox.min(0)
    span = float((centres_vox.max(0) - lo).max())
    c = max(cell, 1.0, span / 31.5)
    q = np.clip(((centres_vox - lo) / c).astype(np.int64), 0, 31)
    key = np.zeros(len(q), np.int64)
    for b in range(5):
        for k in range(3):
            key |= ((q[:, k] >> b) & 1) << (3 * b + k)
    return np.argsort(key, kind="stable")


def morton(q, bits):
    key = np.zeros(len(q), np.int64)
    for b in range(bits):
        for k in range(3):
            key |= ((q[:, k] >> b) & 1) << (3 * b + k)
    return key


def fine_key(centres_vox, cell):
    """bounds_order_kernel's key"""
    lo = centres_vox.min(0)
    c = max(cell, 1.0, float((centres_vox.max(0) - lo).max()) / 31.5)
    return morton(np.clip(((centres_vox - lo) / c).astype(np.int64), 0, 31), 5)


def key_variant(name, centres_vox, depth, cell):
    """the order of one rotation run under another key (ties in arrival order)"""
    lo = centres_vox.min(0)
    if name == "cell_floor_2":
        return np.argsort(fine_key(centres_vox, 2.0), kind="stable")
    if name == "bits10_quarter_voxel_cells":
        return np.argsort(morton(np.clip(((centres_vox - lo) / 0.25).astype(np.int64), 0, 1023), 10), kind="stable")
    if name == "coarse16_depth_fine":
        coarse = morton(np.clip(((centres_vox - lo) / 16.0).astype(np.int64), 0, 31), 5)
        return np.lexsort((np.arange(len(depth)), fine_key(centres_vox, cell), depth, coarse))
    if name == "depth_fine":
        return np.lexsort((np.arange(len(depth)), fine_key(centres_vox, cell), depth))
    raise ValueError(name)


KEY_VARIANTS = ("cell_floor_2", "bits10_quarter_voxel_cells", "coarse16_depth_fine", "depth_fine")


def search_shaped_batch(n_runs, seed, ub_nodes=7, lb_nodes=16):
    """A cube batch shaped like the two inner searches of a rotation child (no recorded batch exists: the shape follows the counts of
    EXPERIMENTS 3.6, bunny: 18 287 / 40 470 expansions of the upper-bound / lower-bound searches over 2 601 roots, the roots and 1.25 depth-1
    nodes per root common to both).  Per run: both searches expand the root; the upper-bound search then descends (a child of its deepest
    node three times in four, else of any node it expanded), the lower-bound search spreads (a child of a random expanded node, shallow
    ones first).  Records as bench.make_batch writes them; the coefficient only tells the passes apart."""
    rng = np.random.default_rng(seed)
    j = np.arange(8)
    off = np.stack([j & 1, (j >> 1) & 1, (j >> 2) & 1], 1).astype(np.float32)
    recs = []
    for run in range(n_runs):
        for coeff, count, deep in ((np.float32(0), ub_nodes, True), (np.float32(0.1), lb_nodes, False)):
            done = [((-0.5, -0.5, -0.5), 1.0)]                 # (corner, width) of the expanded nodes: the root first
            seen = {done[0]}
            while len(done) < count:
                if deep:
                    parent = min(done, key=lambda n: n[1]) if rng.random() < 0.75 else done[int(rng.integers(len(done)))]
                else:
                    w_ = np.array([n[1] for n in done])
                    parent = done[int(rng.choice(len(done), p=w_ / w_.sum()))]
                c = int(rng.integers(8))
                hw = parent[1] / 2
                node = (tuple(float(parent[0][k] + ((c >> k) & 1) * hw) for k in range(3)), hw)
                if node in seen or hw < 1.0 / 64:
                    continue
                seen.add(node)
                done.append(node)
            for corner, width in done:
                w = np.float32(width) / np.float32(2)
                r = np.zeros(8, dtype=[("tx", "<f4"), ("ty", "<f4"), ("tz", "<f4"), ("delta", "<f4"), ("coeff", "<f4"), ("rot", "<i4")])
                cx = np.asarray(corner, np.float32)[None, :] + off * w + w / np.float32(2)
                r["tx"], r["ty"], r["tz"] = cx[:, 0], cx[:, 1], cx[:, 2]
                r["delta"], r["coeff"], r["rot"] = np.float32(np.sqrt(3.0) / 2 * w), coeff, run
                recs.append(r)
    recs = np.concatenate(recs)
    # arrival order inside a run is the caller's: shuffled, so that no tie is decided by the generator
    g = len(recs) // 8
    perm = np.lexsort((rng.random(g), recs["rot"][0::8]))
    return recs.reshape(g, 8)[perm].reshape(-1)


def twins_mode(recs, scale, cell, trials, seed):
    """bounds_pair_kernel's coincident items under a RANDOM order inside every Morton cell (the pre-pass's LDS atomics give no other promise):
    groups of a run with the same six translations and delta, bit for bit, form a family; floor(size / 2) items per family is the most any
    order can give; a trial shuffles every cell, pairs neighbours (2 i, 2 i + 1) of the run's order and counts the pairs inside one family"""
    rng = np.random.default_rng(seed)
    g = len(recs) // 8
    first = recs.reshape(g, 8)
    box = np.stack([first["tx"][:, 0], first["tx"][:, 1], first["ty"][:, 0], first["ty"][:, 2], first["tz"][:, 0], first["tz"][:, 4], first["delta"][:, 0]], 1).astype(np.float32)
    centres = np.stack([(first[a][:, 0] + first[a][:, 7]) * np.float32(0.5) for a in ("tx", "ty", "tz")], 1) * scale
    rot = first["rot"][:, 0]
    starts = np.flatnonzero(np.concatenate([[True], rot[1:] != rot[:-1]]))
    bounds = np.concatenate([starts, [g]])
    eligible, two_member, shared, caught = 0, 0, 0, np.zeros(trials, np.int64)
    for s, e in zip(bounds[:-1], bounds[1:]):
        key = fine_key(centres[s:e], cell)
        _, fam = np.unique(box[s:e].view(np.uint32), axis=0, return_inverse=True)
        fam = fam.ravel()
        size = np.bincount(fam)
        eligible += int((size // 2).sum())
        for f in np.flatnonzero(size == 2):
            two_member += 1
            members = np.flatnonzero(fam == f)
            shared += int((key == key[members[0]]).sum() > 2)
        for t in range(trials):
            order = np.lexsort((rng.random(e - s), key))
            a, b = order[0:len(order) - 1:2], order[1::2]
            caught[t] += int((fam[a] == fam[b]).sum())
    return {"groups": int(g), "runs": int(len(starts)), "items": int(((bounds[1:] - bounds[:-1] + 1) // 2).sum()), "twin_eligible_items": eligible,
            "two_member_families": two_member, "two_member_families_sharing_their_cell": shared, "trials": trials,
            "captured_mean": round(float(caught.mean()), 1), "captured_min": int(caught.min()), "captured_max": int(caught.max()),
            "captured_share_mean": round(float(caught.mean()) / max(eligible, 1), 4), "captured_share_min": round(float(caught.min()) / max(eligible, 1), 4)}


def dedup_mode(recs, twins):
    """bounds_order_kernel's copies (BoundsOrder::alias): per run of equal rotation the full groups whose eight records repeat an earlier group's,
    all 192 bytes.  Gather sets per point chunk: today a coincident item (twins["captured_mean"], the same for every tie order on these batches)
    gathers once for its two groups and every other group once for itself; after, no expansion is gathered for more than once -- at most
    the distinct ones, and never more than today (owners that still meet as twins share a set as before)"""
    g = len(recs) // 8
    raw = np.ascontiguousarray(recs[:8 * g]).view(np.uint8).reshape(g, 192)
    rot = recs["rot"][0:8 * g:8]
    starts = np.flatnonzero(np.concatenate([[True], rot[1:] != rot[:-1]]))
    bounds = np.concatenate([starts, [g]])
    distinct = [len({row.tobytes() for row in raw[s:e]}) for s, e in zip(bounds[:-1], bounds[1:])]
    roots = np.flatnonzero(recs["delta"][0:8 * g:8] == recs["delta"].max())            # width 1 has one position: the root expansion
    root_distinct = len({raw[i].tobytes() for i in roots})
    outside = g - sum(distinct) - (len(roots) - root_distinct)
    before = g - int(round(twins["captured_mean"]))          # a coincident item saves one of its two sets
    return {"groups": int(g), "runs": int(len(starts)), "distinct_groups_per_run": distinct, "distinct_groups": int(sum(distinct)),
            "copies": int(g - sum(distinct)), "root_listings": int(len(roots)), "distinct_root_expansions": int(root_distinct),
            "copies_outside_the_roots": int(outside), "gather_sets_before": int(before), "gather_sets_after": int(min(before, sum(distinct))),
            "ratio": round(min(before, sum(distinct)) / max(before, 1), 4)}


def lines_mode(a, rots, recs, src, mn, scale, V):
    N = len(src)
    chunk_pts = -(-(-(-N // 8)) // 256) * 256                 # bounds_shape: eight chunks, a multiple of 256 points
    n_exp, per_run = len(recs) // 8, len(recs) // 8 // len(rots)

    def line_ids(e, pts):
        r = recs[8 * e:8 * e + 8]
        R = rots[int(r["rot"][0])].reshape(3, 3).astype(np.float32)
        p = src[pts]
        rp = (p[:, 0:1] * R[:, 0] + p[:, 1:2] * R[:, 1]) + p[:, 2:3] * R[:, 2]
        t = [(r["tx"][0], r["tx"][1]), (r["ty"][0], r["ty"][2]), (r["tz"][0], r["tz"][4])]
        idx = [[((rp[:, k] + np.float32(t[k][j]) - mn[k]) * scale + np.float32(0.5)).astype(np.int32) for j in (0, 1)] for k in range(3)]
        ok = np.ones(len(p), bool)
        for k in range(3):
            for j in (0, 1):
                ok &= (idx[k][j] >= 0) & (idx[k][j] < V)
        out = np.full((len(p), 8), -1, np.int64)
        for c in range(8):
            el = element_index(np.clip(idx[0][c & 1], 0, V - 1), np.clip(idx[1][c >> 1 & 1], 0, V - 1), np.clip(idx[2][c >> 2 & 1], 0, V - 1), V, "4x4x1")
            out[:, c] = np.where(ok, el >> 5, -1)                   # 32 floats per 128-B line
        return out

    def distinct(x):
        u = np.unique(x)
        return len(u) - int(u[0] < 0) if len(u) else 0

    centres = np.stack([(recs[f][0::8] + recs[f][7::8]) * np.float32(0.5) for f in ("tx", "ty", "tz")], 1).astype(np.float64) * float(scale)
    orders = {"as_given": [np.arange(per_run) for _ in rots], "ordered": [run_order(centres[r * per_run:(r + 1) * per_run], a.cell) for r in range(len(rots))]}
    width = (recs["tx"][1::8] - recs["tx"][0::8]).astype(np.float64)
    depth = np.unique(-width, return_inverse=True)[1]            # 0 = the widest parent cube of the batch
    if a.keys:
        for name in KEY_VARIANTS:
            orders[name] = [key_variant(name, centres[r * per_run:(r + 1) * per_run], depth[r * per_run:(r + 1) * per_run], a.cell) for r in range(len(rots))]
    out = {"batch": "bench.make_batch(%d expansions, %d rotations, seed 1234); windows every %d expansions" % (n_exp, len(rots), a.every), "N": N, "V": V,
           "chunk_pts": chunk_pts, "cell_voxels": a.cell}
    # per wavefront / workgroup iteration / item, every k-th expansion, chunk 0 .. 7 in turn
    wave, wg_sum, wg_union, item, n_w, n_g, n_i = 0, 0, 0, 0, 0, 0, 0
    for j, e in enumerate(range(0, n_exp, a.every)):
        ch = j % 8
        pts = np.arange(ch * chunk_pts, min((ch + 1) * chunk_pts, N))
        L = line_ids(e, pts)
        item += distinct(L); n_i += 1
        for g0 in range(0, len(pts), 256):
            ws = [distinct(L[w0:w0 + 64]) for w0 in range(g0, min(g0 + 256, len(pts)), 64)]
            wave += sum(ws); n_w += len(ws)
            wg_sum += sum(ws); wg_union += distinct(L[g0:g0 + 256]); n_g += 1
    out["lines_per_wave_iteration"] = round(wave / n_w, 1)
    out["lines_per_workgroup_iteration"] = {"sum_of_wavefronts": round(wg_sum / n_g, 1), "union": round(wg_union / n_g, 1),
                                            "per_wave_if_shared": round(wg_union / n_w, 1)}
    out["lines_per_item"] = round(item / n_i, 1)
    for name, ords in orders.items():
        res = {}
        dist = []
        for r, o in enumerate(ords):
            c = centres[r * per_run:(r + 1) * per_run][o]
            dist.append(np.linalg.norm(np.diff(c, axis=0), axis=1))
        res["median_voxels_between_consecutive"] = round(float(np.median(np.concatenate(dist))), 1)
        same = [depth[r * per_run:(r + 1) * per_run][o][0:per_run - 1:2] == depth[r * per_run:(r + 1) * per_run][o][1:per_run:2] for r, o in enumerate(ords)]
        res["pairs_of_equal_depth"] = round(float(np.mean(np.concatenate(same))), 3)
        for label, k, npts in (("5_expansions_256_points", 5, 256), ("20_expansions_1024_points", 20, 1024), ("pair_64_points", 2, 64), ("pair_256_points", 2, 256)):
            un = sm = 0
            for r, o in enumerate(ords):
                for w, s0 in enumerate(range(0, per_run - k + 1, max(a.every * 4, k))):
                    p0 = ((r * 7 + w * 3) % 8) * chunk_pts + 256 * (w % 4)
                    pts = np.arange(p0, min(p0 + npts, N))
                    sets = [line_ids(r * per_run + int(o[s0 + i]), pts) for i in range(k)]
                    sm += sum(distinct(x) for x in sets)
                    un += distinct(np.concatenate(sets))
            res[label + "_union_over_sum"] = round(un / max(sm, 1), 3)
        out[name] = res
    return out


COST_ROTS = ((0.9, -0.5, 0.3), (-0.4, 1.1, 0.8), (0.6, 0.7, -1.3))     # Rodrigues vectors of device.hip kCostRots[1..3]


def wave_lines(line, N):
    """distinct line ids (>= 0) per wavefront of 64 consecutive points -> (waves,)"""
    pad = (-N) % 64
    s = np.sort(np.pad(line, (0, pad), constant_values=-1).reshape(-1, 64), 1)
    return ((s[:, 1:] != s[:, :-1]) & (s[:, 1:] >= 0)).sum(1) + (s[:, 0] >= 0)


def chunks_mode(a, pkg, src, mn, scale, V):
    """What each of the pair launch's eight point chunks costs (EXPERIMENTS R9.1): distinct 128-B lines per 64-lane gather, per chunk, over
    --rotations random rotations x 12 sibling expansions at depths 0 - 5 (two per depth; corners as bench.make_batch draws them), the eight
    dword gathers of a point each; the same count at the identity pose without translation; and the device's own cost
    (bounds_chunk_cost_kernel: the identity and COST_ROTS at translation 0, one gather per pose), which goicp_debug_bounds_balance reports."""
    N = len(src)
    chunk_pts = -(-(-(-N // 8)) // 256) * 256
    wave_chunk = (np.arange(-(-N // 64)) * 64) // chunk_pts
    rng = np.random.default_rng(a.seed)

    def gather_lines(R, t):
        """t: three (lo, hi) translation pairs -> per child gather the lines per wavefront, lanes with an index outside the grid left out"""
        rp = (src[:, 0:1] * R[:, 0] + src[:, 1:2] * R[:, 1]) + src[:, 2:3] * R[:, 2]
        idx = [[((rp[:, k] + np.float32(t[k][j]) - mn[k]) * scale + np.float32(0.5)).astype(np.int32) for j in range(len(t[k]))] for k in range(3)]
        ok = np.ones(N, bool)
        for k in range(3):
            for v in idx[k]:
                ok &= (v >= 0) & (v < V)
        out = []
        for c in range(8 if len(t[0]) == 2 else 1):
            x, y, z = (np.clip(idx[k][(c >> k) & 1 if len(t[k]) == 2 else 0], 0, V - 1) for k in range(3))
            out.append(wave_lines(np.where(ok, element_index(x, y, z, V, a.chunk_layout) >> 5, -1), N))
        return out

    def per_chunk(ws):
        """sum over the gathers of lines per chunk, and the gathers (wavefront instructions) per chunk"""
        lines = np.zeros(8)
        for w in ws:
            lines += np.bincount(wave_chunk, weights=w, minlength=8)
        return lines, np.bincount(wave_chunk, minlength=8) * len(ws)

    tot_l, tot_g, ratios = np.zeros(8), np.zeros(8), []
    for _ in range(a.rotations):
        R = np.asarray(pkg.fgoicp.rodrigues(rng.uniform(-2.0, 2.0, 3)), np.float32).reshape(3, 3)
        rl, rg = np.zeros(8), np.zeros(8)
        for lev in list(range(6)) * 2:
            pw = np.float32(1.0 / (1 << lev))
            corner = (rng.uniform(-0.5, 0.5, 3) * (1 - pw) - pw / 2).astype(np.float32)
            w = pw / np.float32(2)
            t = [(corner[k] + w / np.float32(2), corner[k] + w + w / np.float32(2)) for k in range(3)]
            l, g = per_chunk(gather_lines(R, t))
            rl += l; rg += g
        tot_l += rl; tot_g += rg
        ratios.append(rl / rl.mean())
    ratios = np.array(ratios)
    ident, _ = per_chunk(gather_lines(np.eye(3, dtype=np.float32), [(0.0,), (0.0,), (0.0,)]))
    dev = np.zeros(8)
    for v in (None,) + COST_ROTS:
        R = np.eye(3, dtype=np.float32) if v is None else np.asarray(pkg.fgoicp.rodrigues(np.asarray(v, np.float64)), np.float32).reshape(3, 3)
        dev += per_chunk(gather_lines(R, [(0.0,), (0.0,), (0.0,)]))[0]
    pts = [int(min((k + 1) * chunk_pts, N) - min(k * chunk_pts, N)) for k in range(8)]
    return {"N": N, "V": V, "layout": a.chunk_layout, "chunk_pts": chunk_pts, "rotations": a.rotations, "expansions_per_rotation": 12, "seed": a.seed,
            "points": pts, "lines_per_gather": np.round(tot_l / tot_g, 2).tolist(), "lines_per_chunk_over_mean": np.round(tot_l / tot_l.mean(), 3).tolist(),
            "ratio_min_over_rotations": np.round(ratios.min(0), 3).tolist(), "ratio_max_over_rotations": np.round(ratios.max(0), 3).tolist(),
            "identity_no_translation_over_mean": np.round(ident / ident.mean(), 3).tolist(),
            "device_cost_lines": [int(x) for x in dev], "device_cost_waves": [int(4 * x) for x in np.bincount(wave_chunk, minlength=8)],
            "device_cost_lines_over_mean": np.round(dev / dev.mean(), 3).tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", action="store_true", help="model the cost of the pair launch's eight point chunks: distinct 128-B lines per 64-lane gather (see chunks_mode)")
    ap.add_argument("--rotations", type=int, default=8, help="--chunks: random rotations")
    ap.add_argument("--seed", type=int, default=0, help="--chunks: seed of the rotations and corners")
    ap.add_argument("--chunk-layout", default="4x4x1", help="--chunks: sector shape inside the brick (4x4x1: the engine's brick_index)")
    ap.add_argument("--layouts", default="4x4x1,4x2x2,2x2x4,2x4x2,linear")
    ap.add_argument("--lanes", type=int, default=4, help="lanes that share one tag lookup (4: a quad)")
    ap.add_argument("--every", type=int, default=16, help="model every k-th expansion of the batch")
    ap.add_argument("--merged", action="store_true", help="also model 16-B x-row loads for x siblings < 4 voxels apart")
    ap.add_argument("--json", default=None)
    ap.add_argument("--lines", action="store_true", help="model 128-B lines and their sharing between consecutive expansions (see above)")
    ap.add_argument("--cell", type=float, default=4.0, help="--lines: smallest Morton cell of the order, voxels")
    ap.add_argument("--keys", action="store_true", help="--lines: also model the other keys of the order (KEY_VARIANTS)")
    ap.add_argument("--twins", action="store_true", help="model the coincident items of the pair launch under a random order inside every cell (see above)")
    ap.add_argument("--trials", type=int, default=200, help="--twins: random tie orders per batch")
    a = ap.parse_args()

    from conftest import load_pkg, cloud
    import bench
    pkg = load_pkg()

    class _Lib:                                              # make_batch's host calls: the geometry does not depend on them
        @staticmethod
        def goicp_trans_delta(w):
            return float(np.float32(np.sqrt(3.0) / 2 * w))

    class _Reg:
        _lib = _Lib()

        @staticmethod
        def rot_coeff(level):
            return np.float32(0)

    rots, recs, _ = bench.make_batch(pkg, _Reg(), 8192, 8, seed=1234)
    model, data = cloud("model_bunny"), cloud("data_bunny")
    src = data[kd_order(data)].astype(np.float32)
    N = len(src)
    pad = (-N) % 64
    V = 300
    mn, scale = dt_geometry(model, V)
    if a.chunks:
        out = chunks_mode(a, pkg, src, mn, scale, V)
        print(json.dumps(out, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.twins:
        out = {"cell_vox": a.cell, "voxels_per_unit": round(float(scale), 2),
               "bench_batch": dict(batch="bench.make_batch(8192 expansions, 8 rotations, seed 1234)", **twins_mode(recs, scale, a.cell, a.trials, 0)),
               "search_shaped_batch": dict(batch="search_shaped_batch(64 runs, seed 1): 7 + 16 expansions per run", **twins_mode(search_shaped_batch(64, 1), scale, a.cell, a.trials, 0))}

        class _RegLevels(_Reg):                              # the copies are told apart by the coefficient too: one value per rotation level, as the engine's table has
            @staticmethod
            def rot_coeff(level):
                return np.float32(2.0 * np.sin(min(np.sqrt(3.0) * np.pi / (1 << level), np.pi) / 2.0))

        levelled = bench.make_batch(pkg, _RegLevels(), 8192, 8, seed=1234)[1]
        out["bench_batch"]["dedup"] = dedup_mode(levelled, out["bench_batch"])
        out["search_shaped_batch"]["dedup"] = dedup_mode(search_shaped_batch(64, 1), out["search_shaped_batch"])
        for name in ("bench_batch", "search_shaped_batch"):
            d = out[name]["dedup"]
            print("%s: groups / distinct %d / %d, gather sets per point chunk %d -> %d (%.3f)" % (name, d["groups"], d["distinct_groups"], d["gather_sets_before"],
                                                                                                d["gather_sets_after"], d["ratio"]), file=sys.stderr)
        print(json.dumps(out, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.lines:
        out = lines_mode(a, rots, recs, src, mn, scale, V)
        print(json.dumps(out, indent=1))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    layouts = a.layouts.split(",")
    res = {lay: {"gather_tags": 0, "gathers": 0, "merged_tags": 0, "merged_instr": 0} for lay in layouts}
    spread = {}                                              # child spacing (voxels) -> [sum of distinct sectors per lane, lanes] per layout
    waves = (N + pad) // 64
    for e in range(0, 8192, a.every):
        r = recs[8 * e:8 * e + 8]
        R = rots[int(r["rot"][0])].reshape(3, 3).astype(np.float32)
        rp = (src[:, 0:1] * R[:, 0] + src[:, 1:2] * R[:, 1]) + src[:, 2:3] * R[:, 2]
        t = [(r["tx"][0], r["tx"][1]), (r["ty"][0], r["ty"][2]), (r["tz"][0], r["tz"][4])]
        idx = [[((rp[:, k] + np.float32(t[k][j]) - mn[k]) * scale + np.float32(0.5)).astype(np.int32) for j in (0, 1)] for k in range(3)]
        inside = np.ones(N, bool)
        for k in range(3):
            for j in (0, 1):
                inside &= (idx[k][j] >= 0) & (idx[k][j] < V)
        ix, iy, iz = ([np.pad(np.clip(v, 0, V - 1), (0, pad)) for v in idx[k]] for k in range(3))
        ok = np.pad(inside, (0, pad))
        spacing = float((np.float32(t[0][1]) - np.float32(t[0][0])) * scale)
        for lay in layouts:
            el = [[[element_index(ix[a_], iy[b], iz[c], V, lay) for c in (0, 1)] for b in (0, 1)] for a_ in (0, 1)]
            d = res[lay]
            sect = []
            for c in range(8):
                ad = el[c & 1][c >> 1 & 1][c >> 2 & 1] * 4
                d["gather_tags"] += tags(ad, ok, a.lanes)
                sect.append(ad >> 6)
            d["gathers"] += 8 * waves
            s = np.sort(np.stack(sect, 1)[:N][inside], 1)
            sp = spread.setdefault("%.2f" % spacing, {})
            acc = sp.setdefault(lay, [0, 0])
            acc[0] += int(((s[:, 1:] != s[:, :-1]).sum(1) + 1).sum()); acc[1] += int(inside.sum())
            if a.merged and lay != "linear":
                if spacing < 4:
                    for b in (0, 1):
                        for c in (0, 1):
                            row = (el[0][b][c] & ~3) * 4
                            second = el[1][b][c] * 4
                            split = ((ix[0] >> 2) != (ix[1] >> 2)) & ok
                            d["merged_tags"] += tags(row, ok, a.lanes) + tags(second, split, a.lanes)
                            d["merged_instr"] += waves * (1 + int(split.reshape(-1, 64).any(1).sum()) / waves)
                else:
                    for c in range(8):
                        d["merged_tags"] += tags(el[c & 1][c >> 1 & 1][c >> 2 & 1] * 4, ok, a.lanes)
                    d["merged_instr"] += 8 * waves
    out = {"batch": "bench.make_batch(8192 expansions, 8 rotations, seed 1234), every %d-th expansion" % a.every, "N": N, "V": V,
           "lanes_per_tag_group": a.lanes, "layouts": {}}
    n_exp = len(range(0, 8192, a.every))
    for lay, d in res.items():
        g = d["gather_tags"] / d["gathers"]
        o = {"tags_per_dt_gather": round(g, 2),
             "tags_per_vmem_instr": round((d["gather_tags"] + 16 * waves * n_exp) / (d["gathers"] + waves * n_exp), 2),
             "sectors_per_lane_by_child_spacing_voxels": {k: round(v[lay][0] / max(v[lay][1], 1), 2) for k, v in sorted(spread.items(), key=lambda kv: -float(kv[0]))}}
        if a.merged and lay != "linear":
            o["merged_tags_per_point"] = round(d["merged_tags"] / (waves * n_exp), 2)
            o["unmerged_tags_per_point"] = round(d["gather_tags"] / (waves * n_exp), 2)
            o["merged_vmem_instr_per_point"] = round(d["merged_instr"] / (waves * n_exp), 2)
        out["layouts"][lay] = o
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
