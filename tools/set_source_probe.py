"""goicp_set_source: what a source swap costs next to creating a handle, and where the time of the source stage goes.

Per case -- bunny (30 k source points), spanner (150 k / 150 k), the synthetic 1 M / 1 M cloud of bench.py's s2 workload:
  (a) create_ms          goicp_create(T, S) wall time, and create_source_stage_ms: its "source order + upload" lap (verbose = 1), which is
                         the HOST ordering (goicp_create keeps the host path) + gather + upload;
      host_order_ms      goicp_source_order_host(S) alone, wall time
  (b) set_source_ms      goicp_set_source(S) wall time on a handle created with (T, S0), S0 = every second point of S in reverse order
  (c) device_order_ms    the device ordering alone inside those swaps (HIP events around launch_source_order; the "device order" figure of
                         the verbose line of goicp_set_source)
  (d) register_ms        goicp_register of the swapped handle and of a fresh handle on (T, S), alternated, --reps each (the poll snapshot's
                         register_ms), and whether the two end on the same bits (best_sse, pose, counters)
Every figure is kept per repetition with its median.  Writes one JSON object stamped with the git head (GOICP_GIT_HEAD, else git) and
goicp_kernel_source_hash.

    python tools/set_source_probe.py --out profiles/set_source_probe.json [--reps 5] [--only bunny,spanner,s2] [--limit 120]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _pkg():
    from conftest import load_pkg
    m = load_pkg()
    m.load_library()
    return m


class Stderr:
    """what the library prints to stderr (fd 2) inside the block"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def cases(only):
    from conftest import cloud
    out = {}
    if "bunny" in only:
        out["bunny"] = (cloud("model_bunny"), cloud("data_bunny"), dict(mse=1e-3))
    if "spanner" in only:
        g = os.path.join(ROOT, "tests", "golden")
        t = np.fromfile(os.path.join(g, "spanner_target.f32"), dtype="<f4").reshape(-1, 3)
        s = np.fromfile(os.path.join(g, "spanner_source.f32"), dtype="<f4").reshape(-1, 3)
        out["spanner"] = (t, s, dict(mse=1e-4))
    if "s2" in only:
        from cuda_go_icp_amd import synth
        t, s, _, _ = synth.make_pair(seed=synth.S2["seed"], M=synth.S2["M"], N=synth.S2["N"])
        out["s2"] = (t, s, dict(mse=1e-3, dt_size=synth.S2["V"]))
    return out


def med(v):
    return round(statistics.median(v), 4) if v else None


def register(reg, limit):
    """goicp_register with a cancel timer -> (register_ms, result bytes, finished in time)"""
    lib = reg._lib
    timer = threading.Timer(limit, lambda: lib.goicp_cancel(reg.handle))
    timer.start()
    t0 = time.perf_counter()
    rc = lib.goicp_register(reg.handle)
    wall = time.perf_counter() - t0
    timer.cancel()
    assert rc == 0, lib.goicp_last_error()
    r = reg.poll()
    key = (np.array(list(r.optR) + list(r.optT) + [r.best_sse], np.float32).tobytes(), tuple(getattr(r.counters, k) for k, _ in r.counters._fields_))
    return r.register_ms, key, wall < limit


def run_case(pkg, name, T, S, kw, reps, limit):
    mse = kw.pop("mse")
    T, S = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(S, np.float32)
    S0 = np.ascontiguousarray(S[::-2])
    res = {"n_target": len(T), "n_source": len(S), "n_source_before_swap": len(S0), "mse_threshold": mse, **kw}
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pkg.source_order(S, 2)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_order_ms"] = {"all": [round(x, 3) for x in host], "median": med(host)}
    create, stage, swap, dev = [], [], [], []
    for _ in range(reps):
        with Stderr() as err:
            v = pkg.Registration(T, S, mse, verbose=1, **kw)
        m = re.search(r"source order \+ upload\s+([0-9.]+) ms", err.text)
        stage.append(float(m.group(1)))
        v.set_source(S0)
        with Stderr() as err:
            v.set_source(S)
        m = re.search(r"set_source: \d+ points, ([0-9.]+) ms \(device order ([0-9.]+) ms\)", err.text)
        dev.append(float(m.group(2)))
        v.close()
        t0 = time.perf_counter()
        f = pkg.Registration(T, S, mse, **kw)
        create.append((time.perf_counter() - t0) * 1e3)
        f.set_source(S0)
        t0 = time.perf_counter()
        f.set_source(S)
        swap.append((time.perf_counter() - t0) * 1e3)
        f.close()
    res["create_ms"] = {"all": [round(x, 3) for x in create], "median": med(create)}
    res["create_source_stage_ms"] = {"all": stage, "median": med(stage)}
    res["set_source_ms"] = {"all": [round(x, 3) for x in swap], "median": med(swap)}
    res["device_order_ms"] = {"all": dev, "median": med(dev)}
    res["set_source_below_create"] = bool(max(swap) < min(create))
    # (d): the swapped handle next to a fresh one
    a = pkg.Registration(T, S0, mse, **kw)
    a.set_source(S)
    b = pkg.Registration(T, S, mse, **kw)
    ra, rb, same, done = [], [], True, True
    for _ in range(reps):
        ma, ka, fa = register(a, limit)
        mb, kb, fb = register(b, limit)
        ra.append(round(ma, 3)); rb.append(round(mb, 3))
        done = done and fa and fb
        same = same and (ka == kb or not (fa and fb))
    a.close(); b.close()
    res["register_swapped_ms"] = {"all": ra, "median": med(ra)}
    res["register_fresh_ms"] = {"all": rb, "median": med(rb)}
    res["register_finished_within_limit"] = done
    res["register_results_identical"] = same
    print("%-8s create %.1f ms (source stage %.1f, host order alone %.1f) | set_source %.2f ms (device order %.3f) | register swapped %.1f fresh %.1f ms, identical %s"
          % (name, res["create_ms"]["median"], res["create_source_stage_ms"]["median"], res["host_order_ms"]["median"], res["set_source_ms"]["median"],
             res["device_order_ms"]["median"], res["register_swapped_ms"]["median"], res["register_fresh_ms"]["median"], same), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_source_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="bunny,spanner,s2")
    ap.add_argument("--limit", type=float, default=120.0)
    args = ap.parse_args()
    pkg = _pkg()
    head = os.environ.get("GOICP_GIT_HEAD")
    if not head:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        head = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    out = {"git_head": head, "kernel_source_hash": pkg.load_library().goicp_kernel_source_hash().decode(),
           "kernel_source_hash_of_tree": pkg.kernel_source_hash(), "reps": args.reps, "cases": {}}
    for name, (T, S, kw) in cases(args.only.split(",")).items():
        out["cases"][name] = run_case(pkg, name, T, S, dict(kw), args.reps, args.limit)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
