"""Record tests/golden/search_paths.json from the BUILT tree (see tests/test_gpu_search_paths.py): python tools/record_search_paths.py OUT.json [COMMIT]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_search_paths as T
pkg = T.load_pkg()
out = {"commit": sys.argv[2] if len(sys.argv) > 2 else "unknown", "kernel_source_hash": pkg.load_library().goicp_kernel_source_hash().decode(), "unstable": {}}
for kind, (table, run) in T.RUNNERS.items():
    out[kind] = {}
    for name in table:
        t0 = time.perf_counter()
        out[kind][name] = run(pkg, name)
        print("%-14s %-28s %6.2f s  %s" % (kind, name, time.perf_counter() - t0, out[kind][name]), flush=True)
with open(sys.argv[1], "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
