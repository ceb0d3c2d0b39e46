"""dev: the stepping out of k_slice on the histogram build (make -C polychordlite_amd/csrc ../libpolychord_hip_slicehist.so, PCHIP_LIB):
for the metric configuration and for the shapes of tests/test_slice_stepping.py, the iterations of the reference's stepping-out loop per
side and slice (every chain, a whole run) and the slices whose loop went on behind the straight-line candidates -- on the
right only, on the left only, on both sides.  Read from the engine's PC_DEBUG=4 lines -> JSON on stdout.
    PCHIP_LIB=$PWD/polychordlite_amd/libpolychord_hip_slicehist.so python tools/dev/gpu_slice_hist.py [metric] [tests]"""
import ctypes as C, json, os, re, subprocess, sys
sys.path.insert(0, ".")
SHAPES = {"metric": [("metric: 20-D Gaussian, nlive 2000, num_repeats 40", 20, 2, 2000, 40, 0, None, 1002)],
          "tests": [("20-D, nDer 2, nlive 32, num_repeats 20, batch 16", 20, 2, 32, 20, 16, None, 11),
                    ("24-D, nDer 2, nlive 40, num_repeats 48, batch 20", 24, 2, 40, 48, 20, None, 11),
                    ("8-D, nDer 0, nlive 16, num_repeats 16, batch 8", 8, 0, 16, 16, 8, None, 11),
                    ("5-D, nDer 2, nlive 24, num_repeats 25, batch 12, box (-0.5, 1.5)", 5, 2, 24, 25, 12, (-0.5, 1.5), 11),
                    ("12-D, nDer 2, nlive 24, num_repeats 25, batch 12, box (-0.5, 1.5)", 12, 2, 24, 25, 12, (-0.5, 1.5), 11)]}
which = [a for a in sys.argv[1:] if a in SHAPES] or ["metric", "tests"]
shapes = [s for w in which for s in SHAPES[w]]
if os.environ.get("SLICE_HIST_CHILD") != "1":
    env = dict(os.environ, SLICE_HIST_CHILD="1", PC_DEBUG="4")
    p = subprocess.run([sys.executable, __file__] + which, env=env, capture_output=True, text=True)
    a = [l for l in p.stderr.splitlines() if "dbg par: stage+search" in l]
    b = [l for l in p.stderr.splitlines() if "dbg par:" in l and "evidence scans" in l]
    res = [json.loads(l) for l in p.stdout.strip().splitlines()]
    if not (len(a) == len(b) == len(res) == len(shapes)):
        sys.stderr.write(p.stderr[-2000:])
        sys.exit("gpu_slice_hist.py: %d / %d counter lines for %d runs of %d shapes" % (len(a), len(b), len(res), len(shapes)))
    out = []
    for sh, la, lb, r in zip(shapes, a, b, res):
        v = [int(x) for x in re.findall(r"(-?\d+)", la.split("stage+search")[1])][:7] + [int(re.findall(r"(-?\d+)", lb.split("dbg par:")[1])[0])]
        lo, hi = (lambda x: x & 0xFFFFFFFF), (lambda x: (x >> 32) & 0xFFFFFFFF)
        n = lo(v[5])
        out.append({"shape": sh[0], "slices": n, "evaluations_per_slice": r["nlike"] / r["niter"] / sh[4],
                    "iterations_right": {k: lo(v[i]) for i, k in enumerate(("0", "1", "2", "3", "4+"))},
                    "iterations_left": {k: hi(v[i]) for i, k in enumerate(("0", "1", "2", "3", "4+"))},
                    "slices_stepping_on_both_sides": hi(v[5]),
                    "loop_behind_the_candidates": {"right_only": lo(v[6]), "left_only": hi(v[6]), "both_sides": lo(v[7])},
                    "share_of_slices": {"right_only": lo(v[6]) / n, "left_only": hi(v[6]) / n, "both_sides": lo(v[7]) / n}})
    print(json.dumps(out, indent=1))
    sys.exit(0)
from polychordlite_amd import _ctypes_api as api
lib = api.load()
for name, D, nDer, nlive, nr, batch, box, seed in shapes:
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    s.nlive, s.num_repeats, s.seed, s.batch = nlive, nr, seed, batch
    L, P, keep = api.make_problem("gaussian", D, nDer, *box) if box else api.make_problem("gaussian", D, nDer)
    r = api.run(s, L, P)
    print(json.dumps({"nlike": int(r["nlike"]), "niter": int(r["niter"]), "nbatches": int(r["nbatches"])}), flush=True)
