#!/usr/bin/env python3
"""What several sums per evaluation (pchip_source_create_sums) buy: the Lorentzian fit of tests/test_source_sums.py -- amplitude and baseline
profiled out, three sums -- in the sums form against the same likelihood as a plain source (its replay: every lane walks all the data, and
the derived parameters walk them again), at 256 and 4096 terms, nlive 500, num_repeats 10: one run, and sixteen runs in step.

    python tools/bench_source_sums.py [out.json]          the two forms, interleaved repeats after a warm-up (compilation, module loads)
    python tools/bench_source_sums.py --line [out.json]   the one-sum straight-line fit (LINE_TERMS, 256 terms) alone: wall time of a run,
                                                          for a comparison of two builds of the library run in turn by the caller

Medians with the spread (min, max) of REPS runs; a figure is a wall time of the whole call, compilation excluded by the warm-up."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polychordlite_amd import _ctypes_api as api      # noqa: E402
from polychordlite_amd import repeats                 # noqa: E402
from tests.test_source_terms import LINE_TERMS, _line_data      # noqa: E402

REPS = 3
SIZES = (256, 4096)
SEEDS16 = list(range(101, 117))


def settings(D, nDer, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def stat(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def one_run(L, P, D, nDer):
    t = time.perf_counter()
    g = api.run(settings(D, nDer, nlive=500, num_repeats=10, seed=7), L, P)
    return time.perf_counter() - t, g


def sixteen(L, P, D, nDer):
    t = time.perf_counter()
    merged, runs = repeats.run_in_step(settings(D, nDer, nlive=500, num_repeats=10), L, P, SEEDS16, max_in_flight=16)
    return time.perf_counter() - t, runs


def line(out_path):
    h = api.source_create(LINE_TERMS, data=_line_data(256), nterms=256)
    L, P, keep = api.make_problem("source", 2, 2, source=h)
    one_run(L, P, 2, 2)
    walls, g = [], None
    for _ in range(2 * REPS + 1):
        w, g = one_run(L, P, 2, 2)
        walls.append(w)
    out = dict(what="LINE_TERMS, 256 terms, one-sum handle, nlive 500, num_repeats 10", wall_s=stat(walls), wall_s_all=walls, nlike=int(g["nlike"]),
               ndead=int(g["ndead"]), logZ=g["logZ"])
    txt = json.dumps(out, indent=1)
    if out_path:
        open(out_path, "w").write(txt + "\n")
    print(txt)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--line":
        return line(args[1] if len(args) > 1 else None)
    from tests.test_source_sums import LORENTZ, REPLAY_WRAPPER, _lorentz_data, LORENTZ_LO, LORENTZ_HI
    out = dict(shape=dict(nDims=2, nDerived=5, nlive=500, num_repeats=10, runs_in_step=16), reps=REPS, sizes={})
    for n in SIZES:
        data = _lorentz_data(n)
        legs = {"sums": api.source_create(LORENTZ, data=data, nterms=n, nsums=3),
                "plain": api.source_create(LORENTZ + REPLAY_WRAPPER, options=(f"-DNTERMS={n}", "-DNSUMS=3"), data=data)}
        prob = {k: api.make_problem("source", 2, 5, source=h, lo=LORENTZ_LO, hi=LORENTZ_HI) for k, h in legs.items()}
        o = {}
        for k in prob:                                  # warm-up: run-time compilation of both launch shapes, module loads, block caches
            one_run(*prob[k][:2], 2, 5)
            sixteen(*prob[k][:2], 2, 5)
        w1 = {k: [] for k in prob}; w16 = {k: [] for k in prob}; last = {}
        for _ in range(REPS):
            for k in prob:                              # interleaved
                w, g = one_run(*prob[k][:2], 2, 5); w1[k].append(w)
                w, runs = sixteen(*prob[k][:2], 2, 5); w16[k].append(w)
                last[k] = (g, runs)
        for k in prob:
            g, runs = last[k]
            o[k] = dict(one_run_s=stat(w1[k]), sixteen_in_step_s=stat(w16[k]), nlike=int(g["nlike"]), ndead=int(g["ndead"]), logZ=g["logZ"],
                        source_terms=g["path"]["source_terms"], slice_step=runs[0]["path"]["slice_step"])
        o["same_run"] = bool(np.array_equal(last["sums"][0]["dead"], last["plain"][0]["dead"]))
        o["plain_over_sums_one_run"] = o["plain"]["one_run_s"]["median"] / o["sums"]["one_run_s"]["median"]
        o["plain_over_sums_sixteen"] = o["plain"]["sixteen_in_step_s"]["median"] / o["sums"]["sixteen_in_step_s"]["median"]
        out["sizes"][str(n)] = o
        print(f"nterms {n}: plain / sums = {o['plain_over_sums_one_run']:.2f} (one run), {o['plain_over_sums_sixteen']:.2f} (sixteen in step)", file=sys.stderr, flush=True)
        for h in legs.values():
            api.load().pchip_source_destroy(h)
    txt = json.dumps(out, indent=1)
    if args:
        open(args[0], "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
