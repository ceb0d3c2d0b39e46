#!/usr/bin/env python3
"""What the quadratic form (pchip_source_create_quad) buys: the straight-line fit under AR(1)-correlated noise of tests/test_source_quad.py
-- chi2 = r^T P r with a dense precision matrix -- as a quad handle against the same likelihood as a plain source (its replay: every lane
forms all the residuals and walks the whole matrix), at 64 and 256 residuals, nlive 500, num_repeats 10, the same seed: the same run.

    python tools/bench_source_quad.py [out.json]

Behind a warm-up (run-time compilation, module loads), REPS interleaved repeats; a figure is the wall time of the whole run, given as the
median with its spread (min, max), and the evaluations a second that run made (nlike / wall time)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polychordlite_amd import _ctypes_api as api      # noqa: E402
from tests.test_source_quad import QUAD, REPLAY_WRAPPER, LO, HI, _line_data, _precision, _replay_block      # noqa: E402

REPS = 5
SIZES = (64, 256)


def settings(D, nDer, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def stat(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def one_run(L, P):
    t = time.perf_counter()
    g = api.run(settings(2, 2, nlive=500, num_repeats=10, seed=7), L, P)
    return time.perf_counter() - t, g


def main():
    args = sys.argv[1:]
    out = dict(shape=dict(nDims=2, nDerived=2, nlive=500, num_repeats=10, seed=7), reps=REPS, sizes={})
    for n in SIZES:
        data, Pm = _line_data(n), _precision("ar1", n)
        opts = (f"-DNRES={n}",)
        legs = {"quad": api.source_create(QUAD, options=opts, data=data, residuals=n, precision=Pm),
                "plain": api.source_create(QUAD + REPLAY_WRAPPER, options=opts, data=_replay_block(data, Pm))}
        prob = {k: api.make_problem("source", 2, 2, source=h, lo=LO, hi=HI) for k, h in legs.items()}
        for k in prob:                                  # warm-up: run-time compilation, module loads, block caches
            one_run(*prob[k][:2])
        walls = {k: [] for k in prob}; last = {}
        for _ in range(REPS):
            for k in prob:                              # interleaved
                w, g = one_run(*prob[k][:2]); walls[k].append(w); last[k] = g
        o = {}
        for k in prob:
            g = last[k]
            st = stat(walls[k])
            o[k] = dict(run_s=st, run_s_all=walls[k], nlike=int(g["nlike"]), ndead=int(g["ndead"]), logZ=g["logZ"],
                        evals_per_s=dict(median=int(g["nlike"]) / st["median"], min=int(g["nlike"]) / st["max"], max=int(g["nlike"]) / st["min"]),
                        source_terms=g["path"]["source_terms"])
        o["same_run"] = bool(np.array_equal(last["quad"]["dead"], last["plain"]["dead"]))
        o["plain_over_quad"] = o["plain"]["run_s"]["median"] / o["quad"]["run_s"]["median"]
        out["sizes"][str(n)] = o
        print(f"nres {n}: plain / quad = {o['plain_over_quad']:.2f}; same run: {o['same_run']}", file=sys.stderr, flush=True)
        for h in legs.values():
            api.load().pchip_source_destroy(h)
    txt = json.dumps(out, indent=1)
    if args:
        open(args[0], "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
