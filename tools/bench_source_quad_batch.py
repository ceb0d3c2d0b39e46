#!/usr/bin/env python3
"""Where the batched quadratic form (pchip_source_create_quad_batch: a round's proposals at once on the matrix cores) stands beside the
in-kernel quadratic form (pchip_source_create_quad: one wavefront a chain walks the matrix): the straight-line fit under AR(1)-correlated
noise of tests/test_source_quad.py at nlive 500, num_repeats 10, the same seed.  At 256 and 1024 residuals both forms run -- the in-kernel
form is unchanged code, the yardstick --; at 2048 and 4096 the batched form alone (the in-kernel form stops at 1024).

    python tools/bench_source_quad_batch.py [out.json]

Behind a warm-up (run-time compilation, module loads), REPS interleaved repeats; a figure is the wall time of the whole run, given as the
median with its spread (min, max), and the evaluations a second that run made (nlike / wall time).  The two forms round differently, so
their runs are not the same run: each leg's own nlike is what its rate is formed from."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polychordlite_amd import _ctypes_api as api      # noqa: E402
from tests.test_source_quad import QUAD, LO, HI, _line_data, _precision      # noqa: E402

REPS = 5
SIZES = (256, 1024, 2048, 4096)
IN_KERNEL_MAX = 1024


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
        legs = {"batch": api.source_create(QUAD, options=opts, data=data, residuals=n, precision=Pm, batched=True)}
        if n <= IN_KERNEL_MAX:
            legs["quad"] = api.source_create(QUAD, options=opts, data=data, residuals=n, precision=Pm)
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
            o[k] = dict(run_s=st, run_s_all=walls[k], nlike=int(g["nlike"]), ndead=int(g["ndead"]), logZ=g["logZ"], logZerr=g["logZerr"], batch=int(g["batch"]),
                        evals_per_s=dict(median=int(g["nlike"]) / st["median"], min=int(g["nlike"]) / st["max"], max=int(g["nlike"]) / st["min"]),
                        device_batch=g["path"]["device_batch"], source_kernels=g["path"]["source_kernels"])
        if "quad" in o:
            o["quad_over_batch_rate"] = o["quad"]["evals_per_s"]["median"] / o["batch"]["evals_per_s"]["median"]
        out["sizes"][str(n)] = o
        print(f"nres {n}: " + "; ".join(f"{k} {o[k]['run_s']['median']:.3f} s, {o[k]['evals_per_s']['median'] / 1e6:.3f} M evals/s" for k in prob), file=sys.stderr, flush=True)
        for h in legs.values():
            api.load().pchip_source_destroy(h)
    txt = json.dumps(out, indent=1)
    if args:
        open(args[0], "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
