#!/usr/bin/env python3
"""A likelihood that lives on the GPU, behind the two batch callbacks: what the device door saves a round.

The likelihood is tools/dev/device_batch_gauss.hip's kernel (one thread a row, 20-D Gaussian).
  path a  polychord_hip_set_batch_callback: what a user writes today -- cubes up, one launch, theta / phi / logL down, and the engine's own
          copy of the answers up again;
  path b  polychord_hip_set_device_batch_callback: the kernel on the engine's stream, on the engine's blocks.
Both at the cheap end (the kernel as it is) and at a dear end (the same kernel repeating its sum, about a millisecond a call), where the
transfers should not matter.  The runs alternate a, b, a, b ... in ONE process on one device; the two paths give the same run (checked:
ndead, nlike, log Z), so ticks/s and evaluations/s compare like with like.  Needs a GPU: there is no other path.

    python tools/dev/bench_device_batch.py --out profiles/device_batch.json

--in-step: the other leg.  R = 4 and 16 seeds of that problem through pchip_run_in_step (one call a tick for the rows of all runs of the
group) against the same seeds one after another through the solo device-batch pchip_run, alternating in one process, at both ends; every
run in step is checked against its solo run (ndead, nlike, log Z).

    python tools/dev/bench_device_batch.py --in-step --out profiles/device_batch_in_step.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


class GaussCtx(C.Structure):
    _fields_ = [("mu", C.c_double), ("sigma", C.c_double), ("c", C.c_double), ("inner", C.c_int), ("calls", C.c_int)]


def build_so(path=None):
    if path and os.path.exists(path):
        return C.CDLL(path)
    out = path or os.path.join(tempfile.mkdtemp(prefix="dbgauss"), "libdbgauss.so")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(ROOT, "tools", "dev", "device_batch_gauss.hip"), "-o", out])
    return C.CDLL(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, default=20)
    ap.add_argument("--nlive", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=40, help="num_repeats")
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--max-ndead", type=int, default=20000, help="dead points of a run at the cheap end (a window of a good fraction of a second)")
    ap.add_argument("--max-ndead-dear", type=int, default=2000, help="... at the dear end (a millisecond a call: the window is long anyway)")
    ap.add_argument("--inner-dear", type=int, default=200, help="passes of the dear end's kernel (about a millisecond a call)")
    ap.add_argument("--runs", type=int, default=5, help="timed runs per path and end, alternating")
    ap.add_argument("--in-step", action="store_true", help="the in-step leg instead: R seeds through pchip_run_in_step against R solo runs")
    ap.add_argument("--seeds", type=int, nargs="*", default=[4, 16], help="--in-step: the numbers of seeds R")
    ap.add_argument("--legs", nargs="*", default=["solo", "in_step"], help="--in-step: the legs to run (one alone: for a kernel trace)")
    ap.add_argument("--so", default=None, help="a prebuilt libdbgauss.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from polychordlite_amd import _ctypes_api as api
    lib = api.load()
    if lib.pchip_device_count() < 1:
        sys.exit("bench_device_batch: no HIP device")
    g = build_so(a.so)
    g.gauss_set_scalar.argtypes = [C.c_double, C.c_double, C.c_double]
    D = a.dims
    c0 = -D * (np.log(0.1) + 0.5 * np.log(2 * np.pi))
    g.gauss_set_scalar(0.5, 0.1, c0)
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, 1)
    s.nlive, s.num_repeats, s.seed, s.batch = a.nlive, a.repeats, 11, a.batch
    L = api.Like(); L.kind = api.LIKE_CALLBACK; L.fn = C.cast(g.gauss_loglike, C.c_void_p)
    P = api.Prior(); P.kind = 0; P.fn = C.cast(g.gauss_prior, C.c_void_p)
    lib.polychord_hip_set_batch_callback.argtypes = [C.c_void_p, C.c_void_p]
    lib.polychord_hip_set_device_batch_callback.argtypes = [C.c_void_p, C.c_void_p]

    def one(path, inner):
        ctx = GaussCtx(0.5, 0.1, c0, inner, 0)
        if path == "a":
            lib.polychord_hip_set_batch_callback(C.cast(g.gauss_host_batch_via_device, C.c_void_p), C.byref(ctx))
        else:
            lib.polychord_hip_set_device_batch_callback(C.cast(g.gauss_device_batch, C.c_void_p), C.byref(ctx))
        try:
            t0 = time.perf_counter()
            r = api.run(s, L, P)                   # (returns after the engine's last synchronise)
            dt = time.perf_counter() - t0
        finally:
            lib.polychord_hip_set_batch_callback(None, None)
            lib.polychord_hip_set_device_batch_callback(None, None)
        return dict(seconds=dt, calls=int(ctx.calls), nlike=int(r["nlike"]), ndead=int(r["ndead"]), logZ=float(r["logZ"]),
                    t_loop=float(r["t_loop"]), t_generate=float(r["t_generate"]), device_batch=int(r["path"]["device_batch"]))

    def solo_seeds(seeds, inner):
        """the seeds one after another through the solo device-batch pchip_run"""
        ctx = GaussCtx(0.5, 0.1, c0, inner, 0)
        lib.polychord_hip_set_device_batch_callback(C.cast(g.gauss_device_batch, C.c_void_p), C.byref(ctx))
        try:
            t0 = time.perf_counter()
            rs = []
            for sd in seeds:
                s.seed = sd
                r = api.run(s, L, P)
                rs.append((int(r["ndead"]), int(r["nlike"]), float(r["logZ"]), int(r["path"]["device_batch"])))
                del r
            dt = time.perf_counter() - t0
        finally:
            lib.polychord_hip_set_device_batch_callback(None, None)
        return dict(seconds=dt, calls=int(ctx.calls), nlike=sum(x[1] for x in rs), runs=rs)

    def step_seeds(seeds, inner):
        """... and in step: one group of len(seeds) runs, one call a tick"""
        from polychordlite_amd import repeats
        ctx = GaussCtx(0.5, 0.1, c0, inner, 0)
        lib.polychord_hip_set_device_batch_callback(C.cast(g.gauss_device_batch, C.c_void_p), C.byref(ctx))
        try:
            s.seed = seeds[0]
            t0 = time.perf_counter()
            merged, runs = repeats.run_in_step(s, L, P, seeds, max_in_flight=len(seeds))
            dt = time.perf_counter() - t0
            rs = [(int(r["ndead"]), int(r["nlike"]), float(r["logZ"]), int(r["path"]["device_batch"])) for r in runs]
            t_runs = float(merged["t_runs_s"])
            del merged, runs
        finally:
            lib.polychord_hip_set_device_batch_callback(None, None)
        return dict(seconds=dt, runs_seconds=t_runs, calls=int(ctx.calls), nlike=sum(x[1] for x in rs), runs=rs)

    if a.in_step:
        report = dict(shape=dict(nDims=D, nlive=a.nlive, num_repeats=a.repeats, batch=a.batch), ends={})
        for end, inner, max_ndead in (("cheap", 0, a.max_ndead), ("dear", a.inner_dear, a.max_ndead_dear)):
            s.max_ndead = max_ndead
            report["ends"][end] = {}
            for R in a.seeds:
                seeds = list(range(11, 11 + R))
                legs = {k: f for k, f in (("solo", solo_seeds), ("in_step", step_seeds)) if k in a.legs}
                for f in legs.values():             # warm-up: code objects, the block caches, the streams
                    f(seeds, inner)
                runs = {k: [] for k in legs}
                for _ in range(a.runs):
                    for k, f in legs.items():
                        runs[k].append(f(seeds, inner))
                same = len(legs) < 2 or runs["solo"][0]["runs"] == runs["in_step"][0]["runs"]
                e = dict(inner=inner, max_ndead=max_ndead, seeds=R, same_runs=same)
                for k in legs:
                    sec = [x["seconds"] for x in runs[k]]
                    med = statistics.median(sec)
                    x0 = runs[k][0]
                    e[k] = dict(seconds=sec, median_s=med, min_s=min(sec), max_s=max(sec), calls=x0["calls"], evaluations=x0["nlike"],
                                rows_per_call=x0["nlike"] / x0["calls"], evals_per_s=x0["nlike"] / med, us_per_call=1e6 * med / x0["calls"])
                    if k == "in_step":
                        e[k]["runs_median_s"] = statistics.median(x["runs_seconds"] for x in runs[k])      # (without the merge of the runs)
                if len(legs) == 2:
                    e["solo_over_in_step"] = e["solo"]["median_s"] / e["in_step"]["median_s"]
                report["ends"][end][str(R)] = e
                print(f"{end:5s} inner {inner:5d}, {R:2d} seeds: same runs: {same}")
                for k in legs:
                    print(f"   {k:8s}: {e[k]['median_s']:.3f} s (min {e[k]['min_s']:.3f}, max {e[k]['max_s']:.3f})  {e[k]['calls']} calls, "
                          f"{e[k]['rows_per_call']:.1f} rows a call, {e[k]['evals_per_s']:.0f} evaluations/s, {e[k]['us_per_call']:.1f} us a call")
        g.gauss_release()
        print(json.dumps(report))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(report, f, indent=1)
                f.write("\n")
        return

    report = dict(shape=dict(nDims=D, nlive=a.nlive, num_repeats=a.repeats, batch=a.batch), ends={})
    for end, inner, max_ndead in (("cheap", 0, a.max_ndead), ("dear", a.inner_dear, a.max_ndead_dear)):
        s.max_ndead = max_ndead
        for p in "ab":                              # warm-up: code objects, the staging blocks, the engine's block caches
            one(p, inner)
        runs = {"a": [], "b": []}
        for _ in range(a.runs):
            for p in "ab":
                runs[p].append(one(p, inner))
        ra, rb = runs["a"][0], runs["b"][0]
        same = all(ra[k] == rb[k] for k in ("nlike", "ndead", "logZ", "calls"))
        e = dict(inner=inner, max_ndead=max_ndead, same_run=same, calls=ra["calls"], nlike=ra["nlike"], ndead=ra["ndead"])
        for p in "ab":
            sec = [x["seconds"] for x in runs[p]]
            med = statistics.median(sec)
            e[p] = dict(seconds=sec, median_s=med, min_s=min(sec), max_s=max(sec), ticks_per_s=runs[p][0]["calls"] / med,
                        evals_per_s=runs[p][0]["nlike"] / med, us_per_tick=1e6 * med / runs[p][0]["calls"])
        e["b_over_a_ticks_per_s"] = e["b"]["ticks_per_s"] / e["a"]["ticks_per_s"]
        report["ends"][end] = e
        print(f"{end:5s} inner {inner:5d}: {ra['calls']} calls, {ra['nlike']} evaluations, same run: {same}")
        for p in "ab":
            print(f"   path {p}: {e[p]['median_s']:.3f} s (min {e[p]['min_s']:.3f}, max {e[p]['max_s']:.3f})  "
                  f"{e[p]['ticks_per_s']:.0f} ticks/s  {e[p]['evals_per_s']:.0f} evaluations/s  {e[p]['us_per_tick']:.1f} us a tick")
    g.gauss_release()
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
