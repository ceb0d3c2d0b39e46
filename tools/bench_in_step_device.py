"""What the user's own problem gains from the runs in step (repeats.run_in_step, pchip_run_in_step): sixteen runs in step against the same
sixteen seeds by pchip_run one after another, same process, same library, evaluations/s = the runs' nlike / wall clock of the sixteen.

  plain_source   the 20-D Gaussian (0.5, 0.1) as a plain device source, nlive 2000, num_repeats 40, two derived parameters, the uniform box
                 (configs/gaussian_nlive2000.ini's shape);
  terms_source   the straight-line fit over 256 data points as a terms source (2-D, nlive 1000, num_repeats 10, one derived parameter: the
                 shape of tools/bench_source_terms.py), the box (-2, 2);
  prior_table    the built-in 20-D Gaussian under a table of twenty `gaussian` priors N(0.5, 1), nlive 2000, num_repeats 40
                 (configs/gaussian_gaussian_prior_nlive2000.ini's shape).

One process; a warm-up of both ways of every leg first (the run-time compilations and module loads outside the timing; their count and seconds
reported from pchip_rtc_stats); then the two ways alternated REPS times.  A call is timed to its return: pchip_run and pchip_run_in_step both
end behind a device synchronise, run_in_step behind the merge of the sixteen runs as well (its wall clock is in).  The runs of the last
repetition are compared: every run in step must be its solo run bit for bit (nlike, ndead, log Z, the dead array), or the figures are not of
the same work.  JSON to argv[1] (default: stdout):

    python tools/bench_in_step_device.py profiles/in_step_device.json"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polychordlite_amd import _ctypes_api as api  # noqa: E402
from polychordlite_amd import repeats  # noqa: E402

RUNS, REPS = 16, 5
SEEDS = [500 + k for k in range(RUNS)]

GAUSS = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s = 0.0, m = 0.0;
    for (int i = 0; i < nDims; ++i) { const double z = (theta[i] - 0.5) / 0.1; s += z * z; m += theta[i]; }
    for (int e = 0; e < nDerived; ++e) phi[e] = (e == 0) ? s : m * (double)e;
    return -s / 2.0 + 1.3836465597893728 * (double)nDims;
}
"""
# data: n x values, then n y values (a structure of arrays: lane-consecutive i reads consecutive addresses)
LINE_TERMS = r"""
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{
    const double r = data[ndata / 2 + i] - (theta[0] * data[i] + theta[1]);
    return r * r;
}
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sum;
    return -sum / 2.0;
}
"""


def line_data(n):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, n)
    return np.concatenate([x, 0.3 * x + 0.6 + rng.normal(0.0, 1.0, n)])


def legs():
    out = {}
    L, P, keep = api.make_problem("source", 20, 2, source=api.source_create(GAUSS))
    out["plain_source"] = dict(D=20, nDer=2, nlive=2000, num_repeats=40, L=L, P=P, keep=keep)
    L, P, keep = api.make_problem("source", 2, 1, source=api.source_create(LINE_TERMS, data=line_data(256), nterms=256), lo=-2.0, hi=2.0)
    out["terms_source"] = dict(D=2, nDer=1, nlive=1000, num_repeats=10, L=L, P=P, keep=keep)
    L, P, keep = api.make_problem("gaussian", 20, 2, prior_table=[("gaussian", (0.5, 1.0))] * 20)
    out["prior_table"] = dict(D=20, nDer=2, nlive=2000, num_repeats=40, L=L, P=P, keep=keep)
    return out


def settings(leg, seed=1):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), leg["D"], leg["nDer"])
    s.nlive, s.num_repeats, s.seed = leg["nlive"], leg["num_repeats"], seed
    return s


def in_step(leg):
    t = time.perf_counter()
    merged, runs = repeats.run_in_step(settings(leg), leg["L"], leg["P"], SEEDS, max_in_flight=RUNS)
    return time.perf_counter() - t, runs


def solo(leg):
    t = time.perf_counter()
    runs = [api.run(settings(leg, seed), leg["L"], leg["P"]) for seed in SEEDS]
    return time.perf_counter() - t, runs


def rtc_stats():
    n, sec = C.c_long(), C.c_double()
    api.load().pchip_rtc_stats(C.byref(n), C.byref(sec))
    return n.value, sec.value


def main():
    lg = legs()
    out = dict(runs=RUNS, reps=REPS, seeds=SEEDS, legs={})
    for name, leg in lg.items():                    # warm-up: run-time compilations, module loads, block caches
        n0, s0 = rtc_stats()
        solo(leg); in_step(leg)
        n1, s1 = rtc_stats()
        out["legs"][name] = dict(shape={k: leg[k] for k in ("D", "nDer", "nlive", "num_repeats")}, compile=dict(units=n1 - n0, seconds=s1 - s0), reps=[])
    last = {}
    for _ in range(REPS):
        for name, leg in lg.items():
            ws, rs = solo(leg)
            wi, ri = in_step(leg)
            nl = sum(int(r["nlike"]) for r in ri)
            assert nl == sum(int(r["nlike"]) for r in rs), name
            out["legs"][name]["reps"].append(dict(solo_wall_s=ws, in_step_wall_s=wi, nlike=nl, solo_evals_per_s=nl / ws, in_step_evals_per_s=nl / wi, x_solo=ws / wi))
            last[name] = (rs, ri)
    for name, (rs, ri) in last.items():
        same = all(a["nlike"] == b["nlike"] and a["ndead"] == b["ndead"] and a["logZ"] == b["logZ"] and np.array_equal(a["dead"], b["dead"]) for a, b in zip(ri, rs))
        o = out["legs"][name]
        o["in_step_is_solo_bit_for_bit"] = bool(same)
        o["path_in_step"] = {k: ri[0]["path"][k] for k in ("slice_wave", "slice_lane", "slice_step", "source_kernels", "source_terms", "device_prior")}
        for key in ("solo_evals_per_s", "in_step_evals_per_s", "x_solo", "solo_wall_s", "in_step_wall_s"):
            v = [r[key] for r in o["reps"]]
            o[key] = dict(median=statistics.median(v), min=min(v), max=max(v))
        o["ms_per_run"] = dict(solo=1e3 * o["solo_wall_s"]["median"] / RUNS, in_step=1e3 * o["in_step_wall_s"]["median"] / RUNS)
    txt = json.dumps(out, indent=1)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")
    print(txt)
    if not all(o["in_step_is_solo_bit_for_bit"] for o in out["legs"].values()):
        sys.exit("a run in step is not its solo run: the figures above are not of the same work")


if __name__ == "__main__":
    main()
