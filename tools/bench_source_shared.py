#!/usr/bin/env python3
"""What shared values (pchip_source_create_shared) buy: INTEGRATION's worked example, a model tabulated on a grid and interpolated to the
data points, with a table entry that costs something -- the comoving distance of flat LCDM at NSH redshifts, each an 8-point midpoint
quadrature of 1 / sqrt(Om (1 + z)^3 + 1 - Om); N supernovae interpolate the table and compare 5 log10((1 + z) D) + M with their moduli.
theta = (Om, M).  Three sources of the same likelihood:

    shared    the table as NSH shared values, one lane per node, once per evaluated point
    terms     what could be written before: a terms-form source in which every term computes the two nodes it interpolates between
    plain     the replay of `shared` as a plain pchip_loglikelihood (every lane fills the table and walks all the terms), which places the
              result beside tools/bench_source_quad.py's table; `shared` and `plain` are the same run (same_run)

at NSH 64 and 256 times N 256 and 1024, nlive 500, num_repeats 10, one seed.

    python tools/bench_source_shared.py [out.json]

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
from tests.test_source_terms import REPLAY_WRAPPER      # noqa: E402

REPS = 5
SIZES = [(nsh, n) for nsh in (64, 256) for n in (256, 1024)]
LO, HI = [0.05, -1.0], [0.95, 1.0]
ZMAX, SIGMA, TRUTH = 1.5, 0.1, (0.3, 0.1)

# data = z[NSH] | j[NPT] | w[NPT] | zp[NPT] | d[NPT]: the grid, the node below every supernova and its weight, its redshift and modulus
COMMON = r"""
#pragma clang fp contract(off)
static __device__ double sn_distance(double om, double z)
{
    double s = 0.0;
    for (int q = 0; q < 8; ++q) {
        const double y = 1.0 + z * ((q + 0.5) / 8.0);
        s = s + 1.0 / sqrt(om * y * y * y + (1.0 - om));
    }
    return z * s / 8.0;
}
static __device__ double sn_term(double d0, double d1, double m, const double *data, long i)
{
    const double dist = d0 + data[NSH + NPT + i] * (d1 - d0);
    const double mu = 5.0 * log10((1.0 + data[NSH + 2 * NPT + i]) * dist) + m;
    const double r = (data[NSH + 3 * NPT + i] - mu) / 0.1;
    return r * r;
}
"""
SHARED = COMMON + r"""
__device__ double pchip_shared_value(const double *theta, int nDims, const double *data, long ndata, long k)
{
    return sn_distance(theta[0], data[k]);
}
__device__ double pchip_logl_term(const double *theta, const double *shared, int nDims, const double *data, long ndata, long i)
{
    const long j = (long)data[NSH + i];
    return sn_term(shared[j], shared[j + 1], theta[1], data, i);
}
__device__ double pchip_logl_finish(double sum, const double *theta, const double *shared, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sum;
    if (nDerived > 1) phi[1] = shared[NSH - 1];
    return -sum / 2.0;
}
"""
TERMS = COMMON + r"""
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{
    const long j = (long)data[NSH + i];
    return sn_term(sn_distance(theta[0], data[j]), sn_distance(theta[0], data[j + 1]), theta[1], data, i);
}
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sum;
    if (nDerived > 1) phi[1] = sn_distance(theta[0], data[NSH - 1]);
    return -sum / 2.0;
}
"""
# the replay of tests/test_source_shared.py: the table filled serially behind a copy of theta, then the terms form's serial replay
PLAIN = SHARED + r"""
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{ return pchip_logl_term(theta, theta + nDims, nDims, data, ndata, i); }
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{ return pchip_logl_finish(sum, theta, theta + nDims, phi, nDims, nDerived, data, ndata); }
""" + REPLAY_WRAPPER.replace("pchip_loglikelihood", "replay_of_the_form") + r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double buf[2 + NSH];
    buf[0] = theta[0]; buf[1] = theta[1];
    for (long k = 0; k < NSH; ++k) buf[2 + k] = pchip_shared_value(theta, nDims, data, ndata, k);
    return replay_of_the_form(buf, phi, nDims, nDerived, data, ndata);
}
"""


def distance(om, z):
    y = 1.0 + z[..., None] * ((np.arange(8) + 0.5) / 8.0)
    return z * np.sum(1.0 / np.sqrt(om * y ** 3 + (1.0 - om)), axis=-1) / 8.0


def sn_data(nsh, n, seed=3):
    rng = np.random.default_rng(seed)
    z = ZMAX * (np.arange(nsh) + 1.0) / nsh
    zp = np.sort(rng.uniform(z[0], z[-1], n))
    j = np.clip(np.searchsorted(z, zp, side="right") - 1, 0, nsh - 2)
    w = (zp - z[j]) / (z[j + 1] - z[j])
    table = distance(TRUTH[0], z)
    d = 5.0 * np.log10((1.0 + zp) * (table[j] + w * (table[j + 1] - table[j]))) + TRUTH[1] + rng.normal(0.0, SIGMA, n)
    return np.concatenate([z, j.astype(np.float64), w, zp, d])


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
    for nsh, n in SIZES:
        data = sn_data(nsh, n)
        opts = (f"-DNSH={nsh}", f"-DNPT={n}", f"-DNTERMS={n}")
        legs = {"shared": api.source_create(SHARED, options=opts, data=data, nterms=n, shared=nsh),
                "terms": api.source_create(TERMS, options=opts, data=data, nterms=n),
                "plain": api.source_create(PLAIN, options=opts, data=data)}
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
        o["same_run"] = bool(np.array_equal(last["shared"]["dead"], last["plain"]["dead"]))
        o["terms_over_shared"] = o["terms"]["run_s"]["median"] / o["shared"]["run_s"]["median"]
        o["plain_over_shared"] = o["plain"]["run_s"]["median"] / o["shared"]["run_s"]["median"]
        out["sizes"][f"{nsh}x{n}"] = o
        print(f"nshared {nsh} nterms {n}: terms / shared = {o['terms_over_shared']:.2f}, plain / shared = {o['plain_over_shared']:.2f}; "
              f"same run: {o['same_run']}", file=sys.stderr, flush=True)
        for h in legs.values():
            api.load().pchip_source_destroy(h)
    txt = json.dumps(out, indent=1)
    if args:
        open(args[0], "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
