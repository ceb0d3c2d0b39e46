"""Evaluations per second of a data-sum likelihood handed over as device source, in its two forms.  The straight-line fit (2-D, nlive 1000,
num_repeats 10, one derived parameter) over NTERMS data points, NTERMS = 64, 1 024, 16 384:

  a  plain   pchip_loglikelihood with the loop over the data inside: every lane of the wavefront runs all of it, and the derived
             parameter of an accepted point is a second call;
  b  terms   pchip_logl_term + pchip_logl_finish (pchip_source_create_terms): the lanes share the loop, the sum is kept for finish;
  r  replay  the terms text behind a plain wrapper that adds in the terms form's order -- run ONCE per size, not timed: its nlike must be
             (b)'s, which shows that (b) is the same run; against (a) the sums differ in the last bits, so compare evaluations/s;
  c  host    the same likelihood compiled for the host as a callback, at 1 024 only -- what a user has without any source.

And the 20-D Gaussian of tools/dev/measure_device_source.py (nlive 2000, num_repeats 40, two derived parameters) as a plain source and as
20 terms + finish, milliseconds a run, next to profiles/device_source_c1.json.

One process; a warm-up run of every leg first (run-time compilation outside the timing, its seconds reported from pchip_rtc_stats); the
legs alternated REPS times; whole runs timed to the end of pchip_run.  JSON to argv[1] (default: stdout):

    python tools/bench_source_terms.py profiles/source_terms.json
    python tools/bench_source_terms.py --single terms 1024        (warm-up + one run of one leg: for a kernel trace)"""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polychordlite_amd import _ctypes_api as api  # noqa: E402

REPS, SIZES = 3, (64, 1024, 16384)

# data: NTERMS x values, then NTERMS y values (a structure of arrays: lane-consecutive i reads consecutive addresses)
LINE_PLAIN = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    const long n = ndata / 2;
    double s = 0.0;
    for (long i = 0; i < n; ++i) { const double r = data[n + i] - (theta[0] * data[i] + theta[1]); s += r * r; }
    if (nDerived > 0) phi[0] = s;
    return -s / 2.0;
}
"""
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
REPLAY = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s[64];
    for (int l = 0; l < 64; ++l) {
        double a = 0.0;
        for (long i = l; i < NTERMS; i += 64) a = a + pchip_logl_term(theta, nDims, data, ndata, i);
        s[l] = a;
    }
    for (int w = 1; w < 16; w *= 2)
        for (int l = 0; l < 64; l += 2 * w) s[l] = s[l] + s[l + w];
    return pchip_logl_finish((s[0] + s[16]) + (s[32] + s[48]), theta, phi, nDims, nDerived, data, ndata);
}
"""
CONTRACT_OFF = "#pragma clang fp contract(off)\n"      # (the replay leg only: same bits as the terms form needs the same arithmetic)

GD, GNDER, GNR, GNLIVE = 20, 2, 40, 2000
LOG_VN = 0.5 * GD * math.log(math.pi) - math.lgamma(1.0 + GD / 2.0)
GAUSS_PLAIN = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s = 0.0, r2 = 0.0;
    for (int i = 0; i < nDims; ++i) { const double z = (theta[i] - 0.5) / 0.1; s += z * z; r2 += (theta[i] - 0.5) * (theta[i] - 0.5); }
    if (nDerived > 0) phi[0] = sqrt(r2);
    if (nDerived > 1) phi[1] = (double)nDims * log(phi[0]) + LOG_VN;
    return -s / 2.0 + 1.3836465597893728 * (double)nDims;
}
"""
GAUSS_TERMS = r"""
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{
    const double z = (theta[i] - 0.5) / 0.1;
    return z * z;
}
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = 0.1 * sqrt(sum);
    if (nDerived > 1) phi[1] = (double)nDims * log(phi[0]) + LOG_VN;
    return -sum / 2.0 + 1.3836465597893728 * (double)nDims;
}
"""


def line_data(n):
    rng = np.random.default_rng(3)
    x = np.linspace(-1.0, 1.0, n)
    return np.concatenate([x, 0.3 * x + 0.6 + rng.normal(0.0, 1.0, n)])


def rtc_stats():
    n, s = C.c_long(), C.c_double()
    api.load().pchip_rtc_stats(C.byref(n), C.byref(s))
    return n.value, s.value


def one(L, P, D, nDer, nlive, nr):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    s.nlive, s.num_repeats, s.seed = nlive, nr, 7
    t = time.perf_counter()
    g = api.run(s, L, P)
    wall = time.perf_counter() - t
    return dict(wall_s=wall, nlike=int(g["nlike"]), ndead=int(g["ndead"]), logZ=g["logZ"], evals_per_s=g["nlike"] / wall,
                source_kernels=g["path"]["source_kernels"], source_terms=g["path"]["source_terms"], slice_wave=g["path"]["slice_wave"])


def line_legs(n, td):
    data = line_data(n)
    legs = {"plain": api.source_create(LINE_PLAIN, data=data), "terms": api.source_create(LINE_TERMS, data=data, nterms=n),
            "replay": api.source_create(CONTRACT_OFF + LINE_TERMS + REPLAY, options=(f"-DNTERMS={n}",), data=data)}
    out = {k: api.make_problem("source", 2, 1, source=h) for k, h in legs.items()}
    if n == 1024:
        cpp, so = os.path.join(td, "line.cpp"), os.path.join(td, "libline.so")
        open(cpp, "w").write(LINE_PLAIN + f"\nstatic double D_[{2 * n}];\nextern \"C\" void set_data(const double *d) {{ for (int i = 0; i < {2 * n}; ++i) D_[i] = d[i]; }}\n"
                             f"extern \"C\" double host_logl(double *t, int D, double *phi, int nDer) {{ return pchip_loglikelihood(t, phi, D, nDer, D_, {2 * n}); }}\n")
        subprocess.check_call(["g++", "-O3", "-march=native", "-shared", "-fPIC", "-D__device__=", "-x", "c++", cpp, "-o", so])
        hl = C.CDLL(so)
        hl.set_data(data.ctypes.data_as(C.c_void_p))
        Lc, Pc, kc = api.make_problem("gaussian", 2, 1)
        Lc.kind = 0; Lc.fn = C.cast(hl.host_logl, C.c_void_p)
        out["host"] = (Lc, Pc, [kc, hl])
    return out


def summary(rs):
    v = sorted(r["evals_per_s"] for r in rs)
    w = sorted(r["wall_s"] for r in rs)
    return dict(evals_per_s_median=v[len(v) // 2], evals_per_s_min=v[0], evals_per_s_max=v[-1], wall_s_median=w[len(w) // 2], wall_s_min=w[0],
                wall_s_max=w[-1], nlike=rs[-1]["nlike"], ndead=rs[-1]["ndead"], logZ=rs[-1]["logZ"], source_terms=rs[-1]["source_terms"])


def main():
    args = sys.argv[1:]
    with tempfile.TemporaryDirectory() as td:
        if args and args[0] == "--single":
            L, P, keep = line_legs(int(args[2]), td)[args[1]]
            one(L, P, 2, 1, 1000, 10)
            print(json.dumps(one(L, P, 2, 1, 1000, 10)))
            return
        out = dict(shape=dict(nDims=2, nDerived=1, nlive=1000, num_repeats=10), reps=REPS, sizes={})
        for n in SIZES:
            legs = line_legs(n, td)
            o = dict(compile={})
            for k, (L, P, keep) in legs.items():          # warm-up: run-time compilation, module loads, block caches
                c0 = rtc_stats()
                w = one(L, P, 2, 1, 1000, 10)
                c1 = rtc_stats()
                o["compile"][k] = dict(units=c1[0] - c0[0], seconds=c1[1] - c0[1], first_run_s=w["wall_s"])
                if k == "replay":
                    o["replay_nlike"] = w["nlike"]
            timed = [k for k in legs if k != "replay"]
            runs = {k: [] for k in timed}
            for _ in range(REPS):
                for k in timed:
                    runs[k].append(one(*legs[k][:2], 2, 1, 1000, 10))
            for k in timed:
                o[k] = summary(runs[k])
            o["same_run_as_replay"] = o["terms"]["nlike"] == o["replay_nlike"]
            o["terms_over_plain"] = o["terms"]["evals_per_s_median"] / o["plain"]["evals_per_s_median"]
            if "host" in o:
                o["terms_over_host"] = o["terms"]["evals_per_s_median"] / o["host"]["evals_per_s_median"]
            out["sizes"][str(n)] = o
            print(f"nterms {n}: terms / plain = {o['terms_over_plain']:.2f}", file=sys.stderr, flush=True)
        # the 20-D Gaussian of profiles/device_source_c1.json
        opts = (f"-DLOG_VN={LOG_VN!r}",)
        g = {"plain": api.source_create(GAUSS_PLAIN, options=opts), "terms": api.source_create(GAUSS_TERMS, options=opts, nterms=GD)}
        gl = {k: api.make_problem("source", GD, GNDER, source=h) for k, h in g.items()}
        for k in gl:
            one(*gl[k][:2], GD, GNDER, GNLIVE, GNR)
        runs = {k: [] for k in gl}
        for _ in range(REPS):
            for k in gl:
                runs[k].append(one(*gl[k][:2], GD, GNDER, GNLIVE, GNR))
        out["gaussian20"] = dict(shape=dict(nDims=GD, nDerived=GNDER, nlive=GNLIVE, num_repeats=GNR),
                                 **{k: dict(ms=sorted(r["wall_s"] for r in runs[k])[REPS // 2] * 1e3, ms_all=[r["wall_s"] * 1e3 for r in runs[k]],
                                            nlike=runs[k][-1]["nlike"], ndead=runs[k][-1]["ndead"], logZ=runs[k][-1]["logZ"]) for k in gl})
    txt = json.dumps(out, indent=1)
    if args:
        open(args[0], "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
