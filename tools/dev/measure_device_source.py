"""Milliseconds per run at BASELINE configs[1]'s shape (20-D Gaussian, nlive 2000, num_repeats 40, two derived parameters) for the
built-in likelihood, the built-in as a general device functor (settings.ablate bit 0), the built-in through the run-time module
(settings.ablate bit 15), the same Gaussian and derived parameters as a device source, and that source compiled for the host as a
callback; plus the first run's compile time.  Writes JSON to argv[1] (default: stdout)."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from polychordlite_amd import _ctypes_api as api  # noqa: E402

SRC = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s = 0.0, r2 = 0.0;
    for (int i = 0; i < nDims; ++i) { const double z = (theta[i] - 0.5) / 0.1; s += z * z; r2 += (theta[i] - 0.5) * (theta[i] - 0.5); }
    if (nDerived > 0) phi[0] = sqrt(r2);
    if (nDerived > 1) phi[1] = (double)nDims * log(phi[0]) + LOG_VN;    /* gaussian.f90:36-37 */
    return -s / 2.0 + 1.3836465597893728 * (double)nDims;                /* - nDims (log 0.1 + log(2 pi) / 2) */
}
"""
D, NDER, NR, NLIVE, REPS = 20, 2, 40, 2000, 3
LOG_VN = 0.5 * D * math.log(math.pi) - math.lgamma(1.0 + D / 2.0)


def settings(ablate=0):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, NDER)
    s.nlive, s.num_repeats, s.seed, s.ablate = NLIVE, NR, 7, ablate
    return s


def timed(L, P, ablate=0):
    ms = []
    for _ in range(REPS):
        t = time.perf_counter(); g = api.run(settings(ablate), L, P); ms.append((time.perf_counter() - t) * 1e3)
    return dict(ms=sorted(ms)[len(ms) // 2], ms_all=ms, ndead=g["ndead"], nlike=g["nlike"], logZ=g["logZ"])


def main():
    lib = api.load()
    out = dict(shape=dict(nDims=D, nDerived=NDER, nlive=NLIVE, num_repeats=NR), reps=REPS)
    L, P, k = api.make_problem("gaussian", D, NDER)
    api.run(settings(), L, P)
    out["builtin"] = timed(L, P)
    out["builtin_general_functor"] = timed(L, P, 1)
    t = time.perf_counter(); api.run(settings(1 << 15), L, P); out["builtin_bit15_first_run_ms"] = (time.perf_counter() - t) * 1e3
    out["builtin_bit15"] = timed(L, P, 1 << 15)
    t = time.perf_counter(); h = api.source_create(SRC, options=(f"-DLOG_VN={LOG_VN!r}",)); out["source_create_ms"] = (time.perf_counter() - t) * 1e3
    Ls, Ps, k2 = api.make_problem("source", D, NDER, source=h)
    n0, s0 = C.c_long(), C.c_double(); lib.pchip_rtc_stats(C.byref(n0), C.byref(s0))
    t = time.perf_counter(); api.run(settings(), Ls, Ps); out["source_first_run_ms"] = (time.perf_counter() - t) * 1e3
    n1, s1 = C.c_long(), C.c_double(); lib.pchip_rtc_stats(C.byref(n1), C.byref(s1))
    out["source_first_run_compiles"] = n1.value - n0.value; out["source_first_run_compile_s"] = s1.value - s0.value
    out["source"] = timed(Ls, Ps)
    with tempfile.TemporaryDirectory() as td:
        cpp, so = os.path.join(td, "g.cpp"), os.path.join(td, "libg.so")
        open(cpp, "w").write("#include <cmath>\nusing std::sqrt; using std::log;\n" + f"#define LOG_VN {LOG_VN!r}\n" + SRC + '\nextern "C" double host_logl(double *t, int D, double *phi, int nDer)'
                             '{ return pchip_loglikelihood(t, phi, D, nDer, 0, 0); }\n')
        subprocess.check_call(["g++", "-O3", "-march=native", "-shared", "-fPIC", "-D__device__=", "-x", "c++", cpp, "-o", so])
        hl = C.CDLL(so)
        Lc, Pc, k3 = api.make_problem("gaussian", D, NDER)
        Lc.kind = 0; Lc.fn = C.cast(hl.host_logl, C.c_void_p)
        out["host_callback"] = timed(Lc, Pc)
    txt = json.dumps(out, indent=1)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
