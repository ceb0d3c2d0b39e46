#!/usr/bin/env python3
"""What a device source costs behind the PolyChord-interface doors (polychord_hip_set_source), two measurements:
 1. wall time of a door run (pypolychord.run, <root>.stats and the dead-point files) with a terms source against pchip_run of the same
    problem: the 256-point line fit of tests/test_source_terms.py, nlive 500, num_repeats 6, the same seed
 2. evaluations a second (nlike / wall time) of a 20-D source under a HOST prior: the door's batched evaluator against the scalar
    polychord_hip_source_loglike as a plain callback (a C shim the library does not recognise), both under the same C identity prior

    python tools/bench_source_doors.py

Behind a warm-up (run-time compilation, module loads), five interleaved repeats; a figure is given as the median with its spread (min, max)."""
import ctypes as C
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polychordlite_amd import _ctypes_api as api          # noqa: E402
from polychordlite_amd import pypolychord                  # noqa: E402
from polychordlite_amd.pypolychord import device_likelihoods as dl   # noqa: E402
from tests.test_device_source import GAUSS_SRC             # noqa: E402
from tests.test_source_terms import LINE_TERMS, _line_data  # noqa: E402

lib = api.load()
tmp = tempfile.mkdtemp()


def median(v):
    return statistics.median(v), min(v), max(v)


# ------------------------------------------------------------------------------------------------------------------ 1
D, nDer, NT = 2, 1, 256
src = dl.Source(LINE_TERMS, nDerived=nDer, data=_line_data(NT), nterms=NT)


def door(i):
    t0 = time.perf_counter()
    pypolychord.run(src, D, nDerived=nDer, prior=dl.UniformPrior(0.0, 1.0), nlive=500, num_repeats=6, seed=5, do_clustering=False, feedback=0,
                    base_dir=os.path.join(tmp, "d%d" % i), file_root="line", read_resume=False, write_resume=False, posteriors=False, equals=False,
                    cluster_posteriors=False, write_live=False, write_prior=False, write_dead=True, write_stats=True)
    return time.perf_counter() - t0


def plain():
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    s.nlive, s.num_repeats, s.seed, s.do_clustering, s.feedback, s.compression_factor = 500, 6, 5, 0, 0, float(np.exp(-1))
    L, P, keep = api.make_problem("source", D, nDer, source=src.handle)
    t0 = time.perf_counter()
    g = api.run(s, L, P)
    return time.perf_counter() - t0, g


import warnings
warnings.simplefilter("ignore")
door(0); plain()
td, tp = [], []
for i in range(5):
    td.append(door(i + 1))
    t, g = plain()
    tp.append(t)
st = open(os.path.join(tmp, "d5", "line.stats")).read()
print("1. line fit 256 points, terms form, nlive 500, num_repeats 6: ndead %d nlike %d (door .stats ndead %s)" % (g["ndead"], g["nlike"], re.search(r"ndead:\s*(\d+)", st).group(1)))
print("   door (pypolychord.run, .stats + _dead files): median %.1f ms (min %.1f max %.1f)" % tuple(1e3 * x for x in median(td)))
print("   pchip_run:                                    median %.1f ms (min %.1f max %.1f); engine t_total %.1f ms" % (tuple(1e3 * x for x in median(tp)) + (1e3 * g["t_total"],)))

# ------------------------------------------------------------------------------------------------------------------ 2
shim_c = os.path.join(tmp, "shim.cpp")
open(shim_c, "w").write("""
extern "C" double polychord_hip_source_loglike(double *, int, double *, int);
extern "C" double shim_like(double *t, int n, double *p, int nd) { return polychord_hip_source_loglike(t, n, p, nd); }
extern "C" void shim_prior(double *c, double *t, int n) { for (int i = 0; i < n; ++i) t[i] = c[i]; }
""")
shim_so = os.path.join(tmp, "libshim.so")
subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", shim_c, "-o", shim_so, "-L" + os.path.join(ROOT, "polychordlite_amd"), "-lpolychord_hip",
                       "-Wl,-rpath," + os.path.join(ROOT, "polychordlite_amd")])
shim = C.CDLL(shim_so)
D2 = 20
gsrc = dl.Source(GAUSS_SRC)
gsrc.configure(D2)
f = lib.polychord_c_interface
f.restype = None
f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_bool, C.c_int, C.c_double,
              C.c_double, C.c_int, C.c_double] + [C.c_bool] * 11 + [C.c_double, C.c_bool, C.c_int, C.c_int, C.c_char_p,
              C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double),
              C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
base = os.path.join(tmp, "b")
os.makedirs(os.path.join(base, "clusters"))


def hostprior(like_ptr, root, max_ndead):
    gf = (C.c_double * 1)(1.0); gd = (C.c_int * 1)(D2); ll = (C.c_double * 1)(0.0); nl = (C.c_int * 1)(0); comm = C.c_int(0)
    t0 = time.perf_counter()
    f(like_ptr, C.cast(shim.shim_prior, C.c_void_p), None, 200, 40, -1, -1, False, 0, 1e-3, -1e30, max_ndead, 0.0, False, False, False, False, False,
      False, True, False, False, False, False, float(np.exp(-1)), True, D2, 0, base.encode(), root.encode(), 1, gf, gd, 0, ll, nl, 9, C.byref(comm))
    dt = time.perf_counter() - t0
    nlike = int(re.search(r"nlike:\s*(\d+)", open(os.path.join(base, root + ".stats")).read()).group(1))
    return nlike / dt, nlike, dt


batched = C.cast(lib.polychord_hip_source_loglike, C.c_void_p)
scalar = C.cast(shim.shim_like, C.c_void_p)
hostprior(batched, "w1", 200); hostprior(scalar, "w2", 50)
rb, rs = [], []
for i in range(5):
    rb.append(hostprior(batched, "bt", 2000))
    rs.append(hostprior(scalar, "sc", 100))
print("2. 20-D Gaussian source under a host prior (a C identity prior), nlive 200, num_repeats 40, auto batch")
print("   batched evaluator (max_ndead 2000): median %.0f evaluations/s (min %.0f max %.0f); nlike %d in %.3f s" % (median([r[0] for r in rb]) + (rb[-1][1], rb[-1][2])))
print("   scalar callback   (max_ndead 100):  median %.0f evaluations/s (min %.0f max %.0f); nlike %d in %.3f s" % (median([r[0] for r in rs]) + (rs[-1][1], rs[-1][2])))
lib.polychord_hip_set_source(0)
src.close(); gsrc.close()
