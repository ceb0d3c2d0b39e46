"""Evaluations per second of configs/gaussian_gaussian_prior_nlive2000.ini's problem (20-D Gaussian likelihood, nlive 2000, num_repeats 40,
two derived parameters, `gaussian` priors N(0.5, 1)) three ways, one process, a warm-up of every leg first, whole runs timed to the end of
pchip_run (which synchronises the device), the legs alternated REPS times, evaluations/s = nlike / wall:

  a  host_prior      the prior table on the host -- what option device_prior = 0 gives and what every ini run with such priors was before:
                     likelihood (polychord_hip_gaussian) and prior (polychord_hip_table_prior) as host callbacks, the device proposes;
  b  device_prior    the table evaluated inside the sampling kernels (pchip_prior.kind = 2);
  c  box_functor     the ceiling: the uniform box with the likelihood as a general device functor (settings.ablate bit 0).

Writes JSON to argv[1] (default: stdout):  python tools/bench_device_priors.py profiles/device_priors.json

--source: the same shape with the likelihood as a device source (pchip_source_create_prior: one handle for all three legs), the prior
three ways -- what a prior written as device source costs next to the table and the box:

  a  table           twenty `gaussian` priors as a table (pchip_prior.kind = 2);
  b  prior_source    the same transform, mu + sigma normcdfinv(cube_i), as the handle's pchip_prior_param (pchip_prior.kind = 3);
  c  box             the uniform box (pchip_prior.kind = 1).

python tools/bench_device_priors.py --source profiles/prior_source.json"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polychordlite_amd import _ctypes_api as api  # noqa: E402

D, NDER, NR, NLIVE, REPS = 20, 2, 40, 2000, 3
TABLE = [("gaussian", (0.5, 1.0))] * D


def settings(ablate=0):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, NDER)
    s.nlive, s.num_repeats, s.seed, s.ablate = NLIVE, NR, 7, ablate
    return s


def legs():
    lib = api.load()
    lib.polychord_hip_set_gaussian(0.5, 0.1)
    api.set_table_prior(TABLE)
    La, Pa, ka = api.make_problem("gaussian", D, NDER)
    La.kind = 0; La.fn = C.cast(lib.polychord_hip_gaussian, C.c_void_p)
    Pa.kind = api.PRIOR_CALLBACK; Pa.fn = C.cast(lib.polychord_hip_table_prior, C.c_void_p)
    Lb, Pb, kb = api.make_problem("gaussian", D, NDER, prior_table=TABLE)
    Lc, Pc, kc = api.make_problem("gaussian", D, NDER)
    return {"host_prior": (La, Pa, 0, ka), "device_prior": (Lb, Pb, 0, kb), "box_functor": (Lc, Pc, 1, kc)}


SOURCE = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s = 0.0, m = 0.0;
    for (int i = 0; i < nDims; ++i) { const double z = (theta[i] - 0.5) / 0.1; s += z * z; m += theta[i]; }
    for (int e = 0; e < nDerived; ++e) phi[e] = (e == 0) ? s : m * (double)e;
    return -s / 2.0 + 1.3836465597893728 * (double)nDims;
}
__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata)
{
    return data[0] + data[1] * normcdfinv(cube[i]);
}
"""


def source_legs():
    h = api.source_create(SOURCE, data=[0.5, 1.0], prior=True)
    La, Pa, ka = api.make_problem("source", D, NDER, source=h, prior_table=TABLE)
    Lb, Pb, kb = api.make_problem("source", D, NDER, source=h, prior_source=True)
    Lc, Pc, kc = api.make_problem("source", D, NDER, source=h)
    return {"table": (La, Pa, 0, ka), "prior_source": (Lb, Pb, 0, kb), "box": (Lc, Pc, 0, kc)}


def one(L, P, ablate):
    t = time.perf_counter()
    g = api.run(settings(ablate), L, P)
    wall = time.perf_counter() - t
    return dict(wall_s=wall, nlike=int(g["nlike"]), ndead=int(g["ndead"]), logZ=g["logZ"], evals_per_s=g["nlike"] / wall,
                device_prior_launches=g["path"]["device_prior"], slice_wave=g["path"]["slice_wave"])


def main():
    source = "--source" in sys.argv
    if source:
        sys.argv.remove("--source")
    lg = source_legs() if source else legs()
    out = dict(shape=dict(nDims=D, nDerived=NDER, nlive=NLIVE, num_repeats=NR, prior="gaussian 0.5 1.0"), reps=REPS, runs={k: [] for k in lg})
    for k, (L, P, ab, keep) in lg.items():          # warm-up: module loads, block caches
        one(L, P, ab)
    for _ in range(REPS):
        for k, (L, P, ab, keep) in lg.items():
            out["runs"][k].append(one(L, P, ab))
    for k, rs in out["runs"].items():
        v = [r["evals_per_s"] for r in rs]
        out[k] = dict(evals_per_s_median=statistics.median(v), evals_per_s_min=min(v), evals_per_s_max=max(v),
                      wall_s_median=statistics.median(r["wall_s"] for r in rs))
    med = {k: out[k]["evals_per_s_median"] for k in lg}
    if source:
        out["likelihood"] = "device source (Gaussian 0.5, 0.1), the same handle in every leg"
        out["prior_source_over_table"] = med["prior_source"] / med["table"]
        out["prior_source_over_box"] = med["prior_source"] / med["box"]
        for k in lg:
            out[k]["ms_per_run_median"] = 1e3 * out[k]["wall_s_median"]
    else:
        out["device_over_host"] = med["device_prior"] / med["host_prior"]
        out["device_over_box_functor"] = med["device_prior"] / med["box_functor"]
    txt = json.dumps(out, indent=1)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
