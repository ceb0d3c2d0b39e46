#!/usr/bin/env python
"""bench_adaptive_priors.py -- the mean k_slice launch time of a 20-D Gaussian run at nlive 2000 under an adaptive_sorted_uniform block of
20 and under a sorted_uniform block of 20 (the nearest table without an adaptive block), by the engine's own stopwatch
(settings.profile = 1).  GPU only.  One warm-up run per table, then the seeds in turn, the two tables alternating; the record goes to
--out (profiles/adaptive_priors.json is such a record).  --tables sorted restricts the run to the tables an older library knows
(PCHIP_LIB names it): the same table through two builds, for the question whether the adaptive code costs the old tables anything."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from polychordlite_amd import _ctypes_api as api  # noqa: E402

D, NLIVE, REPEATS, SEEDS = 20, 2000, 40, (1, 2, 3)
TABLES = {"sorted_uniform_20": [(7, 1, (0.0, 1.0))] * D, "adaptive_sorted_uniform_20": [(11, 1, (0.0, 1.0))] * D}


def one(entries, seed):
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, 0)
    s.nlive, s.num_repeats, s.seed, s.profile = NLIVE, REPEATS, seed, 1
    L, P, keep = api.make_problem("gaussian", D, 0, mu=0.5, sigma=0.1, prior_table=entries)
    g = api.run(s, L, P)
    assert g["path"]["device_prior"] > 0
    k = g["kernel_time"]["k_slice"]
    return dict(seed=seed, k_slice_mean_us=1e6 * k["total_s"] / k["launches"], k_slice_launches=k["launches"], k_slice_total_s=k["total_s"],
                nlike=g["nlike"], ndead=g["ndead"], logZ=g["logZ"], t_loop_s=g["t_loop"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tables", default="sorted,adaptive")
    ap.add_argument("--label", default="this build")
    a = ap.parse_args()
    names = [n for n in TABLES if n.split("_")[0] in a.tables.split(",")]
    for n in names:
        one(TABLES[n], 99)                                  # warm-up: code objects, the first launches of every kernel the shape takes
    runs = {n: [] for n in names}
    for seed in SEEDS:
        for n in names:
            runs[n].append(one(TABLES[n], seed))
            print(n, runs[n][-1], flush=True)
    rec = dict(label=a.label, shape=dict(nDims=D, nlive=NLIVE, num_repeats=REPEATS, likelihood="gaussian 0.5 0.1", seeds=list(SEEDS), warm_up_runs=1),
               k_slice_mean_us={n: sum(r["k_slice_mean_us"] for r in runs[n]) / len(runs[n]) for n in names}, runs=runs)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec["k_slice_mean_us"]))


if __name__ == "__main__":
    main()
