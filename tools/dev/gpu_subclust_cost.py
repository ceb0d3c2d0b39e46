#!/usr/bin/env python
"""gpu_subclust_cost.py -- one BASELINE configs[2] shape (10-D Rastrigin, nlive 1000, num_repeats 30, kNN clustering, seed 1) with
and without sub-dimension clustering on x1 and x2: wall time of the run and its updates, path counters.  Run it under
`rocprofv3 --kernel-trace --stats` (one process per variant) for the clustering kernels' time per update.

usage: gpu_subclust_cost.py [plain|sub] [repeats]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from polychordlite_amd import _ctypes_api as api  # noqa: E402


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "sub"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    lib = api.load()
    L, P, keep = api.make_problem("rastrigin", 10, 0, -5.12, 5.12)
    out = []
    for k in range(reps + 1):                   # (the first run warms the caches and the code objects up)
        s = api.Settings(); lib.pchip_settings_default(C.byref(s), 10, 0)
        s.nlive, s.num_repeats, s.seed, s.do_clustering = 1000, 30, 1, 1
        sd = api.set_sub_clustering(s, [0, 1] if which == "sub" else [])
        g = api.run(s, L, P)
        if k:
            out.append(dict(t_total=g["t_total"], ndead=int(g["ndead"]), nlike=int(g["nlike"]), logZ=g["logZ"], logZerr=g["logZerr"],
                            nupdates=int(g["nupdates"]), ncluster_peak=int(g["ncluster_peak"]), batch=int(g["batch"]),
                            subcluster_passes=g["path"]["subcluster_passes"], subcluster_splits=g["path"]["subcluster_splits"]))
        del sd
    print(json.dumps(dict(variant=which, runs=out)))


if __name__ == "__main__":
    main()
