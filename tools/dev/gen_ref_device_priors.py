#!/usr/bin/env python
"""gen_ref_device_priors.py -- tests/golden/ref_device_priors.json from the REFERENCE itself: small runs whose ini files use the ten
prior types a prior table takes (tests/test_device_priors.py holds the engine, with the table evaluated inside the sampling kernels and
sequential_rng = 1, to these numbers).  CPU machine only, by hand:

    make -C oracle ref                          # the reference's objects in oracle/_ref/obj/
    python tools/dev/gen_ref_device_priors.py   # builds tools/dev/ref_subclust_driver.cpp (unchanged) in a temporary directory, runs it

Like gen_ref_subclust.py, the script first proves its door: an all-uniform ini run must equal the entry of tests/golden/ref_injected.json
with the same shape and seed (ndead, nlike, logZ), or it stops.  Only the reference's OUTPUT goes into the fixture: the ini text, the
counters and the evidences."""
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from gen_ref_subclust import build, read_stats  # noqa: E402
import subprocess  # noqa: E402

# the door's proof: (like, nDims, nDerived, nlive, num_repeats, seed, clustering) of ref_injected.json entries, box of the likelihood
PROOF = [("gaussian", 4, 1, 100, 20, 2, 0, (0.0, 1.0)), ("twin_gaussian", 4, 1, 120, 8, 9, 1, (-1.0, 1.0))]

# name, like, nDerived, nlive, num_repeats, seed, clustering, parameters: (speed, prior type, block, prior parameters), grade_frac
# (the reference wants one prior type per block number: create_priors stops otherwise)
CASES = [
    ("g6_unsorted_types", "gaussian", 1, 100, 12, 3, 0,
     [(1, "uniform", 1, (0.0, 1.0)), (1, "log_uniform", 2, (0.1, 2.0)), (1, "power_uniform", 3, (0.2, 2.0, 2.0)),
      (1, "gaussian", 4, (0.5, 0.3)), (1, "half_gaussian", 5, (0.3, 0.3)), (1, "exponential", 6, (2.0,))], "1"),
    ("g5_sorted_uniform_block", "gaussian", 1, 100, 10, 4, 0,
     [(1, "uniform", 1, (0.0, 1.0))] + [(1, "sorted_uniform", 2, (0.0, 1.0))] * 4, "1"),
    ("g4_sorted_gaussian_and_exponential", "gaussian", 0, 100, 8, 5, 0,
     [(1, "sorted_gaussian", 1, (0.5, 0.5))] * 2 + [(1, "sorted_exponential", 2, (2.0,))] * 2, "1"),
    ("rast4_gaussian_priors_clustering", "rastrigin", 0, 200, 12, 5, 1, [(1, "gaussian", 1, (0.0, 2.0))] * 4, "1"),
    ("twin4_sorted_half_gaussian_clustering", "twin_gaussian", 1, 120, 8, 9, 1,
     [(1, "uniform", 1, (-1.0, 1.0))] * 2 + [(1, "sorted_half_gaussian", 2, (-0.5, 0.5))] * 2, "1"),
    # two speeds, the fast parameters listed first (permuted hypercube order); grade_frac > 1: the repeats per grade as given, no timing
    ("g4_fast_parameters_first", "gaussian", 1, 100, 0, 6, 0,
     [(2, "gaussian", 1, (0.5, 0.5)), (2, "uniform", 2, (0.0, 1.0)), (1, "exponential", 3, (1.0,)), (1, "log_uniform", 4, (0.1, 2.0))], "4 8"),
]


def ini_text(nDer, nlive, nr, seed, clustering, params, grade_frac, base, root):
    lines = [f"nlive = {nlive}", f"num_repeats = {max(nr, 1)}", "nprior = -1", "nfail = -1", f"do_clustering = {'T' if clustering else 'F'}", "feedback = 0",
             "precision_criterion = 0.001", "logzero = -1e30", "max_ndead = -1", "boost_posterior = 0.0", "posteriors = F",
             "equals = F", "cluster_posteriors = F", "write_resume = F", "write_paramnames = F", "read_resume = F",
             "write_stats = T", "write_live = F", "write_dead = F", "write_prior = F", "maximise = F",
             "compression_factor = 0.36787944117144233", "synchronous = T", f"base_dir = {base}", f"file_root = {root}",
             f"seed = {seed}", f"grade_frac = {grade_frac}", ""]
    for d, (speed, kind, block, pp) in enumerate(params):
        lines.append(f"P : x{d + 1} | x_{{{d + 1}}} | {speed} | {kind} | {block} | " + " ".join(repr(float(v)) for v in pp))
    for k in range(nDer):
        lines.append(f"D : phi{k + 1} | \\phi_{{{k + 1}}}")
    return "\n".join(lines) + "\n"


def run_case(drv, tmp, like, seed, ini_args, tag):
    base = os.path.join(tmp, "chains")
    os.makedirs(os.path.join(base, "clusters"), exist_ok=True)
    ini = ini_text(*ini_args, base, tag)
    path = os.path.join(tmp, tag + ".ini")
    open(path, "w").write(ini)
    r = subprocess.run(["bash", "-c", f"ulimit -s unlimited; {drv} {like} {path} {seed}"], capture_output=True, text=True, cwd=tmp)
    if r.returncode != 0:
        sys.exit(f"{tag}: the reference stopped with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    out = read_stats(os.path.join(base, tag + ".stats"))
    # (several grades: the .stats line lists RTI%nlike per grade; read_stats takes the first number)
    out["nlike_grades"] = [int(v) for v in re.search(r"nlike:((?:\s+\d+)+)", open(os.path.join(base, tag + ".stats")).read()).group(1).split()]
    out["ncluster_dead"] = out["ncluster_total"] - out["ncluster"]
    return ini, out


def main():
    injected = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_injected.json")))
    with tempfile.TemporaryDirectory() as tmp:
        drv = build(tmp)
        proofs = []
        for like, D, nDer, nlive, nr, seed, clus, (lo, hi) in PROOF:
            i = [c for c in injected if (c["like"], c["nDims"], c["nDerived"], c["nlive"], c["num_repeats"], c["seed"], c["clustering"]) ==
                 (like, D, nDer, nlive, nr, seed, clus)][0]
            _, r = run_case(drv, tmp, like, seed, (nDer, nlive, nr, seed, clus, [(1, "uniform", 1, (lo, hi))] * D, "1"), f"proof_{like}")
            same = (r["ndead"], r["nlike"]) == (i["ndead"], i["nlike"]) and abs(r["logZ"] - i["logZ"]) < 1e-12 * max(1.0, abs(i["logZ"]))
            print(f"proof {like}: all-uniform ini run vs ref_injected: ndead {r['ndead']}/{i['ndead']} nlike {r['nlike']}/{i['nlike']} "
                  f"logZ {r['logZ']!r}/{i['logZ']!r} -> {'same' if same else 'DIFFERENT'}")
            if not same:
                sys.exit("the ini door does not reproduce ref_injected.json: find out why before using these numbers")
            proofs.append(dict(like=like, nDims=D, seed=seed, ndead=r["ndead"], nlike=r["nlike"], logZ=r["logZ"]))
        cases = []
        for name, like, nDer, nlive, nr, seed, clus, params, gf in CASES:
            ini, r = run_case(drv, tmp, like, seed, (nDer, nlive, nr, seed, clus, params, gf), name)
            rec = dict(name=name, like=like, nDims=len(params), nDerived=nDer, nlive=nlive, num_repeats=nr, seed=seed, clustering=clus,
                       params=[dict(speed=s, type=t, block=b, par=list(p)) for s, t, b, p in params], grade_frac=gf,
                       ini=ini.replace(tmp, "<tmp>"), **{k: r[k] for k in ("logZ", "logZerr", "ndead", "nlike", "nlike_grades", "ncluster", "ncluster_dead")})
            rec["nlike"] = sum(r["nlike_grades"])
            print(name, {k: rec[k] for k in ("ndead", "nlike", "logZ", "logZerr", "ncluster_dead")})
            cases.append(rec)
    json.dump(dict(_comment="the reference binary through its ini door under the sequential RNG shim (tools/dev/gen_ref_device_priors.py); "
                            "only its output: ini text, counters, evidences", door_proof=proofs, cases=cases),
              open(os.path.join(ROOT, "tests", "golden", "ref_device_priors.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
