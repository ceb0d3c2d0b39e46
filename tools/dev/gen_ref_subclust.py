#!/usr/bin/env python
"""gen_ref_subclust.py -- tests/golden/ref_subclust.json from the REFERENCE itself: runs with sub-dimension clustering (`*`
markers on parameter lines of an ini file), which only the reference's ini entry point can ask for.  CPU machine only, by hand:

    make -C oracle ref                      # the reference's objects in oracle/_ref/obj/
    python tools/dev/gen_ref_subclust.py    # builds tools/dev/ref_subclust_driver.cpp in a temporary directory, runs it

Every case is run twice, with its markers and without them.  The unmarked run must equal the entry of
tests/golden/ref_injected.json with the same shape and seed (ndead, nlike, logZ): the ini door draws in the same order as the
C-interface door the engine is already held to, or the fixture proves nothing -- the script stops if it does not.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
FSRC = ["utils", "abort", "array_utils", "settings", "mpi_utils", "random_utils", "calculate", "params", "priors",
        "run_time_info", "read_write", "feedback", "chordal_sampling", "clustering", "generate", "nelder_mead", "maximiser",
        "nested_sampling", "ini", "interfaces"]
BOX = {"gaussian": (0.0, 1.0), "rastrigin": (-5.12, 5.12), "twin_gaussian": (-1.0, 1.0)}

# name, like, nDims, nDerived, nlive, num_repeats, seed, marked parameters (0-based; all speeds 1: hypercube index = parameter index)
CASES = [
    ("twin4_x1", "twin_gaussian", 4, 1, 120, 8, 9, [0]),
    ("twin6_x1x2", "twin_gaussian", 6, 1, 150, 12, 4, [0, 1]),
    ("rast2_x2", "rastrigin", 2, 0, 300, 6, 2, [1]),
    ("rast4_x1x3", "rastrigin", 4, 0, 200, 12, 5, [0, 2]),
    ("twin6_x5", "twin_gaussian", 6, 1, 150, 12, 4, [4]),
    ("rast4_all", "rastrigin", 4, 0, 200, 12, 5, [0, 1, 2, 3]),
]
# the production statistics of the algorithm itself: 10-D twin Gaussian in [-1, 1]^10, marker on x1, eight seeds.  Clustering on one
# coordinate over-splits (40-80 clusters where two modes exist) and the evidence of a run with many small clusters comes out high by
# several of its own error bars -- in the reference as in the engine: the engine's runs are held to THIS distribution, not to -10 ln 2
PRODUCTION = dict(like="twin_gaussian", nDims=10, nDerived=0, nlive=200, num_repeats=20, seeds=list(range(1, 9)), sub_clustering=[0])


def build(tmp):
    objs = [os.path.join(OBJ, f + ".o") for f in FSRC] + [os.path.join(OBJ, f) for f in ("c_interface.o", "ref_rng_shim.o", "pc_oracle.o")]
    missing = [o for o in objs if not os.path.exists(o)]
    if missing:
        sys.exit("missing %s: run `make -C oracle ref` first" % ", ".join(missing))
    drv = os.path.join(tmp, "ref_subclust_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "oracle"), "-c", os.path.join(HERE, "ref_subclust_driver.cpp"),
                           "-o", drv + ".o"])
    subprocess.check_call(["amdflang", drv + ".o"] + objs + ["-o", drv, "-lstdc++", "-lm"])
    return drv


def ini_text(like, D, nDer, nlive, nr, seed, marked, base, root):
    lo, hi = BOX[like]
    lines = [f"nlive = {nlive}", f"num_repeats = {nr}", "nprior = -1", "nfail = -1", "do_clustering = T", "feedback = 0",
             "precision_criterion = 0.001", "logzero = -1e30", "max_ndead = -1", "boost_posterior = 0.0", "posteriors = F",
             "equals = F", "cluster_posteriors = F", "write_resume = F", "write_paramnames = F", "read_resume = F",
             "write_stats = T", "write_live = F", "write_dead = F", "write_prior = F", "maximise = F",
             "compression_factor = 0.36787944117144233", "synchronous = T", f"base_dir = {base}", f"file_root = {root}",
             f"seed = {seed}", "grade_frac = 1", ""]
    for d in range(D):
        star = "*" if d in marked else ""
        lines.append(f"P : x{d + 1}{star} | x_{{{d + 1}}} | 1 | uniform | 1 | {lo!r} {hi!r}")
    for k in range(nDer):
        lines.append(f"D : phi{k + 1} | \\phi_{{{k + 1}}}")
    return "\n".join(lines) + "\n"


def read_stats(path):
    txt = open(path).read()
    num = r"([-+0-9.E]+)"
    g = re.search(r"log\(Z\)\s*=\s*" + num + r"\s*\+/-\s*" + num, txt)
    local = [[float(a), float(b)] for a, b in re.findall(r"log\(Z_\d+\)\s*=\s*" + num + r"\s*\+/-\s*" + num, txt)]
    nc = re.search(r"ncluster:\s*(\d+)\s*/\s*(\d+)", txt)
    return dict(logZ=float(g.group(1)), logZerr=float(g.group(2)),
                ndead=int(re.search(r"ndead:\s*(\d+)", txt).group(1)), nlike=int(re.search(r"nlike:\s*(\d+)", txt).group(1)),
                ncluster=int(nc.group(1)), ncluster_total=int(nc.group(2)), local_logZ=local)


def run_case(drv, tmp, like, D, nDer, nlive, nr, seed, marked, tag):
    base = os.path.join(tmp, "chains")
    os.makedirs(os.path.join(base, "clusters"), exist_ok=True)
    ini = ini_text(like, D, nDer, nlive, nr, seed, marked, base, tag)
    path = os.path.join(tmp, tag + ".ini")
    open(path, "w").write(ini)
    subprocess.run(["bash", "-c", f"ulimit -s unlimited; {drv} {like} {path} {seed}"], check=True, capture_output=True, cwd=tmp)
    out = read_stats(os.path.join(base, tag + ".stats"))
    out["ncluster_dead"] = out["ncluster_total"] - out["ncluster"]
    return ini, out


def main():
    injected = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_injected.json")))
    with tempfile.TemporaryDirectory() as tmp:
        drv = build(tmp)
        cases = []
        for name, like, D, nDer, nlive, nr, seed, marked in CASES:
            key = (like, D, nDer, nlive, nr, seed, 1)
            inj = [c for c in injected if (c["like"], c["nDims"], c["nDerived"], c["nlive"], c["num_repeats"], c["seed"], c["clustering"]) == key]
            ini0, plain = run_case(drv, tmp, like, D, nDer, nlive, nr, seed, [], name + "_plain")
            if inj:      # the acceptance check: the ini door = the C-interface door, draw for draw
                i = inj[0]
                same = (plain["ndead"], plain["nlike"]) == (i["ndead"], i["nlike"]) and abs(plain["logZ"] - i["logZ"]) < 1e-12 * max(1.0, abs(i["logZ"]))
                print(f"{name}: unmarked ini run vs ref_injected: ndead {plain['ndead']}/{i['ndead']} nlike {plain['nlike']}/{i['nlike']} "
                      f"logZ {plain['logZ']!r}/{i['logZ']!r} -> {'same' if same else 'DIFFERENT'}")
                if not same:
                    sys.exit("the ini door does not reproduce ref_injected.json: find out why before using these numbers")
            ini, marked_run = run_case(drv, tmp, like, D, nDer, nlive, nr, seed, marked, name)
            rec = dict(name=name, like=like, nDims=D, nDerived=nDer, nlive=nlive, num_repeats=nr, seed=seed, sub_clustering=marked,
                       ini=ini.replace(tmp, "<tmp>"), unmarked=plain, **marked_run)
            rec["differs_from_unmarked"] = (marked_run["ndead"], marked_run["nlike"], marked_run["logZ"]) != (plain["ndead"], plain["nlike"], plain["logZ"])
            print(name, {k: rec[k] for k in ("ndead", "nlike", "logZ", "ncluster", "ncluster_dead", "differs_from_unmarked")})
            cases.append(rec)
        prod = dict(PRODUCTION, runs=[])
        for seed in prod["seeds"]:
            _, r = run_case(drv, tmp, prod["like"], prod["nDims"], prod["nDerived"], prod["nlive"], prod["num_repeats"], seed,
                            prod["sub_clustering"], "prod%d" % seed)
            prod["runs"].append({k: r[k] for k in ("logZ", "logZerr", "ndead", "nlike", "ncluster_dead")})
            print("production", seed, prod["runs"][-1])
    json.dump(dict(cases=cases, production=prod), open(os.path.join(ROOT, "tests", "golden", "ref_subclust.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
