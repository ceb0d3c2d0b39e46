#!/usr/bin/env python
"""gen_ref_adaptive_priors.py -- tests/golden/ref_adaptive_priors.json from the REFERENCE itself: its five adaptive prior types
(priors.f90:363-488; tests/test_adaptive_priors.py holds the host function and the engine to these numbers).  CPU machine only, by hand:

    make -C oracle ref                            # the reference's objects in oracle/_ref/obj/
    python tools/dev/gen_ref_adaptive_priors.py

Two parts.  (1) Transform values: tools/dev/ref_adaptive_priors.f90, a harness of our own, is built against those objects in a temporary
directory and calls the reference's priors_module at fixed cube points -- types 11 .. 14 at n = 2 and n = 5 with a point in every nfunc
bin, type 15 at n = 4 on both sides of the layer boundary and in both bins of its count.  (2) Runs: the reference binary through its own
ini door under the RNG shim, as gen_ref_device_priors.py does it (the door is proved first, in the same way, or the script stops).
Only the reference's OUTPUT goes into the fixture: cube points and transform values, ini text, counters, evidences."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from gen_ref_subclust import FSRC, OBJ, build  # noqa: E402
from gen_ref_device_priors import PROOF, run_case  # noqa: E402

TYPES = {"adaptive_sorted_uniform": 11, "adaptive_sorted_gaussian": 12, "adaptive_sorted_half_gaussian": 13,
         "adaptive_sorted_exponential": 14, "nn_adaptive_layer_gaussian": 15}
# prior parameters of the k-th parameter of a block, different for every member (the count's and the layer's are ignored: priors.f90:401)
PARS = {"adaptive_sorted_uniform": lambda k: (-1.0 + 0.25 * k, 2.0 + 0.5 * k), "adaptive_sorted_gaussian": lambda k: (0.1 * k, 1.0 + 0.5 * k),
        "adaptive_sorted_half_gaussian": lambda k: (-0.2 * k, 0.5 + 0.25 * k), "adaptive_sorted_exponential": lambda k: (0.5 + k,),
        "nn_adaptive_layer_gaussian": lambda k: (0.3 * k, 0.75 + 0.25 * k)}
TAIL = [0.37, 0.81, 0.052, 0.64]                            # the members' coordinates (not in increasing order)


def transform_points():
    pts = []
    for t in list(TYPES)[:4]:
        for x1 in (0.0, 0.2, 0.95):                         # n = 2: one member, nfunc = 1 whatever the count
            pts.append((t, [x1, 0.37]))
        for x1 in (0.1, 0.3, 0.6, 0.9, 0.25, 0.75):         # n = 5: nfunc = INT(1 + 4 x1) = 1, 2, 3, 4, and the bin edges 0.25 -> 2, 0.75 -> 4
            pts.append((t, [x1] + TAIL))
    for layer in (0.3, 0.8, 0.5, 0.49):                     # n = 4: theta_1 = 1.1, 2.1, 1.5 (not below: gaussian), 1.48
        for x2 in (0.2, 0.7):                               # the count of the inner block of three: nfunc = INT(1 + 2 x2) = 1, 2
            pts.append(("nn_adaptive_layer_gaussian", [layer, x2, 0.81, 0.37]))
    return pts


def transforms(tmp):
    exe = os.path.join(tmp, "ref_adaptive_priors")
    objs = [os.path.join(OBJ, f + ".o") for f in FSRC] + [os.path.join(OBJ, "c_interface.o")]
    subprocess.check_call(["amdflang", "-cpp", "-O2", "-I" + OBJ, "-module-dir", tmp, os.path.join(HERE, "ref_adaptive_priors.f90")] + objs +
                          ["-o", exe, "-lstdc++", "-lm"])
    pts, text = transform_points(), []
    for t, cube in pts:
        pars = [v for k in range(len(cube)) for v in PARS[t](k)]
        text += [f"{TYPES[t]} {len(cube)} {len(pars)}", " ".join(repr(v) for v in cube), " ".join(repr(v) for v in pars)]
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(out) == len(pts), (len(out), len(pts))
    return [dict(type=t, cube=cube, par=[list(PARS[t](k)) for k in range(len(cube))], theta=[float(v) for v in line.split()])
            for (t, cube), line in zip(pts, out)]


# name, like, nDerived, nlive, num_repeats, seed, clustering, parameters: (speed, prior type, block, prior parameters), grade_frac
CASES = [
    ("g6_adaptive_sorted_uniform_block_of_five", "gaussian", 1, 100, 12, 3, 0,
     [(1, "adaptive_sorted_uniform", 1, (0.0, 1.0))] * 5 + [(1, "uniform", 2, (0.0, 1.0))], "1"),
    ("twin4_adaptive_sorted_gaussian_clustering", "twin_gaussian", 1, 120, 8, 9, 1,
     [(1, "uniform", 1, (-1.0, 1.0))] * 2 + [(1, "adaptive_sorted_gaussian", 2, (0.0, 0.5))] * 2, "1"),
    ("g6_nn_layer_and_adaptive_sorted_half_gaussian", "gaussian", 1, 100, 12, 4, 0,
     [(1, "nn_adaptive_layer_gaussian", 1, (0.5, 0.5))] * 4 + [(1, "adaptive_sorted_half_gaussian", 2, (0.3, 0.3))] * 2, "1"),
    # two speeds: the count in the slow grade, the members in the fast one; grade_frac > 1: the repeats per grade as given, no timing
    ("g5_adaptive_sorted_exponential_count_slow_members_fast", "gaussian", 1, 100, 0, 6, 0,
     [(1, "uniform", 1, (0.0, 1.0)), (1, "adaptive_sorted_exponential", 2, (2.0,))] + [(2, "adaptive_sorted_exponential", 2, (2.0,))] * 3, "4 8"),
]


def main():
    injected = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_injected.json")))
    with tempfile.TemporaryDirectory() as tmp:
        values = transforms(tmp)
        print(len(values), "transform points")
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
    json.dump(dict(_comment="the reference's priors_module at fixed cube points (tools/dev/ref_adaptive_priors.f90) and the reference binary "
                            "through its ini door under the sequential RNG shim (tools/dev/gen_ref_adaptive_priors.py); only its output: "
                            "transform values, ini text, counters, evidences", transforms=values, door_proof=proofs, cases=cases),
              open(os.path.join(ROOT, "tests", "golden", "ref_adaptive_priors.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
