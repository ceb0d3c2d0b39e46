"""Sub-dimension clustering on the device (settings%sub_clustering_dimensions, nested_sampling.F90:352-367): at every update the
clusters are first split on a list of cube coordinates, then on all of them.  Held against the REFERENCE BINARY driven through its
ini door with `*` markers (tests/golden/ref_subclust.json, tools/dev/gen_ref_subclust.py), against plain clustering where the two
must agree, against its own solo runs when runs go in step, and against the analytic evidence."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = {"rastrigin": (-5.12, 5.12), "twin_gaussian": (-1.0, 1.0)}


def _settings(api, D, nDer, sub=(), **kw):
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    keep = api.set_sub_clustering(s, sub)
    return s, keep


def _run(api, kind, D, nDer, sub=(), **kw):
    s, keep = _settings(api, D, nDer, sub, **kw)
    L, P, keep2 = api.make_problem(kind, D, nDer, *BOX[kind])
    return api.run(s, L, P)


def test_reproduces_the_reference_binary(engine, golden):
    """sequential-stream mode (the reference's draw order) with each case's list: the reference binary's run, draw for draw"""
    api = engine
    cases = golden["ref_subclust"]["cases"]
    assert sum(c["differs_from_unmarked"] for c in cases) >= 3            # the markers change these runs
    for c in cases:
        g = _run(api, c["like"], c["nDims"], c["nDerived"], c["sub_clustering"], nlive=c["nlive"], num_repeats=c["num_repeats"],
                 seed=c["seed"], do_clustering=1, sequential_rng=1)
        assert (g["ndead"], g["nlike"]) == (c["ndead"], c["nlike"]), (c["name"], g["ndead"], g["nlike"])
        assert abs(g["logZ"] - c["logZ"]) < 1e-8 and abs(g["logZerr"] - c["logZerr"]) < 1e-8, (c["name"], g["logZ"], g["logZerr"])
        # every cluster has died when the run ends (.stats: "ncluster: 0 / n"): the local evidences, one per cluster
        assert c["ncluster"] == 0 and g["ncluster_dead"] == c["ncluster_dead"], (c["name"], g["ncluster_dead"], c["ncluster_dead"])
        ref = np.sort([z for z, _ in c["local_logZ"]])
        assert len(g["logZp"]) == len(ref) == c["ncluster_dead"]
        assert np.abs(np.sort(g["logZp"]) - ref).max() < 1e-8 * max(1.0, np.abs(ref).max())
        assert g["path"]["subcluster_passes"] > 0 and g["path"]["subcluster_splits"] > 0


@pytest.mark.parametrize("kind,D,nDer,nlive,nr,seed", [("twin_gaussian", 6, 1, 150, 12, 4), ("rastrigin", 4, 0, 200, 12, 5)])
def test_every_coordinate_marked_is_plain_clustering(engine, kind, D, nDer, nlive, nr, seed):
    """production mode (default nursery): a sub pass over every coordinate in order is the full pass, bit for bit, and the full pass
    behind it finds nothing more -- the same run; and without clustering the markers do nothing at all"""
    api = engine
    kw = dict(nlive=nlive, num_repeats=nr, seed=seed, do_clustering=1)
    a = _run(api, kind, D, nDer, (), **kw)
    b = _run(api, kind, D, nDer, list(range(D)), **kw)
    assert a["batch"] > 1 and a["ncluster_peak"] >= 2
    assert (a["ndead"], a["nlike"], a["ncluster_dead"]) == (b["ndead"], b["nlike"], b["ncluster_dead"])
    assert a["logZ"] == b["logZ"] and a["logZerr"] == b["logZerr"]
    assert np.array_equal(a["dead"], b["dead"], equal_nan=True) and np.array_equal(a["logZp"], b["logZp"])
    assert b["path"]["subcluster_passes"] > 0 and b["path"]["subcluster_splits"] > 0 and a["path"]["subcluster_passes"] == 0
    assert a["path"]["subcluster_splits"] == 0
    kw["do_clustering"] = 0
    c = _run(api, kind, D, nDer, (), **kw)
    d = _run(api, kind, D, nDer, [0], **kw)
    assert (c["ndead"], c["nlike"], c["logZ"]) == (d["ndead"], d["nlike"], d["logZ"]) and np.array_equal(c["dead"], d["dead"], equal_nan=True)
    assert d["path"]["subcluster_passes"] == 0 and d["path"]["subcluster_splits"] == 0


def test_runs_in_step_are_their_solo_runs(engine):
    """pchip_run_repeats with 8 sub-clustered runs of one device in flight: the first pass of all runs that update in a round is one
    launch (k_similarity_b_many_sub, runs in their sub pass and in their full pass side by side) -- each run bit for bit its solo run"""
    from polychordlite_amd.repeats import run_repeats
    api = engine
    lib = api.load()
    D, nDer = 6, 1
    L, P, keep = api.make_problem("twin_gaussian", D, nDer, *BOX["twin_gaussian"])
    seeds = [41, 42, 43, 44, 45, 46, 47, 48]
    sub = np.array([0, 1], dtype=np.int32)

    def settings(seed):
        s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
        s.nlive, s.num_repeats, s.seed, s.do_clustering = 150, 12, seed, 1
        s.n_sub_cluster, s.sub_cluster_dims = len(sub), sub.ctypes.data_as(C.POINTER(C.c_int))
        return s
    singles = [api.run(settings(sd), L, P) for sd in seeds]
    merged, runs = run_repeats(settings(0), L, P, seeds, max_in_flight=len(seeds))
    assert max(r["ncluster_peak"] for r in singles) >= 2
    for one, r in zip(singles, runs):
        for k in ("ndead", "nlike", "niter", "nupdates", "nbatches", "ncluster_dead", "ncluster_peak"):
            assert one[k] == r[k], (k, one[k], r[k])
        assert one["logZ"] == r["logZ"] and one["logZerr"] == r["logZerr"]
        assert np.array_equal(one["dead"], r["dead"], equal_nan=True) and np.array_equal(one["logweights"], r["logweights"])
    assert merged["n_runs"] == len(seeds)


def _twin10(api, seed, **kw):
    return _run(api, "twin_gaussian", 10, 0, [0], nlive=200, num_repeats=20, seed=seed, do_clustering=1, **kw)


def _reference_production(golden):
    """the reference binary's eight runs of this shape (tests/golden/ref_subclust.json "production"): mean log Z and its scatter"""
    z = np.array([r["logZ"] for r in golden["ref_subclust"]["production"]["runs"]])
    return z.mean(), z.std(ddof=1)


def test_production_statistics(engine, golden):
    """10-D twin Gaussian in [-1, 1]^10, marker on x1 (the coordinate that separates the modes), 8 seeds in production mode (default
    nursery): the modes found by the sub passes, and log Z distributed as the reference binary's runs of the same shape.  Not as
    -10 ln 2: clustering on one coordinate over-splits (40-80 clusters) and such runs come out high by several of their own error
    bars, in the reference (mean -5.44 over its eight seeds against -6.93) as here"""
    api = engine
    ref_mean, ref_sd = _reference_production(golden)
    z = []
    for seed in range(1, 9):
        g = _twin10(api, seed)
        assert g["batch"] > 1 and g["ncluster_peak"] >= 2
        p = g["path"]
        assert p["subcluster_passes"] > 0 and p["subcluster_splits"] > 0, (seed, p)
        z.append(g["logZ"])
    z = np.array(z)
    assert abs(z.mean() - ref_mean) < 3 * np.sqrt((z.var(ddof=1) + ref_sd ** 2) / 8), (z, ref_mean, ref_sd)


def test_epoch_rules(engine, golden):
    """batch > 1 with several clusters: both rules for the chains in flight finish with the reference's distribution of evidence.
    Under the reference farm's rule every split -- a sub pass's too -- discards the nursery, under the engine's only the chains of a
    split cluster are lost: the same seed walks another trajectory under each.  (Evaluations per dead point are no signal at this
    size: the number of clusters a run makes moves them more, 220-500 from seed to seed, than the rule does.)"""
    api = engine
    ref_mean, ref_sd = _reference_production(golden)
    runs = {0: [], 1: []}
    for rule in (0, 1):
        for seed in (11, 12, 13):
            g = _twin10(api, seed, batch=50, epoch_discard=rule)
            assert g["batch"] == 50 and g["epoch_discard"] == rule
            assert g["ncluster_peak"] >= 2 and g["path"]["subcluster_splits"] > 0
            runs[rule].append(g)
        z = [g["logZ"] for g in runs[rule]]
        assert abs(np.mean(z) - ref_mean) < 3 * ref_sd, (rule, z, ref_mean, ref_sd)
    for a, b in zip(runs[0], runs[1]):
        assert (a["ndead"], a["nlike"]) != (b["ndead"], b["nlike"])


def test_bad_list_fails_cleanly_and_the_next_run_is_normal(engine, capfd):
    api = engine
    lib = api.load()
    L, P, keep = api.make_problem("twin_gaussian", 4, 0, *BOX["twin_gaussian"])
    for bad, msg in (([0, 0], "twice"), ([4], "out of range"), ([-1], "out of range")):
        s, k = _settings(api, 4, 0, bad, nlive=60, num_repeats=4, seed=3, do_clustering=1)
        r = api.Result()
        assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(P), C.byref(r)) == 1
        assert msg in capfd.readouterr().err
    a = _run(api, "twin_gaussian", 4, 0, [0], nlive=60, num_repeats=4, seed=3, do_clustering=1)
    assert a["ndead"] > 0 and np.isfinite(a["logZ"]) and a["path"]["subcluster_passes"] > 0


def _stats(path):
    lines = open(path).read().splitlines()
    logZ, err = [float(x) for x in lines[8].split("=")[1].split("+/-")]
    ndead = int([l for l in lines if l.startswith(" ndead:")][0].split(":")[1])
    return ndead, logZ, err


def test_front_doors(engine, tmp_path, monkeypatch):
    """the CLI's header names the list (feedback.f90:48-55) and says nothing more without it; pypolychord's keyword on both binding
    paths is the pchip_run of the same settings; a bad list raises there and the next call is normal"""
    api = engine
    cli = os.path.join(ROOT, "tools", "polychord_hip_cli")
    body = ("nlive = 120\nnum_repeats = 8\ndo_clustering = T\nfeedback = 1\nseed = 9\nwrite_dead = F\nbase_dir = chains\nfile_root = {root}\n"
            "P : x1{star} | x_1 | 1 | uniform | 1 | -1 1\n" + "".join(f"P : x{d} | x_{d} | 1 | uniform | 1 | -1 1\n" for d in range(2, 5)))
    heads = {}
    for star, root in (("*", "m"), ("", "u")):
        ini = tmp_path / (root + ".ini")
        ini.write_text(body.format(star=star, root=root))
        out = subprocess.run([cli, str(ini), "twin_gaussian"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        heads[root] = out.stdout.split("started sampling")[0].splitlines()
    assert "Sub clustering on    1 dimension" in heads["m"] and not any("Sub clustering" in l for l in heads["u"])
    i = heads["m"].index("Sub clustering on    1 dimension")
    assert heads["m"][i + 1].split() == ["1"] and heads["m"][:i] + heads["m"][i + 2:] == heads["u"]
    # pypolychord, compiled and ctypes bindings, against pchip_run with the same settings
    from polychordlite_amd import pypolychord
    from polychordlite_amd.pypolychord import polychord as pcmod, _pypolychord_ctypes as ct
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    ref = _run(api, "twin_gaussian", 4, 0, [0], nlive=120, num_repeats=8, seed=9, do_clustering=1)
    plain = _run(api, "twin_gaussian", 4, 0, (), nlive=120, num_repeats=8, seed=9, do_clustering=1)
    assert (ref["ndead"], ref["nlike"]) != (plain["ndead"], plain["nlike"])
    for name in ("compiled", "ctypes"):
        if name == "ctypes":
            monkeypatch.setattr(pcmod, "_pypolychord", ct)
        base = tmp_path / name
        pypolychord.run(dl.TwinGaussian(), 4, prior=dl.UniformPrior(-1.0, 1.0), nlive=120, num_repeats=8, seed=9, feedback=0,
                        do_clustering=True, sub_clustering_dimensions=[0], read_resume=False, write_resume=False, base_dir=str(base),
                        file_root="p", posteriors=False, equals=False, cluster_posteriors=False, write_live=False, write_prior=False)
        ndead, logZ, err = _stats(base / "p.stats")
        assert ndead == ref["ndead"] and abs(logZ - ref["logZ"]) < 1e-12 * max(1.0, abs(ref["logZ"])), (name, ndead, logZ, ref["ndead"], ref["logZ"])
        with pytest.raises(Exception, match="code 1"):
            pypolychord.run(dl.TwinGaussian(), 4, prior=dl.UniformPrior(-1.0, 1.0), nlive=60, num_repeats=4, seed=3, feedback=0,
                            sub_clustering_dimensions=[7], read_resume=False, write_resume=False, base_dir=str(base), file_root="bad",
                            posteriors=False, equals=False, cluster_posteriors=False, write_live=False, write_prior=False)
        # the setting was cleared behind the failed call: the next call without the keyword is the plain run
        pypolychord.run(dl.TwinGaussian(), 4, prior=dl.UniformPrior(-1.0, 1.0), nlive=120, num_repeats=8, seed=9, feedback=0,
                        do_clustering=True, read_resume=False, write_resume=False, base_dir=str(base), file_root="q",
                        posteriors=False, equals=False, cluster_posteriors=False, write_live=False, write_prior=False)
        ndead, logZ, err = _stats(base / "q.stats")
        assert ndead == plain["ndead"] and abs(logZ - plain["logZ"]) < 1e-12 * max(1.0, abs(plain["logZ"]))


def test_cpp_settings_and_fortran_setter(engine, tmp_path):
    """C++ `Settings::sub_clustering_dimensions` and the Fortran interface of polychord_hip_set_sub_clustering compile and run:
    each gives the pchip_run of the same settings"""
    import shutil
    api = engine
    ref = _run(api, "twin_gaussian", 4, 0, [0], nlive=120, num_repeats=8, seed=9, do_clustering=1)
    lib = os.path.join(ROOT, "polychordlite_amd")
    (tmp_path / "chains" / "clusters").mkdir(parents=True)
    cpp = tmp_path / "sc.cpp"
    cpp.write_text(r'''
#include "polychord_hip.hpp"
#include <cstdio>
int main() {
    polychord_hip_set_uniform_prior(4, std::vector<double>(4, -1.0).data(), std::vector<double>(4, 1.0).data());
    Settings s(4, 0);
    s.nlive = 120; s.num_repeats = 8; s.seed = 9; s.do_clustering = true; s.feedback = 0; s.write_stats = true;
    s.write_dead = false; s.write_prior = false; s.maximise = false; s.file_root = "cpp";
    s.sub_clustering_dimensions = {0};
    run_polychord(polychord_hip_twin_gaussian, polychord_hip_uniform_prior, s);
    s.sub_clustering_dimensions.clear(); s.file_root = "cpp_plain";
    run_polychord(polychord_hip_twin_gaussian, polychord_hip_uniform_prior, s);
    return 0;
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), str(cpp), "-L" + lib, "-lpolychord_hip",
                           "-Wl,-rpath," + lib, "-o", "sc"], cwd=tmp_path)
    out = subprocess.run(["./sc"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    ndead, logZ, err = _stats(tmp_path / "chains" / "cpp.stats")
    assert ndead == ref["ndead"] and abs(logZ - ref["logZ"]) < 1e-12 * max(1.0, abs(ref["logZ"]))
    plain = _run(api, "twin_gaussian", 4, 0, (), nlive=120, num_repeats=8, seed=9, do_clustering=1)
    assert _stats(tmp_path / "chains" / "cpp_plain.stats")[0] == plain["ndead"]
    if shutil.which("amdflang") is None:
        pytest.fail("no Fortran compiler for the Fortran binding")
    f90 = tmp_path / "sc.f90"
    f90.write_text('''
program sc
    use iso_c_binding
    use polychord_hip
    implicit none
    real(c_double) :: lo(4), hi(4)
    integer(c_int) :: dims(1)
    lo = -1d0; hi = 1d0; dims(1) = 0
    call polychord_hip_set_uniform_prior(4_c_int, lo, hi)
    call polychord_hip_set_sub_clustering(1_c_int, dims)
    call run_polychord_hip(c_funloc(polychord_hip_twin_gaussian), c_funloc(polychord_hip_uniform_prior), 4, 0, 120, 8, &
                           "chains", "f90", 9, .true., .false., .false.)
    call polychord_hip_set_sub_clustering(0_c_int, dims)
end program sc
''')
    src = os.path.join(ROOT, "bindings", "fortran")
    subprocess.check_call(["amdflang", "-c", os.path.join(src, "polychord_hip.f90"), "-o", "ph.o"], cwd=tmp_path)
    subprocess.check_call(["amdflang", str(f90), "ph.o", "-L" + lib, "-lpolychord_hip", "-Wl,-rpath," + lib, "-o", "scf"], cwd=tmp_path)
    out = subprocess.run(["./scf"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    ndead, logZ, err = _stats(tmp_path / "chains" / "f90.stats")
    assert ndead == ref["ndead"] and abs(logZ - ref["logZ"]) < 1e-12 * max(1.0, abs(ref["logZ"]))
