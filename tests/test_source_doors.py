"""Device sources behind the PolyChord-interface doors: polychord_hip_set_source, polychord_hip_source_loglike and
polychord_hip_source_prior (pc_abi.hip), `Source` / `SourcePrior` of pypolychord.device_likelihoods, `source:FILE` of the command-line tool
and the C++ example.

CPU: the symbols, the setter's refusals, the fatal condition without a handle, the objects' symbols, the tool's refusal of a missing file.
GPU: a door run with a source IS pchip_run's run (dumper, dead rows, <root>.stats); the two host functions are pchip_source_eval and
pchip_source_prior_eval at one point; `maximise` writes the device maximiser's file; the ini front end; resume; the C++ example; and a
source under the user's own host prior: the host build of the same text gives the same run, bit for bit."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_device_source import GAUSS_SRC, LINE_SRC, _host_like  # noqa: F401  (LINE_SRC: the line fit the terms text restates)
from tests.test_prior_source import TEXTS, _data
from tests.test_source_terms import LINE_TERMS, _line_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "polychord_hip_cli")
NTERMS = 70                 # a lane holds two terms
# the shapes of every run here: the smallest that still go through several nurseries and updates
NLIVE, NREP, BATCH, SEED = 50, 8, 20, 7
# one Gaussian and one sorted_uniform block, for the line fit in four parameters (slope, intercept, two idle ones)
TABLE = [("gaussian", (0.3, 1.0)), ("gaussian", (0.6, 1.0))] + [("sorted_uniform", 1, (0.0, 1.0))] * 2


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _dl():
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    return dl


_SOURCES = {}


def _source(name):
    """one Source object, and so one handle and one set of compiled kernels, per text for the whole module"""
    dl = _dl()
    if name not in _SOURCES:
        if name == "gauss":
            _SOURCES[name] = dl.Source(GAUSS_SRC, nDerived=2)
        elif name == "gauss0":
            _SOURCES[name] = dl.Source(GAUSS_SRC)
        elif name == "terms":
            _SOURCES[name] = dl.Source(LINE_TERMS, nDerived=1, data=_line_data(NTERMS), nterms=NTERMS)
        elif name == "aff":
            _SOURCES[name] = dl.Source(TEXTS["AFF"], data=_data("AFF", 3), prior=True)
    return _SOURCES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_sources():
    yield
    api, lib = _lib()
    lib.polychord_hip_set_source(0)
    for s in _SOURCES.values():
        s.close()
    _SOURCES.clear()


def _settings(api, D, nDer, **kw):
    """pchip_settings of the run `_door` makes"""
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    s.nlive, s.num_repeats, s.seed, s.batch, s.do_clustering, s.feedback = NLIVE, NREP, SEED, BATCH, 0, 0
    s.nprior, s.nfail, s.precision_criterion, s.logzero, s.max_ndead, s.boost_posterior = -1, -1, 1e-3, -1e30, -1, 0.0
    s.posteriors, s.equals, s.cluster_posteriors, s.compression_factor = 0, 0, 0, float(np.exp(-1))
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _door(base, root, like, D, nDer, prior, **kw):
    """pypolychord.run with the settings of `_settings` and the `batch` option; the dumper's calls [(dead, logweights, logZ, logZerr)]"""
    from polychordlite_amd import pypolychord
    api, lib = _lib()
    got = []
    hook = kw.pop("hook", None)

    def dumper(live, dead, w, z, e):
        got.append((np.array(dead), np.array(w), z, e, len(live)))
        if hook is not None:
            hook(len(live), len(dead))
    args = dict(nDerived=nDer, prior=prior, dumper=dumper,
                nlive=NLIVE, num_repeats=NREP, seed=SEED, do_clustering=False, feedback=0, base_dir=str(base), file_root=root,
                read_resume=False, write_resume=False, posteriors=False, equals=False, cluster_posteriors=False, write_live=False,
                write_prior=False, write_dead=True, write_stats=True)
    args.update(kw)
    lib.polychord_hip_set_option(b"batch", float(BATCH))
    try:
        pypolychord.run(like, D, **args)
    finally:
        lib.polychord_hip_set_option(b"batch", 0.0)
    return got


def _stats(path):
    text = open(path).read()
    m = re.search(r"log\(Z\)\s*=\s*([-+0-9.Ee]+)\s*\+/-\s*([-+0-9.Ee]+)", text)
    return float(m.group(1)), float(m.group(2)), int(re.search(r"ndead:\s*(\d+)", text).group(1))


def _e15(v):
    """a double as the files hold it: 15 significant digits (E24.15E3)"""
    return float("%.14E" % v)


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_the_three_symbols_are_declared_and_exported():
    api, lib = _lib()
    header = open(os.path.join(ROOT, "include", "polychord_hip.h")).read()
    for sym, decl in (("polychord_hip_set_source", r"int\s+polychord_hip_set_source\(int handle\);"),
                      ("polychord_hip_source_loglike", r"double\s+polychord_hip_source_loglike\(double \*theta, int nDims, double \*phi, int nDerived\);"),
                      ("polychord_hip_source_prior", r"void\s+polychord_hip_source_prior\(double \*cube, double \*theta, int nDims\);")):
        assert re.search(decl, header), sym
        assert hasattr(lib, sym), sym
    assert lib.pchip_abi_version() == 9
    for fn in ("include/polychord_hip.hpp", "bindings/fortran/polychord_hip.f90"):
        text = open(os.path.join(ROOT, fn)).read()
        for sym in ("polychord_hip_set_source", "polychord_hip_source_loglike", "polychord_hip_source_prior"):
            assert sym in text, (fn, sym)


def test_set_source_takes_a_live_handle_only():
    api, lib = _lib()
    h = api.source_create(GAUSS_SRC)
    try:
        assert lib.polychord_hip_set_source(h) == 0
        assert lib.polychord_hip_set_source(0) == 0                     # clears
        assert lib.polychord_hip_set_source(987654) != 0
        assert b"handle 987654 does not exist" in lib.polychord_hip_last_error()
        with pytest.raises(RuntimeError, match="does not exist"):
            api.set_source(987654)
    finally:
        lib.pchip_source_destroy(h)
    assert lib.polychord_hip_set_source(h) != 0                         # destroyed
    assert b"does not exist" in lib.polychord_hip_last_error()
    lib.polychord_hip_set_source(0)


class _Unset:
    """the source functions without a handle behind them"""
    def __init__(self, symbol):
        self.symbol = symbol

    def configure(self, nDims):
        pass

    def __call__(self, *a):
        raise AssertionError("never called")


def test_a_door_call_without_a_handle_returns_with_the_message(tmp_path, capfd):
    """halt_returns = 1 (the bindings set it): the fatal condition comes back as the message -- before the output directory is looked at
    (it does not exist here) and without a device"""
    from polychordlite_amd.pypolychord import _pypolychord_ctypes as ct
    dl = _dl()
    api, lib = _lib()
    lib.polychord_hip_set_source(0)
    with pytest.raises(RuntimeError, match="polychord_hip_set_source was not called"):
        ct.run(_Unset("polychord_hip_source_loglike"), dl.UniformPrior(0.0, 1.0), lambda *a: None, 3, 0, 20, 3, -1, -1, False, 0, 1e-3, -1e30,
               -1, 0.0, False, False, False, False, False, False, True, False, True, False, False, 0.36787944117144233, True,
               str(tmp_path / "no_such_dir"), "x", [1.0], [3], {}, 1)
    assert b"was not called" in lib.polychord_hip_last_error()
    assert "was not called" in capfd.readouterr().err
    # a handle destroyed between the setter and the door call: the engine's message
    h = api.source_create(GAUSS_SRC)
    api.set_source(h)
    lib.pchip_source_destroy(h)
    with pytest.raises(RuntimeError, match="device source handle %d does not exist" % h):
        ct.run(_Unset("polychord_hip_source_loglike"), dl.UniformPrior(0.0, 1.0), lambda *a: None, 3, 0, 20, 3, -1, -1, False, 0, 1e-3, -1e30,
               -1, 0.0, False, False, False, False, False, False, True, False, True, False, False, 0.36787944117144233, True,
               str(tmp_path / "no_such_dir"), "x", [1.0], [3], {}, 1)
    lib.polychord_hip_set_source(0)
    # ... and so do the two host functions called directly
    th = np.full(3, 0.5); phi = np.zeros(1); out = np.zeros(3)
    assert lib.polychord_hip_source_loglike(api.dptr(th), 3, api.dptr(phi), 0) < -1e300
    assert b"was not called" in lib.polychord_hip_last_error()
    lib.polychord_hip_source_prior(api.dptr(th), api.dptr(out), 3)
    assert b"was not called" in lib.polychord_hip_last_error()


def test_a_source_prior_needs_the_source_likelihood(tmp_path):
    """polychord_hip_source_prior with a built-in likelihood: the engine's wording, at the door, without a device"""
    from polychordlite_amd.pypolychord import _pypolychord_ctypes as ct
    dl = _dl()
    with pytest.raises(RuntimeError, match="needs a device source likelihood of the same handle"):
        ct.run(dl.Gaussian(0.5, 0.1), _Unset("polychord_hip_source_prior"), lambda *a: None, 3, 0, 20, 3, -1, -1, False, 0, 1e-3, -1e30,
               -1, 0.0, False, False, False, False, False, False, True, False, True, False, False, 0.36787944117144233, True,
               str(tmp_path / "no_such_dir"), "x", [1.0], [3], {}, 1)


def test_the_objects_carry_their_symbols():
    dl = _dl()
    api, lib = _lib()
    s = dl.Source(GAUSS_SRC, nDerived=1)
    p = dl.SourcePrior(s)
    assert s.symbol == "polychord_hip_source_loglike" and p.symbol == "polychord_hip_source_prior"
    assert s._handle is None                                            # made on first use
    s.configure(4)
    assert s._handle > 0
    p.configure(4)                                                      # the same handle
    s.close()
    assert s._handle is None
    bad = dl.Source("__device__ double something_else(double x) { return x; }\n")
    with pytest.raises(RuntimeError, match="pchip_loglikelihood"):
        bad.configure(4)
    lib.polychord_hip_set_source(0)


def test_the_cli_refuses_a_source_file_it_cannot_read(tmp_path):
    ini = os.path.join(ROOT, "configs", "gaussian.ini")
    r = subprocess.run([CLI, ini, "source:" + str(tmp_path / "no_such_file.hip")], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "cannot read the source file" in r.stderr and "no_such_file.hip" in r.stderr
    r = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "source:FILE" in r.stderr


# ---------------------------------------------------------------------------------------------------------------------------- GPU
# A run with host hooks (the doors: files, dumper) makes every update when it happens; a run of pchip_run without hooks runs the
# contraction past the update triggers and keeps its babies in the phantom pool (pc_plan.h: defer, pool).  The two are the same run to
# round-off, not to the bit -- the covariance sums group their rows differently (tests/test_gpu_parity.py, test_modes_change_no_number:
# every counter exactly, log Z to 1e-11, the rows to 1e-9).  settings.ablate bits 1 and 2 switch the two modes off: pchip_run then launches
# what the door's run launches, and THAT run the door reproduces to the bit.  Both are held: the bits against the run of the same
# kernels, the round-off bounds of test_modes_change_no_number against the default run.
HOOKS_MODES = 2 | 4


def _pchip_runs(api, D, nDer, L, P, **kw):
    """(the run by the kernels a run with hooks takes, the default run)"""
    return api.run(_settings(api, D, nDer, ablate=HOOKS_MODES, **kw), L, P), api.run(_settings(api, D, nDer, **kw), L, P)


def _same_run(got, runs, D, stats_path):
    """the door's run against the dicts of pchip_run"""
    g, g0 = runs
    dead, logw, logZ, logZerr, nlive_left = got[-1]
    assert nlive_left == 0                                              # the final dump
    assert g["path"]["source_kernels"] > 0 and g0["path"]["source_kernels"] > 0
    assert g["path"]["defer_update"] == 0 and g0["path"]["defer_update"] == 1
    print("door logZ %r +/- %r; pchip_run by the same kernels %r +/- %r; default %r +/- %r" % (logZ, logZerr, g["logZ"], g["logZerr"], g0["logZ"], g0["logZerr"]))
    assert logZ == g["logZ"] and logZerr == g["logZerr"]
    assert dead.shape == (g["ndead"], g["dead"].shape[1] - D)
    assert np.array_equal(dead, g["dead"][:, D:])
    z, e, nd = _stats(stats_path)
    assert nd == g["ndead"]
    assert z == _e15(g["logZ"]) and e == _e15(g["logZerr"])
    nlike = int(re.search(r"nlike:\s*(\d+)", open(stats_path).read()).group(1))
    assert nlike == g["nlike"]
    for k in ("ndead", "nlike", "niter"):
        assert g[k] == g0[k], (k, g[k], g0[k])
    assert abs(logZ - g0["logZ"]) < 1e-11 * max(1.0, abs(g0["logZ"])) and abs(logZerr - g0["logZerr"]) < 1e-11
    want = g0["dead"][:, D:]
    assert np.all(np.abs(dead - want) <= 1e-9 * np.maximum(1.0, np.abs(want)))      # (element by element: the birth column holds logzero)


@pytest.mark.gpu
def test_a_door_run_with_a_plain_source_is_pchip_run(engine, tmp_path):
    api, dl = engine, _dl()
    src = _source("gauss")
    got = _door(tmp_path, "p", src, 4, 2, dl.UniformPrior(0.0, 1.0))
    L, P, keep = api.make_problem("source", 4, 2, source=src.handle)
    runs = _pchip_runs(api, 4, 2, L, P)
    assert all(g["path"]["source_terms"] == 0 and g["path"]["device_prior"] == 0 for g in runs)
    _same_run(got, runs, 4, tmp_path / "p.stats")
    # the ctypes twin of the compiled module resolves the same symbol: the same run
    from polychordlite_amd.pypolychord import _pypolychord_ctypes as ct
    twin = []
    lib = api.load()
    lib.polychord_hip_set_option(b"batch", float(BATCH))
    try:
        ct.run(src, dl.UniformPrior(0.0, 1.0), lambda live, dead, w, z, e: twin.append((np.array(dead), z, e)), 4, 2, NLIVE, NREP, -1, -1, False,
               0, 1e-3, -1e30, -1, 0.0, False, False, False, False, False, False, True, False, True, False, False, float(np.exp(-1)), True,
               str(tmp_path), "pt", [1.0], [4], {}, SEED)
    finally:
        lib.polychord_hip_set_option(b"batch", 0.0)
    assert np.array_equal(twin[-1][0], got[-1][0]) and twin[-1][1] == got[-1][2] and twin[-1][2] == got[-1][3]


@pytest.mark.gpu
def test_a_door_run_with_a_terms_source_under_a_table_is_pchip_run(engine, tmp_path):
    api, dl = engine, _dl()
    src = _source("terms")
    got = _door(tmp_path, "t", src, 4, 1, dl.TablePrior(TABLE))
    L, P, keep = api.make_problem("source", 4, 1, source=src.handle, prior_table=TABLE)
    runs = _pchip_runs(api, 4, 1, L, P)
    assert all(g["path"]["source_terms"] > 0 and g["path"]["device_prior"] > 0 for g in runs)
    _same_run(got, runs, 4, tmp_path / "t.stats")


@pytest.mark.gpu
def test_a_door_run_with_a_source_prior_is_pchip_run(engine, tmp_path):
    api, dl = engine, _dl()
    src = _source("aff")
    got = _door(tmp_path, "a", src, 3, 0, dl.SourcePrior(src))
    L, P, keep = api.make_problem("source", 3, 0, source=src.handle, prior_source=True)
    runs = _pchip_runs(api, 3, 0, L, P)
    assert all(g["path"]["device_prior"] > 0 for g in runs)
    _same_run(got, runs, 3, tmp_path / "a.stats")


@pytest.mark.gpu
def test_the_host_functions_are_the_evaluation_doors(engine):
    api, dl = engine, _dl()
    rng = np.random.default_rng(11)
    for name, D, nDer in (("gauss", 4, 2), ("terms", 4, 1)):
        src = _source(name)
        thetas = rng.uniform(0.0, 1.0, (8, D))
        logL, phi = api.source_eval(src.handle, thetas, nDer)
        for i in range(8):
            l, p = src(thetas[i])
            assert l == logL[i] and np.array_equal(p, phi[i]), (name, i)
    src = _source("aff")
    prior = dl.SourcePrior(src)
    cubes = rng.uniform(0.0, 1.0, (8, 3))
    want = api.source_prior_eval(src.handle, cubes)
    for i in range(8):
        assert np.array_equal(prior(cubes[i]), want[i]), i
    assert src(want[0]) == api.source_eval(src.handle, want[:1], 0)[0][0]          # (no derived parameters: a plain float)
    # a handle that defines no prior: the message, and a return
    with pytest.raises(RuntimeError, match="defines no pchip_prior_param"):
        dl.SourcePrior(_source("gauss"))(cubes[0, :3])


@pytest.mark.gpu
def test_maximise_polishes_a_source_on_the_device(engine, tmp_path, capfd):
    api, dl = engine, _dl()
    src = _source("gauss")
    _door(tmp_path, "m", src, 4, 2, dl.UniformPrior(0.0, 1.0), maximise=True, posteriors=True)
    s = _settings(api, 4, 2, posteriors=1)
    L, P, keep = api.make_problem("source", 4, 2, source=src.handle)
    g = api.run(_settings(api, 4, 2, posteriors=1, ablate=HOOKS_MODES), L, P)      # (the live set of the door's run to the bit: HOOKS_MODES)
    api.maximise_device(s, L, P, g, write=tmp_path / "want.maximum")
    assert (tmp_path / "m.maximum").read_bytes() == (tmp_path / "want.maximum").read_bytes()
    lines = (tmp_path / "m.maximum").read_text().splitlines()
    assert lines[0] == "Maximum LogLikelihood:" and lines[12] == "LogLikelihood(mean):"
    # the built-in Gaussian through the same door: the host maximiser's file, as before
    lib = api.load()
    _door(tmp_path, "b", dl.Gaussian(0.5, 0.1, nDerived=2), 4, 2, dl.UniformPrior(0.0, 1.0), maximise=True, posteriors=True)
    Lb, Pb, keep2 = api.make_problem("gaussian", 4, 2)
    gb = api.run(_settings(api, 4, 2, posteriors=1, ablate=HOOKS_MODES), Lb, Pb)
    lib.polychord_hip_set_gaussian(0.5, 0.1)
    lo, hi = np.zeros(4), np.ones(4)
    lib.polychord_hip_set_uniform_prior(4, api.dptr(lo), api.dptr(hi))
    f = lib.pchip_maximise
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int,
                  C.POINTER(C.c_double), C.c_char_p]
    live = np.ascontiguousarray(gb["live"]); cl = np.ascontiguousarray(gb["live_cluster"], dtype=np.int32)
    assert f(C.cast(lib.polychord_hip_gaussian, C.c_void_p), C.cast(lib.polychord_hip_uniform_prior, C.c_void_p), 4, 2, -1e30, api.dptr(live),
             cl.ctypes.data_as(C.POINTER(C.c_int)), live.shape[0], api.dptr(gb["post_mean"]), str(tmp_path / "wantb.maximum").encode()) == 0
    assert (tmp_path / "b.maximum").read_bytes() == (tmp_path / "wantb.maximum").read_bytes()
    # nDims > 64 (the device maximiser's limit): a message and no file; the call returns and the run's results stand
    capfd.readouterr()
    got = _door(tmp_path, "w", _source("gauss0"), 65, 0, dl.UniformPrior(0.0, 1.0), maximise=True, max_ndead=60)
    assert got[-1][4] == 0 and (tmp_path / "w.stats").exists() and not (tmp_path / "w.maximum").exists()
    err = capfd.readouterr().err
    assert "nDims > 64" in err and "w.maximum is not written" in err


@pytest.mark.gpu
def test_the_cli_runs_an_ini_file_with_a_source(engine, tmp_path):
    """configs/gaussian_gaussian_prior.ini (20 Gaussian priors N(0.5, 1)) with GAUSS_SRC from a file: the header names the handle, the prior
    table is on the device, and <root>.stats is within 4 reported sigma of -(20 / 2) log(2 pi 1.01) -- bound, truth and nlive of
    test_cli_runs_a_gaussian_prior_ini_on_the_device"""
    ini = tmp_path / "g.ini"
    ini.write_text(open(os.path.join(ROOT, "configs", "gaussian_gaussian_prior.ini")).read().replace("nlive = 500", "nlive = 200"))
    (tmp_path / "gauss.hip").write_text(GAUSS_SRC)
    r = subprocess.run([CLI, str(ini), "source:" + str(tmp_path / "gauss.hip")], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    assert re.search(r"device source handle \d+ \(plain form\) evaluated on the device", r.stdout), r.stdout
    assert "prior table evaluated on the device" in r.stdout, r.stdout
    truth = -10.0 * math.log(2.0 * math.pi * 1.01)
    z, e, nd = _stats(tmp_path / "chains" / "gaussian_gaussian_prior.stats")
    print("cli: logZ", z, "+/-", e, "truth", truth)
    assert abs(z - truth) < 4.0 * e, (z, e, truth)


@pytest.mark.gpu
def test_a_cut_run_resumes_with_the_same_source(engine, tmp_path):
    """max_ndead cuts a run that writes its .resume file; read_resume with the same Source goes on from there to the end.  A run that has
    ended leaves the file of its end behind -- no live point, it gives the result back without sampling, for a cut run as for any -- so the
    file the second run starts from is the cut run's last one with live points: the one on disk when the final dump is made (the dumper
    is called in front of the writer).  The .resume grammar holds 15 significant digits, so behind the restart the run is another
    realisation, not the uncut run's bits: its dead points up to the restart are the cut run's rows as written, and its end is the uncut
    run's to their errors.  Both evidences estimate one number with their own reported errors e (and share the points before the restart,
    which only brings them closer): |difference| < 4 sqrt(e1^2 + e2^2).  A run ends where the live evidence falls under the precision
    criterion, at a volume X_end that the likelihood fixes; ndead = -nlive log X_end to the scatter of the run's own volume estimate,
    sqrt(ndead) / nlive in log X: |difference| < 4 sqrt(nd1 + nd2)."""
    import shutil
    dl = _dl()
    src = _source("gauss")
    cutn = 150
    base_u, base_c, base_r = tmp_path / "u", tmp_path / "c", tmp_path / "r"
    _door(base_u, "r", src, 4, 2, dl.UniformPrior(0.0, 1.0))
    zu, eu, ndu = _stats(base_u / "r.stats")

    def keep_the_last_file_with_live_points(nlive_left, ndead):
        if nlive_left == 0:
            (base_r / "clusters").mkdir(parents=True, exist_ok=True)
            shutil.copy(base_c / "r.resume", base_r / "r.resume")
    _door(base_c, "r", src, 4, 2, dl.UniformPrior(0.0, 1.0), max_ndead=cutn, write_resume=True, hook=keep_the_last_file_with_live_points)
    zc, ec, ndc = _stats(base_c / "r.stats")
    assert cutn <= ndc < ndu
    first = np.loadtxt(base_c / "r_dead-birth.txt")
    nres = int(open(base_r / "r.resume").read().splitlines()[5])        # dead points in the file
    assert 0 < nres <= cutn
    got = _door(base_r, "r", src, 4, 2, dl.UniformPrior(0.0, 1.0), read_resume=True)
    zr, er, ndr = _stats(base_r / "r.stats")
    print("resume: uncut", zu, eu, ndu, "cut", zc, ec, ndc, "in the file", nres, "resumed", zr, er, ndr)
    cont = np.loadtxt(base_r / "r_dead-birth.txt")
    assert got[-1][4] == 0 and ndr == cont.shape[0] > ndc
    assert np.array_equal(cont[:nres], first[:nres])
    assert abs(ndr - ndu) < 4.0 * math.sqrt(ndr + ndu), (ndr, ndu)
    assert abs(zr - zu) < 4.0 * math.sqrt(er * er + eu * eu), (zr, er, zu, eu)


@pytest.mark.gpu
def test_the_cpp_example_runs_a_source(engine, tmp_path):
    lib = os.path.join(ROOT, "polychordlite_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "bindings", "cpp", "example_source.cpp"),
                           "-L" + lib, "-lpolychord_hip", "-Wl,-rpath," + lib, "-o", "exs"], cwd=tmp_path)
    (tmp_path / "chains" / "clusters").mkdir(parents=True)
    out = subprocess.run(["./exs", "chains"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "final dump" in out.stdout
    z, e, nd = _stats(tmp_path / "chains" / "cpp_source.stats")
    assert math.isfinite(z) and math.isfinite(e) and nd > 0
    assert (tmp_path / "chains" / "cpp_source.maximum").exists()


# ---- a source likelihood under the user's own host prior ----------------------------------------------------------------------------
def _unit_box(cube):
    """the unit box as a plain host function: nothing the door recognises"""
    return np.array(cube, dtype=np.float64)


def _registered(lib):
    fn, user = C.c_void_p(), C.c_void_p()
    lib.pc_batch_callback_get(C.byref(fn), C.byref(user))
    return fn.value, user.value


@pytest.mark.gpu
def test_a_source_under_a_host_prior_is_the_host_builds_run(engine, tmp_path, capfd):
    """GAUSS_SRC is contract-off + - * / only: the device and the host build of the text give the same bits, so the door's run with the
    source (the prior on the host, a round's proposals in one launch) and the door's run with the host function as a callback agree in
    ndead, nlike, log Z and every dead row"""
    api, lib = engine, engine.load()
    D = 4
    src = _source("gauss0")
    assert _registered(lib) == (None, None)
    got_s = _door(tmp_path, "s", src, D, 0, _unit_box, max_ndead=300, feedback=1)
    assert "source likelihood evaluated on the device in batches; prior on the host" in capfd.readouterr().out
    assert _registered(lib) == (None, None)                             # the caller's registration (none) is back
    hl = _host_like(tmp_path, GAUSS_SRC, "gauss_host")
    hl.host_logl.restype = C.c_double
    zero = np.zeros(1)
    ctx = (C.c_void_p * 2)(zero.ctypes.data, 0)
    dummy = np.zeros(1)

    def host_like(theta):
        t = np.ascontiguousarray(theta, dtype=np.float64)
        return float(hl.host_logl(t.ctypes.data_as(C.c_void_p), D, dummy.ctypes.data_as(C.c_void_p), 0, ctx))
    got_h = _door(tmp_path, "h", host_like, D, 0, _unit_box, max_ndead=300)
    ds, ws, zs, es, _ = got_s[-1]
    dh, wh, zh, eh, _ = got_h[-1]
    assert ds.shape == dh.shape and ds.shape[0] >= 300
    assert np.array_equal(ds, dh) and np.array_equal(ws, wh) and zs == zh and es == eh
    nlike = [re.search(r"nlike:\s*(\d+)", open(tmp_path / (r + ".stats")).read()).group(1) for r in ("s", "h")]
    assert nlike[0] == nlike[1]
    assert _stats(tmp_path / "s.stats") == _stats(tmp_path / "h.stats")
    # a batch callback of the caller's wins: it is called, and the door's own evaluator is not put in
    calls = []
    proto = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                        C.POINTER(C.c_double))

    def mine(_user, n, nd, nder, cube_p, theta_p, phi_p, logL_p):
        calls.append(n)
        cube = np.ctypeslib.as_array(cube_p, shape=(n, nd))
        np.ctypeslib.as_array(theta_p, shape=(n, nd))[:] = cube
        np.ctypeslib.as_array(logL_p, shape=(n,))[:] = api.source_eval(src.handle, cube, 0)[0]
    cb = proto(mine)
    lib.polychord_hip_set_batch_callback.argtypes = [C.c_void_p, C.c_void_p]
    lib.polychord_hip_set_batch_callback(C.cast(cb, C.c_void_p), None)
    try:
        got_m = _door(tmp_path, "m", src, D, 0, _unit_box, max_ndead=300, feedback=1)
        assert _registered(lib)[0] == C.cast(cb, C.c_void_p).value
    finally:
        lib.polychord_hip_set_batch_callback(None, None)
    assert len(calls) > 1 and max(calls) > 1
    assert "in batches" not in capfd.readouterr().out
    assert np.array_equal(got_m[-1][0], ds) and got_m[-1][2] == zs       # (the same values by the same door: the same run)
