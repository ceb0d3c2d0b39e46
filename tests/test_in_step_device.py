"""Runs in step for a problem that is wholly the user's own (pchip_run_in_step, repeats.run_in_step): a device source likelihood, plain or terms
form, and / or a device prior (a table, the handle's own source prior).  The sampling kernel of such a group is k_slice_many with the prior kind
as its seventh template argument, chosen by pc_launch_slice_step (polychordlite_amd/csrc/pc_sample.hip) from a table of its own.

The yardstick is no tolerance: every run of run_in_step IS `_ctypes_api.run` of its seed -- ndead, nlike, niter, log Z and the whole dead array,
bit for bit.  path["slice_step"] tells a shared launch from each run launching its own k_slice (which is exact by construction).

CPU: the door is declared and exported and refuses what is not on the device before any device call; every row of the new variant table
compiles for gfx950 with every kind of handle; the launcher's plan is held against its rules by a host-only recorder under the sanitizers.
GPU: the eight cases of the list below."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polychordlite_amd", "csrc")

# the 0.1-wide Gaussian about 0.5; phi[0] = the sum of squares, phi[e] = e times the sum of theta
GAUSS = r"""
#pragma clang fp contract(off)
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s = 0.0, m = 0.0;
    for (int i = 0; i < nDims; ++i) { const double z = (theta[i] - 0.5) / 0.1; s += z * z; m += theta[i]; }
    for (int e = 0; e < nDerived; ++e) phi[e] = (e == 0) ? s : m * (double)e;
    return -s / 2.0 + 1.3836465597893728 * (double)nDims;
}
"""

# a straight line through the points (x, y) of `data` from index OFF on, one term a point: theta[0] = slope, theta[1] = intercept, unit noise
LINE_TERMS = r"""
#pragma clang fp contract(off)
#ifndef OFF
#define OFF 0
#endif
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{
    const double r = data[OFF + 2 * i + 1] - (theta[0] * data[OFF + 2 * i] + theta[1]);
    return r * r;
}
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sum;
    for (int e = 1; e < nDerived; ++e) phi[e] = theta[0] + theta[1];
    return -sum / 2.0;
}
"""

# two 0.04-wide modes, at 0.3 and at 0.7 in every coordinate
TWO_MODES = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double a = 0.0, b = 0.0;
    for (int i = 0; i < nDims; ++i) { const double u = (theta[i] - 0.3) / 0.04, v = (theta[i] - 0.7) / 0.04; a += u * u; b += v * v; }
    const double la = -a / 2.0, lb = -b / 2.0, hi = la > lb ? la : lb;
    for (int e = 0; e < nDerived; ++e) phi[e] = theta[0];
    return hi + log(exp(la - hi) + exp(lb - hi));
}
"""

# theta_i = data[i] + data[nDims + i] * cube[i]
AFFINE_PRIOR = r"""
__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata)
{
    return data[i] + data[nDims + i] * cube[i];
}
"""


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _settings(api, D, nDer, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _line_data(n):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, n)
    return np.stack([x, 0.3 * x + 0.6 + rng.normal(0.0, 1.0, n)], axis=1).ravel()


def _affine_data(D):
    return np.concatenate([np.linspace(-0.6, -0.2, D), np.linspace(1.5, 2.5, D)])      # (the Gaussian four sigma or more from every edge)


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_the_door_is_declared_and_exported():
    api, lib = _lib()
    from polychordlite_amd import repeats
    hdr = open(os.path.join(ROOT, "include", "polychord_hip.h")).read()
    assert "int  pchip_run_in_step(" in hdr and "PCHIP_PATH_SLICE_STEP = 22" in hdr
    assert hasattr(lib, "pchip_run_in_step") and callable(repeats.run_in_step)
    assert api.PATH_NAMES[22] == "slice_step" and len(api.PATH_NAMES) == 23


def test_a_callback_likelihood_is_refused_with_the_reason(capfd):
    """before any device call: this machine may have no device"""
    api, lib = _lib()
    from polychordlite_amd import repeats
    s = _settings(api, 4, 0, nlive=50, num_repeats=8)
    L, P, keep = api.make_problem("gaussian", 4, 0)
    L.kind = 0                                                        # PCHIP_LIKE_CALLBACK
    with pytest.raises(RuntimeError) as e:
        repeats.run_in_step(s, L, P, [1, 2])
    assert "pchip_run_in_step failed with code 1" in str(e.value)
    err = capfd.readouterr().err
    assert "pchip_run_in_step" in err and "callback likelihood" in err, err


def test_a_host_prior_is_refused_with_the_reason(capfd):
    api, lib = _lib()
    from polychordlite_amd import repeats
    s = _settings(api, 4, 0, nlive=50, num_repeats=8)
    L, P, keep = api.make_problem("gaussian", 4, 0)
    P.kind = 0                                                        # a callback prior
    with pytest.raises(RuntimeError):
        repeats.run_in_step(s, L, P, [1, 2])
    err = capfd.readouterr().err
    assert "host prior" in err and "prior.kind = 0" in err, err


STEP_ROWS = [(nrows, fw, pt) for pt in (0, 1) for nrows, fw in ((1, 0), (2, 0), (4, 0), (1, 8), (1, 16), (2, 24))]


def test_the_step_table_is_the_rows_of_the_issue():
    """PC_SLICE_STEP_VARIANTS, behind pc_slice_launch (the two tables in front of it are pinned by tests/test_launch_plan.py), holds exactly the
    general variants without and with the prior kind"""
    import re
    src = open(os.path.join(CSRC, "pc_sample.hip")).read()
    at = src.index("#define PC_SLICE_STEP_VARIANTS(X)")
    assert at > src.index("static int pc_slice_launch(")
    rows = re.findall(r"\bX\(([^)]*)\)", src[at:src.index("static PcSlicePlan pc_slice_step_plan(")])
    assert sorted(rows) == sorted(f"1, {nrows}, false, 1, {fw}, 0, {pt}" for nrows, fw, pt in STEP_ROWS)


@pytest.mark.parametrize("handle", ["plain", "terms", "prior_plain", "prior_terms"])
def test_every_row_of_the_step_table_compiles_for_gfx950(handle):
    """k_slice_many with its seventh argument, every row of PC_SLICE_STEP_VARIANTS in one program per kind of handle"""
    api, lib = _lib()
    text = (GAUSS if "plain" in handle else LINE_TERMS) + (AFFINE_PRIOR if "prior" in handle else "")
    h = api.source_create(text, data=_line_data(100), nterms=None if "plain" in handle else 100, prior="prior" in handle)
    names = [f"k_slice_many<1, {nrows}, false, 1, {fw}, 0, {pt}>" for nrows, fw, pt in STEP_ROWS]
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(names).encode(), log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_the_step_launcher_follows_its_rules():
    """tools/dev/slice_step_record: pc_launch_slice_step over a grid of fabricated states, host only, built with the host address and undefined-behaviour sanitizers.
    It declines exactly nDims > 64 unfused, what pc_slice_fusable refuses fused, grades, the sequential stream and the correlated Gaussian;
    every launch it makes is a row of its table with the LDS, grid and block of the rules (the tool exits 1 on the first disagreement)"""
    subprocess.run(["make", "-C", CSRC, "slice_step_record"], check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PC_")}
    r = subprocess.run([os.path.join(ROOT, "tools", "dev", "slice_step_record")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "12 of 12 rows reached, 0 disagreements" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------------------- GPU
_HANDLES = {}


def _handle(api, key, text, **kw):
    """one handle per text and data block for the whole module: each of its kernel variants compiles once"""
    if key not in _HANDLES:
        _HANDLES[key] = api.source_create(text, **kw)
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _destroy_handles():
    yield
    api, lib = _lib()
    for h in _HANDLES.values():
        lib.pchip_source_destroy(h)
    _HANDLES.clear()


def _same(a, b, what):
    for k in ("ndead", "nlike", "niter"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["logZ"] == b["logZ"], (what, a["logZ"], b["logZ"])
    assert a["dead"].shape == b["dead"].shape and np.array_equal(a["dead"], b["dead"]), (what, int((a["dead"] != b["dead"]).sum()))


def _in_step_is_solo(api, D, nDer, L, P, seeds, max_in_flight=4, **kw):
    """run_in_step of `seeds`, each run held against pchip_run of its seed; (merged, runs)"""
    from polychordlite_amd import repeats
    merged, runs = repeats.run_in_step(_settings(api, D, nDer, **kw), L, P, seeds, max_in_flight=max_in_flight)
    assert len(runs) == len(seeds)
    for seed, r in zip(seeds, runs):
        assert r["ndead"] > 0
        _same(r, api.run(_settings(api, D, nDer, seed=seed, **kw), L, P), f"seed {seed}")
    return merged, runs


TABLE6 = [("gaussian", (0.5, 0.5))] * 3 + [("sorted_uniform", 1, (0.0, 1.0))] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("D", [4, 12, 20, 30, 40])
def test_1_a_plain_source_under_the_box(engine, D):
    """FW 8, 16, 24 fused; NROWS 2 and 4 behind the bases kernel"""
    api = engine
    L, P, keep = api.make_problem("source", D, 2, source=_handle(api, "gauss", GAUSS))
    merged, runs = _in_step_is_solo(api, D, 2, L, P, [11, 12, 13], nlive=100, num_repeats=min(2 * D, 24), batch=16)
    for r in runs:
        assert r["path"]["slice_step"] > 0 and r["path"]["source_kernels"] > 0, r["path"]
        assert r["path"]["source_terms"] == 0 and r["path"]["device_prior"] == 0, r["path"]


@pytest.mark.gpu
@pytest.mark.parametrize("nterms,D", [(37, 2), (100, 3)])
def test_2_a_terms_source_with_a_derived_parameter(engine, nterms, D):
    """37 terms: lanes without a term; 100: lanes that loop.  The second theta of a bracket lies behind the chain's LDS block"""
    api = engine
    L, P, keep = api.make_problem("source", D, 1, source=_handle(api, ("line", nterms), LINE_TERMS, data=_line_data(nterms), nterms=nterms), lo=-2.0, hi=2.0)
    merged, runs = _in_step_is_solo(api, D, 1, L, P, [21, 22, 23], nlive=100, num_repeats=2 * D, batch=16)
    for r in runs:
        assert r["path"]["source_terms"] > 0 and r["path"]["slice_step"] > 0, r["path"]


@pytest.mark.gpu
@pytest.mark.parametrize("like", ["gaussian", "source"])
def test_3_a_prior_table(engine, like):
    """Gaussian entries and a sorted_uniform block, on the built-in Gaussian (the static kernel) and on a plain source (the module's)"""
    api = engine
    D = 6
    L, P, keep = api.make_problem(like, D, 1, source=_handle(api, "gauss", GAUSS) if like == "source" else 0, prior_table=TABLE6)
    merged, runs = _in_step_is_solo(api, D, 1, L, P, [31, 32, 33], nlive=100, num_repeats=12, batch=16)
    for r in runs:
        assert r["path"]["device_prior"] > 0 and r["path"]["slice_step"] > 0, r["path"]
        assert (r["path"]["source_kernels"] > 0) == (like == "source"), r["path"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "terms"])
def test_4_a_source_prior(engine, form):
    api = engine
    if form == "plain":
        D = 4
        h = _handle(api, "gauss_affine", GAUSS + AFFINE_PRIOR, data=_affine_data(D), prior=True)
    else:
        D = 2
        h = _handle(api, "line_affine", LINE_TERMS + AFFINE_PRIOR, options=("-DOFF=4",), data=np.concatenate([[-2.0, -2.0, 4.0, 4.0], _line_data(64)]), nterms=64, prior=True)
    L, P, keep = api.make_problem("source", D, 1, source=h, prior_source=True)
    assert P.kind == 3
    merged, runs = _in_step_is_solo(api, D, 1, L, P, [41, 42, 43], nlive=100, num_repeats=2 * D, batch=16)
    for r in runs:
        assert r["path"]["slice_step"] > 0 and r["path"]["device_prior"] > 0 and (r["path"]["source_terms"] > 0) == (form == "terms"), r["path"]
        if form == "plain":      # (theta is the handle's prior of the cube, not a box)
            assert np.array_equal(r["dead"][:, D:2 * D], _affine_data(D)[:D] + _affine_data(D)[D:] * r["dead"][:, :D])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
def test_4_a_handle_with_a_prior_under_the_box_and_a_table(engine, kind):
    """the transform's branch is on prior.kind: in step, too, a handle WITH a prior run under kinds 1 and 2 is the handle without one"""
    api = engine
    from polychordlite_amd import repeats
    D = 4
    table = [("gaussian", (0.5, 0.5))] * 2 + [("uniform", (-0.5, 1.5))] * 2
    out = {}
    for who, h in (("prior", _handle(api, "gauss_affine", GAUSS + AFFINE_PRIOR, data=_affine_data(D), prior=True)), ("plain", _handle(api, "gauss", GAUSS))):
        L, P, keep = api.make_problem("source", D, 1, source=h, prior_table=table if kind == 2 else None)
        assert P.kind == kind
        out[who] = repeats.run_in_step(_settings(api, D, 1, nlive=100, num_repeats=8, batch=16), L, P, [44, 45, 46])[1]
    for a, b in zip(out["prior"], out["plain"]):
        _same(a, b, f"kind {kind}")
        assert a["path"] == b["path"] and a["path"]["slice_step"] > 0 and (a["path"]["device_prior"] > 0) == (kind == 2), a["path"]


@pytest.mark.gpu
def test_4_a_source_prior_needs_a_handle_with_a_prior(engine, capfd):
    """as pchip_run fails: code 1 and the two names"""
    api = engine
    from polychordlite_amd import repeats
    L, P, keep = api.make_problem("source", 4, 0, source=_handle(api, "gauss", GAUSS), prior_source=True)
    with pytest.raises(RuntimeError) as e:
        repeats.run_in_step(_settings(api, 4, 0, nlive=50, num_repeats=8), L, P, [1, 2])
    assert "code 1" in str(e.value)
    err = capfd.readouterr().err
    assert "pchip_prior_param" in err and "pchip_source_create_prior" in err, err


@pytest.mark.gpu
def test_5_clustered_runs_in_several_scheduler_groups(engine):
    """five seeds, four in flight, clustering: four scheduler threads of the device ask the run-time registry for the same kernels at once"""
    api = engine
    D = 3
    L, P, keep = api.make_problem("source", D, 1, source=_handle(api, "two_modes", TWO_MODES))
    merged, runs = _in_step_is_solo(api, D, 1, L, P, [51, 52, 53, 54, 55], max_in_flight=4, nlive=150, num_repeats=6, batch=16, do_clustering=1)
    assert merged["n_runs"] == 5
    for r in runs:
        assert r["ncluster_peak"] > 1, r["ncluster_peak"]
        assert r["path"]["source_kernels"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,D,lo,hi", [("rastrigin", 8, -5.12, 5.12), ("twin_gaussian", 6, -1.0, 1.0)])
def test_6_the_builtins_through_the_module(engine, kind, D, lo, hi):
    """settings.ablate bit 15 in step is the static kernels in step, bit for bit; only the former counts run-time compiled launches"""
    api = engine
    from polychordlite_amd import repeats
    L, P, keep = api.make_problem(kind, D, 1, lo=lo, hi=hi)
    kw = dict(nlive=100, num_repeats=2 * D, batch=16, do_clustering=0)
    stat = repeats.run_in_step(_settings(api, D, 1, **kw), L, P, [61, 62, 63])[1]
    rtc = repeats.run_in_step(_settings(api, D, 1, ablate=1 << 15, **kw), L, P, [61, 62, 63])[1]
    for a, b in zip(rtc, stat):
        _same(a, b, kind)
        assert a["path"]["source_kernels"] > 0 and b["path"]["source_kernels"] == 0, (a["path"], b["path"])
        assert a["path"]["slice_step"] > 0 and b["path"]["slice_step"] > 0, (a["path"], b["path"])


@pytest.mark.gpu
def test_7_a_shape_without_a_shared_row(engine):
    """a table at nDims 70: the runs go round by round together, each launches its own k_slice"""
    api = engine
    D = 70
    table = [("gaussian", (0.5, 0.2))] * 60 + [("sorted_uniform", 3, (0.0, 1.0))] * 8 + [("half_gaussian", (0.4, 0.2))] * 2
    L, P, keep = api.make_problem("gaussian", D, 0, prior_table=table)
    merged, runs = _in_step_is_solo(api, D, 0, L, P, [71, 72, 73], nlive=100, num_repeats=20, batch=16, max_ndead=300)
    for r in runs:
        assert r["path"]["slice_step"] == 0 and r["path"]["device_prior"] > 0 and r["path"]["slice_wave"] > 0, r["path"]


@pytest.mark.gpu
def test_8_more_seeds_than_runs_in_flight(engine):
    api = engine
    D = 4
    L, P, keep = api.make_problem("source", D, 2, source=_handle(api, "gauss", GAUSS))
    merged, runs = _in_step_is_solo(api, D, 2, L, P, [81, 82, 83, 84, 85], max_in_flight=2, nlive=100, num_repeats=8, batch=16)
    assert merged["n_runs"] == 5
    # (two, two and one: the last run is a group of one)
    assert all(r["path"]["slice_step"] > 0 for r in runs[:4]) and runs[4]["path"]["slice_step"] == 0, [r["path"]["slice_step"] for r in runs]
