"""Likelihoods written as HIP device source (pchip_source_create, PCHIP_LIKE_SOURCE), compiled at run time and fused into the sampling
kernels (polychordlite_amd/csrc/pc_rtc.hip).

CPU: the embedded kernel text is the files', every variant a launcher can ask for compiles for gfx950, a bad source fails with the log.
GPU: settings.ablate bit 15 (the built-ins through the run-time module) is the static kernel bit for bit; a source Gaussian walks the
oracle, which calls the same text compiled for the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_api as orc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "polychordlite_amd", "csrc")

# no transcendentals and no contraction: host and device give the same bits
GAUSS_SRC = r"""
#pragma clang fp contract(off)
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s = 0.0, m = 0.0;
    for (int i = 0; i < nDims; ++i) { const double z = (theta[i] - 0.5) / 0.1; s += z * z; m += theta[i]; }
    for (int e = 0; e < nDerived; ++e) phi[e] = (e == 0) ? s : m * (double)e;
    return -s / 2.0 + 1.3836465597893728 * (double)nDims;     /* - nDims (log 0.1 + log(2 pi) / 2) */
}
"""

# a straight line through ndata/2 points (x, y) in `data`: theta[0] = slope, theta[1] = intercept, unit noise
LINE_SRC = r"""
#pragma clang fp contract(off)
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s = 0.0;
    for (long i = 0; i + 1 < ndata; i += 2) { const double r = data[i + 1] - (theta[0] * data[i] + theta[1]); s += r * r; }
    if (nDerived > 0) phi[0] = s;
    return -s / 2.0;
}
"""


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_embedded_kernel_text_is_the_files():
    api, lib = _lib()
    seen = []
    i = 0
    while True:
        name = C.c_char_p()
        t = lib.pchip_rtc_embedded_source(i, C.byref(name))
        if t is None:
            break
        fn = name.value.decode()
        with open(os.path.join(CSRC, fn), "rb") as fh:
            assert t == fh.read(), fn
        seen.append(fn)
        i += 1
    assert set(seen) == {"pc_dev.h", "pc_state.h", "pc_seed.h", "pc_sample.hip", "pc_slice_body.inc"}


def test_source_symbols_are_exported():
    api, lib = _lib()
    for sym in ("pchip_source_create", "pchip_source_destroy", "pchip_rtc_embedded_source", "pchip_rtc_compile_check", "pchip_rtc_stats"):
        assert hasattr(lib, sym), sym
    assert lib.pchip_abi_version() == 9
    assert api.PATH_NAMES[19] == "source_kernels" and api.LIKE_KINDS["source"] == 5


def test_a_syntax_error_names_the_users_line():
    api, _ = _lib()
    bad = "\n\n__device__ double pchip_loglikelihood(const double *t, double *p, int D, int n, const double *d, long m)\n{ return t[0] +; }\n"
    with pytest.raises(RuntimeError) as e:
        api.source_create(bad)
    assert "pchip_user_source.h:4" in str(e.value) and "error" in str(e.value)


def test_a_source_without_the_likelihood_is_refused():
    api, _ = _lib()
    with pytest.raises(RuntimeError) as e:
        api.source_create("__device__ double something_else(double x) { return x; }\n")
    assert "pchip_loglikelihood" in str(e.value)


def test_every_general_variant_compiles_for_gfx950():
    """the kernels the launchers of pc_sample.hip can choose for a source likelihood, at every nDims class, in one program"""
    api, lib = _lib()
    h = api.source_create(GAUSS_SRC, options=("-DPCHIP_TEST_OPTION=1",))
    names = ["k_generate_live<1>", "k_generate_live<2>", "k_generate_live<4>"]
    for dpl, nrows in ((1, 1), (1, 2), (1, 4), (2, 4), (4, 4)):
        names += [f"k_slice<{dpl}, {nrows}, false>", f"k_slice<{dpl}, {nrows}, true>"]
    for nrows, fw in ((1, 8), (1, 16), (2, 24)):
        names += [f"k_slice<1, {nrows}, false, 1, {fw}>", f"k_slice_many<1, {nrows}, false, 1, {fw}, 0>"]
    names += [f"k_slice_many<1, {nrows}, false, 1, 0, 0>" for nrows in (1, 2, 4)]
    log = C.create_string_buffer(1 << 16)
    sec = C.c_double()
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(names).encode(), log, len(log), C.byref(sec))
    assert rc == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_user_macros_do_not_reach_the_library_kernels():
    """the user's text follows the library's in the run-time unit, and -D options become #defines in front of the user's text only:
    short names that the kernels use everywhere (D, S, nr) may be macros of the user's"""
    api, lib = _lib()
    src = "#define D 3\n#define nr 7\n" + GAUSS_SRC.replace("nDims; ++i", "nDims + S - 1; ++i")
    h = api.source_create(src, options=("-DS=1",))
    log = C.create_string_buffer(1 << 16)
    assert lib.pchip_rtc_compile_check(h, b"gfx950", b"k_slice<1, 2, false>", log, len(log), None) == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_options_other_than_defines_are_refused():
    api, _ = _lib()
    with pytest.raises(RuntimeError) as e:
        api.source_create(GAUSS_SRC, options=("-DA=1", "-ffast-math"))
    assert "-ffast-math" in str(e.value)


def test_run_repeats_refuses_a_source_likelihood(capfd):
    """the runs in step take k_slice_many from the module: not pinned to the solo runs yet, so refused with a message"""
    api, lib = _lib()
    from polychordlite_amd import repeats
    h = api.source_create(GAUSS_SRC)
    s = _settings(api, 4, 0, nlive=50, num_repeats=8)
    L, P, keep = api.make_problem("source", 4, 0, source=h)
    with pytest.raises(RuntimeError):
        repeats.run_repeats(s, L, P, [1, 2])
    assert "device source likelihood" in capfd.readouterr().err
    lib.pchip_source_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _settings(api, D, nDer, **kw):
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


BOX = {"gaussian": (None, None), "rastrigin": (-5.12, 5.12), "twin_gaussian": (-1.0, 1.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,D,nDer,ablate", [("gaussian", 4, 2, 0), ("gaussian", 20, 2, 0), ("gaussian", 20, 1, 1),
                                                ("gaussian", 40, 0, 1), ("rastrigin", 8, 0, 0), ("rastrigin", 20, 0, 0),
                                                ("twin_gaussian", 6, 1, 0), ("twin_gaussian", 30, 1, 0)])
def test_runtime_module_is_the_static_kernel(engine, kind, D, nDer, ablate):
    api = engine
    lo, hi = BOX[kind]
    out = []
    for bit in (0, 1 << 15):
        s = _settings(api, D, nDer, nlive=150, num_repeats=2 * D, seed=11, ablate=ablate | bit)
        L, P, keep = api.make_problem(kind, D, nDer, lo, hi)
        out.append(api.run(s, L, P))
    a, b = out
    for k in ("ndead", "nlike", "niter"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["logZ"] == b["logZ"]
    assert np.array_equal(a["dead"], b["dead"])
    assert a["path"]["source_kernels"] == 0 and b["path"]["source_kernels"] > 0


def _host_like(tmp_path, src, name):
    """the same source compiled for the host, as the oracle's callback"""
    cpp = tmp_path / f"{name}.cpp"
    so = tmp_path / f"lib{name}.so"
    cpp.write_text(src + "\nextern \"C\" double host_logl(const double *t, int D, double *phi, int nDer, void *ctx)\n"
                   "{ const double *d = ((const double **)ctx)[0]; long n = (long)((const double **)ctx)[1]; "
                   "return pchip_loglikelihood(t, phi, D, nDer, d, n); }\n")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-D__device__=", "-x", "c++", str(cpp), "-o", str(so)])
    return C.CDLL(str(so))


def _source_vs_oracle(api, tmp_path, src, D, nDer, data=None, grades=None, **kw):
    h = api.source_create(src, data=data)
    s = _settings(api, D, nDer, seed=5, **kw)
    keep = []
    if grades:
        keep.append(api.set_grades(s, *grades))
    L, P, k1 = api.make_problem("source", D, nDer, source=h)
    g = api.run(s, L, P)
    assert g["path"]["source_kernels"] > 0
    hl = _host_like(tmp_path, src, f"src{D}_{nDer}")
    d = np.ascontiguousarray(np.zeros(1) if data is None else data, dtype=np.float64)
    ctx = (C.c_void_p * 2)(d.ctypes.data, 0 if data is None else d.size)
    kwo = dict(kw)
    if kw.get("sequential_rng"):   # one gaussian deviate goes to time_speeds (generate.F90:285-287), as in test_gpu_parity.py
        kwo["time_speeds_draw"] = 1 if grades is None else 0
    so = orc.settings(D, nDer, seed=5, **kwo)
    if grades:
        keep.append(orc.set_grades(so, grades[0], grades[1]))
    Lo, Po, k2 = orc.make_problem("gaussian", D)
    Lo.kind = 0
    Lo.fn = C.cast(hl.host_logl, C.c_void_p)
    Lo.ctx = C.cast(ctx, C.c_void_p)
    o = orc.run(so, Lo, Po)
    for k in ("ndead", "nlike", "niter", "nbatches", "ncluster", "ncluster_dead"):
        assert g[k] == o[k], (k, g[k], o[k])
    assert abs(g["logZ"] - o["logZ"]) < 1e-8
    rel = np.abs(g["dead"] - o["dead"]) / np.maximum(1.0, np.abs(o["dead"]))
    assert rel.max() < 1e-7
    api.load().pchip_source_destroy(h)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("D,nDer,extra", [(4, 0, dict(nlive=100, num_repeats=8, batch=16)),
                                          (20, 1, dict(nlive=200, num_repeats=40, batch=32)),
                                          (40, 5, dict(nlive=150, num_repeats=20, batch=32)),
                                          (4, 1, dict(nlive=200, num_repeats=8, batch=40, do_clustering=1)),
                                          (6, 5, dict(nlive=60, num_repeats=12, batch=1, sequential_rng=1))])
def test_source_walks_the_oracle(engine, tmp_path, D, nDer, extra):
    g = _source_vs_oracle(engine, tmp_path, GAUSS_SRC, D, nDer, **extra)
    if nDer >= 2:   # every derived parameter is the user's (the built-ins wrote at most two)
        th = g["dead"][:, D:2 * D]
        assert np.allclose(g["dead"][:, 2 * D + 1], th.sum(axis=1), rtol=1e-12)


@pytest.mark.gpu
def test_graded_source_walks_the_oracle(engine, tmp_path):
    _source_vs_oracle(engine, tmp_path, GAUSS_SRC, 6, 1, grades=([3, 3], [2, 4]), nlive=100, num_repeats=6, batch=20)


@pytest.mark.gpu
def test_data_fit_source_walks_the_oracle(engine, tmp_path):
    rng = np.random.default_rng(3)
    x = np.linspace(-1.0, 1.0, 256)
    y = 0.3 * x + 0.6 + rng.normal(0.0, 1.0, x.size)
    data = np.stack([x, y], axis=1).ravel()
    g = _source_vs_oracle(engine, tmp_path, LINE_SRC, 2, 1, data=data, nlive=100, num_repeats=6, batch=20)
    assert g["ndead"] > 0


@pytest.mark.gpu
def test_host_callback_prior_with_a_source_is_refused(engine, capfd):
    api = engine
    h = api.source_create(GAUSS_SRC)
    s = _settings(api, 4, 0, nlive=50, num_repeats=8)
    L, P, keep = api.make_problem("source", 4, 0, source=h)
    P.kind = 0
    lib = api.load()
    r = api.Result()
    assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(P), C.byref(r)) == 1
    assert "needs a device prior" in capfd.readouterr().err
    lib.pchip_source_destroy(h)


@pytest.mark.gpu
def test_more_than_32_derived_parameters_are_refused(engine, capfd):
    api = engine
    h = api.source_create(GAUSS_SRC)
    s = _settings(api, 4, 33, nlive=50, num_repeats=8)
    L, P, keep = api.make_problem("source", 4, 33, source=h)
    lib = api.load()
    r = api.Result()
    assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(P), C.byref(r)) == 1
    assert "at most 32 derived parameters" in capfd.readouterr().err
    lib.pchip_source_destroy(h)


# a hand-written Rastrigin (transcendentals: not the built-in's bits, the same distribution)
RASTRIGIN_SRC = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s = 0.0;
    for (int i = 0; i < nDims; ++i) s += 8.515435146961291 + theta[i] * theta[i] - 10.0 * cos(6.283185307179586 * theta[i]);
    return -s;
}
"""


@pytest.mark.gpu
def test_a_transcendental_source_has_the_builtins_distribution(engine):
    api = engine
    h = api.source_create(RASTRIGIN_SRC)
    zs, zb, errs = [], [], []
    for seed in (1, 2, 3, 4):
        for kind, out in (("source", zs), ("rastrigin", zb)):
            s = _settings(api, 2, 0, nlive=200, num_repeats=6, seed=seed, do_clustering=1)
            L, P, keep = api.make_problem(kind, 2, 0, -5.12, 5.12, source=h)
            g = api.run(s, L, P)
            out.append(g["logZ"])
            errs.append(g["logZerr"])
    sig = float(np.sqrt(np.mean(np.square(errs)) * (1.0 / len(zs) + 1.0 / len(zb))))
    assert abs(np.mean(zs) - np.mean(zb)) < 3.0 * sig, (zs, zb, sig)
    api.load().pchip_source_destroy(h)
