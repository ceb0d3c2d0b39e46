"""Shared values of a device source (pchip_source_create_shared): what the terms need of theta alone is computed once per evaluated point,
one lane per value, into a block in LDS, and every function of the handle's form -- terms, sums or quadratic -- gets the finished block as
`shared` behind theta (polychordlite_amd/csrc/pc_sample.hip, PCHIP_USER_SHARED).

The fixture GRID is a quadratic in g tabulated on a grid and interpolated to the data points: theta = (a, b, c), data = g[NSH] | w[NPT] |
d[NPT] (abscissae, weights in [0, 1], data), shared_k = a + b g_k + c g_k g_k, and term i interpolates between shared[j_i] and
shared[j_i + 1] with j_i = (7 i + 3) % (NSH - 1) -- almost every lane reads values other lanes wrote, so a missing barrier or a block filled
from the wrong point changes bits.  ONE text carries the overloads of all three forms (the library declares and calls only those of the
handle's form).  It is written with #pragma clang fp contract(off) and + - * / only (the quadratic form's fma is the library's own), so
that a host build gives the device's bits.

Its REPLAY is a plain pchip_loglikelihood source: the same text, wrappers with the signatures without `shared` that find the block behind
theta (theta + nDims), the serial replay of the form as tests/test_source_terms.py, test_source_sums.py and test_source_quad.py define it
-- their REPLAY_WRAPPER texts, imported, under another name --, and a pchip_loglikelihood that copies theta, fills the nshared values
serially in ascending k behind it and calls that replay.  This is the defined order run by code that existed before shared values did.

CPU: the surface, the refusals, every variant a launcher can choose compiles for gfx950 from a shared handle of each form and at the
limits, the other forms beside them compile what they did; the host replay's shared values against the definition in numpy.
GPU: the order bit for bit; a shared run is the replay's run; runs in step; the maximiser; the pypolychord door."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_source_terms import (_terms_variants, _tree64, _strided_partials, _assert_same_run,  # noqa: F401  (the issue's idiom: imported, not copied)
                                     REPLAY_WRAPPER as TERMS_REPLAY, LINE_TERMS, replay_of as line_replay)
from tests.test_source_sums import REPLAY_WRAPPER as SUMS_REPLAY, EIGHT, _eight_data
from tests.test_source_quad import REPLAY_WRAPPER as QUAD_REPLAY, QUAD, _precision, _line_data as _quad_line_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the box of the prior: the tabulated model a + b g + c g^2 stays above 0.2 on g in [-1, 1] (the sums form divides by a sum of m^2)
LO, HI = [1.0, -0.4, -0.4], [2.0, 0.4, 0.4]
TRUTH = (1.5, 0.2, -0.1)

GRID = r"""
#pragma clang fp contract(off)
__device__ double pchip_shared_value(const double *theta, int nDims, const double *data, long ndata, long k)
{
    const double g = data[k];
    return theta[0] + theta[1] * g + theta[2] * g * g;
}
static __device__ double grid_model(const double *shared, const double *data, long i)
{
#if NSH == 1
    return shared[0];
#else
    const long j = (7 * i + 3) % (NSH - 1);
    return shared[j] + data[NSH + i] * (shared[j + 1] - shared[j]);
#endif
}
__device__ double pchip_logl_term(const double *theta, const double *shared, int nDims, const double *data, long ndata, long i)
{
    const double z = (data[NSH + NPT + i] - grid_model(shared, data, i)) / 0.05;
    return z * z;
}
__device__ double pchip_residual(const double *theta, const double *shared, int nDims, const double *data, long ndata, long i)
{
    return data[NSH + NPT + i] - grid_model(shared, data, i);
}
__device__ double pchip_logl_finish(double sum, const double *theta, const double *shared, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sum;
    if (nDerived > 1) phi[1] = shared[NSH - 1];
    if (nDerived > 2) phi[2] = shared[0];
    for (int e = 3; e < nDerived; ++e) phi[e] = 0.0;
    return -sum / 2.0;
}
__device__ void pchip_logl_terms(const double *theta, const double *shared, int nDims, const double *data, long ndata, long i, double *t)
{
    const double m = grid_model(shared, data, i);
    t[0] = m;
    t[1] = m * m;
    t[2] = data[NSH + NPT + i] * m;
}
/* the amplitude A of the model A m_i profiled out in closed form: A = sum d m / sum m m, chi2 = (sum d d - A sum d m) / 0.05^2, of which the
   first part does not depend on theta and is left out */
__device__ double pchip_logl_finish_sums(const double *sums, const double *theta, const double *shared, double *phi, int nDims, int nDerived,
                                         const double *data, long ndata)
{
    const double A = sums[2] / sums[1];
    if (nDerived > 0) phi[0] = A;
    if (nDerived > 1) phi[1] = shared[NSH - 1];
    if (nDerived > 2) phi[2] = shared[0];
    for (int e = 3; e < nDerived; ++e) phi[e] = sums[0];
    return (A * sums[2]) / 0.005;
}
"""

# the signatures without `shared`, for the replays of the three forms: the block lies behind the nDims parameters
OLD_SIGNATURES = r"""
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{ return pchip_logl_term(theta, theta + nDims, nDims, data, ndata, i); }
__device__ double pchip_residual(const double *theta, int nDims, const double *data, long ndata, long i)
{ return pchip_residual(theta, theta + nDims, nDims, data, ndata, i); }
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{ return pchip_logl_finish(sum, theta, theta + nDims, phi, nDims, nDerived, data, ndata); }
__device__ void pchip_logl_terms(const double *theta, int nDims, const double *data, long ndata, long i, double *t)
{ pchip_logl_terms(theta, theta + nDims, nDims, data, ndata, i, t); }
__device__ double pchip_logl_finish_sums(const double *sums, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{ return pchip_logl_finish_sums(sums, theta, theta + nDims, phi, nDims, nDerived, data, ndata); }
"""

# step 1 and 2 of the defined order, serially, then the form's own replay on theta | shared
SHARED_REPLAY = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double buf[MAXD + NSH];
    double *sh = buf + nDims;
    for (int j = 0; j < nDims; ++j) buf[j] = theta[j];
    for (long k = 0; k < NSH; ++k) sh[k] = pchip_shared_value(theta, nDims, data, ndata, k);
    return replay_of_the_form(buf, phi, nDims, nDerived, data, ndata);
}
"""

HOST_WRAPPER = r"""
extern "C" void host_eval(const double *t, long n, int D, int nDer, const double *d, long nd, double *logL, double *phi)
{ double scratch[32]; for (long p = 0; p < n; ++p) logL[p] = pchip_loglikelihood(t + p * D, nDer > 0 ? phi + p * nDer : scratch, D, nDer, d, nd); }
extern "C" void host_shared(const double *t, int D, const double *d, long nd, double *sh)
{ for (long k = 0; k < NSH; ++k) sh[k] = pchip_shared_value(t, D, d, nd, k); }
"""

# the quadratic form's replay takes the user's data as 2 NRES doubles and the matrix behind them: here the user's data are NDATA doubles
FORM_REPLAY = {"terms": TERMS_REPLAY, "sums": SUMS_REPLAY, "quad": QUAD_REPLAY.replace("2 * NRES", "NDATA")}
assert FORM_REPLAY["quad"].count("NDATA") == 3


def replay_of(form):
    inner = FORM_REPLAY[form]
    assert inner.count("pchip_loglikelihood") == 1
    return GRID + OLD_SIGNATURES + inner.replace("pchip_loglikelihood", "replay_of_the_form") + SHARED_REPLAY


def _options(form, nsh, n, D=3):
    o = [f"-DNSH={nsh}", f"-DNPT={n}", f"-DMAXD={max(D, 3)}", f"-DNDATA={nsh + 2 * n}"]
    o += {"terms": [f"-DNTERMS={n}"], "sums": [f"-DNTERMS={n}", "-DNSUMS=3"], "quad": [f"-DNRES={n}"]}[form]
    return tuple(o)


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _create_shared(api, text, **kw):
    """source_create with shared=: the door this file is about (a library without the feature fails here, at the missing symbol)"""
    assert hasattr(api.load(), "pchip_source_create_shared"), "the library does not export pchip_source_create_shared"
    return api.source_create(text, **kw)


def _settings(api, D, nDer, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _model(th, data, nsh, n):
    """[npts][n]: shared values and the interpolation as the source forms them, operation for operation"""
    g, w = data[:nsh], data[nsh:nsh + n]
    a, b, c = th[:, 0:1], th[:, 1:2], th[:, 2:3]
    sh = (a + b * g[None, :]) + (c * g[None, :]) * g[None, :]
    if nsh == 1:
        return sh, np.repeat(sh[:, 0:1], n, axis=1)
    j = (7 * np.arange(n) + 3) % (nsh - 1)
    return sh, sh[:, j] + w[None, :] * (sh[:, j + 1] - sh[:, j])


def _grid_data(nsh, n, seed=3):
    """g = an irregular grid on [-1, 1], w = uniform(0, 1), d = the model at TRUTH + noise of 0.05; the block g | w | d"""
    rng = np.random.default_rng(seed + 1000 * nsh + n)
    g = np.sort(rng.uniform(-1.0, 1.0, nsh))
    w = rng.uniform(0.0, 1.0, n)
    block = np.concatenate([g, w, np.zeros(n)])
    block[nsh + n:] = _model(np.array([TRUTH]), block, nsh, n)[1][0] + rng.normal(0.0, 0.05, n)
    return block


def _host_replay(tmp_path, form, nsh, n, name, D=3):
    cpp = tmp_path / f"{name}.cpp"
    so = tmp_path / f"lib{name}.so"
    cpp.write_text("#include <math.h>\n" + replay_of(form) + HOST_WRAPPER)
    defs = [o for o in _options(form, nsh, n, D)]
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-D__device__=", *defs, "-x", "c++", str(cpp), "-o", str(so)])
    return C.CDLL(str(so))


def _host_eval(hl, th, nDer, block):
    n, D = th.shape
    logL, phi = np.empty(n), np.empty((n, max(nDer, 1)))
    hl.host_eval(th.ctypes.data_as(C.c_void_p), C.c_long(n), D, nDer, block.ctypes.data_as(C.c_void_p), C.c_long(block.size),
                 logL.ctypes.data_as(C.c_void_p), phi.ctypes.data_as(C.c_void_p))
    return logL, phi[:, :nDer]


def _box_points(npts, seed, D=3):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0.0, 1.0, (npts, D))
    th[:, :3] = np.array(LO) + (np.array(HI) - np.array(LO)) * th[:, :3]
    return np.ascontiguousarray(th)


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_the_surface_names_shared_values():
    api, lib = _lib()
    assert hasattr(lib, "pchip_source_create_shared")
    assert lib.pchip_abi_version() == 9
    hdr = open(os.path.join(ROOT, "include", "polychord_hip.h")).read()
    assert "#define PCHIP_SOURCE_MAX_SHARED 512" in hdr and re.search(r"int\s+pchip_source_create_shared\(", hdr)
    assert "pchip_shared_value" in hdr
    import inspect
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    assert "shared" in inspect.signature(api.source_create).parameters
    assert inspect.signature(api.source_create).parameters["shared"].default is None
    assert "shared" in inspect.signature(dl.Source.__init__).parameters
    assert dl.Source(GRID, data=np.zeros(4), nterms=1, shared=2).shared == 2
    assert "pchip_source_create_shared" in open(os.path.join(ROOT, "include", "polychord_hip.hpp")).read()
    assert 'bind(c, name="pchip_source_create_shared")' in open(os.path.join(ROOT, "bindings", "fortran", "polychord_hip.f90")).read()
    cli = open(os.path.join(ROOT, "tools", "polychord_hip_cli.cpp")).read()
    usage = cli[cli.index("USAGE ="):]
    assert "[shared:N]" in usage[:usage.index("\n")] and "pchip_source_create_shared(" in cli


def _refused(lib, api, text, nshared, nterms, nsums, nres, precision, options=b"-DNSH=4 -DNPT=4"):
    p = None if precision is None else api.dptr(precision)
    h = lib.pchip_source_create_shared(text.encode(), options, api.dptr(_grid_data(4, 4)), 12, nshared, nterms, nsums, nres, p, 0)
    msg = lib.polychord_hip_last_error()
    assert h == -1 and msg
    return msg.decode(errors="replace")


@pytest.mark.parametrize("nshared", [0, 513, -2])
def test_nshared_out_of_range_is_refused_with_the_range(nshared):
    api, lib = _lib()
    msg = _refused(lib, api, GRID, nshared, 4, 0, 0, None)
    assert "nshared" in msg and "1 <= nshared <= 512" in msg and "PCHIP_SOURCE_MAX_SHARED" in msg


def test_a_mixed_form_a_missing_matrix_and_too_many_sums_are_refused():
    api, lib = _lib()
    msg = _refused(lib, api, GRID, 4, 4, 0, 4, np.eye(4))
    assert "nres = 4" in msg and "nterms = 4" in msg and "nterms == 0" in msg
    msg = _refused(lib, api, GRID, 4, 0, 2, 4, np.eye(4))
    assert "nsums = 2" in msg and "nsums == 0" in msg
    assert "precision == NULL" in _refused(lib, api, GRID, 4, 0, 0, 4, None)
    msg = _refused(lib, api, GRID, 4, 4, 9, 0, None)
    assert "nsums = 9" in msg and "nsums <= 8" in msg
    msg = _refused(lib, api, GRID, 4, 0, 0, 0, None)
    assert "nterms = 0" in msg and "nterms >= 1" in msg
    assert "nres = 1025" in _refused(lib, api, GRID, 4, 0, 0, 1025, np.eye(4))
    # ... and through the Python door: RuntimeError with the same text
    with pytest.raises(RuntimeError) as e:
        _create_shared(api, GRID, options=("-DNSH=4", "-DNPT=4"), data=_grid_data(4, 4), nterms=4, shared=513)
    assert "1 <= nshared <= 512" in str(e.value)


def test_a_source_that_lacks_one_of_its_functions_is_refused_by_name():
    api, lib = _lib()
    cut = GRID.index("static __device__ double grid_model")
    msg = _refused(lib, api, "#pragma clang fp contract(off)\n" + GRID[cut:], 4, 4, 0, 0, None)
    assert "pchip_shared_value" in msg
    # only the overloads without `shared` (the terms form's own text, and pchip_shared_value beside it): the one with it is missing, by name
    only_old = LINE_TERMS + GRID[:cut]
    msg = _refused(lib, api, only_old, 4, 4, 0, 0, None)
    assert "pchip_logl_term" in msg and "pchip_shared_value" not in msg
    h = api.source_create(only_old, options=("-DNSH=4", "-DNPT=4"), data=_grid_data(4, 4), nterms=4)       # (it is a terms source as it stands)
    lib.pchip_source_destroy(h)
    # the quadratic form lacks its residual, the sums form its finish
    no_res = GRID.replace("double pchip_residual(", "double some_residual(")
    assert "pchip_residual" in _refused(lib, api, no_res, 4, 0, 0, 4, np.eye(4))
    no_fin = GRID.replace("double pchip_logl_finish_sums(", "double some_finish(")
    assert "pchip_logl_finish_sums" in _refused(lib, api, no_fin, 4, 4, 3, 0, None)
    with pytest.raises(RuntimeError) as e:
        _create_shared(api, GRID, options=("-DNSH=4", "-DNPT=4"), data=_grid_data(4, 4), nterms=4, shared=4, prior=True)
    assert "pchip_prior_param" in str(e.value)


def test_a_syntax_error_in_shared_value_names_the_users_line():
    api, _ = _lib()
    bad = ("\n\n__device__ double pchip_shared_value(const double *t, int D, const double *d, long m, long k)\n{ return t[0] +; }\n"
           "__device__ double pchip_logl_term(const double *t, const double *s, int D, const double *d, long m, long i) { return s[0]; }\n"
           "__device__ double pchip_logl_finish(double s, const double *t, const double *sh, double *p, int D, int n, const double *d, long m) { return s; }\n")
    with pytest.raises(RuntimeError) as e:
        _create_shared(api, bad, nterms=4, shared=2)
    assert "pchip_user_source.h:4" in str(e.value) and "error" in str(e.value)


def _names():
    """what the launchers can choose for a terms handle, the in-step kernel of a source and the maximiser's"""
    return _terms_variants() + ["k_slice_many<1, 1, false, 1, 8, 0>", "k_slice_many<1, 1, false, 1, 0, 0, 1>", "k_maximise<1>"]


def _compile_check(lib, h, names):
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(names).encode(), log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")


def _create_form(api, form, nsh, n, text=GRID, prior=False, D=3, extra=()):
    data = _grid_data(nsh, n)
    kw = {"terms": dict(nterms=n), "sums": dict(nterms=n, nsums=3), "quad": dict(residuals=n, precision=_precision("ar1", n))}[form]
    return _create_shared(api, text, options=_options(form, nsh, n, D) + tuple(extra), data=data, shared=nsh, prior=prior, **kw)


@pytest.mark.parametrize("form", ["terms", "sums", "quad"])
def test_every_variant_compiles_for_gfx950_from_a_shared_handle(form):
    api, lib = _lib()
    h = _create_form(api, form, 130, 300, extra=("-DPCHIP_TEST_OPTION=1",))
    _compile_check(lib, h, _names())
    lib.pchip_source_destroy(h)


def test_every_variant_compiles_at_the_limits():
    """512 shared values beside 1024 residuals: 8 KB and 16 KB of the front block"""
    api, lib = _lib()
    h = _create_form(api, "quad", 512, 1024)
    _compile_check(lib, h, _names())
    lib.pchip_source_destroy(h)
    h = _create_form(api, "terms", 512, 300)
    _compile_check(lib, h, ["k_generate_live<1>", "k_source_eval<1>", "k_slice<1, 1, false>", "k_slice<1, 1, false, 1, 8>", "k_slice<2, 4, false, 1, 0, 0, 1>", "k_maximise<1>"])
    lib.pchip_source_destroy(h)


def test_a_text_may_carry_the_overloads_without_shared_as_well():
    api, lib = _lib()
    h = _create_form(api, "terms", 5, 9, text=GRID + OLD_SIGNATURES)
    _compile_check(lib, h, ["k_source_eval<1>", "k_slice<1, 1, false>"])
    lib.pchip_source_destroy(h)


def test_the_other_forms_still_compile_beside_shared_handles_and_the_text_is_five_files():
    api, lib = _lib()
    seen, i = [], 0
    while True:
        name = C.c_char_p()
        if lib.pchip_rtc_embedded_source(i, C.byref(name)) is None:
            break
        seen.append(name.value.decode())
        i += 1
    assert sorted(seen) == sorted(["pc_dev.h", "pc_state.h", "pc_seed.h", "pc_sample.hip", "pc_slice_body.inc"])
    shared = [_create_form(api, form, 16, 16) for form in ("terms", "sums", "quad")]
    hq = api.source_create(QUAD, options=("-DNRES=16",), data=_quad_line_data(16), residuals=16, precision=_precision("rand", 16))
    hs = api.source_create(EIGHT, data=_eight_data(16), nterms=16, nsums=8)
    ht = api.source_create(LINE_TERMS, nterms=16)
    hp = api.source_create(line_replay(LINE_TERMS), options=("-DNTERMS=16",))
    names = ["k_generate_live<1>", "k_slice<1, 1, false>", "k_slice<1, 1, true>", "k_slice<1, 1, false, 1, 8>", "k_slice<2, 4, false>",
             "k_slice_many<1, 1, false, 1, 8, 0>", "k_slice<1, 1, false, 1, 0, 0, 1>", "k_source_eval<1>"]
    for h in (ht, hp, hs, hq):
        _compile_check(lib, h, names)
        lib.pchip_source_destroy(h)
    for h in shared:
        lib.pchip_source_destroy(h)


def test_user_macros_do_not_reach_the_library_kernels():
    api, lib = _lib()
    src = "#define D 3\n#define nr 7\n#define shared sh_\n#define N 5\n" + GRID.replace("theta[2] * g * g;", "theta[2] * g * g * (double)S;")
    assert src.count("(double)S") == 1
    for form in ("terms", "quad"):
        h = _create_form(api, form, 70, 70, text=src, extra=("-DS=1",))
        _compile_check(lib, h, ["k_slice<1, 2, false>", "k_slice<1, 1, false, 1, 8>", "k_source_eval<1>"])
        lib.pchip_source_destroy(h)


@pytest.mark.parametrize("nsh", [1, 2, 65])
def test_the_host_replays_shared_values_are_the_definition(tmp_path, nsh):
    """the yardstick of the GPU tests, checked where no GPU is: sh[k] = (a + b g_k) + (c g_k) g_k in numpy, bit for bit; the derived parameters
    are the last and the first of them and the sum; the sum is the terms in the defined order"""
    _lib()[1].pchip_source_create_shared          # (the file is about that door: without it nothing here passes)
    n = 70
    block, th = _grid_data(nsh, n), _box_points(8, nsh)
    hl = _host_replay(tmp_path, "terms", nsh, n, f"def{nsh}")
    sh, m = _model(th, block, nsh, n)
    for p in range(th.shape[0]):
        got = np.empty(nsh)
        hl.host_shared(th[p].ctypes.data_as(C.c_void_p), 3, block.ctypes.data_as(C.c_void_p), C.c_long(block.size), got.ctypes.data_as(C.c_void_p))
        assert np.array_equal(got, sh[p])
    lh, ph = _host_eval(hl, th, 3, block)
    z = (block[nsh + n:][None, :] - m) / 0.05
    assert np.array_equal(ph[:, 1], sh[:, -1]) and np.array_equal(ph[:, 2], sh[:, 0])
    assert np.array_equal(ph[:, 0], _tree64(_strided_partials(z * z))) and np.array_equal(lh, -ph[:, 0] / 2.0)


# ---------------------------------------------------------------------------------------------------------------------------- GPU
_HANDLES = {}


def _handle(key, make):
    """one handle per form, shape and text for the whole module: each of its kernel variants compiles once"""
    if key not in _HANDLES:
        _HANDLES[key] = make()
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _destroy_handles():
    yield
    api, lib = _lib()
    lib.polychord_hip_set_source(0)
    for h in _HANDLES.values():
        if hasattr(h, "close"):
            h.close()
        else:
            lib.pchip_source_destroy(h)
    _HANDLES.clear()


GRID_PRIOR = r"""
__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata)
{
    return i == 0 ? 1.0 + cube[0] : (i < 3 ? -0.4 + 0.8 * cube[i] : cube[i]);
}
"""


def _replay_block(form, nsh, n):
    data = _grid_data(nsh, n)
    return np.concatenate([data, np.ravel(_precision("ar1", n))]) if form == "quad" else data


def _pair(api, form, nsh, n, prior=False, D=3):
    """(shared handle, its replay as a plain source), made once"""
    extra = GRID_PRIOR if prior else ""
    hs = _handle((form, nsh, n, prior, D, "shared"), lambda: _create_form(api, form, nsh, n, text=GRID + extra, prior=prior, D=D))
    hp = _handle((form, nsh, n, prior, D, "replay"), lambda: api.source_create(replay_of(form) + extra, options=_options(form, nsh, n, D),
                                                                               data=_replay_block(form, nsh, n), prior=prior))
    return hs, hp


ORDER_SHAPES = [("terms", nsh, n) for nsh in (1, 2, 63, 64, 65, 130) for n in (1, 65, 257)] + [("sums", 65, 130), ("quad", 65, 5), ("quad", 65, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,nsh,n", ORDER_SHAPES)
def test_the_order_bit_for_bit(engine, tmp_path, form, nsh, n):
    """pchip_source_eval at eight points inside the box: the shared handle is the host replay and the device build of the replay, logL and
    all three derived parameters.  nshared: one value, under, at and over a wavefront, three strides with an odd count (130)."""
    api = engine
    hs, hp = _pair(api, form, nsh, n)
    th = _box_points(8, 7 * nsh + n)
    ls, ps = api.source_eval(hs, th, 3)
    lp, pp = api.source_eval(hp, th, 3)
    lh, ph = _host_eval(_host_replay(tmp_path, form, nsh, n, f"{form}{nsh}_{n}"), th, 3, _replay_block(form, nsh, n))
    print(f"{form} nshared {nsh} n {n}: device != host replay at {int((ls != lh).sum())} of 8 (derived {int((ps != ph).any(axis=1).sum())}), "
          f"!= device replay at {int((ls != lp).sum())} (derived {int((ps != pp).any(axis=1).sum())})")
    assert np.all(np.isfinite(ps)) and np.all(np.isfinite(ls))
    assert np.array_equal(ps, ph) and np.array_equal(ls, lh)
    assert np.array_equal(ps, pp) and np.array_equal(ls, lp)
    sh, m = _model(th, _grid_data(nsh, n), nsh, n)
    assert np.array_equal(ps[:, 1], sh[:, -1]) and np.array_equal(ps[:, 2], sh[:, 0])
    if form == "terms":       # ... and the definition itself, in numpy
        z = (_grid_data(nsh, n)[nsh + n:][None, :] - m) / 0.05
        assert np.array_equal(ps[:, 0], _tree64(_strided_partials(z * z)))


def _runs(api, hs, hp, D, nDer, lo=None, hi=None, prior_table=None, prior_source=False, seed=7, **kw):
    out = []
    for h in (hs, hp):
        s = _settings(api, D, nDer, seed=seed, **kw)
        L, P, k1 = api.make_problem("source", D, nDer, source=h, lo=lo, hi=hi, prior_table=prior_table, prior_source=prior_source)
        out.append(api.run(s, L, P))
    return out


def _box(D):
    return dict(lo=LO + [0.0] * (D - 3), hi=HI + [1.0] * (D - 3))


KW = dict(nlive=100, num_repeats=6, batch=20)           # (RUN_SHAPES["line256"] of tests/test_source_terms.py)
TABLE = [("gaussian", [1.5, 0.2]), ("gaussian", [0.0, 0.2]), ("gaussian", [0.0, 0.2])]      # (no box: the PT = 1 kernel variants)
RUN_SHAPES = {
    "no_derived": dict(form="terms", nDer=0),
    "derived_in_the_loop": dict(form="terms", nDer=3),
    "prior_table": dict(form="terms", nDer=3, prior_table=TABLE),
    "source_prior": dict(form="terms", nDer=3, prior=True),
    "sums": dict(form="sums", nDer=3),
    "quad": dict(form="quad", nDer=3, n=65),
    # theta spans two registers a lane (the first three coordinates are the model's, the others free): the rows of 20 babies would fit the
    # LDS budget of the end-of-chain pass -- a shared handle writes its derived parameters in the loop all the same
    "two_registers_a_lane": dict(form="terms", nDer=3, D=70, kw=dict(nlive=100, num_repeats=20, batch=20, max_ndead=400)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(RUN_SHAPES))
def test_a_shared_run_is_the_replays_run(engine, shape):
    """counters, logZ, dead and live rows with their derived columns, bit for bit.  With derived parameters a shared handle takes the path
    that writes them inside the slice loop (pc_slice_phi_lds is 0 for it: the end-of-chain pass has lane = baby and no block per lane);
    a result does not say which path wrote them, so the check is the rows' -- finish's own values, of the block filled again."""
    api = engine
    c = RUN_SHAPES[shape]
    form, D, nDer, nsh, n = c["form"], c.get("D", 3), c["nDer"], 65, c.get("n", 130)
    prior = bool(c.get("prior"))
    hs, hp = _pair(api, form, nsh, n, prior=prior, D=D)
    box = {} if (prior or c.get("prior_table")) else _box(D)
    t, p = _runs(api, hs, hp, D, nDer, prior_table=c.get("prior_table"), prior_source=prior, **box, **c.get("kw", KW))
    _assert_same_run(t, p)
    assert (t["path"]["device_prior"] > 0) == bool(prior or c.get("prior_table")), t["path"]
    if nDer == 3:
        dd = t["dead"]
        ok = dd[:, -1] > -1e29
        assert ok.sum() > 50
        sh, _ = _model(dd[ok, D:D + 3], _grid_data(nsh, n), nsh, n)
        assert np.array_equal(dd[ok, 2 * D + 1], sh[:, -1]) and np.array_equal(dd[ok, 2 * D + 2], sh[:, 0])
        if form != "sums":
            assert np.array_equal(dd[ok, -1], -dd[ok, 2 * D] / 2.0)


@pytest.mark.gpu
def test_shared_runs_in_step_are_their_solo_runs(engine):
    api = engine
    from polychordlite_amd import repeats
    hs, _ = _pair(api, "terms", 65, 130)
    L, P, keep = api.make_problem("source", 3, 3, source=hs, lo=LO, hi=HI)
    seeds = [21, 22, 23]
    merged, runs = repeats.run_in_step(_settings(api, 3, 3, **KW), L, P, seeds, max_in_flight=4)
    assert len(runs) == 3
    for seed, r in zip(seeds, runs):
        solo = api.run(_settings(api, 3, 3, seed=seed, **KW), L, P)
        for k in ("ndead", "nlike", "niter"):
            assert r[k] == solo[k], (seed, k, r[k], solo[k])
        assert r["ndead"] > 0 and r["logZ"] == solo["logZ"] and np.array_equal(r["dead"], solo["dead"]), seed
        assert r["path"]["slice_step"] > 0 and r["path"]["source_terms"] > 0, r["path"]


@pytest.mark.gpu
def test_the_device_maximiser_on_a_shared_handle_is_the_replays(engine):
    api = engine
    hs, hp = _pair(api, "terms", 65, 130)
    s = _settings(api, 3, 3, seed=11, do_clustering=0, **KW)
    out = []
    for h in (hs, hp):
        L, Pr, keep = api.make_problem("source", 3, 3, source=h, lo=LO, hi=HI)
        g = api.run(s, L, Pr)
        out.append(api.maximise_device(s, L, Pr, g))
    a, b = out
    assert a["status"] == [0, 0] and a["niter"] == b["niter"] and a["neval"] == b["neval"] and min(a["niter"]) > 0
    for k in ("max_logl", "max_post", "logl_at_post", "logl_mean"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
    for k in ("max_point", "post_point", "mean_point"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k


@pytest.mark.gpu
def test_a_door_run_with_a_shared_source_is_pchip_run(engine, tmp_path, capfd):
    """pypolychord.run of Source(..., shared=) under UniformPrior is the run pchip_run makes by the kernels a run with hooks takes
    (settings.ablate = 2 | 4; tests/test_source_doors.py explains the two modes); the header names the shared values"""
    from tests.test_source_doors import _door, _settings as _door_settings, HOOKS_MODES
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    api = engine
    nsh, n = 65, 130
    src = _handle(("door", nsh, n), lambda: dl.Source(GRID, data=_grid_data(nsh, n), nterms=n, shared=nsh, nDerived=3, options=_options("terms", nsh, n)))
    capfd.readouterr()
    got = _door(tmp_path, "s", src, 3, 3, dl.UniformPrior(LO, HI), feedback=1)
    out = capfd.readouterr().out
    assert f"terms form, {n} terms, {nsh} shared values" in out
    L, P, keep = api.make_problem("source", 3, 3, source=src.handle, lo=LO, hi=HI)
    g = api.run(_door_settings(api, 3, 3, ablate=HOOKS_MODES), L, P)
    dead, logw, logZ, logZerr, nlive_left = got[-1]
    assert nlive_left == 0 and g["path"]["source_terms"] > 0 and g["ndead"] > 0
    assert logZ == g["logZ"] and logZerr == g["logZerr"]
    assert dead.shape == (g["ndead"], g["dead"].shape[1] - 3) and np.array_equal(dead, g["dead"][:, 3:])
