"""Terms-form device sources with SEVERAL SUMS per evaluation (pchip_source_create_sums): one call of pchip_logl_terms per (point, i) writes
the i-th term of every sum, pchip_logl_finish_sums gets the finished sums; an accepted point keeps all of them
(polychordlite_amd/csrc/pc_sample.hip and pc_slice_body.inc, PCHIP_USER_SUMS / PCHIP_SRC_NSUMS).

Two fixture sources, written with #pragma clang fp contract(off) and + - * / only, so that the host build gives the device's bits:
  LORENTZ   a Lorentzian line on a flat baseline, amplitude and baseline profiled out: the three sums  sum m, sum m^2, sum d m
  EIGHT     eight different functions of (theta, datum) of visibly different magnitude: a sum in the wrong slot cannot pass
Each has its REPLAY as a plain source: the text itself followed by one wrapper (-DNTERMS=n -DNSUMS=k) that forms the 64 strided partials of
every sum serially, adds each in the balanced tree of the defined order and applies the same finish.

CPU: the surface, the refusals, every variant a launcher can choose compiles for gfx950 from a three-sum handle; the host replay against numpy.
GPU: the order of every sum bit for bit against the host replay and the device build of the replay; nsums does not change a sum; a sums run
is the replay's run (sums in LDS at the chain's end, phi in the loop, and the shape the sums' block pushes from the one to the other); runs
in step; the device maximiser."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.test_source_terms import _terms_variants, _tree64, _strided_partials, _blocked_partials, _assert_same_run

NOISE = 0.05

# data = x[n] | d[n] | sum d, sum d^2, n  (a structure of arrays: lane-consecutive i reads consecutive doubles).  theta = (centre, width).
# The model is A m_i + B with m_i = 1 / (1 + ((x_i - centre) / width)^2); A and B minimise chi^2 in closed form (the 2 x 2 normal equations),
# and chi^2 at that minimum is  sum d^2 - A sum d m - B sum d.  Derived: the three sums, A, B.
LORENTZ = r"""
#pragma clang fp contract(off)
__device__ void pchip_logl_terms(const double *theta, int nDims, const double *data, long ndata, long i, double *t)
{
    const long n = (ndata - 3) / 2;
    const double z = (data[i] - theta[0]) / theta[1];
    const double m = 1.0 / (1.0 + z * z);
    t[0] = m;
    t[1] = m * m;
    t[2] = data[n + i] * m;
}
__device__ double pchip_logl_finish_sums(const double *sums, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    const double Sd = data[ndata - 3], Sdd = data[ndata - 2], n = data[ndata - 1];
    const double Sm = sums[0], Smm = sums[1], Sdm = sums[2];
    const double det = Smm * n - Sm * Sm;
    const double A = (Sdm * n - Sm * Sd) / det;
    const double B = (Smm * Sd - Sm * Sdm) / det;
    const double chi2 = (Sdd - A * Sdm - B * Sd) / 0.0025;
    if (nDerived > 0) phi[0] = Sm;
    if (nDerived > 1) phi[1] = Smm;
    if (nDerived > 2) phi[2] = Sdm;
    if (nDerived > 3) phi[3] = A;
    if (nDerived > 4) phi[4] = B;
    for (int e = 5; e < nDerived; ++e) phi[e] = 0.0;
    return -chi2 / 2.0;
}
"""

# the box of the Lorentzian's prior as the handle's own prior (with_prior)
LORENTZ_PRIOR = r"""
__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata)
{
    return i == 0 ? -1.0 + 2.0 * cube[0] : 0.05 + 0.95 * cube[1];
}
"""
LORENTZ_LO, LORENTZ_HI = [-1.0, 0.05], [1.0, 1.0]

# the same m^2 as ONE sum: in the existing form, and in the new form with nsums = 1
LORENTZ_M2_OLD = r"""
#pragma clang fp contract(off)
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{
    const double z = (data[i] - theta[0]) / theta[1];
    const double m = 1.0 / (1.0 + z * z);
    return m * m;
}
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sum;
    return -sum;
}
"""
LORENTZ_M2_NEW = r"""
#pragma clang fp contract(off)
__device__ void pchip_logl_terms(const double *theta, int nDims, const double *data, long ndata, long i, double *t)
{
    const double z = (data[i] - theta[0]) / theta[1];
    const double m = 1.0 / (1.0 + z * z);
    t[0] = m * m;
}
__device__ double pchip_logl_finish_sums(const double *sums, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sums[0];
    return -sums[0];
}
"""

# eight sums of magnitudes 1, 1e3, 1e-3, 1e6, 1e-6, 1e9, 1e-9, 1e12.  With data (the evaluation tests): u = x_i - theta[0], v = x_i theta[1].
# -DEIGHT_THETA (the 70-dimensional runs, nterms = nDims, no data): u = (theta[i] - 0.5) / 0.1, v = theta[i] -- sum 0 is the Gaussian's
# exponent, and every other sum weighs in on logL with a weight of its own.  Derived: the sums, in order.
EIGHT = r"""
#pragma clang fp contract(off)
__device__ void pchip_logl_terms(const double *theta, int nDims, const double *data, long ndata, long i, double *t)
{
#ifdef EIGHT_THETA
    const double u = (theta[i] - 0.5) / 0.1, v = theta[i];
#else
    const double u = data[i] - theta[0], v = data[i] * theta[1];
#endif
    t[0] = u * u;
    t[1] = 1.0e3 * (v + 2.0);
    t[2] = 1.0e-3 * (u * v);
    t[3] = 1.0e6 / (1.0 + u * u);
    t[4] = 1.0e-6 * (u + v);
    t[5] = 1.0e9 * (v * v);
    t[6] = 1.0e-9 * (u / (2.0 + v));
    t[7] = 1.0e12 * (u - v);
}
__device__ double pchip_logl_finish_sums(const double *sums, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sums[0];
    if (nDerived > 1) phi[1] = sums[1];
    if (nDerived > 2) phi[2] = sums[2];
    if (nDerived > 3) phi[3] = sums[3];
    if (nDerived > 4) phi[4] = sums[4];
    if (nDerived > 5) phi[5] = sums[5];
    if (nDerived > 6) phi[6] = sums[6];
    if (nDerived > 7) phi[7] = sums[7];
    for (int e = 8; e < nDerived; ++e) phi[e] = 0.0;
    const double w = 2.0 * (sums[1] / 1.0e3) + 3.0 * (sums[2] / 1.0e-3) + 5.0 * (sums[3] / 1.0e6) + 7.0 * (sums[4] / 1.0e-6)
                   + 11.0 * (sums[5] / 1.0e9) + 13.0 * (sums[6] / 1.0e-9) + 17.0 * (sums[7] / 1.0e12);
    return -sums[0] / 2.0 + 1.0e-3 * w / (1.0 + w * w * 1.0e-6);
}
"""

# the defined order of every sum, serially: lane l adds its terms i = l, l + 64, ... to 0.0; the 64 partials of sum k in a balanced pairwise
# tree over the lanes in lane order within rows of sixteen, then (r0 + r1) + (r2 + r3).  REPLAY_WRAPPER of test_source_terms with an inner k.
REPLAY_WRAPPER = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s[64][NSUMS];
    for (int l = 0; l < 64; ++l) {
        double a[NSUMS];
        for (int k = 0; k < NSUMS; ++k) a[k] = 0.0;
        for (long i = l; i < NTERMS; i += 64) {
            double t[NSUMS];
            pchip_logl_terms(theta, nDims, data, ndata, i, t);
            for (int k = 0; k < NSUMS; ++k) a[k] = a[k] + t[k];
        }
        for (int k = 0; k < NSUMS; ++k) s[l][k] = a[k];
    }
    double f[NSUMS];
    for (int k = 0; k < NSUMS; ++k) {
        for (int w = 1; w < 16; w *= 2)
            for (int l = 0; l < 64; l += 2 * w) s[l][k] = s[l][k] + s[l + w][k];
        f[k] = (s[0][k] + s[16][k]) + (s[32][k] + s[48][k]);
    }
    return pchip_logl_finish_sums(f, theta, phi, nDims, nDerived, data, ndata);
}
"""

HOST_WRAPPER = r"""
extern "C" void host_eval(const double *t, long n, int D, int nDer, const double *d, long nd, double *logL, double *phi)
{ double scratch[32]; for (long p = 0; p < n; ++p) logL[p] = pchip_loglikelihood(t + p * D, nDer > 0 ? phi + p * nDer : scratch, D, nDer, d, nd); }
"""

TEXTS = {"lorentz": (LORENTZ, 3), "eight": (EIGHT, 8), "m2new": (LORENTZ_M2_NEW, 1)}


def replay_of(text):
    return text + REPLAY_WRAPPER


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _create_sums(api, text, **kw):
    """source_create with nsums: the door this file is about (a library without the feature fails here, at the missing symbol)"""
    assert hasattr(api.load(), "pchip_source_create_sums"), "the library does not export pchip_source_create_sums"
    return api.source_create(text, **kw)


def _settings(api, D, nDer, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _lorentz_data(n, seed=3):
    """x = uniform(-1, 1), d = 0.7 m(0.2, 0.3) + 0.1 + N(0, 0.05); the block x | d | sum d, sum d^2, n"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n)
    m = 1.0 / (1.0 + ((x - 0.2) / 0.3) ** 2)
    d = 0.7 * m + 0.1 + rng.normal(0.0, NOISE, n)
    return np.concatenate([x, d, [d.sum(), (d * d).sum(), float(n)]])


def _eight_data(n, seed=5):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def _lorentz_terms(th, data):
    """[npts][nterms][3]: the terms as the source forms them, operation for operation"""
    n = (data.size - 3) // 2
    x, d = data[:n], data[n:2 * n]
    z = (x[None, :] - th[:, 0:1]) / th[:, 1:2]
    m = 1.0 / (1.0 + z * z)
    return np.stack([m, m * m, d[None, :] * m], axis=2)


def _eight_terms(th, data):
    x = data
    u, v = x[None, :] - th[:, 0:1], x[None, :] * th[:, 1:2]
    return np.stack([u * u, 1.0e3 * (v + 2.0), 1.0e-3 * (u * v), 1.0e6 / (1.0 + u * u), 1.0e-6 * (u + v), 1.0e9 * (v * v),
                     1.0e-9 * (u / (2.0 + v)), 1.0e12 * (u - v)], axis=2)


def _lorentz_numpy(th, data):
    """logL and the five derived parameters of the Lorentzian from numpy's own sums (any order): the formula, not the bits"""
    n = (data.size - 3) // 2
    d = data[n:2 * n]
    t = _lorentz_terms(th, data)
    Sm, Smm, Sdm = t[:, :, 0].sum(axis=1), t[:, :, 1].sum(axis=1), t[:, :, 2].sum(axis=1)
    Sd, Sdd = d.sum(), (d * d).sum()
    det = Smm * n - Sm * Sm
    A, B = (Sdm * n - Sm * Sd) / det, (Smm * Sd - Sm * Sdm) / det
    return -((Sdd - A * Sdm - B * Sd) / NOISE ** 2) / 2.0, np.stack([Sm, Smm, Sdm, A, B], axis=1)


def _host_replay(tmp_path, text, nsums, nterms, name):
    cpp = tmp_path / f"{name}.cpp"
    so = tmp_path / f"lib{name}.so"
    cpp.write_text(replay_of(text) + HOST_WRAPPER)
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-D__device__=", f"-DNTERMS={nterms}", f"-DNSUMS={nsums}",
                           "-x", "c++", str(cpp), "-o", str(so)])
    return C.CDLL(str(so))


def _host_eval(hl, th, nDer, data):
    n, D = th.shape
    logL, phi = np.empty(n), np.empty((n, nDer))
    hl.host_eval(th.ctypes.data_as(C.c_void_p), C.c_long(n), D, nDer, data.ctypes.data_as(C.c_void_p), C.c_long(data.size),
                 logL.ctypes.data_as(C.c_void_p), phi.ctypes.data_as(C.c_void_p))
    return logL, phi


def _box_points(npts, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.uniform(-1.0, 1.0, npts), rng.uniform(0.05, 1.0, npts)], axis=1))


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_the_symbol_is_exported_and_the_abi_is_still_9():
    api, lib = _lib()
    assert hasattr(lib, "pchip_source_create_sums")
    assert lib.pchip_abi_version() == 9
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "polychord_hip.h")).read()
    assert "#define PCHIP_SOURCE_MAX_SUMS 8" in hdr and "int  pchip_source_create_sums(" in hdr
    assert "pchip_logl_terms" in hdr and "pchip_logl_finish_sums" in hdr


@pytest.mark.parametrize("nsums", [0, 9, -1])
def test_nsums_out_of_range_is_refused_with_the_range(nsums):
    api, _ = _lib()
    with pytest.raises(RuntimeError) as e:
        _create_sums(api, LORENTZ, nterms=8, nsums=nsums)
    assert "nsums" in str(e.value) and "1 <= nsums <= 8" in str(e.value)


def test_no_terms_is_refused_with_the_range():
    api, _ = _lib()
    with pytest.raises(RuntimeError) as e:
        _create_sums(api, LORENTZ, nterms=0, nsums=3)
    assert "nterms" in str(e.value) and ">= 1" in str(e.value)


def test_a_source_that_lacks_one_of_its_functions_is_refused_by_name():
    api, _ = _lib()
    cut = LORENTZ.index("__device__ double pchip_logl_finish_sums")
    with pytest.raises(RuntimeError) as e:
        _create_sums(api, "#pragma clang fp contract(off)\n" + LORENTZ[cut:], nterms=8, nsums=3)
    assert "pchip_logl_terms" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        _create_sums(api, LORENTZ[:cut], nterms=8, nsums=3)
    assert "pchip_logl_finish_sums" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        _create_sums(api, LORENTZ, nterms=8, nsums=3, prior=True)
    assert "pchip_prior_param" in str(e.value)
    h = _create_sums(api, LORENTZ + LORENTZ_PRIOR, nterms=8, nsums=3, prior=True)
    api.load().pchip_source_destroy(h)


def test_a_syntax_error_names_the_users_line():
    api, _ = _lib()
    bad = ("\n\n__device__ void pchip_logl_terms(const double *t, int D, const double *d, long m, long i, double *o)\n{ o[0] = t[0] +; }\n"
           "__device__ double pchip_logl_finish_sums(const double *s, const double *t, double *p, int D, int n, const double *d, long m) { return s[0]; }\n")
    with pytest.raises(RuntimeError) as e:
        _create_sums(api, bad, nterms=4, nsums=2)
    assert "pchip_user_source.h:4" in str(e.value) and "error" in str(e.value)


def test_every_variant_compiles_for_gfx950_from_a_three_sum_handle():
    """what the launchers can choose for a terms handle, the in-step kernel of a source and the maximiser's"""
    api, lib = _lib()
    h = _create_sums(api, LORENTZ, options=("-DPCHIP_TEST_OPTION=1",), data=_lorentz_data(300), nterms=300, nsums=3)
    names = _terms_variants() + ["k_slice_many<1, 1, false, 1, 8, 0>", "k_maximise<1>", "k_max_rank<1>"]
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(names).encode(), log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_the_other_forms_still_compile_beside_a_sums_handle_and_the_text_is_five_files():
    api, lib = _lib()
    from tests.test_source_terms import LINE_TERMS, replay_of as line_replay
    seen, i = [], 0
    while True:
        name = C.c_char_p()
        if lib.pchip_rtc_embedded_source(i, C.byref(name)) is None:
            break
        seen.append(name.value.decode())
        i += 1
    assert sorted(seen) == sorted(["pc_dev.h", "pc_state.h", "pc_seed.h", "pc_sample.hip", "pc_slice_body.inc"])
    hs = _create_sums(api, EIGHT, data=_eight_data(16), nterms=16, nsums=8)
    ht = api.source_create(LINE_TERMS, nterms=16)
    hp = api.source_create(line_replay(LINE_TERMS), options=("-DNTERMS=16",))
    names = ["k_generate_live<1>", "k_slice<1, 1, false>", "k_slice<1, 1, true>", "k_slice<1, 1, false, 1, 8>", "k_slice<2, 4, false>",
             "k_slice_many<1, 1, false, 1, 8, 0>", "k_slice<1, 1, false, 1, 0, 0, 1>", "k_source_eval<1>"]
    log = C.create_string_buffer(1 << 16)
    for h in (ht, hp, hs):
        assert lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(names).encode(), log, len(log), None) == 0, log.value.decode(errors="replace")
        lib.pchip_source_destroy(h)


def test_user_macros_do_not_reach_the_library_kernels():
    api, lib = _lib()
    src = "#define D 3\n#define nr 7\n" + LORENTZ.replace("t[0] = m;", "t[0] = m * (double)S;")
    assert src != "#define D 3\n#define nr 7\n" + LORENTZ
    h = _create_sums(api, src, options=("-DS=1",), nterms=70, nsums=3)
    log = C.create_string_buffer(1 << 16)
    names = b"k_slice<1, 2, false>;k_slice<1, 1, false, 1, 8>;k_source_eval<1>"
    assert lib.pchip_rtc_compile_check(h, b"gfx950", names, log, len(log), None) == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_the_host_replay_of_the_lorentzian_is_the_formula(tmp_path):
    """the yardstick of the GPU tests, checked where no GPU is: the host replay against a numpy evaluation of the same formula, 1e-12 relative"""
    _lib()[0].load().pchip_source_create_sums          # (the file is about that door: without it nothing here passes)
    data = _lorentz_data(257)
    th = _box_points(50, 1)
    lh, ph = _host_eval(_host_replay(tmp_path, LORENTZ, 3, 257, "lor257"), th, 5, data)
    ln, pn = _lorentz_numpy(th, data)
    assert np.all(np.abs(ph - pn) <= 1e-12 * np.abs(pn)), float(np.max(np.abs(ph - pn) / np.abs(pn)))
    assert np.all(np.abs(lh - ln) <= 1e-12 * np.abs(ln)), float(np.max(np.abs(lh - ln) / np.abs(ln)))
    # ... and its three sums are the defined order of the numpy terms, to the bit
    t = _lorentz_terms(th, data)
    for k in range(3):
        assert np.array_equal(ph[:, k], _tree64(_strided_partials(t[:, :, k])))


# ---------------------------------------------------------------------------------------------------------------------------- GPU
_HANDLES = {}


def _handle(api, key, make):
    """one handle per text, data block and form for the whole module: each of its kernel variants compiles once"""
    if key not in _HANDLES:
        _HANDLES[key] = make()
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _destroy_handles():
    yield
    api, lib = _lib()
    for h in _HANDLES.values():
        lib.pchip_source_destroy(h)
    _HANDLES.clear()


def _fixture_data(name, nterms):
    return _lorentz_data(nterms, seed=100 + nterms) if name != "eight" else _eight_data(nterms, seed=100 + nterms)


def _pair(api, name, nterms, data, options=(), prior=False):
    """(sums handle, its replay as a plain source) of a fixture text, made once"""
    text, nsums = TEXTS[name]
    extra = LORENTZ_PRIOR if prior else ""
    hs = _handle(api, (name, nterms, options, prior, "sums"),
                 lambda: _create_sums(api, text + extra, options=options, data=data, nterms=nterms, nsums=nsums, prior=prior))
    hp = _handle(api, (name, nterms, options, prior, "replay"),
                 lambda: api.source_create(replay_of(text) + extra, options=tuple(options) + (f"-DNTERMS={nterms}", f"-DNSUMS={nsums}"), data=data, prior=prior))
    return hs, hp


@pytest.mark.gpu
@pytest.mark.parametrize("nterms", [1, 5, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["lorentz", "eight"])
def test_the_order_of_every_sum(engine, tmp_path, name, nterms):
    api = engine
    text, nsums = TEXTS[name]
    nDer = 5 if name == "lorentz" else 8
    data = _fixture_data(name, nterms)
    th = _box_points(2000, nterms)
    hs, hp = _pair(api, name, nterms, data)
    ls, ps = api.source_eval(hs, th, nDer)
    lp, pp = api.source_eval(hp, th, nDer)
    lh, ph = _host_eval(_host_replay(tmp_path, text, nsums, nterms, f"{name}{nterms}"), th, nDer, data)
    terms = _lorentz_terms(th, data) if name == "lorentz" else _eight_terms(th, data)
    for k in range(nsums):
        t = terms[:, :, k]
        sp = _strided_partials(t)
        serial = np.zeros(2000)
        for l in range(64):
            serial = serial + sp[:, l]
        blocked = _tree64(_blocked_partials(t))
        exact = t.astype(np.longdouble).sum(axis=1)
        bound = (nterms / 64 + 7) * 2.0 ** -53 * np.abs(t).sum(axis=1)
        print(f"{name} nterms {nterms} sum {k}: device != host replay at {int((ps[:, k] != ph[:, k]).sum())} of 2000; numpy tree != device at "
              f"{int((_tree64(sp) != ps[:, k]).sum())}; serial differs at {np.mean(serial != ps[:, k]):.3f}, blocked at {np.mean(blocked != ps[:, k]):.3f}; "
              f"max |sum - long double| / bound {float(np.max(np.abs(ps[:, k].astype(np.longdouble) - exact) / bound)):.3f}")
    # the sums form is the host replay, bit for bit -- every derived parameter and logL -- and the device build of the replay, a plain source
    # (one term: the Lorentzian's normal equations are singular, A, B and logL are 0 / 0 on the host and on the device alike; a NaN's sign
    #  and payload are the machine's, equal_nan compares the rest)
    assert np.array_equal(ps[:, :nsums], ph[:, :nsums]) and np.array_equal(ps[:, :nsums], pp[:, :nsums])
    assert np.array_equal(ps, ph, equal_nan=True) and np.array_equal(ls, lh, equal_nan=True)
    assert np.array_equal(ps, pp, equal_nan=True) and np.array_equal(ls, lp, equal_nan=True)
    if not (name == "lorentz" and nterms == 1):
        assert np.all(np.isfinite(ps)) and np.all(np.isfinite(ls))
    for k in range(nsums):
        t = terms[:, :, k]
        sp = _strided_partials(t)
        if nterms >= 65:        # the inputs can tell the orders apart, for every sum
            serial = np.zeros(2000)
            for l in range(64):
                serial = serial + sp[:, l]
            assert np.mean(serial != ps[:, k]) >= 0.1, k
            assert np.mean(_tree64(_blocked_partials(t)) != ps[:, k]) >= 0.1, k
        exact = t.astype(np.longdouble).sum(axis=1)
        bound = (nterms / 64 + 7) * 2.0 ** -53 * np.abs(t).sum(axis=1)
        assert np.all(np.abs(ps[:, k].astype(np.longdouble) - exact) <= bound), k


@pytest.mark.gpu
def test_nsums_does_not_change_a_sum(engine):
    """sum m^2 from a one-sum handle of the existing form, from a nsums = 1 handle of the new form and from slot 1 of the three-sum handle"""
    api = engine
    nterms = 257
    data = _fixture_data("lorentz", nterms)
    th = _box_points(2000, nterms)
    h3, _ = _pair(api, "lorentz", nterms, data)
    hold = _handle(api, ("m2old", nterms), lambda: api.source_create(LORENTZ_M2_OLD, data=data, nterms=nterms))
    hnew = _handle(api, ("m2new", nterms), lambda: _create_sums(api, LORENTZ_M2_NEW, data=data, nterms=nterms, nsums=1))
    _, p3 = api.source_eval(h3, th, 5)
    lo, po = api.source_eval(hold, th, 1)
    ln, pn = api.source_eval(hnew, th, 1)
    assert np.array_equal(po[:, 0], p3[:, 1]) and np.array_equal(pn[:, 0], p3[:, 1])
    assert np.array_equal(lo, ln) and np.array_equal(lo, -p3[:, 1])


def _runs(api, hs, hp, D, nDer, lo=None, hi=None, prior_table=None, prior_source=False, grades=None, seed=7, **kw):
    out = []
    for h in (hs, hp):
        s = _settings(api, D, nDer, seed=seed, **kw)
        keep = [api.set_grades(s, *grades)] if grades else []
        L, P, k1 = api.make_problem("source", D, nDer, source=h, lo=lo, hi=hi, prior_table=prior_table, prior_source=prior_source)
        out.append(api.run(s, L, P))
    return out


LOR_KW = dict(nlive=100, num_repeats=6, batch=20)
LORENTZ_RUNS = {
    "sums_in_lds": dict(nDer=5, kw=LOR_KW),
    "no_derived": dict(nDer=0, kw=LOR_KW),
    "clustering": dict(nDer=5, kw=dict(LOR_KW, do_clustering=1)),
    "sequential": dict(nDer=5, kw=dict(nlive=60, num_repeats=6, batch=1, sequential_rng=1)),
    "prior_table": dict(nDer=5, kw=LOR_KW, prior_table=[("uniform", [-1.0, 1.0]), ("uniform", [0.05, 1.0])]),
    "source_prior": dict(nDer=5, kw=LOR_KW, prior=True),
    "two_grades": dict(nDer=5, kw=LOR_KW, grades=([1, 1], [2, 4])),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(LORENTZ_RUNS))
def test_a_sums_run_is_the_replays_run(engine, shape):
    """the Lorentzian at 256 terms, nDims 2: row for row and counter for counter the run of its replay as a plain source"""
    api = engine
    c = LORENTZ_RUNS[shape]
    prior = bool(c.get("prior"))
    hs, hp = _pair(api, "lorentz", 256, _lorentz_data(256), prior=prior)
    box = {} if (prior or c.get("prior_table")) else dict(lo=LORENTZ_LO, hi=LORENTZ_HI)
    t, p = _runs(api, hs, hp, 2, c["nDer"], prior_table=c.get("prior_table"), prior_source=prior, grades=c.get("grades"), **box, **c["kw"])
    _assert_same_run(t, p)
    if c["nDer"] == 5:          # the derived parameters are finish's, of the sums the point was accepted with: logL again from the columns
        dd = t["dead"]
        data = _lorentz_data(256)
        Sm, Smm, Sdm, A, B = (dd[:, 4 + e] for e in range(5))
        ok = dd[:, -1] > -1e29
        assert ok.sum() > 100
        assert np.array_equal(dd[ok, -1], (-((data[-2] - A * Sdm - B * data[-3]) / 0.0025) / 2.0)[ok])
        assert np.all(dd[ok, 1 + 2] >= LORENTZ_LO[1]) and np.all(np.abs(dd[ok, 2]) <= 1.0)


# nDims 70 (two coordinates a lane), eight sums, nterms = nDims.  A chain's LDS block, doubles: 70 + nr, then 71 nr for the babies' theta rows
# when 8 (70 + nr) + 16 + 8 * 71 nr + 8 * 8 nr <= 48 KB -- the last term is the sums' own block.  num_repeats 20: all in LDS; 100: the rows
# alone do not fit (phi in the loop); 80: the rows fit (46 656 bytes) and the sums' block is what pushes the chain over (51 776 bytes)
EIGHT_RUNS = {"sums_in_lds": dict(num_repeats=20), "phi_in_the_loop": dict(num_repeats=100, max_ndead=1500),
              "pushed_over_by_the_sums_block": dict(num_repeats=80, max_ndead=1500)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(EIGHT_RUNS))
def test_a_70_dimensional_eight_sum_run_is_the_replays_run(engine, shape):
    api = engine
    nr = EIGHT_RUNS[shape]["num_repeats"]
    rows, sums = 8 * (70 + nr) + 16 + 8 * 71 * nr, 8 * 8 * nr
    assert {"sums_in_lds": rows + sums <= 49152, "phi_in_the_loop": rows > 49152, "pushed_over_by_the_sums_block": rows <= 49152 < rows + sums}[shape]
    hs, hp = _pair(api, "eight", 70, None, options=("-DEIGHT_THETA=1",))
    t, p = _runs(api, hs, hp, 70, 3, nlive=100, batch=20, **EIGHT_RUNS[shape])
    _assert_same_run(t, p)
    dd = t["dead"]
    assert np.array_equal(dd[:, 140], _tree64(_strided_partials(((dd[:, 70:140] - 0.5) / 0.1) ** 2)))     # sum 0 of the row's own theta


@pytest.mark.gpu
def test_sums_runs_in_step_are_their_solo_runs(engine):
    api = engine
    from polychordlite_amd import repeats
    hs, _ = _pair(api, "lorentz", 256, _lorentz_data(256))
    L, P, keep = api.make_problem("source", 2, 5, source=hs, lo=LORENTZ_LO, hi=LORENTZ_HI)
    seeds = [21, 22, 23]
    merged, runs = repeats.run_in_step(_settings(api, 2, 5, **LOR_KW), L, P, seeds, max_in_flight=4)
    assert len(runs) == 3
    for seed, r in zip(seeds, runs):
        solo = api.run(_settings(api, 2, 5, seed=seed, **LOR_KW), L, P)
        for k in ("ndead", "nlike", "niter"):
            assert r[k] == solo[k], (seed, k, r[k], solo[k])
        assert r["ndead"] > 0 and r["logZ"] == solo["logZ"] and np.array_equal(r["dead"], solo["dead"]), seed
        assert r["path"]["slice_step"] > 0 and r["path"]["source_terms"] > 0, r["path"]


@pytest.mark.gpu
def test_the_device_maximiser_on_a_sums_handle_is_the_replays(engine):
    api = engine
    data = _lorentz_data(256)
    hs, hp = _pair(api, "lorentz", 256, data)
    s = _settings(api, 2, 5, seed=11, do_clustering=0, **LOR_KW)
    out = []
    for h in (hs, hp):
        L, P, keep = api.make_problem("source", 2, 5, source=h, lo=LORENTZ_LO, hi=LORENTZ_HI)
        g = api.run(s, L, P)
        out.append(api.maximise_device(s, L, P, g))
    a, b = out
    assert a["status"] == [0, 0] and a["niter"] == b["niter"] and a["neval"] == b["neval"] and min(a["niter"]) > 0
    for k in ("max_logl", "max_post", "logl_at_post", "logl_mean"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
    for k in ("max_point", "post_point", "mean_point"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    # the maximum is the line the data were made with: centre 0.2, width 0.3, amplitude 0.7 on a baseline of 0.1
    assert abs(a["max_point"][0] - 0.2) < 0.02 and abs(a["max_point"][1] - 0.3) < 0.03
    assert abs(a["max_point"][2 + 3] - 0.7) < 0.05 and abs(a["max_point"][2 + 4] - 0.1) < 0.03
