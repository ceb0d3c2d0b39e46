"""The terms form of a device-source likelihood (pchip_source_create_terms): the likelihood is finish(sum of nterms terms), the wavefront
shares the loop over the terms, the derived parameters come from the kept sum (polychordlite_amd/csrc/pc_sample.hip, PCHIP_USER_TERMS).

Every terms text of this file gets its REPLAY for free: the text itself followed by one wrapper (-DNTERMS=n), a plain pchip_loglikelihood
that forms the 64 strided partial sums serially, adds them in the balanced tree of the defined order and applies the same finish.  The
replay compiles for the device as a plain source (the path that existed before) and, with -D__device__=, for the host.

CPU: the surface, the refusals, every variant a launcher can choose for a terms handle compiles for gfx950.
GPU: the order of the sum bit for bit against the host replay (and two wrong orders tell themselves apart on the same inputs); a terms run
is the replay's run, dead points and derived columns included; it walks the oracle within the bounds the plain source meets."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import oracle_api as orc

# the straight-line fit of LINE_SRC (tests/test_device_source.py): data = (x, y) pairs, theta = (slope, intercept), unit noise
LINE_TERMS = r"""
#pragma clang fp contract(off)
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{
    const double r = data[2 * i + 1] - (theta[0] * data[2 * i] + theta[1]);
    return r * r;
}
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = sum;
    if (nDerived > 1) phi[1] = theta[0] + theta[1];
    for (int e = 2; e < nDerived; ++e) phi[e] = 0.0;
    return -sum / 2.0;
}
"""

# the Gaussian of GAUSS_SRC as nDims terms (term i = z_i^2): phi[0] = the sum, phi[e] = e * (theta[0] + theta[nDims - 1])
GAUSS_TERMS = r"""
#pragma clang fp contract(off)
__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i)
{
    const double z = (theta[i] - 0.5) / 0.1;
    return z * z;
}
__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    for (int e = 0; e < nDerived; ++e) phi[e] = (e == 0) ? sum : (theta[0] + theta[nDims - 1]) * (double)e;
    return -sum / 2.0 + 1.3836465597893728 * (double)nDims;
}
"""

# the defined order, serially: lane l adds term(l), term(l + 64), ... to 0.0; the 64 partials in a balanced pairwise tree over the lanes
# in lane order within rows of sixteen, then (r0 + r1) + (r2 + r3)
REPLAY_WRAPPER = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double s[64];
    for (int l = 0; l < 64; ++l) {
        double a = 0.0;
        for (long i = l; i < NTERMS; i += 64) a = a + pchip_logl_term(theta, nDims, data, ndata, i);
        s[l] = a;
    }
    for (int w = 1; w < 16; w *= 2)
        for (int l = 0; l < 64; l += 2 * w) s[l] = s[l] + s[l + w];
    return pchip_logl_finish((s[0] + s[16]) + (s[32] + s[48]), theta, phi, nDims, nDerived, data, ndata);
}
"""

HOST_WRAPPER = r"""
extern "C" double host_logl(const double *t, int D, double *phi, int nDer, void *ctx)
{ const double *d = ((const double **)ctx)[0]; long n = (long)((const double **)ctx)[1]; return pchip_loglikelihood(t, phi, D, nDer, d, n); }
extern "C" void host_eval(const double *t, long n, int D, int nDer, const double *d, long nd, double *logL, double *phi)
{ double scratch[32]; for (long p = 0; p < n; ++p) logL[p] = pchip_loglikelihood(t + p * D, nDer > 0 ? phi + p * nDer : scratch, D, nDer, d, nd); }
"""


def replay_of(terms_text):
    return terms_text + REPLAY_WRAPPER


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _settings(api, D, nDer, **kw):
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _host_replay(tmp_path, terms_text, nterms, name):
    """the replay compiled for the host: host_logl (the oracle's callback) and host_eval (many points)"""
    cpp = tmp_path / f"{name}.cpp"
    so = tmp_path / f"lib{name}.so"
    cpp.write_text(replay_of(terms_text) + HOST_WRAPPER)
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-D__device__=", f"-DNTERMS={nterms}", "-x", "c++",
                           str(cpp), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.host_logl.restype = C.c_double
    return lib


def _line_data(n, seed=3, wide=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n)
    noise = rng.normal(0.0, 1.0, n) * (10.0 ** rng.uniform(-6.0, 6.0, n) if wide else 1.0)
    return np.stack([x, 0.3 * x + 0.6 + noise], axis=1).ravel()


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_terms_symbols_are_exported():
    api, lib = _lib()
    for sym in ("pchip_source_create_terms", "pchip_source_eval"):
        assert hasattr(lib, sym), sym
    assert lib.pchip_abi_version() == 9
    assert api.PATH_NAMES[21] == "source_terms" and api.PATH_NAMES[19] == "source_kernels"


def test_a_terms_source_without_finish_is_refused():
    api, _ = _lib()
    only_term = LINE_TERMS[:LINE_TERMS.index("__device__ double pchip_logl_finish")]
    with pytest.raises(RuntimeError) as e:
        api.source_create(only_term, nterms=8)
    assert "pchip_logl_finish" in str(e.value)


def test_a_terms_source_without_term_is_refused():
    api, _ = _lib()
    only_finish = "#pragma clang fp contract(off)\n" + LINE_TERMS[LINE_TERMS.index("__device__ double pchip_logl_finish"):]
    with pytest.raises(RuntimeError) as e:
        api.source_create(only_finish, nterms=8)
    assert "pchip_logl_term" in str(e.value)


@pytest.mark.parametrize("nterms", [0, -3])
def test_fewer_than_one_term_is_refused(nterms):
    api, _ = _lib()
    with pytest.raises(RuntimeError) as e:
        api.source_create(LINE_TERMS, nterms=nterms)
    assert "nterms" in str(e.value) and ">= 1" in str(e.value)


def test_a_syntax_error_in_a_terms_source_names_the_users_line():
    api, _ = _lib()
    bad = ("\n\n__device__ double pchip_logl_term(const double *t, int D, const double *d, long m, long i)\n{ return t[0] +; }\n"
           "__device__ double pchip_logl_finish(double s, const double *t, double *p, int D, int n, const double *d, long m) { return s; }\n")
    with pytest.raises(RuntimeError) as e:
        api.source_create(bad, nterms=4)
    assert "pchip_user_source.h:4" in str(e.value) and "error" in str(e.value)


def _terms_variants():
    """the kernels the launchers can choose for a terms handle: the list of test_every_general_variant_compiles_for_gfx950 without
    k_slice_many (runs in step refuse a source), with the prior-table variants (PT = 1) and the evaluation kernel"""
    names = [f"k_generate_live<{d}>" for d in (1, 2, 4)] + [f"k_generate_live<{d}, 1>" for d in (1, 2, 4)]
    names += [f"k_source_eval<{d}>" for d in (1, 2, 4)]
    for dpl, nrows in ((1, 1), (1, 2), (1, 4), (2, 4), (4, 4)):
        for gr in ("false", "true"):
            names += [f"k_slice<{dpl}, {nrows}, {gr}>", f"k_slice<{dpl}, {nrows}, {gr}, 1, 0, 0, 1>"]
    for nrows, fw in ((1, 8), (1, 16), (2, 24)):
        names += [f"k_slice<1, {nrows}, false, 1, {fw}>", f"k_slice<1, {nrows}, false, 1, {fw}, 0, 1>"]
    return names


def test_every_terms_variant_compiles_for_gfx950():
    api, lib = _lib()
    h = api.source_create(LINE_TERMS, options=("-DPCHIP_TEST_OPTION=1",), data=_line_data(300), nterms=300)
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(_terms_variants()).encode(), log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_user_macros_of_a_terms_source_do_not_reach_the_library_kernels():
    api, lib = _lib()
    src = "#define D 3\n#define nr 7\n" + LINE_TERMS.replace("theta[1];\n    return r * r", "theta[1] * (double)S;\n    return r * r")
    h = api.source_create(src, options=("-DS=1",), nterms=70)
    log = C.create_string_buffer(1 << 16)
    names = b"k_slice<1, 2, false>;k_slice<1, 1, false, 1, 8>;k_source_eval<1>"
    assert lib.pchip_rtc_compile_check(h, b"gfx950", names, log, len(log), None) == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_a_plain_handle_still_compiles_the_plain_list_and_the_text_is_five_files():
    """the terms code lives INSIDE pc_sample.hip / pc_slice_body.inc, behind the handle's #defines: no sixth embedded file, and a plain
    source next to a terms source in one process compiles what it always did (plus the evaluation kernel)"""
    api, lib = _lib()
    seen, i = [], 0
    while True:
        name = C.c_char_p()
        if lib.pchip_rtc_embedded_source(i, C.byref(name)) is None:
            break
        seen.append(name.value.decode())
        i += 1
    assert sorted(seen) == sorted(["pc_dev.h", "pc_state.h", "pc_seed.h", "pc_sample.hip", "pc_slice_body.inc"])
    ht = api.source_create(LINE_TERMS, nterms=16)
    hp = api.source_create(replay_of(LINE_TERMS), options=("-DNTERMS=16",))
    names = ["k_generate_live<1>", "k_slice<1, 1, false>", "k_slice<1, 1, true>", "k_slice<1, 1, false, 1, 8>", "k_slice<2, 4, false>",
             "k_slice_many<1, 1, false, 1, 8, 0>", "k_slice<1, 1, false, 1, 0, 0, 1>", "k_source_eval<1>"]
    log = C.create_string_buffer(1 << 16)
    assert lib.pchip_rtc_compile_check(hp, b"gfx950", ";".join(names).encode(), log, len(log), None) == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(ht)
    lib.pchip_source_destroy(hp)


def test_the_replay_compiles_for_the_host_and_is_the_sum(tmp_path):
    """the yardstick of the GPU tests, checked where no GPU is: the host replay of the straight line is -chi^2 / 2 to rounding"""
    data = _line_data(300)
    hl = _host_replay(tmp_path, LINE_TERMS, 300, "line300")
    th = np.array([[0.25, 0.5], [-1.0, 1.0]])
    logL, phi = np.empty(2), np.empty((2, 2))
    hl.host_eval(th.ctypes.data_as(C.c_void_p), 2, 2, 2, data.ctypes.data_as(C.c_void_p), C.c_long(data.size),
                 logL.ctypes.data_as(C.c_void_p), phi.ctypes.data_as(C.c_void_p))
    x, y = data[0::2], data[1::2]
    for p in range(2):
        chi2 = float(np.sum((y - (th[p, 0] * x + th[p, 1])) ** 2))
        assert abs(phi[p, 0] - chi2) < 1e-12 * chi2 and logL[p] == -phi[p, 0] / 2.0 and phi[p, 1] == th[p, 0] + th[p, 1]


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _tree64(p):
    """[npts][64] partials -> the balanced pairwise tree of the defined order"""
    s = p.copy()
    for w in (1, 2, 4, 8):
        s[:, 0::2 * w] = s[:, 0::2 * w] + s[:, w::2 * w]
    return (s[:, 0] + s[:, 16]) + (s[:, 32] + s[:, 48])


def _strided_partials(terms):
    npts, n = terms.shape
    pad = np.zeros((npts, -(-n // 64) * 64))
    pad[:, :n] = terms
    p = np.zeros((npts, 64))
    for j in range(pad.shape[1] // 64):
        p = p + pad[:, 64 * j:64 * (j + 1)]          # (a lane without a term adds +0.0 to a sum of squares: the same bits as not adding)
    return p


def _blocked_partials(terms):
    npts, n = terms.shape
    b = -(-n // 64)
    pad = np.zeros((npts, 64 * b))
    pad[:, :n] = terms
    blk = pad.reshape(npts, 64, b)
    p = np.zeros((npts, 64))
    for j in range(b):
        p = p + blk[:, :, j]
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("nterms", [1, 5, 63, 64, 65, 256, 4099])
def test_the_order_of_the_sum(engine, tmp_path, nterms):
    api = engine
    lib = api.load()
    data = _line_data(nterms, seed=100 + nterms, wide=True)
    rng = np.random.default_rng(nterms)
    th = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (2000, 2)))
    ht = api.source_create(LINE_TERMS, data=data, nterms=nterms)
    hp = api.source_create(replay_of(LINE_TERMS), options=(f"-DNTERMS={nterms}",), data=data)
    lt, pt = api.source_eval(ht, th, 2)
    lp, pp = api.source_eval(hp, th, 2)
    hl = _host_replay(tmp_path, LINE_TERMS, nterms, f"line{nterms}")
    lh, ph = np.empty(2000), np.empty((2000, 2))
    hl.host_eval(th.ctypes.data_as(C.c_void_p), 2000, 2, 2, data.ctypes.data_as(C.c_void_p), C.c_long(data.size),
                 lh.ctypes.data_as(C.c_void_p), ph.ctypes.data_as(C.c_void_p))
    x, y = data[0::2], data[1::2]
    r = y[None, :] - (th[:, 0:1] * x[None, :] + th[:, 1:2])
    terms = r * r
    serial = np.zeros(2000)
    sp = _strided_partials(terms)
    for l in range(64):
        serial = serial + sp[:, l]
    blocked = _tree64(_blocked_partials(terms))
    exact = terms.astype(np.longdouble).sum(axis=1)
    bound = (nterms / 64 + 7) * 2.0 ** -53 * terms.sum(axis=1)
    print(f"nterms {nterms}: device != host replay at {int((pt[:, 0] != ph[:, 0]).sum())} of 2000; numpy tree != device at "
          f"{int((_tree64(sp) != pt[:, 0]).sum())}; serial differs at {np.mean(serial != pt[:, 0]):.3f}, blocked at {np.mean(blocked != pt[:, 0]):.3f}; "
          f"max |sum - long double| / bound {float(np.max(np.abs(pt[:, 0].astype(np.longdouble) - exact) / bound)):.3f}")
    # the terms form is the host replay, bit for bit -- sum (phi[0]), logL and the second derived parameter
    assert np.array_equal(pt, ph) and np.array_equal(lt, lh)
    # ... and the device build of the replay (a plain source, the path that existed)
    assert np.array_equal(pt, pp) and np.array_equal(lt, lp)
    # the inputs can tell the orders apart: the two wrong replays differ from the device at a tenth of the points or more
    if nterms >= 65:
        assert np.mean(serial != pt[:, 0]) >= 0.1
        assert np.mean(blocked != pt[:, 0]) >= 0.1
    # a strided serial part of ceil(nterms / 64) adds, then six tree levels
    assert np.all(np.abs(pt[:, 0].astype(np.longdouble) - exact) <= bound)
    lib.pchip_source_destroy(ht)
    lib.pchip_source_destroy(hp)


def _pair_of_runs(api, terms_text, nterms, D, nDer, data=None, prior_table=None, grades=None, seed=7, **kw):
    """the same run with the terms source and with its replay as a plain source"""
    out = []
    for terms in (True, False):
        h = (api.source_create(terms_text, data=data, nterms=nterms) if terms
             else api.source_create(replay_of(terms_text), options=(f"-DNTERMS={nterms}",), data=data))
        s = _settings(api, D, nDer, seed=seed, **kw)
        keep = [api.set_grades(s, *grades)] if grades else []
        L, P, k1 = api.make_problem("source", D, nDer, source=h, prior_table=prior_table)
        out.append(api.run(s, L, P))
        api.load().pchip_source_destroy(h)
    return out


def _assert_same_run(t, p):
    for k in ("ndead", "nlike", "niter", "nbatches"):
        assert t[k] == p[k], (k, t[k], p[k])
    assert t["nlike_grade"] == p["nlike_grade"]
    assert t["logZ"] == p["logZ"]
    assert np.array_equal(t["dead"], p["dead"])          # derived columns included
    assert np.array_equal(t["live"], p["live"])
    assert t["path"]["source_terms"] > 0 and p["path"]["source_terms"] == 0
    assert t["path"]["source_kernels"] > 0 and p["path"]["source_kernels"] > 0
    assert t["path"]["source_terms"] == t["path"]["source_kernels"]
    assert t["ndead"] > 0


RUN_SHAPES = {
    "line256": dict(text="line", nterms=256, D=2, nDer=2, kw=dict(nlive=100, num_repeats=6, batch=20)),
    "line4099_clustering": dict(text="line", nterms=4099, D=2, nDer=2, kw=dict(nlive=100, num_repeats=6, batch=20, do_clustering=1)),
    "line256_table_prior": dict(text="line", nterms=256, D=2, nDer=2, kw=dict(nlive=100, num_repeats=6, batch=20),
                                prior_table=[("gaussian", [0.3, 0.5]), ("gaussian", [0.6, 0.5])]),
    "line256_sequential": dict(text="line", nterms=256, D=2, nDer=2, kw=dict(nlive=60, num_repeats=6, batch=1, sequential_rng=1)),
    "line256_no_derived": dict(text="line", nterms=256, D=2, nDer=0, kw=dict(nlive=100, num_repeats=6, batch=20)),
    "gauss70": dict(text="gauss", nterms=70, D=70, nDer=3, kw=dict(nlive=100, num_repeats=20, batch=20)),
    # (num_repeats x (nDims + 1) doubles do not fit the LDS budget of the end-of-chain pass: the derived parameters are written inside the slice loop)
    "gauss70_phi_in_the_loop": dict(text="gauss", nterms=70, D=70, nDer=3, kw=dict(nlive=100, num_repeats=100, batch=20, max_ndead=1500)),
    "gauss30": dict(text="gauss", nterms=30, D=30, nDer=1, kw=dict(nlive=100, num_repeats=30, batch=20)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(RUN_SHAPES))
def test_a_terms_run_is_the_replays_run(engine, shape):
    c = RUN_SHAPES[shape]
    data = _line_data(c["nterms"]) if c["text"] == "line" else None
    t, p = _pair_of_runs(engine, LINE_TERMS if c["text"] == "line" else GAUSS_TERMS, c["nterms"], c["D"], c["nDer"], data=data,
                         prior_table=c.get("prior_table"), **c["kw"])
    _assert_same_run(t, p)
    if c["nDer"] >= 2 and c["text"] == "line":    # the derived parameters are finish's: the sum and slope + intercept
        D = c["D"]
        assert np.array_equal(t["dead"][:, 2 * D], -2.0 * t["dead"][:, -1])
        assert np.array_equal(t["dead"][:, 2 * D + 1], t["dead"][:, D] + t["dead"][:, D + 1])


def _oracle_run(tmp_path, terms_text, nterms, D, nDer, data, grades=None, seed=5, **kw):
    """the reference walk (tests/oracle_api.py) with the host build of the replay as its callback: _source_vs_oracle's scheme"""
    hl = _host_replay(tmp_path, terms_text, nterms, f"orc{D}_{nterms}")
    d = np.ascontiguousarray(np.zeros(1) if data is None else data, dtype=np.float64)
    ctx = (C.c_void_p * 2)(d.ctypes.data, 0 if data is None else d.size)
    kwo = dict(kw)
    if kw.get("sequential_rng"):
        kwo["time_speeds_draw"] = 1 if grades is None else 0
    so = orc.settings(D, nDer, seed=seed, **kwo)
    keep = [orc.set_grades(so, grades[0], grades[1])] if grades else []
    Lo, Po, k2 = orc.make_problem("gaussian", D)
    Lo.kind = 0
    Lo.fn = C.cast(hl.host_logl, C.c_void_p)
    Lo.ctx = C.cast(ctx, C.c_void_p)
    return orc.run(so, Lo, Po)


def _assert_walks_the_oracle(g, o):
    for k in ("ndead", "nlike", "niter", "nbatches", "ncluster", "ncluster_dead"):
        assert g[k] == o[k], (k, g[k], o[k])
    assert abs(g["logZ"] - o["logZ"]) < 1e-8
    rel = np.abs(g["dead"] - o["dead"]) / np.maximum(1.0, np.abs(o["dead"]))
    assert rel.max() < 1e-7


@pytest.mark.gpu
def test_a_terms_source_walks_the_oracle(engine, tmp_path):
    api = engine
    data = _line_data(256)
    kw = dict(nlive=100, num_repeats=6, batch=20)
    h = api.source_create(LINE_TERMS, data=data, nterms=256)
    L, P, k1 = api.make_problem("source", 2, 2, source=h)
    g = api.run(_settings(api, 2, 2, seed=5, **kw), L, P)
    assert g["path"]["source_terms"] > 0
    _assert_walks_the_oracle(g, _oracle_run(tmp_path, LINE_TERMS, 256, 2, 2, data, **kw))
    api.load().pchip_source_destroy(h)


@pytest.mark.gpu
def test_a_graded_terms_source_books_every_grade_as_the_replay_and_the_oracle(engine, tmp_path):
    """the replay evaluates every bracket end alone, the terms form two ends in one pass: the evaluations of every grade are the same"""
    grades = ([3, 3], [2, 4])
    kw = dict(nlive=100, num_repeats=6, batch=20)
    t, p = _pair_of_runs(engine, GAUSS_TERMS, 6, 6, 1, grades=grades, seed=5, **kw)
    _assert_same_run(t, p)
    o = _oracle_run(tmp_path, GAUSS_TERMS, 6, 6, 1, None, grades=grades, **kw)
    _assert_walks_the_oracle(t, o)
    assert list(t["nlike_grade"][:2]) == list(p["nlike_grade"][:2]) == [int(v) for v in o["nlike_grade"][:2]]
    assert all(v > 0 for v in t["nlike_grade"][:2])


@pytest.mark.gpu
def test_a_long_loop(engine):
    """256 strided terms a lane: the same run as its replay, phi included"""
    t, p = _pair_of_runs(engine, LINE_TERMS, 16384, 2, 2, data=_line_data(16384), nlive=50, num_repeats=4)
    _assert_same_run(t, p)


@pytest.mark.gpu
def test_source_eval_of_a_plain_source_and_its_refusals(engine):
    """the evaluation door takes both forms; a handle that does not exist is refused with a message"""
    api = engine
    data = _line_data(40)
    h = api.source_create(replay_of(LINE_TERMS), options=("-DNTERMS=40",), data=data)
    th = np.array([[0.3, 0.6], [0.0, 0.0]])
    logL, phi = api.source_eval(h, th, 2)
    x, y = data[0::2], data[1::2]
    for k in range(2):
        chi2 = float(np.sum((y - (th[k, 0] * x + th[k, 1])) ** 2))
        assert abs(phi[k, 0] - chi2) <= 1e-13 * chi2 and logL[k] == -phi[k, 0] / 2.0
    logL0, _ = api.source_eval(h, th, 0)
    assert np.array_equal(logL0, logL)
    api.load().pchip_source_destroy(h)
    with pytest.raises(RuntimeError) as e:
        api.source_eval(h, th, 0)
    assert "does not exist" in str(e.value)
