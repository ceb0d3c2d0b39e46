"""The quadratic form of a device source (pchip_source_create_quad): a Gaussian in data space with a dense precision matrix, chi2 = r^T P r.
The source defines pchip_residual (one lane per i) and the terms form's pchip_logl_finish; P is copied at creation and lies behind the
user's data in the run's block (polychordlite_amd/csrc/pc_sample.hip, PCHIP_USER_QUAD).

The fixture is a straight line a + b x_i under AR(1)-correlated noise: theta = (a, b), data = x[n] | d[n], P the dense inverse of the AR(1)
covariance, derived parameters chi2 and the first residual.  It is written with #pragma clang fp contract(off) and + - * / plus explicit
fma() only, so that a host build gives the device's bits.  Its REPLAY is a plain pchip_loglikelihood source: the same text followed by a
wrapper (-DNRES=n, the data block x | d | P) that forms the residuals, the fma chain of every column in ascending i, the products, the 64
strided partials and the balanced tree serially -- the defined order of the header, run by the code that existed before this form.
For the order tests a dense random NON-symmetric P as well, entries over six decades with mixed signs: a transposed read or a symmetrised
matrix cannot pass.

CPU: the surface, the refusals, every variant a launcher can choose compiles for gfx950 from a quad handle; the host replay against exact
rational arithmetic.  GPU: the order bit for bit against the host replay and the device build of the replay; a quad run is the replay's
run (no derived parameters, rows in LDS, phi in the loop, the shape the residual blocks push from the one to the other, a prior table,
the handle's own prior); runs in step; the device maximiser against the replay's and against generalised least squares."""
import ctypes as C
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.test_source_terms import _terms_variants, _tree64, _strided_partials, _assert_same_run

SIGMA, RHO = 0.1, 0.6
LO, HI = [-1.0, -1.0], [2.0, 2.0]

# data = x[NRES] | d[NRES] (a structure of arrays: lane-consecutive i reads consecutive doubles); -DNRES=n reaches the user's text alone
QUAD = r"""
#pragma clang fp contract(off)
__device__ double pchip_residual(const double *theta, int nDims, const double *data, long ndata, long i)
{
    return data[NRES + i] - (theta[0] + theta[1] * data[i]);
}
__device__ double pchip_logl_finish(double chi2, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = chi2;
    if (nDerived > 1) phi[1] = data[NRES] - (theta[0] + theta[1] * data[0]);
    for (int e = 2; e < nDerived; ++e) phi[e] = 0.0;
    return -chi2 / 2.0;
}
"""

# the box of the line's prior as the handle's own prior (with_prior)
QUAD_PRIOR = r"""
__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata)
{
    return -1.0 + 3.0 * cube[i];
}
"""

# The defined order, serially.  The replay's data block is x | d | P: the user's functions get ndata = 2 NRES, what the quad handle shows them.
#   1. r_i;  2. q_j = fma(P[i][j], r_i, q_j) for i ascending from 0.0;  3. t_j = r_j * q_j;  4. lane l adds t_l, t_(l + 64), ... to 0.0,
#   the 64 partials in the balanced tree of the terms form
REPLAY_WRAPPER = r"""
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    const double *P = data + 2 * NRES;
    double r[NRES], s[64];
    for (long i = 0; i < NRES; ++i) r[i] = pchip_residual(theta, nDims, data, 2 * NRES, i);
    for (int l = 0; l < 64; ++l) {
        double a = 0.0;
        for (long j = l; j < NRES; j += 64) {
            double q = 0.0;
            for (long i = 0; i < NRES; ++i) q = fma(P[i * NRES + j], r[i], q);
            const double t = r[j] * q;
            a = a + t;
        }
        s[l] = a;
    }
    for (int w = 1; w < 16; w *= 2)
        for (int l = 0; l < 64; l += 2 * w) s[l] = s[l] + s[l + w];
    return pchip_logl_finish((s[0] + s[16]) + (s[32] + s[48]), theta, phi, nDims, nDerived, data, 2 * NRES);
}
"""

HOST_WRAPPER = r"""
extern "C" void host_eval(const double *t, long n, int D, int nDer, const double *d, long nd, double *logL, double *phi)
{ double scratch[32]; for (long p = 0; p < n; ++p) logL[p] = pchip_loglikelihood(t + p * D, nDer > 0 ? phi + p * nDer : scratch, D, nDer, d, nd); }
"""


def replay_of(text):
    return text + REPLAY_WRAPPER


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _create_quad(api, text, **kw):
    """source_create with residuals / precision: the door this file is about (a library without the feature fails here, at the missing symbol)"""
    assert hasattr(api.load(), "pchip_source_create_quad"), "the library does not export pchip_source_create_quad"
    return api.source_create(text, **kw)


def _settings(api, D, nDer, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _ar1_cov(n):
    i = np.arange(n)
    return SIGMA ** 2 * RHO ** np.abs(i[:, None] - i[None, :])


def _line_data(n, seed=3):
    """x = uniform(-1, 1), d = 0.6 + 0.3 x + AR(1) noise; the block x | d"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n)
    noise = np.linalg.cholesky(_ar1_cov(n)) @ rng.normal(0.0, 1.0, n)
    return np.concatenate([x, 0.6 + 0.3 * x + noise])


def _precision(kind, n, seed=11):
    """ar1: the dense inverse of the AR(1) covariance; rand: dense, NOT symmetric, |entries| over six decades, mixed signs"""
    if kind == "ar1":
        return np.ascontiguousarray(np.linalg.inv(_ar1_cov(n)))
    rng = np.random.default_rng(seed + n)
    return np.ascontiguousarray(rng.choice([-1.0, 1.0], (n, n)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, n)))


def _replay_block(data, P):
    return np.concatenate([data, np.ravel(P)])


def _host_replay(tmp_path, nres, name):
    cpp = tmp_path / f"{name}.cpp"
    so = tmp_path / f"lib{name}.so"
    cpp.write_text("#include <math.h>\n" + replay_of(QUAD) + HOST_WRAPPER)
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-D__device__=", f"-DNRES={nres}", "-x", "c++", str(cpp), "-o", str(so)])
    return C.CDLL(str(so))


def _host_eval(hl, th, nDer, block):
    n, D = th.shape
    logL, phi = np.empty(n), np.empty((n, nDer))
    hl.host_eval(th.ctypes.data_as(C.c_void_p), C.c_long(n), D, nDer, block.ctypes.data_as(C.c_void_p), C.c_long(block.size),
                 logL.ctypes.data_as(C.c_void_p), phi.ctypes.data_as(C.c_void_p))
    return logL, phi


def _box_points(npts, seed, D=2):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(LO[0], HI[0], (npts, D)))


def _residuals(th, data):
    """[npts][nres]: the residuals as the source forms them, operation for operation"""
    n = data.size // 2
    x, d = data[:n], data[n:]
    return d[None, :] - (th[:, 0:1] + th[:, 1:2] * x[None, :])


def _fma(a, b, c):
    """the fused multiply-add of IEEE 754 on doubles: exact in rationals, rounded once (float(Fraction) rounds to nearest, ties to even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _chi2_defined_order(r, P):
    """one point: the four steps of the header's contract in Python, every fma through exact rationals"""
    n = r.size
    t = np.zeros((1, n))
    for j in range(n):
        q = 0.0
        for i in range(n):
            q = _fma(P[i, j], r[i], q)
        t[0, j] = r[j] * q
    return float(_tree64(_strided_partials(t))[0])


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_the_symbol_is_exported_and_the_abi_is_still_9():
    api, lib = _lib()
    assert hasattr(lib, "pchip_source_create_quad")
    assert lib.pchip_abi_version() == 9
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "polychord_hip.h")).read()
    assert "#define PCHIP_SOURCE_MAX_RES 1024" in hdr and "int  pchip_source_create_quad(" in hdr
    assert "pchip_residual" in hdr and "fma(P[i * nres + j], r_i, q_j)" in hdr


@pytest.mark.parametrize("nres", [0, 1025, -1])
def test_nres_out_of_range_is_refused_with_the_range(nres):
    api, lib = _lib()
    assert hasattr(lib, "pchip_source_create_quad")
    one = np.ones(1)
    h = lib.pchip_source_create_quad(QUAD.encode(), b"-DNRES=4", None, 0, nres, api.dptr(one), 0)
    msg = lib.polychord_hip_last_error().decode()
    assert h == -1 and "nres" in msg and "1 <= nres <= 1024" in msg


def test_no_precision_is_refused():
    api, _ = _lib()
    with pytest.raises(RuntimeError) as e:
        _create_quad(api, QUAD, options=("-DNRES=4",), data=_line_data(4), residuals=4, precision=None)
    assert "precision == NULL" in str(e.value)


def test_a_precision_of_another_shape_is_a_value_error():
    api, _ = _lib()
    for bad in (np.eye(5), np.ones(16), np.ones((2, 8))):
        with pytest.raises(ValueError):
            _create_quad(api, QUAD, options=("-DNRES=4",), data=_line_data(4), residuals=4, precision=bad)


def test_a_source_that_lacks_one_of_its_functions_is_refused_by_name():
    api, _ = _lib()
    kw = dict(options=("-DNRES=8",), data=_line_data(8), residuals=8, precision=_precision("ar1", 8))
    cut = QUAD.index("__device__ double pchip_logl_finish")
    with pytest.raises(RuntimeError) as e:
        _create_quad(api, "#pragma clang fp contract(off)\n" + QUAD[cut:], **kw)
    assert "pchip_residual" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        _create_quad(api, QUAD[:cut], **kw)
    assert "pchip_logl_finish" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        _create_quad(api, QUAD, prior=True, **kw)
    assert "pchip_prior_param" in str(e.value)
    h = _create_quad(api, QUAD + QUAD_PRIOR, prior=True, **kw)
    api.load().pchip_source_destroy(h)


def test_a_syntax_error_names_the_users_line():
    api, _ = _lib()
    bad = ("\n\n__device__ double pchip_residual(const double *t, int D, const double *d, long m, long i)\n{ return t[0] +; }\n"
           "__device__ double pchip_logl_finish(double s, const double *t, double *p, int D, int n, const double *d, long m) { return s; }\n")
    with pytest.raises(RuntimeError) as e:
        _create_quad(api, bad, residuals=4, precision=np.eye(4))
    assert "pchip_user_source.h:4" in str(e.value) and "error" in str(e.value)


@pytest.mark.parametrize("nres", [300, 1024])
def test_every_variant_compiles_for_gfx950_from_a_quad_handle(nres):
    """what the launchers can choose for a terms handle, the in-step kernel of a source and the maximiser's; at the largest nres as well"""
    api, lib = _lib()
    h = _create_quad(api, QUAD, options=("-DPCHIP_TEST_OPTION=1", f"-DNRES={nres}"), data=_line_data(nres), residuals=nres, precision=_precision("ar1", nres))
    names = _terms_variants() + ["k_slice_many<1, 1, false, 1, 8, 0>", "k_slice_many<1, 1, false, 1, 0, 0, 1>", "k_maximise<1>", "k_max_rank<1>"]
    if nres == 1024:
        names = ["k_generate_live<1>", "k_source_eval<1>", "k_slice<1, 1, false>", "k_slice<1, 1, false, 1, 8>", "k_maximise<1>"]
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(names).encode(), log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_the_other_forms_still_compile_beside_a_quad_handle_and_the_text_is_five_files():
    api, lib = _lib()
    from tests.test_source_terms import LINE_TERMS, replay_of as line_replay
    from tests.test_source_sums import EIGHT, _eight_data
    seen, i = [], 0
    while True:
        name = C.c_char_p()
        if lib.pchip_rtc_embedded_source(i, C.byref(name)) is None:
            break
        seen.append(name.value.decode())
        i += 1
    assert sorted(seen) == sorted(["pc_dev.h", "pc_state.h", "pc_seed.h", "pc_sample.hip", "pc_slice_body.inc"])
    hq = _create_quad(api, QUAD, options=("-DNRES=16",), data=_line_data(16), residuals=16, precision=_precision("rand", 16))
    hs = api.source_create(EIGHT, data=_eight_data(16), nterms=16, nsums=8)
    ht = api.source_create(LINE_TERMS, nterms=16)
    hp = api.source_create(line_replay(LINE_TERMS), options=("-DNTERMS=16",))
    names = ["k_generate_live<1>", "k_slice<1, 1, false>", "k_slice<1, 1, true>", "k_slice<1, 1, false, 1, 8>", "k_slice<2, 4, false>",
             "k_slice_many<1, 1, false, 1, 8, 0>", "k_slice<1, 1, false, 1, 0, 0, 1>", "k_source_eval<1>"]
    log = C.create_string_buffer(1 << 16)
    for h in (ht, hp, hs, hq):
        assert lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(names).encode(), log, len(log), None) == 0, log.value.decode(errors="replace")
        lib.pchip_source_destroy(h)


def test_user_macros_do_not_reach_the_library_kernels():
    api, lib = _lib()
    src = "#define D 3\n#define nr 7\n#define N 5\n#define U 2\n#define G 9\n" + QUAD.replace("theta[1] * data[i]);\n}", "theta[1] * data[i]) * (double)S;\n}")
    assert src.count("(double)S") == 1
    h = _create_quad(api, src, options=("-DS=1", "-DNRES=70"), data=_line_data(70), residuals=70, precision=_precision("ar1", 70))
    log = C.create_string_buffer(1 << 16)
    names = b"k_slice<1, 2, false>;k_slice<1, 1, false, 1, 8>;k_source_eval<1>"
    assert lib.pchip_rtc_compile_check(h, b"gfx950", names, log, len(log), None) == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


@pytest.mark.parametrize("kind", ["ar1", "rand"])
def test_the_host_replay_is_the_quadratic_form_in_exact_arithmetic(tmp_path, kind):
    """the yardstick of the GPU tests, checked where no GPU is: the host replay against r^T P r in rationals, of the residuals and the matrix
    as the doubles they are.  The bound is derived: nres roundings of relative size 2^-53 on the way to every q_j, one for the product, at
    most nres / 64 + 6 for the adds -- under 2 nres of them in all -- each on a quantity bounded by sum |P_ij r_i r_j|."""
    _lib()[1].pchip_source_create_quad          # (the file is about that door: without it nothing here passes)
    nres = 65
    data, P = _line_data(nres), _precision(kind, nres)
    th = _box_points(8, 1)
    lh, ph = _host_eval(_host_replay(tmp_path, nres, f"ex{kind}"), th, 2, _replay_block(data, P))
    r = _residuals(th, data)
    assert np.array_equal(ph[:, 1], r[:, 0]) and np.array_equal(lh, -ph[:, 0] / 2.0)
    PF = [[Fraction(v) for v in row] for row in P]
    for p in range(th.shape[0]):
        rF = [Fraction(v) for v in r[p]]
        exact = sum(rF[j] * sum(PF[i][j] * rF[i] for i in range(nres)) for j in range(nres))
        mag = sum(abs(rF[j] * PF[i][j] * rF[i]) for i in range(nres) for j in range(nres))
        err, bound = abs(Fraction(ph[p, 0]) - exact), nres * Fraction(2) ** -52 * mag
        print(f"{kind} point {p}: |chi2 - exact| / bound = {float(err / bound):.4f}")
        assert err <= bound


@pytest.mark.parametrize("kind", ["ar1", "rand"])
def test_the_replays_fma_chain_is_the_rational_chain_rounded_once_a_step(tmp_path, kind):
    """nres = 5: every fused multiply-add of the wrapper formed in rationals and rounded once, the products and the tree in numpy: bit for bit"""
    _lib()[1].pchip_source_create_quad
    nres = 5
    data, P = _line_data(nres), _precision(kind, nres)
    th = _box_points(8, 2)
    lh, ph = _host_eval(_host_replay(tmp_path, nres, f"fma{kind}"), th, 2, _replay_block(data, P))
    r = _residuals(th, data)
    want = np.array([_chi2_defined_order(r[p], P) for p in range(th.shape[0])])
    assert np.array_equal(ph[:, 0], want)
    # ... and a chain that multiplies and adds with a rounding each differs somewhere: the fma is not decoration
    q_plain = np.zeros((th.shape[0], nres))
    for i in range(nres):
        q_plain = q_plain + P[i][None, :] * r[:, i:i + 1]
    if kind == "rand":
        assert np.any(_tree64(_strided_partials(r * q_plain)) != want)


# ---------------------------------------------------------------------------------------------------------------------------- GPU
_HANDLES = {}


def _handle(key, make):
    """one handle per form, matrix and size for the whole module: each of its kernel variants compiles once"""
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


def _pair(api, kind, nres, prior=False):
    """(quad handle, its replay as a plain source with the data block x | d | P), made once; and the two blocks"""
    data, P = _line_data(nres, seed=100 + nres), _precision(kind, nres)
    extra = QUAD_PRIOR if prior else ""
    opts = (f"-DNRES={nres}",)
    hq = _handle((kind, nres, prior, "quad"), lambda: _create_quad(api, QUAD + extra, options=opts, data=data, residuals=nres, precision=P, prior=prior))
    hp = _handle((kind, nres, prior, "replay"), lambda: api.source_create(replay_of(QUAD) + extra, options=opts, data=_replay_block(data, P), prior=prior))
    return hq, hp, data, P


@pytest.mark.gpu
@pytest.mark.parametrize("nres", [1, 5, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["ar1", "rand"])
def test_the_order_of_the_quadratic_form(engine, tmp_path, kind, nres):
    api = engine
    hq, hp, data, P = _pair(api, kind, nres)
    th = _box_points(8, nres)
    lq, pq = api.source_eval(hq, th, 2)
    lp, pp = api.source_eval(hp, th, 2)
    hl = _host_replay(tmp_path, nres, f"{kind}{nres}")
    lh, ph = _host_eval(hl, th, 2, _replay_block(data, P))
    lt, pt = _host_eval(hl, th, 2, _replay_block(data, np.ascontiguousarray(P.T)))
    print(f"{kind} nres {nres}: device != host replay at {int((pq[:, 0] != ph[:, 0]).sum())} of 8, != device replay at {int((pq[:, 0] != pp[:, 0]).sum())}, "
          f"!= host replay of the transposed matrix at {int((pq[:, 0] != pt[:, 0]).sum())}")
    assert np.all(np.isfinite(pq)) and np.all(np.isfinite(lq))
    # the quad form is the host replay, bit for bit -- chi2, the first residual and logL -- and the device build of the replay, a plain source
    assert np.array_equal(pq, ph) and np.array_equal(lq, lh)
    assert np.array_equal(pq, pp) and np.array_equal(lq, lp)
    assert np.array_equal(pq[:, 1], _residuals(th, data)[:, 0])
    # the inputs can tell a transposed read apart (a non-symmetric matrix of more than one residual; r^T P^T r is the same number, in other
    # roundings): the equalities above fail for a kernel that reads P[j][i] -- the test can fail
    if kind == "rand" and nres > 1:
        assert not np.array_equal(pt[:, 0], pq[:, 0])


def _runs(api, hq, hp, D, nDer, lo=None, hi=None, prior_table=None, prior_source=False, seed=7, **kw):
    out = []
    for h in (hq, hp):
        s = _settings(api, D, nDer, seed=seed, **kw)
        L, P, k1 = api.make_problem("source", D, nDer, source=h, lo=lo, hi=hi, prior_table=prior_table, prior_source=prior_source)
        out.append(api.run(s, L, P))
    return out


# A chain's LDS block in bytes (pc_slice_plan): 8 (nDims + nr) + 16, then 8 nr (nDims + 1) for the babies' theta rows when that and the
# form's own block fit under 48 KB -- for a quadratic form pc_terms_lds adds the second theta, 8 nDims, and the two residual blocks,
# 16 * (nres rounded up to even), and pc_slice_phi_lds counts the residual blocks in the decision.  nDims 70 (the line in theta[0], theta[1];
# the other coordinates are free): num_repeats 100, the rows alone do not fit (phi in the loop); num_repeats 80, nres 157: the rows fit
# (46 656 bytes) and the residual blocks, 16 * 158 = 2 528 bytes, are what pushes the chain over (49 184 bytes > 49 152; the smallest odd
# nres that does: the replay, whose every lane walks the whole matrix, is what such a test costs)
def _rows(D, nr):
    return 8 * (D + nr) + 16 + 8 * nr * (D + 1)


def _blocks(nres):
    return 16 * ((nres + 1) // 2 * 2)


KW = dict(nlive=50, num_repeats=5, batch=10)
RUN_SHAPES = {
    "no_derived_65": dict(nres=65, D=2, nDer=0, kw=KW, where="none"),
    "rows_in_lds": dict(nres=65, D=2, nDer=2, kw=KW, where="lds"),
    "phi_in_the_loop": dict(nres=65, D=70, nDer=2, kw=dict(nlive=50, num_repeats=100, batch=10, max_ndead=200), where="loop"),
    "pushed_over_by_the_residual_blocks": dict(nres=157, D=70, nDer=2, kw=dict(nlive=50, num_repeats=80, batch=10, max_ndead=100), where="pushed"),
    "prior_table": dict(nres=65, D=2, nDer=2, kw=KW, where="lds", prior_table=[("uniform", [-1.0, 2.0]), ("uniform", [-1.0, 2.0])]),
    "source_prior": dict(nres=65, D=2, nDer=2, kw=KW, where="lds", prior=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(RUN_SHAPES))
def test_a_quad_run_is_the_replays_run(engine, shape):
    """row for row and counter for counter the run of the replay as a plain source"""
    api = engine
    c = RUN_SHAPES[shape]
    D, nr, nres = c["D"], c["kw"]["num_repeats"], c["nres"]
    rows, blocks = _rows(D, nr), _blocks(nres)
    assert {"none": True, "lds": rows + blocks <= 49152, "loop": rows > 49152, "pushed": rows <= 49152 < rows + blocks}[c["where"]]
    prior = bool(c.get("prior"))
    hq, hp, data, P = _pair(api, "ar1", nres, prior=prior)
    box = {} if (prior or c.get("prior_table")) else dict(lo=[LO[0]] * D, hi=[HI[0]] * D)
    t, p = _runs(api, hq, hp, D, c["nDer"], prior_table=c.get("prior_table"), prior_source=prior, **box, **c["kw"])
    _assert_same_run(t, p)
    if c["nDer"] == 2:          # the derived parameters are finish's, of the chi2 the point was accepted with
        dd = t["dead"]
        ok = dd[:, -1] > -1e29
        assert ok.sum() > 50
        assert np.array_equal(dd[ok, -1], -dd[ok, 2 * D] / 2.0)
        assert np.array_equal(dd[ok, 2 * D + 1], _residuals(dd[ok, D:D + 2], data)[:, 0])


@pytest.mark.gpu
def test_quad_runs_in_step_are_their_solo_runs(engine):
    api = engine
    from polychordlite_amd import repeats
    hq, _, _, _ = _pair(api, "ar1", 65)
    L, P, keep = api.make_problem("source", 2, 2, source=hq, lo=LO, hi=HI)
    seeds = [21, 22, 23]
    merged, runs = repeats.run_in_step(_settings(api, 2, 2, **KW), L, P, seeds, max_in_flight=4)
    assert len(runs) == 3
    for seed, r in zip(seeds, runs):
        solo = api.run(_settings(api, 2, 2, seed=seed, **KW), L, P)
        for k in ("ndead", "nlike", "niter"):
            assert r[k] == solo[k], (seed, k, r[k], solo[k])
        assert r["ndead"] > 0 and r["logZ"] == solo["logZ"] and np.array_equal(r["dead"], solo["dead"]), seed
        assert r["path"]["slice_step"] > 0 and r["path"]["source_terms"] > 0, r["path"]


@pytest.mark.gpu
def test_the_device_maximiser_on_a_quad_handle_is_the_replays_and_the_gls_solution(engine):
    api = engine
    nres = 65
    hq, hp, data, P = _pair(api, "ar1", nres)
    s = _settings(api, 2, 2, seed=11, do_clustering=0, **KW)
    out = []
    for h in (hq, hp):
        L, Pr, keep = api.make_problem("source", 2, 2, source=h, lo=LO, hi=HI)
        g = api.run(s, L, Pr)
        out.append(api.maximise_device(s, L, Pr, g))
    a, b = out
    assert a["status"] == [0, 0] and a["niter"] == b["niter"] and a["neval"] == b["neval"] and min(a["niter"]) > 0
    for k in ("max_logl", "max_post", "logl_at_post", "logl_mean"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
    for k in ("max_point", "post_point", "mean_point"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    # generalised least squares (r^T P r sees the symmetric part of P alone): theta = (A^T P A)^-1 A^T P d, the tolerances of
    # tests/test_maximum_device.py for a maximum against its closed form (1e-4 in logL, 2e-3 in the point)
    x, d = data[:nres], data[nres:]
    A, Ps = np.stack([np.ones(nres), x], axis=1), (P + P.T) / 2.0
    gls = np.linalg.solve(A.T @ Ps @ A, A.T @ Ps @ d)
    rr = d - A @ gls
    print(f"max_point {a['max_point'][:2]} gls {gls}: |dlogL| {abs(a['max_logl'] + rr @ Ps @ rr / 2.0):.3e}")
    assert np.all(np.abs(a["max_point"][:2] - gls) < 2e-3) and abs(a["max_logl"] - (-(rr @ Ps @ rr) / 2.0)) < 1e-4
