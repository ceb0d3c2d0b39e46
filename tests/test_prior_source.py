"""The user's own prior as device source (pchip_source_create_prior, pchip_prior.kind = PCHIP_PRIOR_SOURCE): pchip_prior_param in the same
text and the same handle as the likelihood, evaluated inside the sampling kernels (pc_source_theta, polychordlite_amd/csrc/pc_sample.hip).

Every text uses `#pragma clang fp contract(off)` and -- but for LOGSORT -- only + - * /: the same text compiled for the host is then the
device bit for bit, and it is the oracle's callback prior and likelihood.

CPU: the surface, the refusals at create, every variant a launcher can choose for kind 3 compiles for gfx950 (plain and terms handle).
GPU: the transform door against the host build; runs walk the oracle; one handle under prior kinds 1, 2 and 3; the refusals of a run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_api as orc
from tests.test_device_priors import _table_variants
from tests.test_device_source import GAUSS_SRC
from tests.test_source_terms import LINE_TERMS, REPLAY_WRAPPER, _line_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = "__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata)\n"

# theta_i = data[i] + data[D + i] * cube[i]
AFF_PRIOR = DECL + r"""{
    return data[i] + data[nDims + i] * cube[i];
}
"""

# a correlated affine prior: theta_i = m_i + sum_{j <= i} L_ij cube_j;  data = m [D], then the lower triangle of L packed row by row
TRI_PRIOR = DECL + r"""{
    const double *row = data + nDims + ((long)i * (i + 1)) / 2;
    double s = data[i];
    for (int j = 0; j <= i; ++j) s = s + row[j] * cube[j];
    return s;
}
"""

# a bound that depends on another parameter: theta_0 from cube_0, theta_i = theta_0 * cube_i, theta_0 recomputed in lane i
DEP_PRIOR = DECL + r"""{
    const double t0 = data[0] + data[1] * cube[0];
    return i == 0 ? t0 : t0 * cube[i];
}
"""

# a sorted log-uniform block over all parameters, the chain of pc_table_theta's sorted blocks: y_n = x_n^(1/n), y_k = y_{k+1} x_k^(1/k),
# then lo (hi / lo)^y;  data = (lo, hi)
LOGSORT_PRIOR = DECL + r"""{
    double r = pow(cube[nDims - 1], 1.0 / (double)nDims);
    for (int k = nDims - 2; k >= i; --k) r = r * pow(cube[k], 1.0 / (double)(k + 1));
    return data[0] * pow(data[1] / data[0], r);
}
"""

# the straight-line fit of tests/test_source_terms.py behind TRI's data block (nDims 2: two means and three entries of L)
LINE_TERMS_AT5 = LINE_TERMS.replace("data[2 * i", "data[5 + 2 * i")
assert LINE_TERMS_AT5.count("data[5 + 2 * i") == 2

TEXTS = {"AFF": GAUSS_SRC + AFF_PRIOR, "TRI": GAUSS_SRC + TRI_PRIOR, "DEP": GAUSS_SRC + DEP_PRIOR, "LOGSORT": GAUSS_SRC + LOGSORT_PRIOR,
         "TRI_LINE": LINE_TERMS_AT5 + TRI_PRIOR}

HOST_WRAPPER = r"""
extern "C" double host_logl(const double *t, int D, double *phi, int nDer, void *ctx)
{ const double *d = ((const double **)ctx)[0]; long n = (long)((const double **)ctx)[1]; return pchip_loglikelihood(t, phi, D, nDer, d, n); }
extern "C" void host_prior(const double *c, double *t, int D, void *ctx)
{ const double *d = ((const double **)ctx)[0]; long n = (long)((const double **)ctx)[1]; for (int i = 0; i < D; ++i) t[i] = pchip_prior_param(c, i, D, d, n); }
extern "C" void host_prior_eval(const double *c, long n, int D, const double *d, long nd, double *t)
{ for (long p = 0; p < n; ++p) for (int i = 0; i < D; ++i) t[p * D + i] = pchip_prior_param(c + p * D, i, D, d, nd); }
"""


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _settings(api, D, nDer, **kw):
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _data(name, D):
    """the data block of a text at nDims D: the prior's parameters (and, behind them, the line's points).  The priors cover the Gaussian
    of GAUSS_SRC (0.5, 0.1) with four sigma or more to every edge"""
    i = np.arange(D, dtype=np.float64)
    if name == "AFF":
        return np.concatenate([np.linspace(-0.6, -0.2, D), np.linspace(1.5, 2.5, D)])
    if name in ("TRI", "TRI_LINE"):
        rows = []
        for r in range(D):
            rows += [0.01 * (((r + 2 * j) % 5) - 2) for j in range(r)] + [1.6]
        tri = np.concatenate([-0.3 + 0.005 * i, np.array(rows)])
        return tri if name == "TRI" else np.concatenate([tri, _line_data(256)])
    if name == "DEP":
        return np.array([0.2, 0.8])
    return np.array([1e-3, 5.0])


_HANDLES = {}


def _handle(api, name, D, nterms=None):
    """one handle per (text, data block) for the whole module: every kernel variant of it compiles once"""
    key = (name, D, nterms)
    if key not in _HANDLES:
        _HANDLES[key] = api.source_create(TEXTS[name], data=_data(name, D), nterms=nterms, prior=True)
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _destroy_handles():
    yield
    api, lib = _lib()
    for h in _HANDLES.values():
        lib.pchip_source_destroy(h)
    _HANDLES.clear()


_HOSTS = {}


def _host(tmp_path_factory, name, nterms=None):
    """the same text compiled for the host: host_logl and host_prior (the oracle's callbacks), host_prior_eval (many points)"""
    key = (name, nterms)
    if key not in _HOSTS:
        d = tmp_path_factory.mktemp(f"host_{name}")
        cpp, so = d / f"{name}.cpp", d / f"lib{name}.so"
        cpp.write_text("#include <math.h>\n" + TEXTS[name] + (REPLAY_WRAPPER if nterms else "") + HOST_WRAPPER)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-D__device__=", "-Wno-unknown-pragmas"] +
                              ([f"-DNTERMS={nterms}"] if nterms else []) + ["-x", "c++", str(cpp), "-o", str(so)])
        lib = C.CDLL(str(so))
        lib.host_logl.restype = C.c_double
        _HOSTS[key] = lib
    return _HOSTS[key]


def _host_thetas(hl, cubes, data):
    th = np.empty_like(cubes)
    hl.host_prior_eval(cubes.ctypes.data_as(C.c_void_p), C.c_long(cubes.shape[0]), cubes.shape[1], data.ctypes.data_as(C.c_void_p),
                       C.c_long(data.size), th.ctypes.data_as(C.c_void_p))
    return th


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_prior_source_surface():
    api, lib = _lib()
    for sym in ("pchip_source_create_prior", "pchip_source_prior_eval"):
        assert hasattr(lib, sym), sym
    hdr = open(os.path.join(ROOT, "include", "polychord_hip.h")).read()
    assert "PCHIP_PRIOR_SOURCE = 3" in hdr and api.PRIOR_SOURCE == 3
    assert "pchip_source_create_prior" in hdr and "pchip_source_prior_eval" in hdr and "pchip_prior_param" in hdr
    assert lib.pchip_abi_version() == 9
    assert lib.pchip_sizeof(b"prior") == C.sizeof(api.Prior) == 48


@pytest.mark.parametrize("nterms", [None, 8])
def test_a_source_without_the_prior_is_refused(nterms):
    """pchip_source_create_prior probes every function of the handle's form and pchip_prior_param: the one that is missing is named"""
    api, _ = _lib()
    with pytest.raises(RuntimeError) as e:
        api.source_create(GAUSS_SRC if nterms is None else LINE_TERMS, nterms=nterms, prior=True)
    assert "pchip_prior_param" in str(e.value)


def test_a_prior_source_without_the_likelihood_is_refused():
    api, _ = _lib()
    with pytest.raises(RuntimeError) as e:
        api.source_create("#pragma clang fp contract(off)\n" + AFF_PRIOR, prior=True)
    assert "pchip_loglikelihood" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        api.source_create(GAUSS_SRC + AFF_PRIOR, nterms=-1, prior=True)
    assert "nterms" in str(e.value)


def test_a_syntax_error_in_the_prior_names_the_users_line():
    api, _ = _lib()
    bad = ("\n\n__device__ double pchip_loglikelihood(const double *t, double *p, int D, int n, const double *d, long m) { return t[0]; }\n"
           "__device__ double pchip_prior_param(const double *c, int i, int D, const double *d, long m)\n{ return c[i] +; }\n")
    with pytest.raises(RuntimeError) as e:
        api.source_create(bad, prior=True)
    assert "pchip_user_source.h:5" in str(e.value) and "error" in str(e.value)


def _prior_variants():
    """what the launchers choose for prior.kind = 3: the PT = 1 variants of a table, and the transform door's kernel"""
    return _table_variants() + [f"k_prior_transform<{d}>" for d in (1, 2, 4)]


@pytest.mark.parametrize("form", ["plain", "terms"])
def test_every_prior_source_variant_compiles_for_gfx950(form):
    api, lib = _lib()
    src = open(os.path.join(ROOT, "polychordlite_amd", "csrc", "pc_sample.hip")).read()
    assert "S->prior.kind >= 2" in src and '"k_prior_transform<1>"' in src      # (kind 3 takes the table's rows; the door's kernel by name)
    h = (api.source_create(TEXTS["TRI"], data=_data("TRI", 4), prior=True) if form == "plain"
         else api.source_create(TEXTS["TRI_LINE"], data=_data("TRI_LINE", 2), nterms=256, prior=True))
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(_prior_variants()).encode(), log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_the_host_build_is_the_formula(tmp_path_factory):
    """the yardstick of the GPU tests, checked where no GPU is: the host build of TRI is m + L cube to rounding, DEP scales by theta_0"""
    D = 20
    data = _data("TRI", D)
    cubes = np.random.default_rng(1).random((50, D))
    th = _host_thetas(_host(tmp_path_factory, "TRI"), cubes, data)
    Lm = np.zeros((D, D))
    Lm[np.tril_indices(D)] = data[D:]
    assert np.allclose(th, data[:D] + cubes @ Lm.T, rtol=1e-13, atol=1e-15)
    th = _host_thetas(_host(tmp_path_factory, "DEP"), cubes, _data("DEP", D))
    assert np.array_equal(th[:, 0], 0.2 + 0.8 * cubes[:, 0]) and np.array_equal(th[:, 1:], th[:, :1] * cubes[:, 1:])


def test_run_repeats_refuses_a_prior_source(capfd):
    api, lib = _lib()
    from polychordlite_amd import repeats
    h = api.source_create(TEXTS["AFF"], data=_data("AFF", 4), prior=True)
    s = _settings(api, 4, 0, nlive=50, num_repeats=8)
    L, P, keep = api.make_problem("source", 4, 0, source=h, prior_source=True)
    assert P.kind == 3
    with pytest.raises(RuntimeError):
        repeats.run_repeats(s, L, P, [1, 2])
    assert "device source likelihood" in capfd.readouterr().err
    lib.pchip_source_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _cubes(D, seed):
    """2 000 seeded points; the first 200 have coordinates within 1e-12 of 0 (rows 0 - 99) or of 1 (rows 100 - 199)"""
    rng = np.random.default_rng(seed)
    cubes = rng.random((2000, D))
    edge = rng.random((100, D)) < 0.5
    cubes[0:100][edge] = rng.random(int(edge.sum())) * 1e-12
    edge = rng.random((100, D)) < 0.5
    cubes[100:200][edge] = 1.0 - rng.random(int(edge.sum())) * 1e-12
    return np.ascontiguousarray(cubes)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 20, 70])
@pytest.mark.parametrize("name", ["AFF", "TRI", "DEP"])
def test_the_transform_door_is_the_host_build(engine, tmp_path_factory, name, D):
    """pchip_source_prior_eval (k_prior_transform of the handle's module, through pc_source_theta) against the host build of the same text,
    bit for bit.  nDims 70: two coordinates share a lane, and TRI's loop crosses index 63 / 64"""
    api = engine
    cubes = _cubes(D, 1000 + D)
    dev = api.source_prior_eval(_handle(api, name, D), cubes)
    host = _host_thetas(_host(tmp_path_factory, name), cubes, _data(name, D))
    print(f"{name} nDims {D}: device != host at {int((dev != host).sum())} of {dev.size} values")
    assert np.array_equal(dev, host)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 20, 70])
def test_a_transcendental_prior_is_the_host_build_to_rounding(engine, tmp_path_factory, D):
    """LOGSORT (pow): 1e-9 relative to max(1, |theta|), the bound of test_device_transform_is_the_host_function"""
    api = engine
    cubes = _cubes(D, 2000 + D)
    dev = api.source_prior_eval(_handle(api, "LOGSORT", D), cubes)
    host = _host_thetas(_host(tmp_path_factory, "LOGSORT"), cubes, _data("LOGSORT", D))
    assert np.all(np.isfinite(host)) and np.all(np.isfinite(dev))
    rel = np.abs(dev - host) / np.maximum(1.0, np.abs(host))
    print(f"LOGSORT nDims {D}: max deviation {rel.max():.3e} relative to max(1, |theta|)")
    assert rel.max() <= 1e-9


def _prior_vs_oracle(api, tmp_path_factory, name, D, nDer, nterms=None, grades=None, **kw):
    """engine with prior.kind = 3 against pc_oracle_run whose callback prior and likelihood are the host build of the same text"""
    h = _handle(api, name, D, nterms)
    s = _settings(api, D, nDer, seed=5, **kw)
    keep = []
    if grades:
        keep.append(api.set_grades(s, *grades))
    L, P, k1 = api.make_problem("source", D, nDer, source=h, prior_source=True)
    g = api.run(s, L, P)
    assert g["path"]["device_prior"] > 0 and g["path"]["source_kernels"] > 0 and g["path"]["slice_wave"] > 0, g["path"]
    hl = _host(tmp_path_factory, name, nterms)
    d = _data(name, D)
    ctx = (C.c_void_p * 2)(d.ctypes.data, d.size)
    kwo = dict(kw)
    if kw.get("sequential_rng"):   # one gaussian deviate goes to time_speeds (generate.F90:285-287), as in _source_vs_oracle
        kwo["time_speeds_draw"] = 1 if grades is None else 0
    so = orc.settings(D, nDer, seed=5, **kwo)
    if grades:
        keep.append(orc.set_grades(so, grades[0], grades[1]))
    Lo, Po, k2 = orc.make_problem("gaussian", D)
    Lo.kind = 0
    Lo.fn = C.cast(hl.host_logl, C.c_void_p)
    Lo.ctx = C.cast(ctx, C.c_void_p)
    Po.kind = 0
    Po.fn = C.cast(hl.host_prior, C.c_void_p)
    Po.ctx = C.cast(ctx, C.c_void_p)
    o = orc.run(so, Lo, Po)
    for k in ("ndead", "nlike", "niter", "nbatches", "ncluster", "ncluster_dead"):
        assert g[k] == o[k], (k, g[k], o[k])
    print(f"{name} nDims {D}: |dlogZ| {abs(g['logZ'] - o['logZ']):.3e}, ndead {g['ndead']}, nlike {g['nlike']}")
    assert abs(g["logZ"] - o["logZ"]) < 1e-8, (g["logZ"], o["logZ"])
    rel = np.abs(g["dead"] - o["dead"]) / np.maximum(1.0, np.abs(o["dead"]))
    assert rel.max() < 1e-7, rel.max()
    assert g["ndead"] > 0
    return g


ORACLE_CASES = {
    "1_tri4": dict(name="TRI", D=4, nDer=1, nlive=100, num_repeats=8, batch=16),
    "2_aff20_fused": dict(name="AFF", D=20, nDer=2, nlive=200, num_repeats=40, batch=32),
    "3_tri40_nhats_q": dict(name="TRI", D=40, nDer=0, nlive=150, num_repeats=20, batch=32),
    "4_aff70_capped": dict(name="AFF", D=70, nDer=0, nlive=100, num_repeats=20, batch=16, max_ndead=300),
    "5_dep4_clustering": dict(name="DEP", D=4, nDer=1, nlive=200, num_repeats=8, batch=40, do_clustering=1),
    "6_aff6_two_grades": dict(name="AFF", D=6, nDer=1, nlive=100, num_repeats=6, batch=20, grades=([3, 3], [2, 4])),
    "7_aff6_sequential": dict(name="AFF", D=6, nDer=5, nlive=60, num_repeats=12, batch=1, sequential_rng=1),
    "8_tri2_terms_line": dict(name="TRI_LINE", D=2, nDer=1, nterms=256, nlive=100, num_repeats=6, batch=20),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_a_prior_source_walks_the_oracle(engine, tmp_path_factory, case):
    """the same counters, log Z to 1e-8, dead rows to 1e-7 relative: the bounds of test_source_walks_the_oracle"""
    c = dict(ORACLE_CASES[case])
    g = _prior_vs_oracle(engine, tmp_path_factory, c.pop("name"), c.pop("D"), c.pop("nDer"), **c)
    if "terms" in case:
        assert g["path"]["source_terms"] > 0


@pytest.mark.gpu
def test_one_handle_under_three_prior_kinds(engine):
    """the transform's branch is on S.prior.kind, not on the define: a handle WITH a prior run under the box (kind 1) and under a table
    (kind 2) is the run of a handle without one; kind 3 is the handle's own prior"""
    api = engine
    lib = api.load()
    D, nDer = 6, 1
    data = _data("AFF", D)
    table = [("gaussian", (0.5, 0.5))] * 3 + [("uniform", (-0.5, 1.5))] * 3
    hp = _handle(api, "AFF", D)
    h0 = api.source_create(GAUSS_SRC, data=data)
    runs = {}
    for who, h in (("prior", hp), ("plain", h0)):
        for kind in ((1, 2, 3) if who == "prior" else (1, 2)):
            s = _settings(api, D, nDer, seed=9, nlive=100, num_repeats=12, batch=20)
            L, P, keep = api.make_problem("source", D, nDer, source=h, prior_table=table if kind == 2 else None, prior_source=kind == 3)
            assert P.kind == kind
            runs[who, kind] = api.run(s, L, P)
    for kind in (1, 2):
        a, b = runs["prior", kind], runs["plain", kind]
        for k in ("ndead", "nlike", "niter", "nbatches"):
            assert a[k] == b[k], (kind, k, a[k], b[k])
        assert a["logZ"] == b["logZ"], kind
        assert np.array_equal(a["dead"], b["dead"]), kind
        assert (a["path"]["device_prior"] > 0) == (kind == 2) and a["path"] == b["path"]
    g = runs["prior", 3]
    assert g["path"]["device_prior"] > 0 and g["ndead"] > 0
    th = g["dead"][:, D:2 * D]
    assert np.array_equal(th, data[:D] + data[D:] * g["dead"][:, :D])       # (theta is the handle's prior of the cube, not a box or the table)
    lib.pchip_source_destroy(h0)


@pytest.mark.gpu
def test_a_prior_source_needs_a_handle_with_a_prior(engine, capfd):
    api = engine
    lib = api.load()
    h = api.source_create(GAUSS_SRC)
    s = _settings(api, 4, 0, nlive=50, num_repeats=8)
    L, P, keep = api.make_problem("source", 4, 0, source=h, prior_source=True)
    r = api.Result()
    assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(P), C.byref(r)) == 1
    err = capfd.readouterr().err
    assert "pchip_prior_param" in err and "pchip_source_create_prior" in err, err
    with pytest.raises(RuntimeError) as e:          # the transform door says the same of such a handle, and of one that is gone
        api.source_prior_eval(h, np.full((2, 4), 0.5))
    assert "pchip_prior_param" in str(e.value)
    lib.pchip_source_destroy(h)
    with pytest.raises(RuntimeError) as e:
        api.source_prior_eval(h, np.full((2, 4), 0.5))
    assert "does not exist" in str(e.value)


@pytest.mark.gpu
def test_a_prior_source_needs_a_source_likelihood(engine, capfd):
    api = engine
    lib = api.load()
    s = _settings(api, 4, 0, nlive=50, num_repeats=8)
    L, P, keep = api.make_problem("gaussian", 4, 0, prior_source=True)
    r = api.Result()
    assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(P), C.byref(r)) == 1
    err = capfd.readouterr().err
    assert "prior.kind = 3" in err and "needs a device source likelihood" in err, err
