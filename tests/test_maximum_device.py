"""The device maximiser (k_max_rank, k_maximise: pc_sample.hip; pchip_maximise_device[_many]: pc_engine.hip) on the GPU.

Its arithmetic is fixed so that a replay can follow it bit for bit: `replay` below is Nelder-Mead written from those rules in numpy, its
function values from `api.source_eval` (and its thetas, behind a table, from `api.prior_transform`) -- doors that run the same device code.
The host side (the choice of simplex, the writer, the refusals) is tests/test_maximum_host.py."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOGZERO = -1e30
DL = 1e-5


@pytest.fixture(scope="module")
def api(engine):
    return engine


# ---------------------------------------------------------------------------------------------------------------- the sources
# one plain source for every plain shape (the number of dimensions selects the function: one module to compile), one terms source
PLAIN = r"""
__device__ double pchip_loglikelihood(const double *t, double *phi, int D, int nDer, const double *d, long nd)
{
    double l;
    if (D == 1) { const double z = (t[0] - 0.3137) / 0.05; l = -0.5 * z * z - 0.1 * z * z * z * z; }
    else if (D == 2) {                                  // a curved valley under a ripple (not separable): contractions and shrinks
        const double x = 3.0 * t[0] - 1.5, y = 3.0 * t[1] - 0.5;
        l = -(20.0 * (y - x * x) * (y - x * x) + (1.0 - x) * (1.0 - x)) + 2.0 * sin(60.0 * t[0] + 25.0 * t[1]);
    } else if (D == 3) {                                // a Gaussian peaked at 0.97: reflections leave the unit cube
        l = 0.0;
        for (int i = 0; i < 3; ++i) { const double z = (t[i] - 0.97) / (0.1 + 0.02 * i); l -= 0.5 * z * z; }
    } else if (D == 4) {                                // a correlated quadratic about (0.5, 0.7, 0.3, 0.6)
        const double c[4] = { 0.5, 0.7, 0.3, 0.6 };
        l = 0.0;
        for (int i = 0; i < 4; ++i) {
            const double z = (t[i] - c[i]) / 0.08;
            l -= 0.5 * z * z;
            if (i) l -= 0.3 * z * (t[i - 1] - c[i - 1]) / 0.08;
        }
    } else {                                            // separable, every coordinate its own width
        l = 0.0;
        for (int i = 0; i < D; ++i) { const double z = (t[i] - 0.4 - 0.003 * i) / (0.05 + 0.002 * i); l -= 0.5 * z * z; }
    }
    for (int e = 0; e < nDer; ++e) phi[e] = l + e;
    return l;
}
"""
# 70 terms (the lane wraps): a cubic through 70 points, four coefficients
NTERMS = 70
TERMS = r"""
__device__ double pchip_logl_term(const double *t, int D, const double *d, long nd, long i)
{
    const double x = d[i], y = d[70 + i];
    const double r = (y - (t[0] + x * (t[1] + x * (t[2] + x * t[3])))) / 0.05;
    return -0.5 * r * r;
}
__device__ double pchip_logl_finish(double s, const double *t, double *phi, int D, int nDer, const double *d, long nd)
{
    for (int e = 0; e < nDer; ++e) phi[e] = t[e] * s;
    return s;
}
"""


def _terms_data():
    rng = np.random.default_rng(70)
    x = np.linspace(0.0, 1.0, NTERMS)
    y = 0.31 + x * (0.62 + x * (0.27 + x * 0.55)) + 0.05 * rng.standard_normal(NTERMS)
    return np.concatenate([x, y])


@pytest.fixture(scope="module")
def plain(api):
    h = api.source_create(PLAIN)
    yield h
    api.load().pchip_source_destroy(h)


@pytest.fixture(scope="module")
def terms(api):
    h = api.source_create(TERMS, data=_terms_data(), nterms=NTERMS)
    yield h
    api.load().pchip_source_destroy(h)


# ---------------------------------------------------------------------------------------------------------------- the replay
def _det_cm(E):
    """det_cm's elimination (pc_maximise.hip): E[r, c], row swaps on a zero pivot"""
    M = E.copy()
    n = M.shape[0]
    sign = 1.0
    for k in range(n - 1):
        if M[k, k] == 0.0:
            nz = [i for i in range(k + 1, n) if M[i, k] != 0.0]
            if not nz:
                return 0.0
            M[[k, nz[0]]] = M[[nz[0], k]]
            sign = -sign
        for j in range(k + 1, n):
            m = M[j, k] / M[k, k]
            M[j, k + 1:] -= m * M[k, k + 1:]
    d = sign
    for i in range(n):
        d *= M[i, i]
    return d


class Replay:
    """Nelder-Mead by the kernel's rules.  func(cube) -> value of a point INSIDE the unit cube.  Asserts on the way that no termination
    comparison came within a relative 1e-6 of its threshold and that no two values it compared were equal: a knife-edge cannot hide."""

    def __init__(self, func, max_iter=200000):
        self.func, self.max_iter, self.neval, self.niter, self.ntrial = func, max_iter, 0, 0, 0
        self.moves = dict(reflect=0, expand=0, contract=0, shrink=0)

    def f(self, x):
        self.ntrial += 1
        if np.any(x < 0.0) or np.any(x > 1.0):
            return LOGZERO                                        # calculate.f90:36-38: no likelihood call
        self.neval += 1
        return float(self.func(x))

    @staticmethod
    def _far(v, thr):
        assert abs(v - thr) > 1e-6 * abs(thr), f"a termination comparison on the knife-edge: {v!r} against {thr!r}"

    @staticmethod
    def _ne(a, b):
        assert a != b, f"two compared values are equal: {a!r}"

    def order(self, f):
        assert len(set(f.tolist())) == len(f), "two vertices of the simplex have the same value"
        return np.argsort(f, kind="stable")                       # ascending: idx[0] worst, idx[n] best

    def run(self, x, f):
        x, f = np.array(x, dtype=np.float64), np.array(f, dtype=np.float64)
        n = x.shape[1]
        det0 = -1.0
        for _ in range(self.max_iter):
            idx = self.order(f)
            b, w = idx[n], idx[0]
            E = np.array([x[idx[c]] - x[b] for c in range(n)]).T          # column c = edge c
            det1 = abs(_det_cm(E))
            if det0 < 0.0:
                det0 = det1
            assert det0 > 0.0
            self._far(f[b] - f[w], DL)
            ratio = (det1 / det0) ** (1.0 / n)
            self._far(ratio, DL)
            if f[b] - f[w] < DL or ratio < DL:
                break
            s = np.zeros(n)
            for k in range(1, n + 1):
                s = s + x[idx[k]]                                         # in the order of idx
            xo = s / n                                                    # a true division
            xw = x[w].copy()
            xr = xo + (xo - xw)
            fr = self.f(xr)
            self._ne(fr, f[b]); self._ne(fr, f[idx[1]])
            if fr <= f[b] and f[idx[1]] < fr:
                x[w], f[w] = xr, fr
                self.moves["reflect"] += 1
            elif fr > f[b]:
                self.moves["expand"] += 1
                xe = xo + 2.0 * (xr - xo)
                fe = self.f(xe)
                self._ne(fe, fr)
                if fe > fr:
                    x[w], f[w] = xe, fe
                else:
                    x[w], f[w] = xr, fr
            else:
                xc = xo + 0.5 * (xw - xo)
                fc = self.f(xc)
                self._ne(fc, f[w])
                if fc > f[w]:
                    x[w], f[w] = xc, fc
                    self.moves["contract"] += 1
                else:
                    self.moves["shrink"] += 1
                    for j in range(n):
                        v = idx[j]
                        x[v] = x[b] + 0.5 * (x[v] - x[b])
                        f[v] = self.f(x[v])
            self.niter += 1
        idx = self.order(f)
        return x[idx[n]].copy(), float(f[idx[n]])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bit1(v):
    return int(np.float64(v).view(np.uint64))


def _settings(api, D, nDer=0, **kw):
    s = api.Settings()
    api.load().pchip_settings_default(C.byref(s), D, nDer)
    s.logzero = LOGZERO
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _live_of(api, handle, cubes, nDer, theta_of):
    """live rows [cube | theta | phi | birth | logL] of a source at `cubes`, its values from pchip_source_eval"""
    n, D = cubes.shape
    rows = np.zeros((n, 2 * D + nDer + 2))
    th = theta_of(cubes)
    logL, phi = api.source_eval(handle, th, nDer)
    rows[:, :D], rows[:, D:2 * D], rows[:, 2 * D:2 * D + nDer], rows[:, -2], rows[:, -1] = cubes, th, phi, LOGZERO, logL
    return rows


TABLE4 = [("gaussian", (0.5, 0.5)), ("log_uniform", (0.1, 2.0)), ("sorted_uniform", 1, (0.0, 1.0)), ("sorted_uniform", 1, (0.0, 1.0))]
HYPER4 = [2, 3, 0, 1]

# name -> (source, nDims, nDerived, start cubes: centre and spread, seed, number of live rows, table?, max_iter)
REPLAY_CASES = {
    "d1": ("plain", 1, 0, 0.4, 0.1, 101, 5, False, 0),
    "d2_curved_valley": ("plain", 2, 1, 0.5, 0.3, 102, 8, False, 0),
    "d4_plain": ("plain", 4, 2, 0.5, 0.1, 103, 12, False, 0),
    "d4_terms_70": ("terms", 4, 1, 0.45, 0.1, 104, 12, False, 0),
    "d3_peak_at_the_edge": ("plain", 3, 0, 0.93, 0.04, 105, 9, False, 0),
    "d4_permuted_table_sorted_block": ("plain", 4, 0, 0.5, 0.08, 106, 12, True, 0),
    "d64_forty_iterations": ("plain", 64, 0, 0.5, 0.05, 107, 80, False, 40),
}


@pytest.mark.parametrize("name", list(REPLAY_CASES))
def test_replay_exact(api, plain, terms, name):
    """the likelihood leg against the numpy replay: the final vertex bit for bit, the same niter, the same neval"""
    src, D, nDer, centre, spread, seed, n, table, max_iter = REPLAY_CASES[name]
    h = plain if src == "plain" else terms
    rng = np.random.default_rng(seed)
    cubes = np.clip(centre + spread * rng.standard_normal((n, D)), 0.01, 0.99)
    theta_of = (lambda c: api.prior_transform(TABLE4, np.atleast_2d(c), hyper=HYPER4)) if table else (lambda c: np.atleast_2d(c))
    live = _live_of(api, h, cubes, nDer, theta_of)
    s = _settings(api, D, nDer)
    L, P, keep = api.make_problem("source", D, nDer, source=h, prior_table=TABLE4 if table else None, hyper=HYPER4 if table else None)
    run = dict(live=live, live_cluster=np.zeros(n, dtype=np.int32), post_mean=None)
    m = api.maximise_device(s, L, P, run, max_iter=max_iter)
    assert m["status"][0] == 0 and m["cluster"][0] == 0
    # the replay from the same choice of simplex: the D + 1 best rows by stable sort, ascending
    pick = np.argsort(live[:, -1], kind="stable")[-(D + 1):]
    rp = Replay(lambda x: api.source_eval(h, theta_of(x), nDer)[0][0], max_iter or 200000)
    xb, fb = rp.run(live[pick, :D], live[pick, -1])
    print(f"{name}: niter {m['niter'][0]} (replay {rp.niter}), neval {m['neval'][0]} (replay {rp.neval}), max_logl {m['max_logl']!r} (replay {fb!r}), moves {rp.moves}")
    assert m["niter"][0] == rp.niter and m["neval"][0] == rp.neval
    tb = theta_of(xb)[0]
    assert np.array_equal(_bits(m["max_point"][:D]), _bits(tb)), (m["max_point"][:D] - tb)
    lb, pb = api.source_eval(h, tb, nDer)
    assert _bit1(m["max_logl"]) == _bit1(lb[0]) == _bit1(fb)
    assert np.array_equal(_bits(m["max_point"][D:]), _bits(pb[0]))
    if max_iter:
        assert rp.niter == max_iter
    else:
        assert 0 < rp.niter < 20000
    if name == "d2_curved_valley":
        assert rp.moves["contract"] > 0 and rp.moves["shrink"] > 0
    if name == "d3_peak_at_the_edge":
        assert rp.ntrial > rp.neval                  # reflections left the cube: fewer likelihood calls than trial points


# ---------------------------------------------------------------------------------------------------------------- against the host maximiser
def _phi_norm(z):
    return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))


def host_and_device_problem(api, D, table, n=None, seed=7):
    """the built-in Gaussian (mu 0.5, sigma 0.1) under the unit box or under a Gaussian table prior (m 0.3, s 1.0 per parameter): a live
    set around the peak, the host function pointers, the device problem, and the analytic maximum-likelihood and MAP points and values"""
    lib = api.load()
    mu, sig, pm, ps = 0.5, 0.1, 0.3, 1.0
    n = n or 10 * (D + 1)
    rng = np.random.default_rng(seed)
    entries = [("gaussian", (pm, ps))] * D
    lib.polychord_hip_set_gaussian(mu, sig)
    if table:
        api.set_table_prior(entries)
        prior_fn = C.cast(lib.polychord_hip_table_prior, C.c_void_p)
        target = 0.5 + 0.003 * rng.standard_normal((n, D))
        cubes = np.vectorize(_phi_norm)((target - pm) / ps)
        theta = np.array([api.table_prior(c) for c in cubes])
    else:
        lo, hi = np.zeros(D), np.ones(D)
        lib.polychord_hip_set_uniform_prior(D, api.dptr(lo), api.dptr(hi))
        prior_fn = C.cast(lib.polychord_hip_uniform_prior, C.c_void_p)
        cubes = 0.5 + 0.003 * rng.standard_normal((n, D))
        theta = cubes.copy()
    norm = -D * (math.log(sig) + 0.5 * math.log(2 * math.pi))
    live = np.zeros((n, 2 * D + 2))
    live[:, :D], live[:, D:2 * D], live[:, -2] = cubes, theta, LOGZERO
    live[:, -1] = norm - 0.5 * np.sum(((theta - mu) / sig) ** 2, axis=1)
    if table:
        tmap = (mu / sig ** 2 + pm / ps ** 2) / (1 / sig ** 2 + 1 / ps ** 2)
        vmap = norm - 0.5 * D * ((tmap - mu) / sig) ** 2 + D * (-0.5 * math.log(2 * math.pi * ps ** 2) - 0.5 * ((tmap - pm) / ps) ** 2)
    else:
        tmap, vmap = mu, norm
    like_fn = C.cast(lib.polychord_hip_gaussian, C.c_void_p)
    L, P, keep = api.make_problem("gaussian", D, 0, mu=mu, sigma=sig, prior_table=entries if table else None)
    return dict(live=live, cl=np.zeros(n, dtype=np.int32), like_fn=like_fn, prior_fn=prior_fn, L=L, P=P, keep=keep, norm=norm, mu=mu, tmap=tmap, vmap=vmap)


def host_distance(api, D, table):
    """the host maximiser's own distance from the analytic MAP: (largest coordinate distance, distance in value)"""
    q = host_and_device_problem(api, D, table)
    m = api.maximise_values(q["like_fn"], q["prior_fn"], D, 0, LOGZERO, q["live"], q["cl"])
    return float(np.max(np.abs(m["post_point"][:D] - q["tmap"]))), abs(m["max_post"] - q["vmap"]), m


# The host path's own distance from the analytic MAP, measured on the CPU with host_distance (pchip_maximise_values needs no device):
# (nDims, table) -> (largest coordinate distance, distance in value).  The device gets twice that: device and host differ by rounding
# only, the margin pays for one flipped decision.
# The live set is the problem's to choose, and it is drawn like the final live set of a run: 10 (D + 1) rows within 0.03 sigma of the peak,
# under a prior wide enough (m 0.3, s 1.0: the MAP 0.002 from the peak) that the MAP lies inside it.  A 20-D Nelder-Mead that has to TRAVEL
# is erratic on the host path itself (rows 0.3 sigma wide, s 0.2: over four seeds it ended between 2e-5 and 1e-2 of the peak's logL after
# 1000 to 6000 iterations); from a set like this one the host ends within 5e-5 and 150 iterations on the likelihood leg for every seed tried.
HOST_MAP_DISTANCE = {
    (4, False): (8.736e-04, 4.809e-05),
    (20, False): (2.946e-04, 2.280e-05),
    (4, True): (2.121e-04, 1.274e-05),
    (20, True): (9.175e-04, 1.706e-04),
}


@pytest.mark.parametrize("D,table", [(4, False), (20, False), (4, True), (20, True)])
def test_against_the_host_maximiser(api, tmp_path, D, table):
    """built-in Gaussians, sigma 0.1, under the box and under a Gaussian table prior: the likelihood leg within the bounds
    test_maximiser_on_the_host holds the host path to (1e-4 in logL, 2e-3 in a coordinate of the analytic peak); the posterior leg within
    TWICE the host path's own measured distance from the analytic MAP (mu / sigma^2 + m / s^2) / (1 / sigma^2 + 1 / s^2) and from its value.
    Measured host figures (largest coordinate distance, distance in value) on this live set: 4-D box 8.736e-04, 4.809e-05; 20-D box
    2.946e-04, 2.280e-05; 4-D table 2.121e-04, 1.274e-05; 20-D table 9.175e-04, 1.706e-04 (HOST_MAP_DISTANCE; the test measures them again
    and prints both)."""
    q = host_and_device_problem(api, D, table)
    s = _settings(api, D, 0)
    path = tmp_path / "dev.maximum"
    m = api.maximise_device(s, q["L"], q["P"], dict(live=q["live"], live_cluster=q["cl"], post_mean=np.full(D, 0.5)), write=path)
    hc, hv, mh = host_distance(api, D, table)
    dc, dv = float(np.max(np.abs(m["post_point"][:D] - q["tmap"]))), abs(m["max_post"] - q["vmap"])
    print(f"D={D} table={table}: likelihood leg |dlogL| {abs(m['max_logl'] - q['norm']):.3e} max|dtheta| {np.max(np.abs(m['max_point'][:D] - q['mu'])):.3e}; "
          f"posterior leg device ({dc:.3e}, {dv:.3e}) host now ({hc:.3e}, {hv:.3e}) host recorded {HOST_MAP_DISTANCE[(D, table)]}; "
          f"niter {m['niter']} neval {m['neval']} (host {mh['niter']} {mh['neval']})")
    assert m["status"] == [0, 0]
    assert abs(m["max_logl"] - q["norm"]) < 1e-4 and np.all(np.abs(m["max_point"][:D] - q["mu"]) < 2e-3)
    bc, bv = HOST_MAP_DISTANCE[(D, table)]
    assert dc <= 2 * bc and dv <= 2 * bv
    # the file parses in the reference layout (as test_maximiser_reproduces_the_reference reads it)
    lines = path.read_text().splitlines()
    num = lambda k: np.array([float(x) for x in lines[k].split()])
    assert lines[0] == "Maximum LogLikelihood:" and lines[2] == "Maximum Likelihood point:" and lines[5] == "Maximum Posterior:"
    assert lines[7] == "Maximum Likelihood at posterior:" and lines[9] == "Maximum Posterior point:" and lines[12] == "LogLikelihood(mean):"
    assert abs(num(1)[0] - m["max_logl"]) <= 1e-14 * abs(m["max_logl"]) + 1e-300 and np.allclose(num(3), m["max_point"], rtol=1e-14, atol=0)
    assert np.allclose(num(6)[0], m["max_post"], rtol=1e-14) and np.allclose(num(8)[0], m["logl_at_post"], rtol=1e-14)
    assert np.allclose(num(10), m["post_point"], rtol=1e-14, atol=0) and len(lines[1]) == 24
    assert abs(num(13)[0] - q["norm"]) < 1e-12 and np.allclose(num(15), 0.5)


def test_the_mean_row_is_the_host_maximisers_with_derived_parameters(api, tmp_path):
    """nDerived = 2 (the built-in Gaussian's radius and log ball volume): the `mean point:` row the one writer writes for the device result is
    the row it writes for the host path -- the mean theta as given and phi evaluated THERE, whatever phi the posterior mean carried in.
    theta exactly; phi to 1e-12 (absolute and relative): host and device sum four squares in another order and form the log volume
    differently, a few ulp of values of order 0.1 to 10."""
    D, nDer, mu, sig = 4, 2, 0.5, 0.1
    lib = api.load()
    lib.polychord_hip_set_gaussian(mu, sig)
    lo, hi = np.zeros(D), np.ones(D)
    lib.polychord_hip_set_uniform_prior(D, api.dptr(lo), api.dptr(hi))
    like_fn, prior_fn = C.cast(lib.polychord_hip_gaussian, C.c_void_p), C.cast(lib.polychord_hip_uniform_prior, C.c_void_p)
    n = 10 * (D + 1)
    cubes = 0.5 + 0.003 * np.random.default_rng(8).standard_normal((n, D))
    live = np.zeros((n, 2 * D + nDer + 2))
    live[:, :D], live[:, D:2 * D], live[:, -2] = cubes, cubes, LOGZERO
    live[:, -1] = -D * (math.log(sig) + 0.5 * math.log(2 * math.pi)) - 0.5 * np.sum(((cubes - mu) / sig) ** 2, axis=1)
    cl = np.zeros(n, dtype=np.int32)
    mean = np.array([0.47, 0.52, 0.55, 0.44, 99.0, -99.0])          # a phi no point has: it must not reach the row
    L, P, keep = api.make_problem("gaussian", D, nDer, mu=mu, sigma=sig)
    md = api.maximise_device(_settings(api, D, nDer), L, P, dict(live=live, live_cluster=cl, post_mean=mean), write=tmp_path / "dev.maximum")
    mh = api.maximise_values(like_fn, prior_fn, D, nDer, LOGZERO, live, cl, post_mean=mean, write=tmp_path / "host.maximum")
    r = math.sqrt(sum((t - mu) ** 2 for t in mean[:D]))
    want = [r, D * math.log(r) + 0.5 * D * math.log(math.pi) - math.lgamma(1.0 + D / 2.0)]
    for m in (md, mh):
        assert m["status"] == [0, 0] and np.array_equal(m["mean_point"][:D], mean[:D])
        assert np.allclose(m["mean_point"][D:], want, rtol=1e-12, atol=1e-12)
    assert np.allclose(md["mean_point"][D:], mh["mean_point"][D:], rtol=1e-12, atol=1e-12) and abs(md["logl_mean"] - mh["logl_mean"]) < 1e-12
    rows = [[float(x) for x in (tmp_path / f).read_text().splitlines()[15].split()] for f in ("dev.maximum", "host.maximum")]
    assert len(rows[0]) == D + nDer and np.allclose(rows[0], rows[1], rtol=1e-12, atol=1e-12) and rows[0][:D] == rows[1][:D]


# ---------------------------------------------------------------------------------------------------------------- after a real run
def test_after_a_real_run(api, terms):
    """pchip_run of the terms-form fit, then maximise_device on its final live set"""
    D, nDer = 4, 1
    s = _settings(api, D, nDer, nlive=200, num_repeats=8, seed=11, do_clustering=0)
    L, P, keep = api.make_problem("source", D, nDer, source=terms)
    g = api.run(s, L, P)
    m = api.maximise_device(s, L, P, g)
    assert m["status"] == [0, 0]
    assert m["max_logl"] >= g["live"][:, -1].max()
    # the mean point is [mean theta | phi AT the mean theta], as loglikelihood(mean) leaves it (maximiser.F90:77-80): not the posterior mean of phi
    lm, pm = api.source_eval(terms, g["post_mean"][:D], nDer)
    assert _bit1(m["logl_mean"]) == _bit1(lm[0]) and np.array_equal(m["mean_point"][:D], g["post_mean"][:D])
    assert np.array_equal(_bits(m["mean_point"][D:]), _bits(pm[0])) and not np.array_equal(m["mean_point"][D:], g["post_mean"][D:])
    lp, pp = api.source_eval(terms, m["max_point"][:D], nDer)
    assert _bit1(m["max_logl"]) == _bit1(lp[0]) and np.array_equal(_bits(m["max_point"][D:]), _bits(pp[0]))
    lq, pq = api.source_eval(terms, m["post_point"][:D], nDer)
    assert _bit1(m["logl_at_post"]) == _bit1(lq[0]) and np.array_equal(_bits(m["post_point"][D:]), _bits(pq[0]))
    assert abs(m["max_post"] - m["logl_at_post"]) < 1e-9          # the unit box


# ---------------------------------------------------------------------------------------------------------------- many = solo
def _same(a, b):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        elif isinstance(a[k], float):
            assert _bit1(a[k]) == _bit1(b[k]), k
        else:
            assert a[k] == b[k], k


def test_many_is_solo(api):
    """four seeds through run_in_step(..., maximise=True): every run's maximum is, bit for bit, maximise_device on that run alone"""
    from polychordlite_amd import repeats
    D, nDer = 4, 2
    s = _settings(api, D, nDer, nlive=60, num_repeats=8, do_clustering=0)
    L, P, keep = api.make_problem("gaussian", D, nDer)
    merged, runs = repeats.run_in_step(s, L, P, [3, 4, 5, 6], max_in_flight=4, maximise=True)
    _, plain_runs = repeats.run_in_step(s, L, P, [3], max_in_flight=4)
    assert "maximum" not in plain_runs[0]                           # the default leaves the dicts what they were
    for r in runs:
        assert r["maximum"]["status"] == [0, 0] and min(r["maximum"]["niter"]) > 0
        _same(r["maximum"], api.maximise_device(s, L, P, r))
    assert len({r["maximum"]["max_logl"] for r in runs}) > 1


def test_two_clusters_take_the_better(api):
    """a twin-Gaussian live set in two clusters, one per mode: the cluster whose best row is higher gives both simplexes"""
    D = 4
    rng = np.random.default_rng(21)
    a = np.array([-0.5, -0.5, 0.0, 0.0]) + 0.06 * rng.standard_normal((15, D))      # farther from its mode
    b = np.array([0.5, 0.5, 0.0, 0.0]) + 0.02 * rng.standard_normal((11, D))
    theta = np.vstack([a, b])
    s = _settings(api, D, 0)
    L, P, keep = api.make_problem("twin_gaussian", D, 0, lo=-1.0, hi=1.0, sigma=0.1)
    norm = -D * (math.log(0.1) + 0.5 * math.log(2 * math.pi))
    l1 = norm - 0.5 * np.sum(((theta - [-0.5, -0.5, 0, 0]) / 0.1) ** 2, axis=1)
    l2 = norm - 0.5 * np.sum(((theta - [0.5, 0.5, 0, 0]) / 0.1) ** 2, axis=1)
    live = np.zeros((26, 2 * D + 2))
    live[:, :D], live[:, D:2 * D], live[:, -1] = (theta + 1.0) / 2.0, theta, np.logaddexp(l1, l2) - math.log(2.0)
    cl = np.array([0] * 15 + [1] * 11, dtype=np.int32)
    assert live[15:, -1].max() > live[:15, -1].max()
    m = api.maximise_device(s, L, P, dict(live=live, live_cluster=cl, post_mean=None))
    assert m["status"] == [0, 0] and m["cluster"] == [1, 1]
    assert np.all(np.abs(m["max_point"] - [0.5, 0.5, 0.0, 0.0]) < 2e-3) and abs(m["max_logl"] - (norm - math.log(2.0))) < 1e-4
    # the box is [-1, 1]: dX/dtheta = 2^-D
    assert abs(m["max_post"] - m["logl_at_post"] + D * math.log(2.0)) < 1e-6
    # ... and a live set without a simplex: status 1 on both legs, a result all the same
    m0 = api.maximise_device(s, L, P, dict(live=live[:4], live_cluster=np.zeros(4, dtype=np.int32), post_mean=None))
    assert m0["status"] == [1, 1] and m0["niter"] == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- the run-time module
def test_ablate_bit_15_is_the_static_kernel(api):
    """a built-in through the run-time compiled module (settings.ablate bit 15) gives the static kernels' result bit for bit"""
    D = 4
    q = host_and_device_problem(api, D, True)
    run = dict(live=q["live"], live_cluster=q["cl"], post_mean=np.full(D, 0.45))
    a = api.maximise_device(_settings(api, D, 0), q["L"], q["P"], run)
    b = api.maximise_device(_settings(api, D, 0, ablate=1 << 15), q["L"], q["P"], run)
    assert a["status"] == [0, 0] and min(a["niter"]) > 0
    _same(a, b)


def test_kind_3_without_a_prior_fails_as_pchip_run_does(api, plain):
    D = 4
    s = _settings(api, D, 0)
    L, P, keep = api.make_problem("source", D, 0, source=plain, prior_source=True)
    live = _live_of(api, plain, np.random.default_rng(1).uniform(0.3, 0.7, (8, D)), 0, np.atleast_2d)
    with pytest.raises(RuntimeError) as e:
        api.maximise_device(s, L, P, dict(live=live, live_cluster=np.zeros(8, dtype=np.int32), post_mean=None))
    assert "code 1" in str(e.value) and "defines no pchip_prior_param" in str(e.value) and "pchip_source_create_prior" in str(e.value)


# a source prior with a known Jacobian: theta_i = a_i + b_i cube_i + 0.25 cube_{i-1}, lower triangular, det = b_0 b_1 b_2; the likelihood a
# Gaussian of width 0.1 about data[2 D ..]
PRIOR_SRC = r"""
__device__ double pchip_loglikelihood(const double *t, double *phi, int D, int nDer, const double *d, long nd)
{
    double l = 0.0;
    for (int i = 0; i < D; ++i) { const double z = (t[i] - d[2 * D + i]) / 0.1; l -= 0.5 * z * z; }
    return l;
}
__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata)
{
    return data[i] + data[nDims + i] * cube[i] + (i ? 0.25 * cube[i - 1] : 0.0);
}
"""


def test_a_source_prior_with_a_known_jacobian(api):
    """prior kind 3 through k_max_rank and k_maximise (pc_max_dxdtheta over the handle's own pchip_prior_param): the prior is affine, so its
    density in theta is the constant 1 / (b_0 b_1 b_2) and max_post - logl_at_post = -sum log b_i.  Bound 1e-8: an entry of the finite
    difference Jacobian, theta(cube + dx) - theta(cube) with dx = 1e-5, is of size b dx >= 5e-6 and carries the rounding of thetas up to 4
    (at most 2 * 4.4e-16) and of cube + dx (1.1e-16 b), a relative 2e-10 at most; three diagonal entries and the logs add to under 1e-9.
    The likelihood leg: the bounds test_maximiser_on_the_host holds the host path to, 1e-4 in logL and 2e-3 in a coordinate."""
    D = 3
    a, b, c0 = np.array([-1.0, 0.5, 2.0]), np.array([0.5, 2.0, 1.25]), np.array([0.4, 0.5, 0.6])
    peak = a + b * c0 + 0.25 * np.array([0.0, c0[0], c0[1]])
    h = api.source_create(PRIOR_SRC, data=np.concatenate([a, b, peak]), prior=True)
    try:
        n = 12
        cubes = c0 + 0.003 * np.random.default_rng(33).standard_normal((n, D))
        live = _live_of(api, h, cubes, 0, lambda c: api.source_prior_eval(h, np.atleast_2d(c)))
        L, P, keep = api.make_problem("source", D, 0, source=h, prior_source=True)
        m = api.maximise_device(_settings(api, D, 0), L, P, dict(live=live, live_cluster=np.zeros(n, dtype=np.int32), post_mean=None))
        print(f"source prior: max_logl {m['max_logl']!r} max_post - logl_at_post {m['max_post'] - m['logl_at_post']!r} (analytic {-np.sum(np.log(b))!r}) niter {m['niter']}")
        assert m["status"] == [0, 0] and min(m["niter"]) > 0
        assert abs(m["max_logl"]) < 1e-4 and np.all(np.abs(m["max_point"][:D] - peak) < 2e-3)
        assert abs(m["max_post"] - m["logl_at_post"] + np.sum(np.log(b))) < 1e-8
        assert abs(m["logl_at_post"]) < 1e-4 and np.all(np.abs(m["post_point"][:D] - peak) < 2e-3)      # a constant density: the MAP is the peak
    finally:
        api.load().pchip_source_destroy(h)
