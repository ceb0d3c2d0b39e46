"""The two numerical results of an update -- the covariance of a cluster's live and phantom cube coordinates and its Cholesky factor
(S.cov, S.chol) -- against a long double reference, through the kernel-level door pchip_update_factors, which runs the launchers of
Engine::do_update's non-deferred branch on given rows:
  path 1  the fused update (pc_update.hip): one-pass moments about a shift on the fp64 matrix cores (k_upd_gather<NT>, pool and compacting
          mode; k_upd_chain<NT> under settings.ablate bit 16), k_upd_fold, then upd_final_stage<8|16|24|32> below 32 dimensions,
          k_upd_final_w + k_chol_blocked<2..8> (+ k_cov_final_chol when it says chol_suspect) from 32 on;
  path 0  the general steps (pc_update_steps.hip): clean, k_cov_mean_partial / k_cov_partial (plain below 32 dimensions, matrix cores from 32),
          k_fold_partials, k_cov_final_chol in its three memory layouts (both matrices in LDS up to 101, L alone 102...143, in HBM from 144).

THE REFERENCE is written out here: per cluster the mean and the centred products divided by n (population normalisation,
run_time_info.f90:601-641) in np.longdouble; the rows that count are the cluster's live rows and its phantoms with !(logL < threshold).

THE BOUNDS are derived, not tuned.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.).
  covariance, steps   |cov - ref|_ab <= gamma_{n+8} sum_i |c_ia c_ib| / n + eps_a m_b + eps_b m_a + eps_a eps_b,   c = x - mu in long
                      double, eps_a = gamma_n mean|x_a| (the mean's own summation bound), m_a = mean|c_a|: section 4.2 composed over mean,
                      centring, products and division; any summation order, any use of FMA; + 8 for the handful of further roundings.
  covariance, fused   with y = x - shift, d = mean(y):  |cov - ref|_ab <= gamma_{n+8} (sum_i |y_ia y_ib| / n + |d_a d_b|).  It grows with
                      the distance of the shift from the mean: that growth is the claim under test.
  factor              with A the device's OWN covariance:  |L L^T - A|_ab <= gamma_{D+1} (|L| |L|^T)_ab, in long double (Theorem 10.3: any
                      order of the inner sums, blocked or not).  With the covariance bound a lower triangular L of positive diagonal is pinned.
  structure           cov exactly symmetric, the strict upper triangle of chol exactly 0.0, diagonals > 0, everything finite, the rows
                      counted = the reference's count, new shift = shift + mean(y) within the mean's bound (and the rounding of that sum).
(The sums |c|^T |c| of the bounds themselves are taken in fp64 and enlarged by 1e-9, a thousand times their own gamma_n.)

On the CPU the same generator and the same bounds are applied to the oracle's pc_covmat + pc_cholesky (plain fp64, the reference's order) and
to a one-pass fp64 evaluation about a shift: the bounds are attainable and the harness is right before a GPU sees it.
Every case prints its worst error / bound ratio for covariance and factor (pytest -s), and the largest error of a covariance element in
units of u sd_a sd_b.  Seen on an MI355X: covariance <= 0.11 (fused), <= 0.009 (steps); factor <= 0.38 (upd_final_stage<8>), 0.24 (<24>),
0.13 (k_chol_blocked), 0.47 (k_cov_final_chol, nDims 2); on the CPU <= 0.015 and <= 0.21 (DESIGN.md section 5a has the table)."""
import numpy as np
import pytest

from tests import oracle_api as orc

LD = np.longdouble
U = LD(2) ** -53
NO_POOL, CHAIN = 1 << 1, 1 << 16


def gam(k):
    k = LD(k)
    return k * U / (1 - k * U)


def _need_long_double():
    assert np.finfo(LD).nmant >= 63, ("np.longdouble has a %d-bit mantissa on this machine: the reference would be fp64 against fp64 "
                                      "(an x87 long double, 64 bits, is what these bounds are checked against)" % (np.finfo(LD).nmant + 1))


# ---------------------------------------------------------------------------------------------------------------- cases
def cloud(rng, n, D, centre, sigma, kappa):
    """centre + sigma (Gaussian of a random orthogonal basis, covariance eigenvalues geometric from 1 to 1 / kappa), clipped into (0, 1)"""
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = np.asarray(kappa, dtype=np.float64) ** (-np.arange(D) / max(D - 1, 1))
    x = centre + sigma * (rng.standard_normal((n, D)) * np.sqrt(lam)) @ Q.T
    return np.clip(x, 1e-12, 1.0 - 1e-12)


class Case:
    """live [nlive][D] + cluster, phantom [nph][D] + logL + cluster (-1: a hole), threshold per cluster; rows(c): the rows that count"""

    def __init__(self, live, lc, ph, pl, pc, thr):
        self.live, self.lc, self.ph, self.pl, self.pc, self.thr = live, lc.astype(np.int32), ph, pl, pc.astype(np.int32), thr
        self.D, self.nc = live.shape[1], len(thr)
        self._ref = {}

    def rows(self, c):
        keep = (self.pc == c) & ~(self.pl < self.thr[np.maximum(self.pc, 0)])
        return np.vstack([self.live[self.lc == c], self.ph[keep]])

    def ref(self, c):
        """(rows, mean, centred rows, covariance) of cluster c in long double, computed once"""
        if c not in self._ref:
            x = self.rows(c)
            xl = x.astype(LD)
            mu = xl.sum(0) / len(x)
            cen = xl - mu
            self._ref[c] = (x, mu, cen, (cen.T @ cen) / len(x))
        return self._ref[c]


def build(seed, D, clusters, nlive, n_below=0, n_holes=0, pin=None):
    """clusters: (rows that count, centre, sigma, kappa) each; nlive of all those rows are live points, the rest phantoms at or above their
    cluster's threshold (some exactly at it); n_below more phantoms below it and n_holes rows of no cluster, both with coordinates from
    all over the cube so that a row counted by mistake shows; labels interleaved at random.  pin: a coordinate that is 0.5 in every row"""
    rng = np.random.default_rng(seed)
    nc = len(clusters)
    x = np.vstack([cloud(rng, n, D, ce, sg, ka) for n, ce, sg, ka in clusters])
    lab = np.concatenate([np.full(n, c) for c, (n, _, _, _) in enumerate(clusters)])
    p = rng.permutation(len(x))
    x, lab = x[p], lab[p]
    thr = rng.uniform(-5.0, 5.0, nc)
    nphc = len(x) - nlive
    assert 1 <= nlive <= len(x)
    pl = thr[lab[nlive:]] + np.where(rng.random(nphc) < 0.1, 0.0, rng.exponential(1.0, nphc))      # (logL == threshold counts)
    cb = rng.integers(0, nc, n_below)
    ph = np.vstack([x[nlive:], rng.random((n_below, D)), rng.random((n_holes, D))])
    pl = np.concatenate([pl, thr[cb] - 1e-9 - rng.exponential(1.0, n_below), np.full(n_holes, 100.0)])
    pc = np.concatenate([lab[nlive:], cb, np.full(n_holes, -1)])
    q = rng.permutation(len(ph))
    live, ph = np.ascontiguousarray(x[:nlive]), np.ascontiguousarray(ph[q])
    if pin is not None:
        live[:, pin] = 0.5; ph[:, pin] = 0.5
    return Case(live, lab[:nlive], ph, pl[q], pc[q], thr)


# ---------------------------------------------------------------------------------------------------------------- bounds
def _ratio(err, bound):
    """worst |err| / bound; an entry whose bound is zero must be exact"""
    err = np.asarray(err, dtype=LD); bound = np.asarray(bound, dtype=LD)
    assert np.all(np.isfinite(err.astype(np.float64))), "not finite"
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def _abs_gram(a, n):
    a = np.abs(a).astype(np.float64)
    return ((a.T @ a) / n * (1.0 + 1e-9)).astype(LD)


def cov_ratio_steps(cov, x, cen, ref):
    n = len(x)
    eps = gam(n) * np.abs(x).astype(LD).mean(0)
    m = np.abs(cen).mean(0)
    bound = gam(n + 8) * _abs_gram(cen, n) + np.outer(eps, m) + np.outer(m, eps) + np.outer(eps, eps)
    return _ratio(np.abs(cov.astype(LD) - ref), bound)


def cov_ratio_fused(cov, x, shift, ref):
    n = len(x)
    y = x.astype(LD) - np.asarray(shift, dtype=np.float64).astype(LD)
    d = y.sum(0) / n
    bound = gam(n + 8) * (_abs_gram(y, n) + np.abs(np.outer(d, d)))
    return _ratio(np.abs(cov.astype(LD) - ref), bound)


def shift_ratio(new, x, shift):
    """new shift = shift + mean(x - shift): the mean's bound gamma_n mean|y_a| (+ 2 for the roundings of y and of the division) and the rounding
    of the sum itself"""
    n = len(x)
    y = x.astype(LD) - np.asarray(shift, dtype=np.float64).astype(LD)
    want = np.asarray(shift, dtype=np.float64).astype(LD) + y.sum(0) / n
    return _ratio(np.abs(new.astype(LD) - want), gam(n + 2) * np.abs(y).mean(0) + U * np.abs(want))


def factor_ratio(A, L):
    Al, Ll = A.astype(LD), L.astype(LD)
    return _ratio(np.abs(Ll @ Ll.T - Al), gam(len(A) + 1) * (np.abs(Ll) @ np.abs(Ll).T))


def check_structure(cov, chol):
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(chol)), "not finite"
    assert np.array_equal(cov, cov.T), "cov is not exactly symmetric"
    assert np.all(np.triu(chol, 1) == 0.0), "the strict upper triangle of chol is not exactly 0.0"


def factor_kind(cov, chol):
    """'factor' (a Cholesky factor within the backward bound), 'identity' (sqrt(trace) I within gamma_D, off-diagonals exactly 0: the fallback of
    utils.F90:633-638) or 'zero' (all zeros, the fallback of a zero matrix); fails on anything else.  Returns (kind, ratio)"""
    D = len(cov)
    check_structure(cov, chol)
    dg = np.diag(chol)
    if np.all(chol == 0.0):
        assert np.all(np.diag(cov) == 0.0), "a zero factor of a covariance that is not zero"
        return "zero", 0.0
    if D > 1 and np.all(chol == np.diag(dg)) and np.all(dg == dg[0]):
        want = np.sqrt(np.diag(cov).astype(LD).sum())
        r = _ratio(abs(LD(dg[0]) - want), gam(D) * want)
        assert r <= 1.0, "scaled identity off sqrt(trace): ratio %.3g" % r
        return "identity", r
    assert np.all(dg > 0.0), "a diagonal element of the factor is not positive (a partial factor?)"
    r = factor_ratio(cov, chol)
    assert r <= 1.0, "factor outside the backward bound: ratio %.3g" % r
    return "factor", r


def check_cluster(tag, case, c, cov, chol, count, path, shift=None, want="factor"):
    """all assertions for one cluster; prints and returns (covariance ratio, factor ratio, kind of factor)"""
    x, mu, cen, ref = case.ref(c)
    assert count == len(x), "%s: %d rows counted, the reference counts %d" % (tag, count, len(x))
    check_structure(cov, chol)
    rc = cov_ratio_fused(cov, x, shift, ref) if path == 1 else cov_ratio_steps(cov, x, cen, ref)
    kind, rf = factor_kind(cov, chol)
    sd = np.sqrt(np.diag(ref))
    scale = np.outer(sd, sd)
    eu = float(np.max(np.where(scale > 0, np.abs(cov.astype(LD) - ref) / np.where(scale > 0, scale, 1), 0)) / U)      # (printed, not asserted)
    print("UF %s n=%d cov_ratio=%.4g chol_ratio=%.4g chol=%s cov_err=%.3g u sd_a sd_b" % (tag, len(x), rc, rf, kind, eu))
    assert rc <= 1.0, "%s: covariance outside its bound, ratio %.3g" % (tag, rc)
    if want is not None:
        assert kind == want, "%s: the factor is '%s', expected '%s'" % (tag, kind, want)
    return rc, rf, kind


# ---------------------------------------------------------------------------------------------------------------- CPU: the oracle
def _oracle_cluster(case, c):
    lib = orc.load()
    D = case.D
    live = np.ascontiguousarray(case.live[case.lc == c])
    keep = (case.pc == c) & ~(case.pl < case.thr[np.maximum(case.pc, 0)])
    ph = np.ascontiguousarray(case.ph[keep])
    cov = np.zeros((D, D)); L = np.zeros((D, D))
    dummy = np.zeros(1)
    lib.pc_covmat(orc.dptr(live if len(live) else dummy), len(live), orc.dptr(ph if len(ph) else dummy), len(ph), D, D, orc.dptr(cov))
    lib.pc_cholesky(orc.dptr(cov), D, orc.dptr(L))
    return cov, L, len(live) + len(ph)


def _one_pass_fp64(x, shift):
    """the fused update's arithmetic in plain fp64: moments about the shift, cov = M2 / n - d d^T"""
    y = x - shift
    n = len(x)
    d = y.sum(0) / n
    cov = (y.T @ y) / n - np.outer(d, d)
    return np.triu(cov) + np.triu(cov, 1).T, shift + d          # (the upper triangle mirrored, as the kernels store it)


CONDITIONING = [(0.5, 0.05, 1.0), (0.9, 1e-5, 1e6), (0.7, 1e-3, 1e8)]
SHIFT_SIGMAS = (0.0, 0.5, 3.0, 30.0)


@pytest.mark.parametrize("D", [1, 2, 17, 33, 100, 128])
def test_cpu_oracle_meets_the_bounds(D):
    _need_long_double()
    n = max(300, 3 * D)
    case = build(100 + D, D, [(n, 0.45, 0.05, 100.0)], nlive=n // 3, n_below=n // 4, n_holes=n // 3)
    cov, L, cnt = _oracle_cluster(case, 0)
    check_cluster("oracle steps D=%d" % D, case, 0, cov, L, cnt, 0)
    # three clusters, labels interleaved: most of the rows, nDims + 5, one
    case = build(200 + D, D, [(n, 0.3, 0.05, 10.0), (D + 5, 0.7, 0.02, 10.0), (1, 0.5, 0.1, 1.0)], nlive=n // 2, n_below=n // 4, n_holes=n // 5)
    for c, want in ((0, "factor"), (1, "factor"), (2, "zero")):
        cov, L, cnt = _oracle_cluster(case, c)
        check_cluster("oracle steps D=%d cluster %d" % (D, c), case, c, cov, L, cnt, 0, want=want)
        if c == 2:
            assert np.all(cov == 0.0)


@pytest.mark.parametrize("D", [20, 100])
@pytest.mark.parametrize("centre,sigma,kappa", CONDITIONING)
def test_cpu_conditioning_two_pass_and_one_pass(D, centre, sigma, kappa):
    _need_long_double()
    case = build(300 + D, D, [(2000, centre, sigma, kappa)], nlive=500)
    cov, L, cnt = _oracle_cluster(case, 0)
    check_cluster("oracle steps D=%d centre=%g sigma=%g kappa=%g" % (D, centre, sigma, kappa), case, 0, cov, L, cnt, 0)
    x, mu, cen, ref = case.ref(0)
    for k in SHIFT_SIGMAS:
        shift = mu.astype(np.float64) + k * sigma
        cov1, new = _one_pass_fp64(x, shift)
        L1 = np.zeros((D, D))
        orc.load().pc_cholesky(orc.dptr(np.ascontiguousarray(cov1)), D, orc.dptr(L1))
        tag = "fp64 one-pass D=%d centre=%g sigma=%g kappa=%g shift=mean+%g sigma" % (D, centre, sigma, kappa, k)
        check_cluster(tag, case, 0, cov1, L1, len(x), 1, shift=shift)
        assert shift_ratio(new, x, shift) <= 1.0


@pytest.mark.parametrize("D", [12, 40, 120, 150])
def test_cpu_fallbacks(D):
    _need_long_double()
    n = 2 * D + 30
    # (i) one coordinate pinned at 0.5: its variance is exactly 0 in any order of summation -> sqrt(trace) I
    case = build(400 + D, D, [(n, 0.5, 0.05, 10.0)], nlive=n // 2, n_below=9, n_holes=9, pin=D // 3)
    cov, L, cnt = _oracle_cluster(case, 0)
    assert np.all(cov[D // 3] == 0.0)
    check_cluster("oracle pinned D=%d" % D, case, 0, cov, L, cnt, 0, want="identity")
    # (ii) a cluster of one row
    case = build(500 + D, D, [(1, 0.4, 0.05, 1.0)], nlive=1, n_below=5, n_holes=5)
    cov, L, cnt = _oracle_cluster(case, 0)
    assert np.all(cov == 0.0)
    check_cluster("oracle one row D=%d" % D, case, 0, cov, L, cnt, 0, want="zero")
    # (iii) n <= nDims: round-off decides between a factor and the scaled identity
    for m in (D, max(2, D // 2)):
        case = build(600 + D + m, D, [(m, 0.5, 0.05, 10.0)], nlive=max(1, m // 2), n_below=5, n_holes=5)
        cov, L, cnt = _oracle_cluster(case, 0)
        rc, rf, kind = check_cluster("oracle rank-deficient D=%d n=%d" % (D, m), case, 0, cov, L, cnt, 0, want=None)
        assert kind in ("factor", "identity")


# ---------------------------------------------------------------------------------------------------------------- GPU
def cov_rows(D):
    """rows per chunk of the general covariance kernels (pc_update_steps.hip cov_rows: the centred tile [rows][stride] within 120 KB of LDS)"""
    ts = ((D + 15) & ~15) + 1 if D >= 32 else D + 1
    r = 256
    while r > 8 and 8 * r * ts + 4 * r > 120 * 1024:
        r >>= 1
    return r


def fused_kernel(D, suspect):
    if D < 32:
        return "upd_final_stage<%d>" % (8 if D <= 8 else 16 if D <= 16 else 24 if D <= 24 else 32)
    return "k_cov_final_chol(behind k_chol_blocked<%d>)" % ((D + 15) // 16) if suspect else "k_chol_blocked<%d>" % ((D + 15) // 16)


def steps_kernel(D):
    return "k_cov_final_chol[%s]" % ("A+L in LDS" if D <= 101 else "L in LDS" if D <= 143 else "HBM")


def run_fused(api, tag, case, ablate=0, shift=None, want="factor"):
    g = api.update_factors(case.live, case.lc, case.ph, case.pl, case.pc, case.thr, 1, shift=shift, ablate=ablate)
    sh = np.full(case.D, 0.5) if shift is None else shift
    mode = "chain" if ablate & CHAIN else "compact" if ablate & NO_POOL else "pool"
    tag = "fused/%s %s D=%d %s" % (mode, fused_kernel(case.D, g["chol_suspect"]), case.D, tag)
    g["ratios"] = check_cluster(tag, case, 0, g["cov"][0], g["chol"][0], g["count"][0], 1, shift=sh, want=want)
    x = case.ref(0)[0]
    rs = shift_ratio(g["shift"], x, sh)
    assert rs <= 1.0, "%s: new shift off shift + mean, ratio %.3g" % (tag, rs)
    if case.D < 32:
        assert g["chol_suspect"] == 0
    return g


def run_steps(api, tag, case, want=None):
    g = api.update_factors(case.live, case.lc, case.ph, case.pl, case.pc, case.thr, 0)
    assert g["chol_suspect"] == 0
    g["ratios"] = []
    for c in range(case.nc):
        n = len(case.rows(c))
        w = (want[c] if want else ("zero" if n == 1 else "factor"))
        t = "steps %s D=%d nc=%d cluster %d %s" % (steps_kernel(case.D), case.D, case.nc, c, tag)
        g["ratios"].append(check_cluster(t, case, c, g["cov"][c], g["chol"][c], g["count"][c], 0, want=w))
    return g


def _same_bits(a, b):
    for k in ("cov", "chol", "shift", "count"):
        assert np.array_equal(a[k], b[k]), "the chain's %s differs from the five launches'" % k
    assert a["chol_suspect"] == b["chol_suspect"]


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 2, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 47, 48, 63, 64, 65, 100, 127, 128])
def test_fused_every_final_stage_and_tile_edge(engine, D):
    """nDims at every bound of the final stage (8, 16, 24, 32) and of the 16-wide tiles of the gather and of the blocked factorisation; the
    pool mode, the compacting mode (ablate bit 1) and the chain (bit 16), which must also give the five launches' bits"""
    _need_long_double()
    nlive = max(50, D + 20)
    case = build(1000 + D, D, [(nlive + 190, 0.47, 0.06, 100.0)], nlive=nlive, n_below=33, n_holes=34)
    assert len(case.ph) == 257
    a = run_fused(engine, "", case)
    run_fused(engine, "", case, ablate=NO_POOL)
    b = run_fused(engine, "", case, ablate=CHAIN)
    _same_bits(a, b)
    if D >= 32:
        assert a["chol_suspect"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("nlive", [256, 257, 1000])
@pytest.mark.parametrize("nph", [1, 63, 64, 65, 255, 256, 257, 1027])
@pytest.mark.parametrize("D", [20, 70])
def test_fused_row_count_edges(engine, D, nph, nlive):
    """the 64-row pieces and 256-row blocks of the flag / index / gather kernels: a third of the phantom rows holes, a quarter below the threshold"""
    _need_long_double()
    holes, below = nph // 3, nph // 4
    case = build(2000 + 7 * D + nph + nlive, D, [(nlive + nph - holes - below, 0.55, 0.04, 30.0)], nlive=nlive, n_below=below, n_holes=holes)
    assert len(case.ph) == nph and len(case.live) == nlive
    a = run_fused(engine, "nlive=%d nph=%d" % (nlive, nph), case)
    run_fused(engine, "nlive=%d nph=%d" % (nlive, nph), case, ablate=NO_POOL)
    _same_bits(a, run_fused(engine, "nlive=%d nph=%d" % (nlive, nph), case, ablate=CHAIN))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [20, 100])
@pytest.mark.parametrize("centre,sigma,kappa", CONDITIONING)
def test_fused_conditioning_and_shift_distance(engine, D, centre, sigma, kappa):
    """a live set far from the cube centre, sigma << |mean - shift|, a strongly correlated cluster: the shift at mean + {0, 0.5, 3, 30} sigma in
    every coordinate.  The bound grows with the distance; the covariance has to stay inside it"""
    _need_long_double()
    case = build(3000 + D, D, [(2000, centre, sigma, kappa)], nlive=500, n_below=100, n_holes=100)
    mu = case.ref(0)[1].astype(np.float64)
    for k in SHIFT_SIGMAS:
        g = run_fused(engine, "centre=%g sigma=%g kappa=%g shift=mean+%gsigma" % (centre, sigma, kappa, k), case, shift=mu + k * sigma)
        if D == 100 and kappa == 1e6:
            assert g["chol_suspect"] == 0          # the blocked factor stood
    # and a first update's shift, the cube centre, up to 40000 sigma away: the bound then exceeds the smallest eigenvalue of the two narrow
    # clusters (u 0.4^2 against sigma^2 / kappa), so the covariance stays inside it but need not come out positive definite -- a factor
    # or the scaled identity, nothing else
    g = run_fused(engine, "centre=%g sigma=%g kappa=%g shift=cube centre" % (centre, sigma, kappa), case, want="factor" if kappa == 1.0 else None)
    assert g["ratios"][2] in ("factor", "identity")


def _suspect_rule(cov):
    """k_chol_blocked's own rule in long double: smallest pivot^2 / diagonal element"""
    A = cov.astype(LD).copy()
    q = np.inf
    for i in range(len(A)):                                 # right-looking: A[i, i] is the pivot^2 when column i's turn comes
        q = min(q, float(A[i, i] / cov[i, i]))
        if not A[i, i] > 0:
            break
        col = A[i + 1:, i] / np.sqrt(A[i, i])
        A[i + 1:, i + 1:] -= np.outer(col, col)
    return q


@pytest.mark.gpu
def test_fused_blocked_hands_over_at_kappa_1e11(engine):
    """kappa = 1e11 at nDims 100: k_chol_blocked does not trust a pivot below 1e-9 of its diagonal element and hands over to the
    reference-order kernel (chol_suspect = 1), whose factor has to meet the same bounds.  The population matrix of this spectrum in a random
    basis has its smallest pivot at about 5e-9 of the diagonal, so the live set is a small one (nDims + 15 rows), whose sample covariance
    is worse by the usual (1 - sqrt(D / n))^2 and more: the case asserts of itself that the rule's quantity, taken from the reference
    covariance, is below a quarter of the threshold -- then the device has to say suspect"""
    _need_long_double()
    D = 100
    case = build(4001, D, [(D + 15, 0.6, 1e-2, 1e11)], nlive=60, n_below=20, n_holes=20)
    q = _suspect_rule(case.ref(0)[3])
    print("UF kappa=1e11: smallest pivot^2 / diagonal of the reference covariance = %.3g" % q)
    assert 0 < q < 0.25e-9, q
    mu = case.ref(0)[1].astype(np.float64)
    g = run_fused(engine, "kappa=1e11 shift=mean+0.5sigma", case, shift=mu + 0.5e-2)
    assert g["chol_suspect"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("D", [2, 15, 16, 17, 31, 32, 33, 64, 100, 101, 102, 128, 143, 144, 200, 256])
def test_steps_every_variant(engine, D):
    """the two-pass kernels plain (below 32 dimensions) and on the matrix cores, the three layouts of k_cov_final_chol (switches at 102 and
    144); one cluster (the kernels clamp to the device's count of surviving phantoms) and three with labels interleaved at random: most of the
    rows, nDims + 5, one"""
    _need_long_double()
    n = max(300, 2 * D + 40)
    run_steps(engine, "", build(5000 + D, D, [(n, 0.45, 0.05, 100.0)], nlive=n // 3, n_below=n // 4, n_holes=n // 3))
    case = build(5500 + D, D, [(n, 0.3, 0.05, 10.0), (D + 5, 0.7, 0.02, 10.0), (1, 0.5, 0.1, 1.0)], nlive=n // 2, n_below=n // 4, n_holes=n // 5)
    g = run_steps(engine, "", case)
    assert np.all(g["cov"][2] == 0.0) and np.all(g["chol"][2] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [20, 100, 256])
@pytest.mark.parametrize("edge", [-1, 0, 1])
def test_steps_chunk_edges(engine, D, edge):
    """live slots + phantom rows = a whole number of chunks of cov_rows, one less, one more"""
    _need_long_double()
    cr = cov_rows(D)
    assert cr == {20: 256, 100: 128, 256: 32}[D]
    total = cr * max(2, (2 * D + 40 + cr - 1) // cr) + edge
    run_steps(engine, "rows=%d chunk=%d" % (total, cr), build(6000 + D + edge, D, [(total, 0.5, 0.08, 50.0)], nlive=total // 4))


@pytest.mark.gpu
@pytest.mark.parametrize("D,total", [(20, 129 * 256 + 7), (32, 258 * 256 + 7)])
def test_steps_many_chunks(engine, D, total):
    """more than 128 chunks at nDims 20: k_fold_partials on the sums and on the partial matrices; more than 256 at nDims 32: the persistent
    workgroups of the matrix-core kernel walk several chunks each"""
    _need_long_double()
    assert (total + cov_rows(D) - 1) // cov_rows(D) > (128 if D == 20 else 256)
    run_steps(engine, "rows=%d" % total, build(7000 + D, D, [(total, 0.5, 0.08, 50.0)], nlive=300))


@pytest.mark.gpu
@pytest.mark.parametrize("path,D", [(1, 12), (1, 40), (1, 100), (0, 12), (0, 120), (0, 150)])
def test_fallback_one_coordinate_pinned(engine, path, D):
    """(i) one coordinate is 0.5 in every row and the shift the cube centre: its variance is exactly 0 whatever the order of summation, the
    pivot is not positive, the factor is sqrt(trace) I (utils.F90:633-638); the blocked kernel must have handed over"""
    _need_long_double()
    n = 2 * D + 30
    case = build(8000 + D, D, [(n, 0.5, 0.05, 10.0)], nlive=n // 2, n_below=9, n_holes=9, pin=D // 3)
    if path == 1:
        g = run_fused(engine, "pinned", case, want="identity")
        if D >= 32:
            assert g["chol_suspect"] == 1
    else:
        g = run_steps(engine, "pinned", case, want=["identity"])
    assert np.all(g["cov"][0][D // 3] == 0.0) and np.all(g["cov"][0][:, D // 3] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("path,D", [(1, 12), (1, 40), (0, 12), (0, 120), (0, 150)])
def test_fallback_cluster_of_one_row(engine, path, D):
    """(ii) one row: the covariance and the factor are all zeros"""
    _need_long_double()
    case = build(8500 + D, D, [(1, 0.4, 0.05, 1.0)], nlive=1, n_below=5, n_holes=5)
    g = run_fused(engine, "one row", case, want="zero") if path == 1 else run_steps(engine, "one row", case, want=["zero"])
    assert np.all(g["cov"][0] == 0.0) and np.all(g["chol"][0] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("path,D", [(1, 12), (1, 40), (0, 12), (0, 120), (0, 150)])
def test_fallback_rank_deficient(engine, path, D):
    """(iii) n <= nDims: the covariance is singular in exact arithmetic and round-off decides -- a factor within the backward bound or the
    scaled identity, nothing else (NaN, a partial factor)"""
    _need_long_double()
    for m in (D, max(2, D // 2)):
        case = build(9000 + D + m, D, [(m, 0.5, 0.05, 10.0)], nlive=max(1, m // 2), n_below=5, n_holes=5)
        g = run_fused(engine, "n=%d" % m, case, want=None) if path == 1 else run_steps(engine, "n=%d" % m, case, want=[None])
        kind = g["ratios"][2] if path == 1 else g["ratios"][0][2]
        assert kind in ("factor", "identity"), kind
