"""The device merge (pc_merge.hip) against a high-precision replay, at the sizes, run counts, widths and edges its kernels branch on.

CPU: the tie rule of the live counts restated the way the kernels apply it, against the generator's true live
counts and the issue's hand examples; replay_hp pinned against the reference's .stats, mpmath and the float64 replay; the
synthetic-run generator's invariants; the moment method (sums about a pivot) against the one-pass formula it replaced.
GPU (-m gpu): pchip_merge_records[_ex] on synthetic unions -- across SC_CHUNK (2048), the carry of k_scan_totals (> 524,288 records),
k_pack_scan's carry (> 262,144 dead points in a run), > 256 parameters, 4096 runs, both evidence rules, ties, plateaus and narrow
posteriors far from zero -- each against replay_hp; the packing of host and device records; two ranks of very uneven size; the
engine's own posterior moments of a narrow posterior far from zero."""
import ctypes as C

import numpy as np
import pytest

from tests import synth_runs as sr
from tests.replay_oracle import live_counts, replay, replay_hp, combined_evidence

LZ = sr.LOGZERO


# ------------------------------------------------------------------------------------------------ restatements of the kernels' rules
def _kernel_counts(logL, entry, counts, rule="tie", rng=None):
    """k_merge_hist + k_merge_livecount + k_merge_rank restated: per run a histogram of birth positions in the run's own death sequence
    (rule "tie": the counter of each tie group hands out t in a random order, as atomics may; rule "first": the rule before this
    change, every point after the FIRST tied death), the live points per run from its prefix sum, then every record's rank and live
    count by binary searches in the other runs (equal logL: the lower run dies first)."""
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    R, N = len(counts), off[-1]
    G = []
    for q in range(R):
        L, e = logL[off[q]:off[q + 1]], entry[off[q]:off[q + 1]]
        ln = L.size
        hist = np.zeros(ln + 1, dtype=np.int64)
        ctr = {}
        idx = np.arange(e.size) if rng is None else rng.permutation(e.size)
        for g in idx:
            pos = np.searchsorted(L, e[g], side="left")
            if pos < ln and L[pos] == e[g]:
                if rule == "first":
                    pos += 1
                else:
                    m = np.searchsorted(L, e[g], side="right") - pos
                    t = ctr.get(pos, 0); ctr[pos] = t + 1
                    pos += 1 + min(t, m - 1)
            hist[pos] += 1
        G.append(np.cumsum(hist) - np.arange(ln + 1))
    nl = np.zeros(N, dtype=np.int64); perm = np.zeros(N, dtype=np.int64)
    for r in range(R):
        for a in range(off[r + 1] - off[r]):
            x = logL[off[r] + a]
            rank, n = a, G[r][a]
            for q in range(R):
                if q == r:
                    continue
                Lq = logL[off[q]:off[q + 1]]
                k = np.searchsorted(Lq, x, side="right" if q < r else "left")
                rank += k; n += G[q][k]
            perm[rank] = off[r] + a; nl[rank] = max(n, 1)
    return perm, nl


def test_tie_rule_on_the_hand_examples():
    """one run with deaths [1, 2, 2, 2, 3]: the rule before this change counted [2, 2, 3, 2, 1], the float64 checker [2, 2, 1, 1, 1], the
    truth (one birth after each death) is [2, 2, 2, 2, 1].  Two runs tying across each other: the kernel's cross-run order, which the
    checker now follows."""
    L = np.array([1., 2, 2, 2, 3]); e = np.array([LZ, LZ, 1, 2, 2])
    assert list(_kernel_counts(L, e, [5], rule="first")[1]) == [2, 2, 3, 2, 1]
    assert list(_kernel_counts(L, e, [5])[1]) == [2, 2, 2, 2, 1]
    assert list(live_counts(L, e)[1]) == [2, 2, 2, 2, 1]
    assert list(replay(L, e)["nlive"]) == [2, 2, 2, 2, 1] and list(replay_hp(L, e)["nlive"]) == [2, 2, 2, 2, 1]
    L2 = np.array([1., 2, 3, 2, 2.5, 4]); e2 = np.array([LZ, LZ, 2, LZ, LZ, 2])
    perm, nl = _kernel_counts(L2, e2, [3, 3])
    assert list(nl) == [4, 3, 3, 3, 2, 1]
    order, n = live_counts(L2, e2, [3, 3])
    assert list(n) == [4, 3, 3, 3, 2, 1] and np.array_equal(order, perm)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tie_rule_gives_the_true_live_count_of_plateau_runs(seed):
    """constant-nlive runs with plateaus of 2 and more tied deaths: the records alone give the run's true live counts back -- by the
    checker and by the kernels' rule whatever order the atomics hand t out in; the rule before this change did not"""
    rs = sr.runs(seed, [900, 400, 1], [12, 7, 1], plateaus=(2, 3, 5, 2, 4))
    assert all(len(r["plateaus"]) == 5 for r in rs[:2])
    for r in rs:
        L, e = r["rows"][:, -1], r["entry"]
        assert np.array_equal(live_counts(L, e)[1], r["nlive_true"])
        assert np.array_equal(_kernel_counts(L, e, [L.size], rng=np.random.default_rng(seed))[1], r["nlive_true"])
    L, e = rs[0]["rows"][:, -1], rs[0]["entry"]
    assert not np.array_equal(_kernel_counts(L, e, [L.size], rule="first")[1], rs[0]["nlive_true"])


@pytest.mark.parametrize("seed", [3, 4])
def test_checker_follows_the_kernels_rule_across_runs(seed):
    """a shared logL grid (ties inside and across runs, entries equal to other runs' deaths), dynamic live counts, an empty and a one-row
    run: the checker's merged order and live counts are the kernels'"""
    rs = sr.runs(seed, [700, 0, 350, 1, 500], [20, 1, 9, 1, 15], grid=4, dynamic=6)
    rows, entry, counts = sr.union(rs)
    L = rows[:, -1]
    assert np.unique(L).size < L.size * 0.9                                  # many ties
    perm, nl = _kernel_counts(L, entry, counts, rng=np.random.default_rng(seed))
    order, n = live_counts(L, entry, counts)
    assert np.array_equal(order, perm) and np.array_equal(n, nl)


# ------------------------------------------------------------------------------------------------ replay_hp
def test_replay_hp_reproduces_the_reference_stats(golden):
    g = golden["ref_replay"]
    r = replay_hp(g["logL"], g["birth"])
    assert abs(float(r["logZ"]) - g["stats"]["logZ"]) < 1e-9
    assert abs(np.sqrt(float(r["varlogZ"])) - g["stats"]["logZerr"]) < 1e-9


def _mp_replay(logL, entry, rows, p0, nP):
    """the recursion and the moments in mpmath at 50 digits, from the checker's live counts"""
    import mpmath as mp
    mp.mp.dps = 50
    order, n = live_counts(logL, entry)
    d = [mp.mpf(float(x)) for x in np.asarray(logL)[order]]
    logX, logXX = mp.mpf(0), mp.mpf(0)
    Z, ZX, Z2, XX = mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)
    X = mp.mpf(1)
    lws = []
    for L, k in zip(d, n):
        k = mp.mpf(int(k))
        lw = logX - mp.log(k + 1)
        lws.append(lw)
        # update_evidence (run_time_info.f90:211-296), one volume
        LL = mp.exp(L)
        Z2 = Z2 + 2 * ZX * LL / (k + 1) + 2 * XX * LL ** 2 / ((k + 1) * (k + 2))
        ZX = ZX * k / (k + 1) + XX * LL * k / ((k + 1) * (k + 2))
        Z = Z + X * LL / (k + 1)
        X = X * k / (k + 1); XX = XX * k / (k + 2)
        logX = mp.log(X)
    logZ = 2 * mp.log(Z) - mp.log(Z2) / 2
    var = mp.log(Z2) - 2 * mp.log(Z)
    w = [mp.exp(lw + L) for lw, L in zip(lws, d)]
    W = mp.fsum(w)
    x = np.asarray(rows)[order][:, p0:p0 + nP]
    mean = [mp.fsum(wi * mp.mpf(float(x[i, c])) for i, wi in enumerate(w)) / W for c in range(nP)]
    var_p = [mp.fsum(wi * (mp.mpf(float(x[i, c])) - mean[c]) ** 2 for i, wi in enumerate(w)) / W for c in range(nP)]
    return logZ, var, lws, mean, var_p


@pytest.mark.parametrize("seed", [5, 6])
def test_replay_hp_against_mpmath(seed):
    rs = sr.runs(seed, [160], [9], plateaus=(2, 3), offsets=[1e4, -3.0], spreads=[1e-4, 0.2])
    rows, entry, _ = sr.union(rs)
    r = replay_hp(rows[:, -1], entry, rows=rows, p0=2, nP=2)
    lz, var, lws, mean, var_p = _mp_replay(rows[:, -1], entry, rows, 2, 2)
    assert abs(float(r["logZ"] - np.longdouble(str(lz)))) < 1e-15 and abs(float(r["varlogZ"] - np.longdouble(str(var)))) < 1e-15
    assert max(abs(float(a - np.longdouble(str(b)))) for a, b in zip(r["logweights"], lws)) < 1e-15
    for c in range(2):
        assert abs(float(r["post_mean"][c] - np.longdouble(str(mean[c])))) < 1e-15 * max(1.0, abs(float(mean[c])))
        assert abs(float(r["post_var"][c] / np.longdouble(str(var_p[c])) - 1)) < 1e-12


def test_float64_replay_within_the_bound_of_replay_hp():
    """well-conditioned data (theta near 0.5, sd 0.1): the float64 checker meets replay_hp's forward-error bound on every log weight and
    agrees on the evidence and the moments"""
    rs = sr.runs(7, [60000, 30000, 45000], [500, 300, 400])
    rows, entry, counts = sr.union(rs)
    a = replay(rows[:, -1], entry, rows=rows, p0=2, nP=2, counts=counts)
    h = replay_hp(rows[:, -1], entry, rows=rows, p0=2, nP=2, counts=counts)
    assert np.array_equal(a["nlive"], h["nlive"]) and np.array_equal(a["order"], h["order"])
    assert np.all(np.abs(a["logweights"] - h["logweights"]) <= h["lw_bound"])
    assert abs(a["logZ"] - float(h["logZ"])) < 1e-10 and abs(a["varlogZ"] - float(h["varlogZ"])) < 1e-10
    assert np.allclose(a["post_mean"], h["post_mean"].astype(float), rtol=0, atol=1e-13)
    assert np.allclose(a["post_var"], h["post_var"].astype(float), rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------ the generator
def test_generator_invariants():
    rs = sr.runs(8, [3000, 0, 1, 2500, 700], [40, 1, 1, 25, 12], dynamic=0, plateaus=(2, 3, 6), grid=0,
                 offsets=[1e5, -1e5, 3.0], spreads=[1e-5, 1e-5, 2.0], nDims=2, nDerived=1,
                 fail=dict(frac=0.2, blocks=[1, 3], edges=[4, 5]))
    for r in rs:
        rows, e = r["rows"], r["entry"]
        n = rows.shape[0]
        assert rows.shape[1] == 2 * 2 + 1 + 2
        L = rows[:, -1]
        assert np.all(np.diff(L) >= 0) and np.array_equal(rows[:, -2], e)
        # every entry is logzero or the logL of an EARLIER death of the same run
        for k in range(n):
            assert e[k] == LZ or np.any(L[:k] == e[k]), k
        assert np.all(r["nlive_true"] >= 1) and (n == 0 or r["nlive_true"][-1] == 1)
        for s, m in r["plateaus"]:
            assert np.all(L[s:s + m] == L[s]) and m >= 2
        # the full dead array: lived rows in order, failed spawns at logzero, whole failed blocks and block edges
        lived = r["logweights"] > LZ
        assert np.array_equal(lived, r["lived"]) and np.array_equal(r["dead"][lived], rows) and np.array_equal(r["entry_all"][lived], e)
        if r["dead"].shape[0] > 6 * 256:
            assert not lived[256:512].any() and not lived[768:1024].any()
            assert not lived[1024] and not lived[1279] and not lived[1280] and not lived[1535]
    assert rs[0]["plateaus"] and max(m for _, m in rs[0]["plateaus"]) >= 3
    th = np.concatenate([r["rows"][:, 2:5] for r in rs])
    assert abs(th[:, 0].mean() - 1e5) < 1e-5 and abs(th[:, 1].mean() + 1e5) < 1e-5 and 0.5e-5 < th[:, 0].std() < 2e-5
    # dynamic live counts; ties across runs on a shared grid, an entry equal to another run's death
    d = sr.runs(9, [4000, 3000], [30, 20], dynamic=9, grid=8)
    assert d[0]["nlive_true"][:3000].max() > d[0]["nlive_true"][:3000].min() + 5
    L0, L1 = d[0]["rows"][:, -1], d[1]["rows"][:, -1]
    assert np.intersect1d(L0, L1).size > 10 and np.isin(d[1]["entry"], L0).sum() > 10


def test_generator_makes_millions_of_rows_in_seconds():
    import time
    t = time.perf_counter()
    rs = sr.runs(10, [2_000_000, 1_000_000], [50_000, 20_000], fail=dict(frac=0.05, blocks=[3]))
    assert time.perf_counter() - t < 20.0 and sum(r["rows"].shape[0] for r in rs) == 3_000_000


# ------------------------------------------------------------------------------------------------ the moment method
def _one_pass(w, x, chunk=512):
    """sum w x and sum w x^2 in chunks of 512 rows, then E[x^2] - mean^2 (the method before this change)"""
    s1 = s2 = sw = 0.0
    for i in range(0, x.size, chunk):
        ww, xx = w[i:i + chunk], x[i:i + chunk]
        s1 += (ww * xx).sum(); s2 += (ww * xx * xx).sum(); sw += ww.sum()
    m = s1 / sw
    return m, s2 / sw - m * m


def _pivot(w, x, p, chunk=512):
    """the same chunked sums about a pivot (the method of k_merge_moments / k_post_moments)"""
    s1 = s2 = sw = 0.0
    for i in range(0, x.size, chunk):
        ww, xx = w[i:i + chunk], x[i:i + chunk] - p
        s1 += (ww * xx).sum(); s2 += (ww * xx * xx).sum(); sw += ww.sum()
    d = s1 / sw
    return p + d, max(0.0, s2 / sw - d * d)


@pytest.mark.parametrize("mu,sd", [(1e3, 1e-3), (1e4, 1e-4), (1e5, 1e-4), (-1e5, 1e-5), (0.5, 0.1)])
def test_moments_about_a_pivot_keep_the_variance(mu, sd):
    rng = np.random.default_rng(11)
    n = 200_000
    w = np.exp(-rng.standard_exponential(n) * 3)
    x = mu + sd * rng.standard_normal(n)
    wl, xl = w.astype(np.longdouble), x.astype(np.longdouble)
    ml = (wl * xl).sum() / wl.sum()
    vl = float((wl * (xl - ml) ** 2).sum() / wl.sum())
    m, v = _pivot(w, x, x[np.argmax(w)])
    assert abs(v / vl - 1) < 1e-9 and abs(m - float(ml)) < 1e-9 * sd + 4 * np.spacing(abs(mu))
    if abs(mu) / sd >= 1e8:                                   # what the one-pass formula made of it
        assert abs(_one_pass(w, x)[1] / vl - 1) > 1e-3


# ------------------------------------------------------------------------------------------------ GPU
def _merge(nDims, nDerived, rows, entry, counts, want_rows=True, **kw):
    from polychordlite_amd import merge as mg
    return mg.merge_records(nDims, nDerived, counts, rows, entry, want_rows=want_rows, **kw)


def _check(m, rows, entry, counts, nDims, nDerived, want_rows=True, spreads=None):
    """the merged result against replay_hp: live counts exact, evidence to 1e-9, log weights within the data's forward-error bound (which
    the float64 checker meets too), posterior mean within 1e-9 of the spread (+ the rounding of the mean itself), variance >= 0 and to
    1e-6, merged rows in death order with the entry contour in the birth column"""
    nP = nDims + nDerived
    h = replay_hp(rows[:, -1], entry, rows=rows, p0=nDims, nP=nP, counts=counts)
    n = rows.shape[0]
    assert m["records"] == n and m["n_runs"] == len(counts)
    assert np.array_equal(m["nlive"], h["nlive"]), np.nonzero(m["nlive"] != h["nlive"])[0][:10]
    assert abs(m["logZ"] - float(h["logZ"])) <= 1e-9 and abs(m["varlogZ"] - float(h["varlogZ"])) <= 1e-9, (m["logZ"], float(h["logZ"]), m["varlogZ"], float(h["varlogZ"]))
    err = np.abs(m["logweights"] - h["logweights"]).astype(float)
    assert np.all(err <= h["lw_bound"]), (err.max(), h["lw_bound"][np.argmax(err)])
    a = replay(rows[:, -1], entry, counts=counts)
    assert np.all(np.abs(a["logweights"] - h["logweights"]).astype(float) <= h["lw_bound"])
    sd = np.sqrt(h["post_var"].astype(float))
    tol = 1e-9 * sd + 4 * np.spacing(np.abs(h["post_mean"].astype(float)))
    assert np.all(np.abs(m["post_mean"] - h["post_mean"]).astype(float) <= tol), (m["post_mean"] - h["post_mean"]).astype(float)
    assert np.all(m["post_var"] >= 0)
    dv = np.abs(m["post_var"] - h["post_var"]).astype(float)
    assert np.all(dv <= 1e-6 * h["post_var"].astype(float)), (dv / h["post_var"].astype(float)).max()
    if want_rows:
        o = h["order"]
        assert np.array_equal(m["rows"][:, :-2], rows[o, :-2]) and np.array_equal(m["rows"][:, -1], rows[o, -1])
        assert np.array_equal(m["rows"][:, -2], entry[o])
    return h


SIZES = [1, 2047, 2048, 2049, 524288, 524289, 1_729_760, 4_000_000]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_merge_of_one_run_at_every_size(engine, n):
    """one run of n records (nTotal 10): k_scan_local's chunk of 2048, k_scan_totals' carry between groups of 256 chunks (> 524,288
    records), the configs[4] union size, ~4 M; runs of a size that crosses multiples of 1024"""
    rs = sr.runs(100 + n % 97, [n], [max(1, min(n, n // 40 + 7))], nDims=4, offsets=[0.5, 1e4, -3.0, 1e5], spreads=[0.1, 1e-4, 2.0, 1e-5])
    rows, entry, counts = sr.union(rs)
    m = _merge(4, 0, rows, entry, counts, want_rows=n <= 2_000_000)
    _check(m, rows, entry, counts, 4, 0, want_rows=n <= 2_000_000)
    assert np.array_equal(m["nlive"], rs[0]["nlive_true"])


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 7, 64, 4096])
def test_merge_of_many_runs(engine, R):
    """R runs (R = 4096: the library's cap, runs of 0 .. 40 records, empty ones among them); lengths that cross multiples of 1024"""
    rng = np.random.default_rng(R)
    if R == 4096:
        sizes = rng.integers(0, 41, R); sizes[::97] = 0; sizes[5] = 1
        nl = np.maximum(1, sizes // 3)
    else:
        sizes = rng.integers(900, 300_000 // R + 2048, R); sizes[0] = 1024 * 3 + 1
        nl = np.maximum(1, sizes // 30)
    rs = sr.runs(200 + R, sizes, nl, nDims=3, nDerived=1, offsets=[0.5, -2e3, 7.0, 0.0], spreads=[0.1, 1e-3, 1.0, 1e-2])
    rows, entry, counts = sr.union(rs)
    m = _merge(3, 1, rows, entry, counts)
    _check(m, rows, entry, counts, 3, 1)


@pytest.mark.gpu
def test_merge_with_empty_runs_in_between(engine):
    rs = sr.runs(300, [5000, 0, 3000, 0, 0, 1, 2049, 0], [60, 1, 40, 1, 1, 1, 30, 1], nDims=2)
    rows, entry, counts = sr.union(rs)
    _check(_merge(2, 0, rows, entry, counts), rows, entry, counts, 2, 0)


@pytest.mark.gpu
def test_merge_of_more_than_256_parameters(engine):
    """nDims + nDerived = 300: k_merge_moments' column loop goes round twice"""
    nD, nDer = 200, 100
    off = np.linspace(-1e4, 1e4, nD + nDer); spr = np.geomspace(1e-4, 1.0, nD + nDer)
    rs = sr.runs(400, [12000, 8000], [200, 150], nDims=nD, nDerived=nDer, offsets=off, spreads=spr)
    rows, entry, counts = sr.union(rs)
    _check(_merge(nD, nDer, rows, entry, counts), rows, entry, counts, nD, nDer)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plateaus", "grid", "grid_dynamic"])
def test_merge_of_ties_and_plateaus(engine, case):
    """plateaus of 2 and more tied deaths inside runs (constant nlive: the true live counts come back), a shared logL grid (exact ties
    across runs, entries equal to other runs' deaths), dynamic live counts; narrow columns far from zero of both signs"""
    kw = dict(nDims=3, offsets=[1e5, -1e5, 0.5], spreads=[1e-5, 1e-4, 0.1])
    if case == "plateaus":
        rs = sr.runs(500, [30000], [300], plateaus=(2, 3, 3, 7, 2, 4, 2, 5), **kw)
    elif case == "grid":
        rs = sr.runs(501, [20000, 15000, 9000, 1], [200, 150, 90, 1], grid=16, plateaus=(2, 3), **kw)
    else:
        rs = sr.runs(502, [20000, 15000, 0, 9000], [200, 150, 1, 90], grid=16, dynamic=11, **kw)
    rows, entry, counts = sr.union(rs)
    assert np.unique(rows[:, -1]).size < rows.shape[0]
    m = _merge(3, 0, rows, entry, counts)
    _check(m, rows, entry, counts, 3, 0)
    if case == "plateaus":
        assert np.array_equal(m["nlive"], rs[0]["nlive_true"])


@pytest.mark.gpu
def test_merge_evidence_rule_1(engine):
    """a clustered run in the union: weights are the records' own over the number of runs (k_merge_ownw, several chunks of 1024), the
    evidence the runs' own combined; moments about the pivot of those weights"""
    rs = sr.runs(600, [9000, 7000, 5000], [100, 80, 60], nDims=2, offsets=[1e4, 0.5], spreads=[1e-4, 0.1], fail=dict(frac=0.0))
    rows, entry, counts = sr.union(rs)
    own = np.concatenate([r["logweights"][r["lived"]] for r in rs])
    lz, vz, cl = [-3.1, -2.9, -3.4], [0.02, 0.03, 0.025], [1, 0, 0]
    m = _merge(2, 0, rows, entry, counts, ownw=own, run_logZ=lz, run_varlogZ=vz, run_clustered=cl)
    assert m["evidence_rule"] == 1
    z, v = combined_evidence(lz, vz)
    assert abs(m["logZ"] - z) < 1e-10 and abs(m["varlogZ"] - v) < 1e-10
    h = replay_hp(rows[:, -1], entry, counts=counts)
    o = h["order"]
    assert np.array_equal(m["nlive"], h["nlive"]) and abs(m["logZ_replay"] - float(h["logZ"])) < 1e-9
    assert np.abs(m["logweights"] - (own[o] - np.log(3))).max() < 1e-12
    lp = (own[o] - np.log(np.longdouble(3))) + rows[o, -1].astype(np.longdouble)
    w = np.exp(lp - lp.max()); x = rows[o, 2:4].astype(np.longdouble)
    mean = (w[:, None] * x).sum(0) / w.sum(); var = (w[:, None] * (x - mean) ** 2).sum(0) / w.sum()
    assert np.all(np.abs(m["post_mean"] - mean).astype(float) <= 1e-9 * np.sqrt(var.astype(float)) + 4 * np.spacing(np.abs(mean.astype(float))))
    assert np.all(np.abs(m["post_var"] / var - 1).astype(float) < 1e-6)


# ---- packing
class _HostRuns:
    """pchip_result structs over synthetic host arrays (d_records = NULL: the library packs them itself); the arrays stay alive with this
    object, and the structs are never freed through the library"""

    def __init__(self, api, runs, nT):
        self.keep = []
        self.res = (api.Result * len(runs))()
        for k, r in enumerate(runs):
            dead = np.ascontiguousarray(r["dead"]); lw = np.ascontiguousarray(r["logweights"]); en = np.ascontiguousarray(r["entry_all"])
            self.keep += [dead, lw, en]
            x = self.res[k]
            x.ndead, x.nTotal, x.logZ, x.varlogZ, x.ncluster_peak = dead.shape[0], nT, -3.0, 0.04, 2      # (clustered: own weights travel)
            x.dead = dead.ctypes.data_as(C.POINTER(C.c_double)); x.logweights = lw.ctypes.data_as(C.POINTER(C.c_double))
            x.entry = en.ctypes.data_as(C.POINTER(C.c_double)); x.d_records = None


def _comm_merge_host(api, runs, nDims, nDerived, comm=None):
    from polychordlite_amd import merge as mg
    lib = mg._lib()
    hr = _HostRuns(api, runs, 2 * nDims + nDerived + 2)
    m = mg.Merged()
    rc = lib.pchip_comm_merge_many(comm.h if comm is not None else None, hr.res, len(runs), LZ, nDims, nDerived, 1, C.byref(m))
    if rc != 0:
        raise RuntimeError("pchip_comm_merge_many failed with code %d" % rc)
    try:
        return mg.merged_dict(m, nDims, nDerived, True)
    finally:
        lib.pchip_merged_free(C.byref(m))


@pytest.mark.gpu
def test_host_packing_is_exact(engine):
    """pchip_comm_merge_many without a communicator on host arrays: runs of 255, 256, 257 and > 262,144 dead points (k_pack_scan's carry
    between groups of 1024 blocks) with scattered failed spawns, whole failed 256-row blocks and failures on block edges -- the merged
    output must be, bit for bit, the merge of the numpy-compacted records"""
    fails = [dict(frac=0.1, blocks=[0], edges=[1]), dict(frac=0.0, edges=[0]), dict(frac=0.3), dict(frac=0.2, blocks=[3, 4, 900, 1030], edges=[1023, 1024, 1025])]
    rng = np.random.default_rng(700)
    rs = []
    for nd, f in zip([255, 256, 257, 280_000], fails):
        # size the lived count so the full dead array has about nd rows
        r = sr.run(rng, max(1, int(nd * (1 - f.get("frac", 0.0))) - 256 * len(f.get("blocks", ()))), 20, nDims=2, fail=f)
        rs.append(r)
    assert rs[3]["dead"].shape[0] > 262_144 and rs[0]["dead"].shape[0] < 512
    got = _comm_merge_host(engine, rs, 2, 0)
    rows, entry, counts = sr.union(rs)
    ref = _merge(2, 0, rows, entry, counts, ownw=np.concatenate([r["logweights"][r["lived"]] for r in rs]), run_logZ=[-3.0] * 4,
                 run_varlogZ=[0.04] * 4, run_clustered=[1] * 4)
    assert got["records"] == rows.shape[0] and got["evidence_rule"] == ref["evidence_rule"] == 1
    assert np.array_equal(got["rows"], ref["rows"]) and np.array_equal(got["logweights"], ref["logweights"]) and np.array_equal(got["nlive"], ref["nlive"])
    assert got["logZ_replay"] == ref["logZ_replay"] and np.array_equal(got["post_mean"], ref["post_mean"])


@pytest.mark.gpu
def test_two_thread_ranks_of_very_uneven_size(engine):
    """pchip_comm_merge_many over a caller's all-gather, two ranks on one GPU: rank 0 holds ONE record, rank 1 more than 524,288 -- every
    rank gets pchip_merge_records_ex of the union bit for bit (k_unpad with a block padded by ~600k rows)"""
    from polychordlite_amd import merge as mg
    from tests.test_merge import _ThreadGather, _ranks_in_threads
    rng = np.random.default_rng(800)
    mine = [[sr.run(rng, 1, 1, nDims=2, fail=dict(frac=0.0))], [sr.run(rng, 600_000, 2000, nDims=2, fail=dict(frac=0.05, blocks=[7]))]]
    tg = _ThreadGather(2)
    comms = [mg.CallbackComm(r, 2, 0, tg.rank(r)) for r in range(2)]
    try:
        got = _ranks_in_threads(2, lambda r: _comm_merge_host(engine, mine[r], 2, 0, comm=comms[r]))
    finally:
        for c in comms:
            c.close()
    union = mine[0] + mine[1]
    rows, entry, counts = sr.union(union)
    ref = _merge(2, 0, rows, entry, counts, ownw=np.concatenate([r["logweights"][r["lived"]] for r in union]), run_logZ=[-3.0] * 2,
                 run_varlogZ=[0.04] * 2, run_clustered=[1] * 2)
    for g in got:
        assert not isinstance(g, Exception), g
        assert g["records"] == 600_001 and g["n_runs"] == 2
        assert g["logZ"] == ref["logZ"] and g["logZ_replay"] == ref["logZ_replay"]
        assert np.array_equal(g["rows"], ref["rows"]) and np.array_equal(g["logweights"], ref["logweights"]) and np.array_equal(g["nlive"], ref["nlive"])
        assert np.array_equal(g["post_mean"], ref["post_mean"]) and np.array_equal(g["post_var"], ref["post_var"])


@pytest.mark.gpu
def test_device_packing_of_a_long_run(engine):
    """one engine run of more than 262,144 dead points: its records picked on the device when it ends (settings.device_records,
    pc_pack_lived_device) and picked by the merge from the host arrays must give bit-identical merged output"""
    from polychordlite_amd import merge as mg
    api = engine
    lib = api.load()
    D = 5
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, 0)
    s.nlive, s.num_repeats, s.seed, s.device_records = 5000, 10, 9, 1
    L, P, keep = api.make_problem("gaussian", D, 0, mu=0.5, sigma=1e-6)      # log X of the posterior ~ -64: ~70 nlive deaths
    a_run = api.run(s, L, P)
    assert a_run["ndead"] > 262_144 and a_run["n_records"] == int((a_run["logweights"] > a_run["logzero"]).sum())
    a = mg.comm_merge(a_run, None, D, 0, want_rows=True)
    s.device_records = 0
    b_run = api.run(s, L, P)
    assert b_run["n_records"] is None and np.array_equal(b_run["dead"], a_run["dead"], equal_nan=True)
    b = mg.comm_merge(b_run, None, D, 0, want_rows=True)
    assert a["records"] == b["records"] == a_run["n_records"] and a["logZ"] == b["logZ"]
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["logweights"], b["logweights"]) and np.array_equal(a["nlive"], b["nlive"])
    assert np.array_equal(a["post_mean"], b["post_mean"]) and np.array_equal(a["post_var"], b["post_var"])


@pytest.mark.gpu
def test_engine_moments_of_a_narrow_posterior_far_from_zero(engine):
    """a Gaussian of sd 1e-4 at 1e4: the run's post_var against replay_hp's two-pass moments of its own dead rows and log weights (the
    one-pass E[x^2] - mean^2 lost every digit here); post_mean to the rounding of the mean"""
    api = engine
    lib = api.load()
    D = 3
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, 0)
    s.nlive, s.num_repeats, s.seed = 200, 6, 21
    L, P, keep = api.make_problem("gaussian", D, 0, 1e4 - 1e-3, 1e4 + 1e-3, mu=1e4, sigma=1e-4)
    g = api.run(s, L, P)
    lw = g["logweights"]
    keepm = lw > g["logzero"]
    lp = lw[keepm].astype(np.longdouble) + g["dead"][keepm, -1].astype(np.longdouble)
    w = np.exp(lp - lp.max())
    x = g["dead"][keepm, D:2 * D].astype(np.longdouble)
    mean = (w[:, None] * x).sum(0) / w.sum()
    var = (w[:, None] * (x - mean) ** 2).sum(0) / w.sum()
    assert np.all(np.abs(g["post_var"] / var - 1).astype(float) < 1e-6), (g["post_var"], var.astype(float))
    assert np.all(np.abs(g["post_mean"] - mean).astype(float) <= 1e-9 * np.sqrt(var.astype(float)) + 4 * np.spacing(1e4))
    assert np.all(np.abs(np.sqrt(g["post_var"]) / 1e-4 - 1) < 0.3)
