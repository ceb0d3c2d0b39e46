"""numpy restatement of the evidence recursion over a death sequence -- TEST INFRASTRUCTURE ONLY (the checker of the
device merge pchip_merge_records and of the engine's own evidence; never imported by the product).

update_evidence / calculate_logZ_estimate (src/polychord/run_time_info.f90:211-296, 652-678) for one volume with any
number of live points n(L); pinned against the reference by tests/golden/ref_replay.json (a dead-birth file the reference
wrote and the evidence its .stats reports).

Live points: the records of a run are its deaths (logL) and the contour each point entered the live set
at (entry: logzero, or the logL of an earlier death of the same run).  A point whose entry contour is the logL of m tied
deaths of its run is born after the t-th of them when it is the t-th point entering there (t from 0), after the last one
when t >= m - 1; a contour that is no death of the run: after the run's last death below it.  Runs are merged in logL
order, equal logL -> the lower run first, then record order.  With no ties this is n = #{entry < L} - #{deaths before}.

replay: float64, the kernels' own formulas (one-pass sums).  replay_hp: the same recursion in np.longdouble (80-bit on
x86-64), two-pass posterior moments -- the yardstick of tests/test_merge_kernels.py."""
import numpy as np


def live_counts(logL, entry, counts=None):
    """-> (order, nlive): merged death order of the records and the live points just before each death, by the tie rule above.
    counts: records per run, runs one after the other (None: one run)"""
    logL = np.asarray(logL, dtype=np.float64); entry = np.asarray(entry, dtype=np.float64)
    N = logL.size
    counts = [N] if counts is None else [int(c) for c in counts]
    assert sum(counts) == N, (sum(counts), N)
    order = np.argsort(logL, kind="stable")           # equal logL: the lower record index = the lower run first
    rank = np.empty(N, dtype=np.int64); rank[order] = np.arange(N)
    gpos = []                                         # merged position from which each point is alive
    o = 0
    for c in counts:
        if c == 0:
            continue
        Lq, eq = logL[o:o + c], entry[o:o + c]
        oq = np.argsort(Lq, kind="stable"); dq = Lq[oq]
        lo = np.searchsorted(dq, eq, side="left"); hi = np.searchsorted(dq, eq, side="right")
        tied = hi > lo
        t = np.zeros(c, dtype=np.int64)
        if tied.any():                                # t = rank of the point among the points entering at the same contour
            et = eq[tied]
            s = np.argsort(et, kind="stable"); es = et[s]
            tt = np.empty(et.size, dtype=np.int64); tt[s] = np.arange(et.size) - np.searchsorted(es, es, side="left")
            t[tied] = tt
        pos = np.where(tied, lo + 1 + np.minimum(t, hi - lo - 1), lo)      # born after `pos` deaths of its run
        gpos.append(np.where(pos > 0, rank[o + oq[np.maximum(pos - 1, 0)]] + 1, 0))
        o += c
    born = np.bincount(np.concatenate(gpos), minlength=N + 1) if gpos else np.zeros(N + 1, dtype=np.int64)
    n = np.cumsum(born)[:N] - np.arange(N)
    return order, np.maximum(n, 1)


def _recursion(d, n, dt):
    n = n.astype(dt); d = d.astype(dt)
    l1, l2 = np.log(n + 1), np.log(n + 2)
    d1, d2 = -np.log1p(1 / n), -np.log1p(2 / n)      # log n/(n+1), log n/(n+2) (as the kernels: no cancellation of two logs)
    zero = np.zeros(1, dtype=dt)
    logX = np.concatenate((zero, np.cumsum(d1)))
    logXX = np.concatenate((zero, np.cumsum(d2)))
    Xm, XXm, Xi = logX[:-1], logXX[:-1], logX[1:]
    logZ = np.logaddexp.reduce(Xm + d - l1)
    t = XXm + d + d1 - l2 - Xi
    ZX = np.logaddexp.accumulate(t) + Xi
    ZXm = np.concatenate((np.full(1, -np.inf, dtype=dt), ZX[:-1]))
    log2 = np.log(dt(2))
    logZ2 = np.logaddexp.reduce(np.logaddexp(log2 + ZXm + d - l1, log2 + XXm + 2 * d - l1 - l2))
    return 2 * logZ - logZ2 / 2, logZ2 - 2 * logZ, Xm - l1


def replay(logL, entry, rows=None, p0=0, nP=0, counts=None):
    """-> dict(logZ, varlogZ, logweights (death order), nlive, order[, post_mean, post_var]); logL need not be sorted"""
    logL = np.asarray(logL, dtype=np.float64)
    order, n = live_counts(logL, entry, counts)
    d = logL[order]
    logZ, varlogZ, lw = _recursion(d, n, np.float64)
    out = dict(logZ=float(logZ), varlogZ=float(varlogZ), logweights=lw, nlive=n.astype(np.int64), order=order)
    if rows is not None:
        w = np.exp(lw + d - (lw + d).max())
        x = np.asarray(rows)[order][:, p0:p0 + nP]
        mean = (w[:, None] * x).sum(0) / w.sum()
        out["post_mean"] = mean
        out["post_var"] = (w[:, None] * x * x).sum(0) / w.sum() - mean ** 2
    return out


def replay_hp(logL, entry, rows=None, p0=0, nP=0, counts=None):
    """replay in np.longdouble: logZ, varlogZ, logweights (longdouble arrays / scalars), nlive, order; lw_bound = a forward-error bound of
    float64 log weights made by ANY order of the running sums (|error of S_i| <= (i u) sum |terms| + the rounding of the terms);
    post_mean / post_var by two passes over the weighted rows, about a row of the sample"""
    ld = np.longdouble
    logL = np.asarray(logL, dtype=np.float64)
    order, n = live_counts(logL, entry, counts)
    d = logL[order]
    logZ, varlogZ, lw = _recursion(d, n, ld)
    u = 2.0 ** -53
    nf = n.astype(np.float64)
    l0, l1 = np.log(nf), np.log(nf + 1.0)
    x = np.abs(l0 - l1)
    i = np.arange(n.size, dtype=np.float64)
    S = np.concatenate(([0.0], np.cumsum(x)))[:-1]                     # sum of |terms| before death i
    T = np.concatenate(([0.0], np.cumsum(l0 + l1)))[:-1]              # rounding of the logs inside each term
    bound = u * (i * S + 4.0 * T + 4.0 * (S + l1)) + 1e-300
    out = dict(logZ=logZ, varlogZ=varlogZ, logweights=lw, nlive=n.astype(np.int64), order=order, lw_bound=bound)
    if rows is not None:
        lp = lw + d.astype(ld)
        w = np.exp(lp - lp.max())
        x = np.asarray(rows)[order][:, p0:p0 + nP]
        xs = (x - x[np.argmax(w)]).astype(ld)            # (about a row of the sample: exact differences, sums of the spread's size)
        W = w.sum()
        shift = (w[:, None] * xs).sum(0) / W
        mean = x[np.argmax(w)].astype(ld) + shift
        dev = xs - shift
        out["post_mean"] = mean
        out["post_var"] = (w[:, None] * dev * dev).sum(0) / W
    return out


def evidence_replay(logL, entry):
    r = replay(logL, entry)
    return r["logZ"], r["varlogZ"]


def lived_records(run):
    """(logL, entry contour) of the points of a run that entered the live set"""
    dead, lw = run["dead"], run["logweights"]
    keep = lw > -1e29
    entry = run["entry"] if "entry" in run else dead[:, -2]
    return dead[keep, -1], entry[keep]


def combined_evidence(run_logZ, run_varlogZ):
    """evidence of R independent runs from the runs' own log-normal evidences (pchip_merged.evidence_rule 1): mean of the Z_r in linear
    space; variance of its log = the larger of the propagated one and the scatter between the runs.  -> (logZ, varlogZ)"""
    lz = np.asarray(run_logZ, dtype=np.float64); v = np.asarray(run_varlogZ, dtype=np.float64)
    R = lz.size
    m = np.exp(lz + 0.5 * v)                 # <Z_r>
    q = np.exp(2.0 * lz + 2.0 * v)           # <Z_r^2>
    mean = m.mean()
    second = (q.sum() + m.sum() ** 2 - (m ** 2).sum()) / R ** 2
    var = np.log(second) - 2.0 * np.log(mean)
    if R > 1:
        var = max(var, np.log1p(m.var(ddof=1) / R / mean ** 2))
    var = max(var, 0.0)
    return float(np.log(mean) - 0.5 * var), float(var)
