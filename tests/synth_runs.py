"""Seeded synthetic nested-sampling runs in the engine's record layout -- TEST INFRASTRUCTURE ONLY (the inputs of
tests/test_merge_kernels.py; numpy, vectorised: millions of rows in a second or two).

A run: deaths ascending in logL; initial points enter at logzero, every later point at the logL of an earlier death of the
same run (first in, first out: record k carries the k-th entry in birth order).  Rows are [cube | theta | phi | birth | logL]
with the birth column = the entry contour.  Constant live counts (one birth after each death until the final kill-off) or
dynamic ones (zero or two births after a death in alternating stretches).  Knobs: plateaus of length 2 and >= 3 inside a run,
a shared logL grid (exact ties across runs, entries equal to another run's deaths), failed spawns in the run's full dead
array (logweight == logzero: scattered, whole 256-row blocks, block edges), per-column offset and spread of theta / phi."""
import numpy as np

LOGZERO = -1e30


def _logL(rng, nlive_before, grid):
    """ascending logL of a run whose live count before death j is nlive_before[j]: log X shrinks by ~1/n a death, logL of a 4-D
    Gaussian-like shell -A X^(1/2); on a grid of 1/grid when asked"""
    t = np.cumsum(rng.standard_exponential(nlive_before.size) / np.maximum(nlive_before, 1))
    L = -60.0 * np.exp(-0.5 * t)
    if grid:
        L = np.floor(L * grid) / grid
    return np.maximum.accumulate(L)


def _plateaus(rng, L, lengths, reserve):
    """flatten stretches of the given lengths (non-overlapping, away from the last `reserve` deaths) -> list of (start, length)"""
    N = L.size
    out = []
    if not lengths:
        return out
    room = N - reserve - 2
    k = len(lengths)
    if room < sum(lengths) + 2 * k:
        return out
    starts = np.sort(rng.choice(room // (max(lengths) + 2), size=k, replace=False)) * (max(lengths) + 2) + 1
    for s, m in zip(starts, lengths):
        L[s:s + m] = L[s]
        out.append((int(s), int(m)))
    return out


def run(rng, n, nlive, nDims=2, nDerived=0, dynamic=0, plateaus=(), grid=0, offsets=None, spreads=None, fail=None):
    """one run of n deaths.  dynamic = h > 0: births alternate between two and none in stretches of h deaths (live count between nlive and
    nlive + h).  plateaus: lengths of flat stretches.  fail: None, or dict(frac=, blocks=[k, ..], edges=[k, ..]) for the full dead array.
    -> dict(rows [n][nT], entry [n], nlive_true [n] (the live points before each death), plateaus, and with fail: dead [nd][nT],
    logweights [nd], entry_all [nd], lived (mask))"""
    nT = 2 * nDims + nDerived + 2
    nP = nDims + nDerived
    if n == 0:
        rows = np.zeros((0, nT))
        out = dict(rows=rows, entry=np.zeros(0), nlive_true=np.zeros(0, dtype=np.int64), plateaus=[])
    else:
        K = min(nlive, n)
        if dynamic:
            b = np.where((np.arange(n) // dynamic) % 2 == 0, 2, 0)           # births after each death
        else:
            b = np.ones(n, dtype=np.int64)
        cum = np.minimum(K + np.cumsum(b), n)                                # no more points than records: then the kill-off
        b = np.diff(np.concatenate(([K], cum)))
        born = K + np.concatenate(([0], np.cumsum(b)))[:n]                   # points born before death j
        nlive_true = born - np.arange(n)
        assert nlive_true.min() >= 1 and K + b.sum() == n
        L = _logL(rng, nlive_true, grid)
        pl = _plateaus(rng, L, list(plateaus), reserve=nlive + (dynamic or 0) + 2)
        # entries in birth order: K at logzero, then b[j] copies of L[j]; record k gets the k-th
        entry = np.concatenate((np.full(K, LOGZERO), np.repeat(L, b)))
        assert entry.size == n
        rows = np.empty((n, nT))
        rows[:, :nDims] = rng.random((n, nDims))
        off = np.zeros(nP) if offsets is None else np.asarray(offsets, dtype=np.float64)
        spr = np.full(nP, 0.1) if spreads is None else np.asarray(spreads, dtype=np.float64)
        rows[:, nDims:nDims + nP] = off + spr * rng.standard_normal((n, nP))
        rows[:, -2] = entry
        rows[:, -1] = L
        out = dict(rows=rows, entry=entry, nlive_true=nlive_true.astype(np.int64), plateaus=pl)
    if fail is not None:
        out.update(_with_failures(rng, out["rows"], out["entry"], **fail))
    return out


def _with_failures(rng, rows, entry, frac=0.0, blocks=(), edges=()):
    """the run's full dead array: lived rows in order with failed spawns (logweight = logzero, junk row) between them.  blocks: indices k of
    whole failed rows [256 k, 256 k + 256) of the full array; edges: blocks whose rows 0 and 255 fail"""
    n, nT = rows.shape
    nd = int(n / max(1e-3, 1.0 - frac)) + 6 * int(np.sqrt(n + 1)) + 256 * (len(blocks) + 1) + 2 * len(edges) + 16
    fail = rng.random(nd) < frac
    for k in blocks:
        fail[256 * k:256 * (k + 1)] = True
    for k in edges:
        fail[[i for i in (256 * k, 256 * k + 255) if i < nd]] = True
    keep_idx = np.nonzero(~fail)[0][:n]
    assert keep_idx.size == n
    nd = int(keep_idx[-1]) + 1 if n else 300                 # (a run of failed spawns only: 300 rows, none lived)
    fail = np.ones(nd, dtype=bool); fail[keep_idx] = False
    dead = rng.standard_normal((nd, nT))                # failed rows: junk
    dead[keep_idx] = rows
    lw = np.full(nd, LOGZERO)
    lw[keep_idx] = -np.arange(n) / max(n, 1) - 3.0 + 0.01 * rng.standard_normal(n)
    ent = rng.standard_normal(nd)
    ent[keep_idx] = entry
    return dict(dead=dead, logweights=lw, entry_all=ent, lived=~fail)


def union(runs):
    """(rows, entry, counts) of runs one after the other"""
    nT = next((r["rows"].shape[1] for r in runs), 0)
    rows = np.concatenate([r["rows"] for r in runs]) if runs else np.zeros((0, nT))
    return np.ascontiguousarray(rows), np.ascontiguousarray(np.concatenate([r["entry"] for r in runs])), [r["rows"].shape[0] for r in runs]


def runs(seed, sizes, nlive, **kw):
    """runs of the given sizes (nlive: one value or one per run; the other knobs as in run(), shared) from one seed"""
    rng = np.random.default_rng(seed)
    nl = list(nlive) if np.ndim(nlive) else [nlive] * len(sizes)
    return [run(rng, int(n), int(k), **kw) for n, k in zip(sizes, nl)]
