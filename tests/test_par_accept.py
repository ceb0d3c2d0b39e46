"""The acceptance of the one-cluster parallel contraction (pc_par.hip, phase 3: par_accept).

A nursery's steps t = 0 .. T-1 each bring a candidate c_t; with the sorted snapshot S of the live set the contraction's rule is the recurrence

    a_t  =  v_t  and  r_t > #{ s < t : a_s and c_s >= c_t }            r_t = #{ e in S : e < c_t },  v_t: a step of the current epoch

(equal candidates: the earlier step counts as the larger).  The kernel evaluates the closed form

    a_t  =  v_t  and  r_t > #{ s < t : v_s and c_s >= c_t }

for all steps at once (DESIGN section 5 has the proof); settings.ablate bit 18 keeps the recurrence, resolved sixty-four steps at a time by one
wavefront, as the independent second implementation.

CPU: the recurrence, the closed form and -- for inputs without ties -- the literal loop "the lowest live point is replaced if the candidate lies
above it" in numpy, over a few thousand seeded cases.
GPU, door level (pchip_par_accept: the contraction's own device functions for the search, the ranks and the acceptance, one workgroup, on given
values): both implementations against the numpy recurrence, exactly, at the sizes where the code takes another way -- a chunk is 64 steps, a
bitmap word 64 ranks, the workgroup 1024 steps.
GPU, run level: the default run, the run under bit 18 and the run under bit 5 agree in every counter and every array, byte for byte.  (For a run
with one cluster bit 5 chooses no other kernel -- pc_plan.h asks it for several clusters only -- so that leg holds the default run against
itself; it is kept because it is cheap and stays meaningful should bit 5 ever reach these runs.)
"""
import ctypes as C

import numpy as np
import pytest

SERIAL = 1 << 18                                      # PC_ABL_ACCEPT_SERIAL
GENERAL = 1 << 5                                      # PC_ABL_CONSUME_GENERAL


# ---------------------------------------------------------------------------------------------------------------- the rule, three times
def recurrence(snap, cand, valid):
    snap, cand, valid = np.asarray(snap, dtype=np.float64), np.asarray(cand, dtype=np.float64), np.asarray(valid, dtype=bool)
    r = np.searchsorted(snap, cand, side="left")      # strictly below
    acc = np.zeros(cand.size, dtype=bool)
    for t in range(cand.size):
        acc[t] = valid[t] and r[t] > np.count_nonzero(acc[:t] & (cand[:t] >= cand[t]))
    return acc


def closed_form(snap, cand, valid):
    snap, cand, valid = np.asarray(snap, dtype=np.float64), np.asarray(cand, dtype=np.float64), np.asarray(valid, dtype=bool)
    r = np.searchsorted(snap, cand, side="left")
    acc = np.zeros(cand.size, dtype=bool)
    for t in range(cand.size):
        acc[t] = valid[t] and r[t] > np.count_nonzero(valid[:t] & (cand[:t] >= cand[t]))
    return acc


def literal_loop(snap, cand, valid):
    live = np.array(snap, dtype=np.float64)
    acc = np.zeros(len(cand), dtype=bool)
    for t in range(len(cand)):
        if not valid[t]:
            continue
        i = int(np.argmin(live))
        if cand[t] > live[i]:
            live[i] = cand[t]; acc[t] = True
    return acc


def _random_case(rng, k):
    """T <= 200 candidates, n <= 40 snapshot points; a third each: no ties, heavy ties (a few distinct values, shared between candidates and
    snapshot), candidates around and below the snapshot's minimum; 20 % invalid steps in half of the cases"""
    T, n = int(rng.integers(1, 201)), int(rng.integers(1, 41))
    kind = k % 3
    if kind == 0:
        v = rng.permutation(T + n).astype(np.float64)                 # all distinct
        snap, cand = np.sort(v[:n]), v[n:]
    elif kind == 1:
        m = int(rng.integers(1, 6))
        snap, cand = np.sort(rng.integers(0, m, n).astype(np.float64)), rng.integers(0, m + 1, T).astype(np.float64) - (k % 2)
    else:
        snap = np.sort(rng.standard_normal(n))
        cand = rng.standard_normal(T) + (snap[0] - 1.0 if k % 2 else 0.0)
        if k % 4 == 0:
            cand[:] = snap[0] - 1.0 - rng.random(T)                   # below every snapshot point
    valid = rng.random(T) >= 0.2 if (k // 3) % 2 else np.ones(T, dtype=bool)
    return snap, cand, valid, kind == 0


def test_the_closed_form_is_the_recurrence():
    rng = np.random.default_rng(20240518)
    naccept = ntie_free = 0
    for k in range(4000):
        snap, cand, valid, tie_free = _random_case(rng, k)
        want = recurrence(snap, cand, valid)
        assert np.array_equal(closed_form(snap, cand, valid), want), k
        if tie_free:
            assert np.array_equal(literal_loop(snap, cand, valid), want), k
            ntie_free += 1
        naccept += int(want.sum())
    assert ntie_free > 1000 and naccept > 10000       # (the cases are not trivially empty)


# ---------------------------------------------------------------------------------------------------------------- the door
TS = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 1024)
NS = (1, 2, 25, 64, 2000)


def _door_cases(T, n):
    """(name, snapshot, candidates, valid) for one pair of sizes"""
    rng = np.random.default_rng(1000 * T + n)
    snap = np.sort(rng.standard_normal(n))
    allv = np.ones(T, dtype=bool)
    rnd = rng.standard_normal(T)
    out = [("random", snap, rnd, allv),
           ("ascending", snap, np.sort(rnd), allv),
           ("descending", snap, np.sort(rnd)[::-1].copy(), allv),          # the largest counts: every earlier step is larger
           ("below", snap, snap[0] - 1.0 - rng.random(T), allv),           # nothing accepted
           ("above", snap, snap[-1] + 1.0 + rng.random(T), allv),
           ("snapshot values", snap, rng.choice(snap, T), allv),           # candidates equal to snapshot points, and to each other
           ("few values", np.sort(rng.integers(0, 4, n).astype(np.float64)), rng.integers(0, 5, T).astype(np.float64), allv),
           ("invalid 20 %", snap, rnd, rng.random(T) >= 0.2),
           ("invalid 20 %, descending", snap, np.sort(rnd)[::-1].copy(), rng.random(T) >= 0.2)]
    if T > 70:
        eq = rnd.copy(); eq[60:71] = np.median(snap)                       # equal candidates across the edge of chunks 0 and 1
        out.append(("equal 60..70", snap, eq, allv))
        eq2 = rnd.copy(); eq2[60:71] = snap[-1] + 5.0
        out.append(("equal 60..70 on top", snap, eq2, rng.random(T) >= 0.2))
    if T >= 128:
        v = allv.copy(); v[64:128] = False                                 # one chunk without a valid step
        out.append(("chunk 1 invalid", snap, rnd, v))
        out.append(("chunk 1 invalid, descending", snap, np.sort(rnd)[::-1].copy(), v))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
def test_door_equals_the_recurrence(engine, T):
    for n in NS:
        for name, snap, cand, valid in _door_cases(T, n):
            want = recurrence(snap, cand, valid)
            if name == "below":
                assert not want.any()
            if name == "above":
                assert want[0] and int(want.sum()) >= min(T, n)       # (the first n at the least: each takes a snapshot point's place)
            for serial in (False, True):
                got = engine.par_accept(snap, cand, valid, serial=serial)
                assert np.array_equal(got, want), (T, n, name, serial, np.flatnonzero(got != want)[:8])


@pytest.mark.gpu
def test_door_refuses_what_it_cannot_take(engine):
    lib = engine.load()
    bp = C.POINTER(C.c_ubyte)
    lib.pchip_par_accept.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), bp, C.c_int, bp, C.c_int]
    lib.pchip_par_accept.restype = C.c_int
    two = np.array([1.0, 0.0]); v = np.ones(2, dtype=np.uint8); a = np.zeros(2, dtype=np.uint8)
    assert lib.pchip_par_accept(0, engine.dptr(two), 2, engine.dptr(two), v.ctypes.data_as(bp), 0, a.ctypes.data_as(bp), -1) == 1
    assert lib.pchip_par_accept(2, engine.dptr(two), 1025, engine.dptr(two), v.ctypes.data_as(bp), 0, a.ctypes.data_as(bp), -1) == 1
    assert lib.pchip_par_accept(2, engine.dptr(two), 2, engine.dptr(two), v.ctypes.data_as(bp), 0, a.ctypes.data_as(bp), -1) == 1      # descending snapshot
    assert lib.pchip_par_accept(2, engine.dptr(two), 2, engine.dptr(two), None, 0, a.ctypes.data_as(bp), -1) == 1


# ---------------------------------------------------------------------------------------------------------------- whole runs
#         nDims nlive batch num_repeats
SHAPES = {"small": (3, 40, 20, 6),                    # a nursery inside one chunk
          "edge": (3, 130, 65, 6),                    # a chunk edge inside the nursery
          "full": (2, 2048, 1024, 2)}                 # the workgroup's full width
SCALARS = ("logZ", "varlogZ", "ndead", "nlike", "niter", "nbatches", "nrounds", "nupdates", "ncluster", "ncluster_dead", "nTotal", "batch",
           "nlike_failed", "ncluster_peak", "nlike_grade", "path")
ARRAYS = ("dead", "logweights", "entry", "live", "live_cluster", "logZp", "varlogZp", "post_mean", "post_var")


def _settings(api, shape, ablate, cut, seed=11):
    D, nlive, batch, nr = SHAPES[shape]
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, 0)
    s.nlive, s.batch, s.num_repeats, s.seed, s.ablate = nlive, batch, nr, seed, ablate
    if cut:
        s.max_ndead = 3 * nlive
    return s, api.make_problem("gaussian", D, 0)


def _run(api, shape, ablate, cut, seed=11):
    s, (L, P, keep) = _settings(api, shape, ablate, cut, seed)
    r = api.run(s, L, P)
    assert r["path"]["consume_par"] > 0 and r["path"]["consume_general"] == 0 and r["path"]["consume_fast"] == 0, r["path"]
    return r


def _same(a, b):
    for k in SCALARS:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("cut", (True, False), ids=("max_ndead", "termination"))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_runs_agree(engine, shape, cut):
    want = _run(engine, shape, SERIAL, cut)
    nlive = SHAPES[shape][1]
    if cut:
        assert want["ndead"] >= 3 * nlive             # (stopped by max_ndead, inside a nursery: the kill-off adds the live points)
    else:
        assert want["ndead"] > 6 * nlive
    _same(_run(engine, shape, 0, cut), want)
    _same(_run(engine, shape, GENERAL, cut), want)


@pytest.mark.gpu
def test_three_seeds_in_step_equal_their_solo_runs(engine):
    from polychordlite_amd import repeats
    seeds = [11, 12, 13]
    s, (L, P, keep) = _settings(engine, "edge", 0, False)
    merged, runs = repeats.run_repeats(s, L, P, seeds, max_in_flight=3)
    for seed, step in zip(seeds, runs):
        own = _run(engine, "edge", 0, False, seed=seed)
        for k in ("ndead", "nlike", "niter", "nupdates", "logZ", "varlogZ"):
            assert own[k] == step[k], (k, own[k], step[k])
        for k in ("dead", "logweights", "entry", "live"):
            assert np.asarray(own[k]).tobytes() == np.asarray(step[k]).tobytes(), (seed, k)
