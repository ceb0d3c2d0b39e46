"""Several seeds in step through the device batch callback (pchip_run_in_step with a callback likelihood while
polychord_hip_set_device_batch_callback holds a function): one call a tick for the parked proposals of all runs of a group.

The reference of every comparison is the solo device-batch pchip_run of each seed, which tests/test_device_batch.py pins to the host batch
callback.  The callees are its numpy functions, whose sums are taken column by column: a row's answer depends neither on its place in the block
nor on n, so every run in step must be its solo run in every counter, in log Z and in every bit of every dead row.  A solo run is made once
per (problem, settings, seed) and shared by the tests that need it."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import test_device_batch as tdb
from tests.test_device_batch import gauss_so  # noqa: F401  (the fixture: tools/dev/device_batch_gauss.hip built the same way)

D, NDER = tdb.D, tdb.NDER
SEEDS = (7, 8, 9)
BOX_LO, BOX_HI = np.full(D, -1.0), np.full(D, 1.0)        # np_prior's box, for the engine to evaluate


def _cb(api, like, prior, calls, blocks=None, fail_at=None, seen=None):
    """tests/test_device_batch.py's Python callee, with a record of the cube blocks it was handed and a call that returns 1"""
    hip = tdb._hip()

    def cb(_user, n, nd, nder, cube_p, theta_p, phi_p, logL_p, flags, stream):
        try:
            if fail_at is not None and len(calls) >= fail_at:
                return 1
            calls.append(n)
            if seen is not None:
                seen.append(flags)
            assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
            if blocks is not None:
                blocks.append(tdb._down(hip, cube_p, (n, nd)))
            if flags & 1:
                theta = tdb._down(hip, theta_p, (n, nd))
            else:
                theta = prior(tdb._down(hip, cube_p, (n, nd)))
                tdb._up(hip, theta_p, theta)
            logL, phi = like(theta)
            if nder > 0:
                tdb._up(hip, phi_p, phi)
            tdb._up(hip, logL_p, logL)
            return 0
        except BaseException:       # noqa: BLE001 -- nothing may cross the C frames: the run ends and the test sees it
            return 4
    return api.DEVICE_BATCH_FN(cb)


class Problem:
    """likelihood + prior + settings of a case; `keep` holds what the structs point at"""

    def __init__(self, api, lib, like, prior_kind, batch, clustering=False, max_ndead=-1):
        self.api, self.lib, self.like, self.batch, self.clustering, self.max_ndead = api, lib, like, batch, clustering, max_ndead
        self.key = (like.__name__, prior_kind, batch, clustering, max_ndead)
        self.fl, self.fp = tdb._scalars(api, like, tdb.np_prior)
        self.keep = []
        if prior_kind == "box":
            lo, hi = BOX_LO.copy(), BOX_HI.copy()
            self.L, self.P = tdb._problem(api, self.fl, None, kind=api.PRIOR_BOX, lo=api.dptr(lo), hi=api.dptr(hi))
            self.keep += [lo, hi]
        elif prior_kind == "table":
            arr, _ = api.prior_table(tdb.TABLE)
            self.L, self.P = tdb._problem(api, self.fl, None, kind=api.PRIOR_TABLE, table=arr)
            self.keep.append(arr)
        else:       # "own": prior.kind 0, the callee makes the prior (flags 0); no host prior function is handed over
            self.L, self.P = tdb._problem(api, self.fl, None, kind=api.PRIOR_CALLBACK)
        self.flags = 0 if prior_kind == "own" else 1

    def settings(self, seed):
        return tdb._settings(self.api, self.lib, self.batch, clustering=self.clustering, max_ndead=self.max_ndead, seed=seed)


_SOLO = {}


def _solo(pb, seed):
    """the solo device-batch run of `seed`: its result, the n of every call and the cube block of every call -- made once, never changed"""
    k = pb.key + (seed,)
    if k not in _SOLO:
        calls, blocks, seen = [], [], []
        pb.api.set_device_batch_callback(_cb(pb.api, pb.like, tdb.np_prior, calls, blocks=blocks, seen=seen))
        try:
            r = tdb._run(pb.api, pb.settings(seed), pb.L, pb.P)
        finally:
            pb.api.set_device_batch_callback(None)
        assert set(seen) == {pb.flags} and r["path"]["device_batch"] == len(calls) > 0
        _SOLO[k] = (r, tuple(calls), blocks)
    return _SOLO[k]


def _in_step(pb, seeds, max_in_flight, callee=None, calls=None, blocks=None, devices=None):
    """the seeds through pchip_run_in_step under a Python callee (or `callee`, registered as it is); the runs' dicts with their arrays
    copied and their blocks given back"""
    from polychordlite_amd import repeats
    calls = [] if calls is None else calls
    seen = []
    pb.api.set_device_batch_callback(callee if callee is not None else _cb(pb.api, pb.like, tdb.np_prior, calls, blocks=blocks, seen=seen))
    try:
        merged, runs = repeats.run_in_step(pb.settings(seeds[0]), pb.L, pb.P, list(seeds), max_in_flight=max_in_flight, devices=devices)
    finally:
        pb.api.set_device_batch_callback(None)
    out = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items() if k != "_owner"} for r in runs]
    del runs, merged
    gc.collect()
    if callee is None:
        assert set(seen) == {pb.flags}
    return out, calls


def _same(step, solo):
    for k in tdb.COUNTERS:
        assert step[k] == solo[k], (k, step[k], solo[k])
    for k in ("dead", "logweights", "entry", "live"):
        a, b = np.ascontiguousarray(step[k]), np.ascontiguousarray(solo[k])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), k
    assert step["path"]["device_batch"] == solo["path"]["device_batch"]


def _same_runs(pb, seeds, max_in_flight, **kw):
    solos = [_solo(pb, s) for s in seeds]
    before = tdb._blocks(pb.lib)
    runs, calls = _in_step(pb, seeds, max_in_flight, **kw)
    assert tdb._blocks(pb.lib) == before
    assert len(runs) == len(seeds)
    for r, (s, _, _) in zip(runs, solos):
        _same(r, s)
    return runs, calls, solos


# ---- 1. the same runs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prior_kind", ["box", "table"])
@pytest.mark.parametrize("batch", [32, 1, 65])
def test_runs_in_step_are_their_solo_runs(engine, batch, prior_kind):
    """three seeds in one group (batch 1: one proposal a run and tick, held to the first 150 dead points for the suite's sake -- nlive is 80, so points born in the run die too)"""
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_gauss, prior_kind, batch, max_ndead=150 if batch == 1 else -1)
    runs, calls, solos = _same_runs(pb, SEEDS, 3)
    assert all(r["batch"] == batch for r in runs)


# ---- 2. one call a tick --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_call_a_tick_for_the_group(engine):
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_gauss, "box", 32)
    runs, calls, solos = _same_runs(pb, SEEDS, 3)
    solo_calls = [c for _, c, _ in solos]
    print("calls in step", len(calls), "solo", [len(c) for c in solo_calls], "largest n in step", max(calls), "solo", [max(c) for c in solo_calls])
    assert sum(calls) == sum(sum(c) for c in solo_calls)                       # every row once
    assert max(len(c) for c in solo_calls) <= len(calls) <= sum(len(c) for c in solo_calls) - 1
    assert max(calls) > max(max(c) for c in solo_calls)                         # a block no run on its own could have made


# ---- 3. the order of the rows -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rows_are_the_solo_blocks_in_seed_order(engine):
    """every block in step is the concatenation, in the order of the seeds, of the blocks the runs' solo callees saw at that tick: walked
    run by run, each run's NEXT solo block either lies at the current place of the block in step, bit for bit, or the run has no rows in this
    tick; every block in step is covered to its end and every solo block is used once.  (prior.kind 0: the callee makes the prior, so the
    cubes come down in every call anyway.)"""
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_gauss, "own", 32)
    solos = [_solo(pb, s) for s in SEEDS]
    blocks = []
    runs, calls = _in_step(pb, SEEDS, 3, blocks=blocks)
    for r, (s, _, _) in zip(runs, solos):
        _same(r, s)
    nxt = [0] * len(SEEDS)
    shared = 0
    for t, blk in enumerate(blocks):
        o, owners = 0, 0
        for k, (_, _, sb) in enumerate(solos):
            if nxt[k] < len(sb):
                b = sb[nxt[k]]
                if o + len(b) <= len(blk) and np.array_equal(blk[o:o + len(b)].view(np.uint64), b.view(np.uint64)):
                    o += len(b); nxt[k] += 1; owners += 1
        assert o == len(blk), (t, o, len(blk))
        shared += owners > 1
    assert nxt == [len(sb) for _, _, sb in solos]
    assert shared > 100


# ---- 4. a callee that never synchronises ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_kernel_callee_never_synchronises(engine, gauss_so):  # noqa: F811
    """the enqueue-only kernel callee: the group's pack in front of its kernel, the group's next tick behind it, in stream order alone"""
    lib = engine.load()
    c0 = -D * (np.log(0.1) + 0.5 * np.log(2 * np.pi))
    gauss_so.gauss_set_scalar(0.5, 0.1, c0)
    L, P = tdb._problem(engine, gauss_so.gauss_loglike, gauss_so.gauss_prior)
    lib.polychord_hip_set_device_batch_callback.argtypes = [C.c_void_p, C.c_void_p]
    solos, solo_calls = [], 0
    for seed in SEEDS:
        ctx = tdb.GaussCtx(0.5, 0.1, c0, 0, 0)
        lib.polychord_hip_set_device_batch_callback(C.cast(gauss_so.gauss_device_batch, C.c_void_p), C.byref(ctx))
        try:
            solos.append(tdb._run(engine, tdb._settings(engine, lib, 32, seed=seed), L, P))
        finally:
            lib.polychord_hip_set_device_batch_callback(None, None)
        assert ctx.calls == solos[-1]["path"]["device_batch"]
        solo_calls += ctx.calls
    from polychordlite_amd import repeats
    before = tdb._blocks(lib)
    ctx = tdb.GaussCtx(0.5, 0.1, c0, 0, 0)
    lib.polychord_hip_set_device_batch_callback(C.cast(gauss_so.gauss_device_batch, C.c_void_p), C.byref(ctx))
    try:
        merged, runs = repeats.run_in_step(tdb._settings(engine, lib, 32, seed=SEEDS[0]), L, P, list(SEEDS), max_in_flight=3)
    finally:
        lib.polychord_hip_set_device_batch_callback(None, None)
    for r, s in zip(runs, solos):
        _same(r, s)
    assert max(s["path"]["device_batch"] for s in solos) <= ctx.calls < solo_calls
    del runs, merged, r
    gc.collect()
    assert tdb._blocks(lib) == before


# ---- 5. clustering, two groups -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_runs_in_step_with_clustering(engine):
    """the twin Gaussian under do_clustering, two seeds, held to 1500 dead points: clusters split, chains in flight are lost mid-nursery, and
    the runs' updates wait as fibers between the tick phases"""
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_twin, "box", 32, clustering=True, max_ndead=1500)
    runs, calls, solos = _same_runs(pb, SEEDS[:2], 2)
    assert all(r["ncluster_peak"] >= 2 for r in runs)


@pytest.mark.gpu
def test_two_groups_one_after_the_other(engine):
    """max_in_flight 2 with three seeds: a group of two, then a group of one, each with a block of its own"""
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_gauss, "box", 32)
    runs, calls, solos = _same_runs(pb, SEEDS, 2)
    assert sum(calls) == sum(sum(c) for _, c, _ in solos)


# ---- 6. endings and refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_callee_returning_one_stops_the_group(engine):
    """... in the middle of a nursery: every run of the group stops, the call returns 5, and nothing is left held"""
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_gauss, "box", 32)
    before = tdb._blocks(lib)
    calls = []
    pb.api.set_device_batch_callback(_cb(engine, pb.like, tdb.np_prior, calls, fail_at=60))
    try:
        from polychordlite_amd import repeats
        with pytest.raises(RuntimeError, match="code 5"):
            repeats.run_in_step(pb.settings(SEEDS[0]), pb.L, pb.P, list(SEEDS), max_in_flight=3)
    finally:
        pb.api.set_device_batch_callback(None)
    gc.collect()
    assert len(calls) == 60 and tdb._blocks(lib) == before


@pytest.mark.gpu
def test_refusals_before_any_device_work(engine, capfd):
    from polychordlite_amd import repeats
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_gauss, "box", 32)
    before = tdb._blocks(lib)
    # no device batch callback registered: today's refusal and message
    engine.set_device_batch_callback(None)
    capfd.readouterr()
    with pytest.raises(RuntimeError, match="code 1"):
        repeats.run_in_step(pb.settings(7), pb.L, pb.P, list(SEEDS), max_in_flight=3)
    assert "pchip_run_in_step does not take a host callback likelihood" in capfd.readouterr().err
    calls = []
    engine.set_device_batch_callback(_cb(engine, pb.like, tdb.np_prior, calls))
    try:
        with pytest.raises(RuntimeError, match="code 1"):
            repeats.run_in_step(pb.settings(7), pb.L, pb.P, list(SEEDS), max_in_flight=3, devices=[0, 0])
        assert "on one device only (ndevices = 2)" in capfd.readouterr().err
        L3, P3 = tdb._problem(engine, pb.fl, None, kind=engine.PRIOR_SOURCE)
        with pytest.raises(RuntimeError, match="code 1"):
            repeats.run_in_step(pb.settings(7), L3, P3, list(SEEDS), max_in_flight=3)
        assert "prior.kind = 3 (source prior) needs a device source likelihood of the same handle" in capfd.readouterr().err
        Ln, Pn = tdb._problem(engine, pb.fl, None, kind=engine.PRIOR_BOX)
        Ln.fn = None
        with pytest.raises(RuntimeError, match="code 1"):
            repeats.run_in_step(pb.settings(7), Ln, pb.P, list(SEEDS), max_in_flight=3)
        assert "needs like.fn" in capfd.readouterr().err
    finally:
        engine.set_device_batch_callback(None)
    assert calls == [] and tdb._blocks(lib) == before


# ---- 7. the callee's own prior --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_prior_kind_0_is_the_callees_own(engine):
    """prior.kind 0 without a host prior function: the callee writes theta from the cubes (flags 0), in step as on its own"""
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_gauss, "own", 32)
    assert not pb.P.fn
    _same_runs(pb, SEEDS, 3)


# ---- 8. torch ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_torch_callable_in_step(engine):
    """repeats.run_in_step_callable: a torch Gaussian marked device_batch under UniformPrior(-1, 1), three seeds.  The callable sums column by
    column in elementwise operations, so a row's answer does not depend on the block; the reference is each seed's solo run through the SAME
    callable and evaluator (`_ctypes_api.run` of repeats.callable_problem).  (Held to numpy's solo runs of the same formula, every counter
    agreed and the dead rows did not: torch's arithmetic with a Python scalar is not numpy's to the last bit.)"""
    import torch
    from polychordlite_amd import repeats
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    lib = engine.load()
    pb = Problem(engine, lib, tdb.np_gauss, "box", 32)
    shapes = []

    def t_like(theta):
        shapes.append((theta.is_cuda, theta.dtype, tuple(theta.shape)))
        r2 = torch.zeros(theta.shape[0], dtype=torch.float64, device=theta.device)
        for d in range(theta.shape[1]):
            r2 = r2 + theta[:, d] * theta[:, d]
        return -np.log(2 * np.pi * 0.01) * theta.shape[1] / 2.0 - r2 / 0.02, r2[:, None]
    t_like.device_batch = True
    prior = dl.UniformPrior(-1.0, 1.0)
    like, pr, ev, keep = repeats.callable_problem(t_like, prior, pb.settings(SEEDS[0]))
    solos = []
    ev.register()
    try:
        for seed in SEEDS:
            solos.append(tdb._run(engine, pb.settings(seed), like, pr))
    except RuntimeError as e:
        if "torch and libpolychord_hip do not share a HIP runtime" in str(e) or "do not share a HIP runtime" in str(ev.error):
            pytest.skip(str(ev.error or e))
        raise
    finally:
        ev.unregister(lib)
    assert ev.error is None
    solo_largest = max(sh[0] for _, _, sh in shapes)
    del shapes[:]
    before = tdb._blocks(lib)
    merged, runs = repeats.run_in_step_callable(t_like, prior, pb.settings(SEEDS[0]), SEEDS, max_in_flight=3)
    assert merged["n_runs"] == 3
    for r, s in zip(runs, solos):
        _same(r, s)
    assert all(c and t == torch.float64 and sh[1] == D for c, t, sh in shapes)
    assert max(sh[0] for _, _, sh in shapes) > solo_largest
    del runs, merged, r
    gc.collect()
    assert tdb._blocks(lib) == before

    def bad(theta):
        raise KeyError("device boom")
    bad.device_batch = True
    with pytest.raises(KeyError):
        repeats.run_in_step_callable(bad, dl.UniformPrior(-1.0, 1.0), pb.settings(SEEDS[0]), SEEDS, max_in_flight=3)
    gc.collect()
    assert tdb._blocks(lib) == before
