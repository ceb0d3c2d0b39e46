"""A run owns its device and pinned blocks through one ledger (RunBlocks, pc_blocks.h) and its teardown releases from it.

CPU: tools/dev/blocks_record -- the ledger's rules over malloc-backed primitives that count, a stand-alone program under the host
address and undefined-behaviour sanitizers.
GPU (-m gpu): pchip_blocks_in_use counts the blocks the two caches have obtained from the driver and somebody holds.  After a first run
of a scenario (and pchip_result_free) that count is the baseline; whatever the scenario does afterwards -- the same run again, a run that
fails at an injected host fault, a host likelihood that raises, runs in step that fail -- must leave it where it was.  The same for the
kernel-level doors of the tests (pc_doors.h) and the device maximiser: each twice, and two of them failing at an injected fault."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polychordlite_amd", "csrc")


def test_the_ledger_follows_its_rules():
    """allocate / release all; release one in the middle, then all; regrow keeps the first `keep` elements and releases the old block; a
    block handed over outlives release-all; an exception between allocations, then release-all, leaves nothing out; release-all twice;
    10 000 transient pairs leave the ledger as long as it was; the destructor releases nothing.  (A missing compiler fails this test.)"""
    subprocess.run(["make", "-C", CSRC, "blocks_record"], check=True, capture_output=True, text=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "dev", "blocks_record")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "8 scenarios, 0 checks failed" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _counts(lib):
    """(device, pinned) blocks in use, once every result nobody refers to any more has been freed"""
    gc.collect()
    d, p = C.c_long(-1), C.c_long(-1)
    lib.pchip_blocks_in_use(C.byref(d), C.byref(p))
    return d.value, p.value


def _settings(api, D, nDer, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.fixture
def lib(engine):
    lib = engine.load()
    lib.pchip_set_capacity.argtypes = [C.c_int, C.c_int]
    lib.pchip_blocks_in_use.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    lib.pchip_blocks_in_use.restype = None
    yield lib
    lib.pchip_set_capacity(128, 0)
    lib.pchip_inject_fault(0)


CLUSTERED = dict(nlive=300, num_repeats=6, seed=5, batch=40, do_clustering=1)


def _plain(api, lib, what):
    """the scenario's run: a function that makes it once and returns its dead points (a copy: the result is freed before it returns)"""
    if what == "gaussian":
        L, P, keep = api.make_problem("gaussian", 6, 1)
        s = _settings(api, 6, 1, nlive=200, num_repeats=12, seed=7)
    elif what in ("clustered", "cluster_growth"):
        L, P, keep = api.make_problem("rastrigin", 2, 0, -5.12, 5.12)
        s = _settings(api, 2, 0, **CLUSTERED)
    elif what == "callback":
        lib.polychord_hip_set_gaussian.argtypes = [C.c_double, C.c_double]
        lib.polychord_hip_set_gaussian(0.5, 0.1)
        L, P, keep = api.make_problem("gaussian", 3, 0)
        L.kind, L.fn = api.LIKE_CALLBACK, C.cast(lib.polychord_hip_gaussian, C.c_void_p)
        s = _settings(api, 3, 0, nlive=60, num_repeats=6, seed=3)
    elif what == "phantom_growth":
        L, P, keep = api.make_problem("gaussian", 6, 1)
        s = _settings(api, 6, 1, nlive=200, num_repeats=12, seed=7, batch=32, compression_factor=0.01)

    def once():
        if what == "phantom_growth":
            lib.pchip_set_capacity(-1, 600)
        if what == "cluster_growth":
            lib.pchip_set_capacity(2, -1)
        g = api.run(s, L, P)
        assert g["ndead"] > 0 and (what != "cluster_growth" or g["ncluster_dead"] > 8)
        return np.array(g["dead"]), keep
    return once


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["gaussian", "clustered", "callback", "phantom_growth", "cluster_growth"])
def test_a_run_gives_back_what_it_took(engine, lib, what):
    """the same run three times: after the second and the third the caches' counts are what they were after the first"""
    once = _plain(engine, lib, what)
    once()
    base = _counts(lib)
    assert base[0] >= 0 and base[1] >= 0
    for _ in range(2):
        once()
        assert _counts(lib) == base


# the kernel-level doors (pc_doors.h) and the device maximiser: an engine's ledger or a ledger of their own, given back by the one guard
def _chains(api, lib, D, nchains, nr):
    """pchip_slice_chains for nchains chains seeded near the peak of the built-in Gaussian: (code, babies)"""
    nT = 2 * D + 2
    L, P, keep = api.make_problem("gaussian", D, 0)
    seeds = _live_rows(D, nchains)
    chol = np.ascontiguousarray(0.02 * np.eye(D))
    babies = np.zeros((nchains, nr, nT))
    s = _settings(api, D, 0, num_repeats=nr, seed=11)
    rc = lib.pchip_slice_chains(C.byref(s), C.byref(L), C.byref(P), 5, nchains, api.dptr(seeds), api.dptr(chol), float(seeds[:, -1].min()) - 4.0,
                                api.dptr(babies), None, None)
    return rc, babies


def _live_rows(D, n):
    """n rows [cube | theta | birth | logL] of the built-in Gaussian (mu 0.5, sigma 0.1) in the unit box, one cluster"""
    rows = np.zeros((n, 2 * D + 2))
    cubes = 0.5 + 0.04 * np.random.default_rng(10 * D + n).standard_normal((n, D))
    rows[:, :D], rows[:, D:2 * D], rows[:, -2] = cubes, cubes, -1e30
    rows[:, -1] = -D * (np.log(0.1) + 0.5 * np.log(2 * np.pi)) - 0.5 * np.sum(((cubes - 0.5) / 0.1) ** 2, axis=1)
    return rows


def _maximise(api, D, n, raw=False):
    """pchip_maximise_device on n rows of the built-in Gaussian: the wrapper's dict, or (raw) the code alone"""
    L, P, keep = api.make_problem("gaussian", D, 0)
    s = _settings(api, D, 0, logzero=-1e30)
    live, cl = _live_rows(D, n), np.zeros(n, dtype=np.int32)
    if not raw:
        return api.maximise_device(s, L, P, dict(live=live, live_cluster=cl, post_mean=None))
    lib, m = api.load(), api.Maximum()
    rc = lib.pchip_maximise_device(C.byref(s), C.byref(L), C.byref(P), api.dptr(live), cl.ctypes.data_as(C.POINTER(C.c_int)), n, None, 0, C.byref(m))
    lib.pchip_maximum_free(C.byref(m))
    return rc


def _doors(api, lib):
    """every door once at a small shape, by name: nDims 2 ... 4, 4 ... 8 chains or rows, one or two clusters"""
    D, n = 3, 6
    L, P, keep = api.make_problem("gaussian", D, 0)
    rows = _live_rows(D, n)
    chol = np.tril(np.full((D, D), 0.01)) + 0.05 * np.eye(D)
    s = lambda: _settings(api, D, 0, num_repeats=2 * D, seed=5)
    rng = np.random.default_rng(3)
    x = rng.uniform(0.2, 0.8, (8, D)); ph = rng.uniform(0.2, 0.8, (4, D))
    two = np.vstack([0.2 + 0.01 * rng.standard_normal((4, 2)), 0.8 + 0.01 * rng.standard_normal((4, 2))])
    need, prop = np.array([1, 0, 1, 1, 0], dtype=np.int32), rng.uniform(size=(5, D))

    def chains():
        rc, babies = _chains(api, lib, D, n, 2 * D)
        assert rc == 0

    return {
        "slice_chains": chains,
        "directions path 0": lambda: api.directions(s(), L, P, 5, rows, chol, 0),
        "directions path 1": lambda: api.directions(s(), L, P, 5, rows, chol, 1),
        "deck_records": lambda: api.deck_records(s(), L, P, 5, n),
        "prior_transform": lambda: api.prior_transform([("uniform", (0, 1)), ("uniform", (10, 20))], rng.uniform(size=(4, 2))),
        "park_pack": lambda: api.park_pack(need, prop),
        "park_pack_many": lambda: api.park_pack_many([3, 2], need, prop),
        "par_accept": lambda: api.par_accept(np.arange(6.0), np.array([0.5, 2.5, 7.0, 1.5])),
        "update_factors path 0": lambda: api.update_factors(x, np.array([0, 1] * 4), ph, np.zeros(4), np.array([0, 1, 0, 1]), [-1.0, -1.0], 0),
        "update_factors path 1": lambda: api.update_factors(x, np.zeros(8, dtype=np.int32), ph, np.zeros(4), np.zeros(4, dtype=np.int32), [-1.0], 1),
        "cluster_update path 0": lambda: api.cluster_update([dict(live=two, cluster=np.zeros(8, dtype=np.int32))], path=0),
        "cluster_update path 1": lambda: api.cluster_update([dict(live=two, cluster=np.zeros(8, dtype=np.int32))] * 2, path=1),
        "maximise_device": lambda: _maximise(api, D, 2 * (D + 1)),
    }


@pytest.mark.gpu
def test_each_door_gives_back_what_it_took(engine, lib):
    """every kernel-level door and the device maximiser twice: the caches' counts after the second call are those after the first"""
    for name, door in _doors(engine, lib).items():
        door()
        base = _counts(lib)
        door()
        assert _counts(lib) == base, name


@pytest.mark.gpu
def test_a_failed_door_gives_back_what_it_took(engine, lib):
    """pchip_inject_fault(1) -- the next device block of at least 256 KB is refused: a host exception before any launch -- under
    pchip_slice_chains and under pchip_maximise_device: each returns 7 (an injection nobody consumed would return 0 and fail here), leaves
    the counts at the baseline, and the good call after it gives the first good call's output bit for bit.  nDims = 10 is the smallest at
    which both set-ups ask for such a block whatever the caches round to: the dead points' array, (64 nlive + 4 batch + 1024) rows of
    2 nDims + 2 doubles, is 1568 x 22 x 8 = 275 968 bytes for eight chains and 1540 x 22 x 8 = 271 040 for the maximiser's engine."""
    api, D = engine, 10
    rc, good = _chains(api, lib, D, 8, 4)
    assert rc == 0
    base = _counts(lib)
    lib.pchip_inject_fault(1)
    rc, _ = _chains(api, lib, D, 8, 4)
    assert rc == 7
    assert _counts(lib) == base
    rc, again = _chains(api, lib, D, 8, 4)
    assert rc == 0 and again.tobytes() == good.tobytes()
    assert _counts(lib) == base

    good = _maximise(api, D, 2 * (D + 1))
    assert good["status"] == [0, 0]
    base = _counts(lib)
    lib.pchip_inject_fault(1)
    assert _maximise(api, D, 2 * (D + 1), raw=True) == 7
    assert _counts(lib) == base
    again = _maximise(api, D, 2 * (D + 1))
    assert _counts(lib) == base
    assert good.keys() == again.keys()
    for k, v in good.items():
        assert (v is None and again[k] is None) or np.asarray(v).tobytes() == np.asarray(again[k]).tobytes(), k


@pytest.mark.gpu
def test_the_door_counts_what_is_held(engine, lib):
    """a result that has not been freed holds its three pinned arrays (dead points, weights, entry contours) and no device block; NULL for
    either count is allowed"""
    api = engine
    L, P, keep = api.make_problem("gaussian", 6, 1)
    s = _settings(api, 6, 1, nlive=200, num_repeats=12, seed=7)
    del api.run(s, L, P)["dead"]
    base = _counts(lib)
    g = api.run(s, L, P)
    assert _counts(lib) == (base[0], base[1] + 3)
    d = C.c_long(-1)
    lib.pchip_blocks_in_use(C.byref(d), None); lib.pchip_blocks_in_use(None, None)
    assert d.value == base[0]
    del g
    assert _counts(lib) == base


@pytest.mark.gpu
@pytest.mark.parametrize("fault,code", [(1, 7), (2, 8), (3, 7)])
def test_a_failed_run_gives_back_what_it_took(engine, lib, fault, code, capfd):
    """pchip_inject_fault 1, 2, 3 (a device allocation, the cluster capacity at a split, the growth of the phantom array: host exceptions, all
    three) on the clustered shape of test_robustness.py: the failed call leaves the counts at the baseline, and so does the good run
    after it, whose dead points are the first good run's bit for bit"""
    api = engine
    L, P, keep = api.make_problem("rastrigin", 2, 0, -5.12, 5.12)
    good = np.array(api.run(_settings(api, 2, 0, **CLUSTERED), L, P)["dead"])
    base = _counts(lib)
    if fault == 3:
        lib.pchip_set_capacity(-1, 300)
    lib.pchip_inject_fault(fault)
    r = api.Result(); s = _settings(api, 2, 0, **CLUSTERED)
    assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(P), C.byref(r)) == code
    assert not r.dead and not r.logweights and not r.entry
    assert _counts(lib) == base
    lib.pchip_set_capacity(128, 0)
    again = np.array(api.run(_settings(api, 2, 0, **CLUSTERED), L, P)["dead"])
    assert _counts(lib) == base
    assert np.array_equal(again, good)


@pytest.mark.gpu
def test_a_host_likelihood_that_raises_gives_back_what_the_run_took(engine, lib, tmp_path):
    """a Python likelihood that raises while the live points are generated (generate_live_callback), through the binding's own route for a
    host exception: the callback keeps the exception, asks the run to stop and the run returns early; run_polychord raises it afterwards"""
    from polychordlite_amd import pypolychord
    from polychordlite_amd.pypolychord.settings import PolyChordSettings
    st = PolyChordSettings(3, 0, nlive=60, num_repeats=6, base_dir=str(tmp_path), file_root="f", feedback=0, write_resume=False,
                           read_resume=False, maximise=False, write_prior=False, seed=3)
    calls = [0]; fail_at = [0]

    def like(theta):
        calls[0] += 1
        if calls[0] == fail_at[0]:
            raise ValueError("the likelihood raised")
        return float(-0.5 * np.sum(((theta - 0.5) / 0.1) ** 2))

    pypolychord.run_polychord(like, 3, 0, st, lambda c: c.copy())
    base = _counts(lib)
    assert calls[0] > 60
    calls[0] = 0; fail_at[0] = 25                               # (of the sixty prior samples the live set starts from)
    with pytest.raises(ValueError, match="the likelihood raised"):
        pypolychord.run_polychord(like, 3, 0, st, lambda c: c.copy())
    assert 25 <= calls[0] <= 60                                 # (the run ended inside the generation of its live points)
    assert _counts(lib) == base
    fail_at[0] = 0
    pypolychord.run_polychord(like, 3, 0, st, lambda c: c.copy())
    assert _counts(lib) == base


@pytest.mark.gpu
def test_runs_in_step_give_back_what_they_took(engine, lib):
    """four runs in step, then the same with a device allocation failing in one run's set-up (1) and with the cluster capacity failing
    (2: these runs do not cluster, so the fault stays armed and is disarmed here -- the case tests/test_merge.py has is a clustered
    one, below), then four clustered ones with it: the counts are the baseline after each call"""
    from polychordlite_amd.repeats import run_repeats
    api = engine
    L, P, keep = api.make_problem("gaussian", 6, 1)
    s = _settings(api, 6, 1, nlive=150, num_repeats=12)
    seeds = [71, 72, 73, 74]
    merged, runs = run_repeats(s, L, P, seeds, max_in_flight=4)
    logZ = merged["logZ"]
    del merged, runs
    base = _counts(lib)
    for fault in (1, 2):
        lib.pchip_inject_fault(fault)
        if fault == 1:
            with pytest.raises(RuntimeError):
                run_repeats(s, L, P, seeds, max_in_flight=4)
        else:
            merged, runs = run_repeats(s, L, P, seeds, max_in_flight=4)
            assert merged["logZ"] == logZ
            del merged, runs
        lib.pchip_inject_fault(0)
        assert _counts(lib) == base
    merged, runs = run_repeats(s, L, P, seeds, max_in_flight=4)
    assert merged["logZ"] == logZ
    del merged, runs
    assert _counts(lib) == base
    # the clustered case of tests/test_merge.py: one run fails at a split, the fibers still suspended are cancelled and unwind
    L, P, keep = api.make_problem("rastrigin", 3, 0, -5.12, 5.12)
    s = _settings(api, 3, 0, nlive=200, num_repeats=9, do_clustering=1)
    seeds = [81, 82, 83, 84]
    merged, runs = run_repeats(s, L, P, seeds, max_in_flight=4)
    del merged, runs
    base = _counts(lib)
    lib.pchip_inject_fault(2)
    with pytest.raises(RuntimeError):
        run_repeats(s, L, P, seeds, max_in_flight=4)
    assert _counts(lib) == base
