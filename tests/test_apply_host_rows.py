"""GPU (-m gpu): a run on its own in pool mode whose row kernel's launch carries the update's flag pass (k_apply_pool_flag, pc_rows.hip,
pc_upd_flag.h), held against the parent's path: settings.ablate bit 17, the flags by k_upd_flag in a launch of its own behind k_apply_pool.
Only who writes the ids of a round's rows and the update's keep bytes, and in which launch, differs, so every array and counter a run returns
is the same, byte for byte.  (The other half of the same proposal -- k_apply_pool storing the dead rows into the host's pinned mirror --
was measured and taken out, with its cases: profiles/apply_fused.json.  The file keeps the name the proposal gave it.)

A built-in Gaussian, one cluster, no files: pool mode and the deferred update are taken (asserted from path[]).

Shapes, the smallest at which the new code can go wrong:
  (a) nDims 4, nlive 50, num_repeats 7      a nursery's region is 25 chains of 7 rows = 175 rows: its ends are never on a 256-row block of the flag
                                            pass, every boundary block holds rows with ids in memory and rows whose ids the pass forms itself, and
                                            a lane's four rows lie in two chains
  (b) nDims 20, nlive 64, num_repeats 40    32 chains of 40 rows = 1280 rows: exactly five blocks, every lane's rows whole in the region
  (d) max_ndead                             10: inside the first nursery of (a); 105 and 160: just behind the update marks at about 2 and 3 nlive
                                            deaths, in the round that passes the mark: truncated launches, with and without a pending update
  (e) precision_criterion                   sixteen values a factor 1.35 apart on (a): the loop ends after 25 deaths a round at the most while the marks
                                            come every nlive = 50 deaths, so the ending round passes a mark for about a quarter of the values -- the
                                            round whose flags are made and never used, the unused-nursery corner of Engine::round_finish
  (f) two runs back to back                 the second run's keep bytes and block counts come back from the block cache with the first run's in them

The library has no test entry that hands back the update's keep bytes and block counts (pchip_update_factors returns the covariance, the
factor and the count), so the flag pass is held by these whole-run equalities: a keep byte, a block count or a dropped id that differed would
change the covariance the next nursery is sampled from, and with it every later row.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARENT = 1 << 17                                      # PC_ABL_FLAG_LAUNCH
SEED = 11
#        nDims nlive num_repeats sigma  more settings
CASES = {"a": (4, 50, 7, 0.1, {}),
         "b": (20, 64, 40, 0.1, {}),
         "d10": (4, 50, 7, 0.1, {"max_ndead": 10}), "d105": (4, 50, 7, 0.1, {"max_ndead": 105}), "d160": (4, 50, 7, 0.1, {"max_ndead": 160})}
CASES.update({"e%02d" % k: (4, 50, 7, 0.1, {"precision_criterion": 0.5 / 1.35 ** k}) for k in range(16)})
SCALARS = ("logZ", "varlogZ", "ndead", "nlike", "niter", "nbatches", "nrounds", "nupdates", "ncluster", "ncluster_dead", "nTotal", "batch",
           "nlike_failed", "ncluster_peak", "nlike_grade", "path")
ARRAYS = ("dead", "logweights", "entry", "live", "live_cluster", "logZp", "varlogZp", "post_mean", "post_var")
_parent_runs = {}


def _settings(api, case, ablate, seed=SEED):
    D, nlive, nr, sigma, more = CASES[case]
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, 0)
    s.nlive, s.num_repeats, s.seed, s.ablate = nlive, nr, seed, ablate
    for k, v in more.items():
        setattr(s, k, v)
    return s, api.make_problem("gaussian", D, 0, sigma=sigma)


def _run(api, case, ablate, seed=SEED):
    s, (L, P, keep) = _settings(api, case, ablate, seed)
    r = api.run(s, L, P)
    assert r["path"]["pool_mode"] == 1 and r["path"]["defer_update"] == 1, r["path"]
    return r


def _parent(api, case):
    """the run by the parent's paths, made once a case and left as it is"""
    if case not in _parent_runs:
        _parent_runs[case] = _run(api, case, PARENT)
    return _parent_runs[case]


def _same(a, b):
    for k in SCALARS:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_run_is_the_parents(engine, case):
    want = _parent(engine, case)
    if case.startswith("d"):
        assert want["ndead"] < _parent(engine, "a")["ndead"] and want["nrounds"] < _parent(engine, "a")["nrounds"], want["ndead"]      # (the loop was cut short)
    _same(_run(engine, case, 0), want)


def test_two_runs_back_to_back(engine):
    want = _parent(engine, "b")
    first = _run(engine, "b", 0)
    _same(first, want)
    del first                                         # (its blocks go back to the cache)
    other = _run(engine, "b", 0, seed=SEED + 1)
    _same(other, _run(engine, "b", PARENT, seed=SEED + 1))
    del other
    _same(_run(engine, "b", 0), want)


def test_three_seeds_in_step_equal_their_solo_runs(engine):
    from polychordlite_amd import repeats
    seeds = [SEED, SEED + 1, SEED + 2]
    s, (L, P, keep) = _settings(engine, "a", 0)
    merged, runs = repeats.run_repeats(s, L, P, seeds, max_in_flight=3)
    for seed, step in zip(seeds, runs):
        own = _run(engine, "a", 0, seed=seed)
        for k in ("ndead", "nlike", "niter", "nupdates", "logZ", "varlogZ"):
            assert own[k] == step[k], (k, own[k], step[k])
        for k in ("dead", "logweights", "entry", "live"):
            assert np.asarray(own[k]).tobytes() == np.asarray(step[k]).tobytes(), (seed, k)
