"""GPU (-m gpu): the clustered contraction with MORE THAN 64 CLUSTERS ALIVE -- two clusters a lane, the `<2>` instantiations of k_consume_clp,
k_consume_cl and their `_many` forms (pc_clus.hip: wide = nc > 64) -- and the one-wave kill-off beyond 32 clusters, in live sets that the
LDS-resident kernels take, against the CPU oracle and against each other.

What `<2>` has of its own: cl_get / cl_geti with c >= 64, the second register of every per-cluster array, delete_cluster's move-up across the
63 | 64 lane boundary, a split that appends clusters past lane 63, the cross-volume matrix share of a thread.  Until this file the suite ran
none of it: test_gpu_parity.py's shape above 64 clusters (3-D Rastrigin, nlive 2400, 1024 chains) goes through the general kernel in all of
its runs, and its largest shape that fits the LDS peaks at 40 clusters.

Two shapes reach it cheaply (built-in Rastrigin, box (-5.12, 5.12), do_clustering = 1, nDerived = 0, a nursery of 128: cl_layout and clp_layout
come to about 100 KB of the 160 KB budget), found by a scan on the oracle; smaller ones do not (3-D at nlive 1600 - 1800 peaks near 50, 6-D at
nlive 1000 reaches 60, 10-D at nlive 600 - 800 stays below 50):

  A   nDims 10, nlive 1000, num_repeats 10          B   nDims 8, nlive 1000, num_repeats 8, seed 21
      seed  max_ndead  alive at the stop  dead  ndead          max_ndead  alive at the stop  dead  ndead
      21    19000      45                 54    20000          19000      64                 75    20000
      21    20000      73                 86    21000          19500      70                 82    20500
      21    21000      80                 99    22000          20500      69                 88    21500
      21    22000      73                 102   23000          21000      63                 88    22000
      21    whole run  1                  105   43562          whole run  1                  89    37671
      22    22000      77                 103   23000
      23    22000      75                 101   23000

At A's 22000 deaths 102 clusters have died while between 45 and 85 were alive: clusters with an index of 64 or more have died, and others were
moved down across the lane boundary.  B's whole run rises through 64, stays above it and comes back down to one cluster.

Tolerances: test_gpu_parity.py's (_same_run for the oracle, test_clustered_contraction_kernels_agree and test_clustered_kill_off_kernels_agree
for the kernels next to each other), test_par_accept.py's for the runs in step.  pchip_result.path has no slot for a wide launch:
ncluster_peak > 64 in a run whose contractions all went to one LDS-resident kernel (consume_general == 0) means that at least one launch had
nc > 64 and took that kernel's `<2>`.

Engine runs and oracle runs are made once and shared by the tests (the dicts below); nothing writes to them."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_api as orc

pytestmark = pytest.mark.gpu

BOX = (-5.12, 5.12)
#         nDims nlive num_repeats batch
SHAPES = {"A": (10, 1000, 10, 128), "B": (8, 1000, 8, 128)}
GENERAL, END_AT_DEATH, KILLOFF_GENERAL, SERIAL = 1 << 5, 1 << 8, 1 << 9, 1 << 10      # settings.ablate (pc_state.h)
KO_MAXC = 56                                                                            # pc_clus.hip

_engine_runs, _oracle_runs = {}, {}


def _settings(api, shape, seed, max_ndead, ablate=0):
    D, nlive, nr, batch = SHAPES[shape]
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, 0)
    s.nlive, s.num_repeats, s.seed, s.batch, s.do_clustering, s.max_ndead, s.ablate = nlive, nr, seed, batch, 1, max_ndead, ablate
    return s, api.make_problem("rastrigin", D, 0, *BOX)


def _engine(api, shape, seed, max_ndead, ablate=0):
    key = (shape, seed, max_ndead, ablate)
    if key not in _engine_runs:
        s, (L, P, keep) = _settings(api, shape, seed, max_ndead, ablate)
        _engine_runs[key] = api.run(s, L, P)
    return _engine_runs[key]


def _oracle(shape, seed, max_ndead):
    key = (shape, seed, max_ndead)
    if key not in _oracle_runs:
        D, nlive, nr, batch = SHAPES[shape]
        so = orc.settings(D, 0, nlive=nlive, num_repeats=nr, seed=seed, batch=batch, do_clustering=1, max_ndead=max_ndead)
        Lo, Po, keep = orc.make_problem("rastrigin", D, *BOX)
        _oracle_runs[key] = orc.run(so, Lo, Po)
    return _oracle_runs[key]


def _same_run(g, o):
    """test_gpu_parity.py's _same_run with clustering.  These runs have clusters that are down to one live point: no covariance, directions 0/0 in
    the reference, in the oracle and in the engine alike, and the babies of such a chain are NaN rows in all three (none of them ever lived:
    one row of A's 23000, five of B's 37671).  As in test_random_configurations_match_oracle the NaNs must sit in the same places, and every
    other number is held to _same_run's 1e-7"""
    for k in ("ndead", "nlike", "niter", "nbatches", "ncluster", "ncluster_dead"):
        assert g[k] == o[k], (k, g[k], o[k])
    assert abs(g["logZ"] - o["logZ"]) < 1e-8
    assert np.allclose(g["logZp"], o["logZp"], atol=1e-8)            # per-cluster evidences of the dead clusters, in order of death
    assert abs(g["logZerr"] - o["logZerr"]) < 1e-8
    assert np.array_equal(np.isnan(g["dead"]), np.isnan(o["dead"]))
    assert not np.isnan(o["dead"][o["logweights"] > -1e29]).any()      # (no point that lived is such a row)
    rel = np.nan_to_num(np.abs(g["dead"] - o["dead"]) / np.maximum(1.0, np.abs(o["dead"])), nan=0.0)
    assert rel.max() < 1e-7
    ok = o["logweights"] > -1e29
    assert np.array_equal(ok, g["logweights"] > -1e29)
    assert np.abs(g["logweights"][ok] - o["logweights"][ok]).max() < 1e-9
    nD = o["post_mean"].size
    assert np.allclose(g["post_mean"][:nD], o["post_mean"], atol=1e-8)


def test_parallel_kernel_above_64_clusters_is_the_oracles_run(engine):
    """k_consume_clp<2>: shape A, seed 21, stopped at 22000 deaths with 73 clusters alive and 102 dead"""
    g = _engine(engine, "A", 21, 22000)
    o = _oracle("A", 21, 22000)
    assert o["ncluster"] > 64 and g["ncluster_peak"] > 64, (o["ncluster"], g["ncluster_peak"])
    assert g["path"]["consume_cl"] > 0 and g["path"]["consume_general"] == 0 and g["path"]["consume_cl_serial"] == 0, g["path"]
    assert g["path"]["killoff_general"] == 1 and o["ncluster"] > KO_MAXC, g["path"]      # (more clusters than k_killoff_cl takes)
    _same_run(g, o)


def test_serial_kernel_through_a_rise_and_a_fall_is_the_oracles_run(engine):
    """k_consume_cl<2> (settings.ablate bit 10), the arbiter of the parallel kernel, against something other than its siblings: shape B as a
    whole run -- up through 64 clusters, 89 deaths of clusters, down to one"""
    g = _engine(engine, "B", 21, -1, SERIAL)
    o = _oracle("B", 21, -1)
    assert g["path"]["consume_cl_serial"] > 0 and g["path"]["consume_cl"] == 0 and g["path"]["consume_general"] == 0, g["path"]
    assert g["ncluster_peak"] > 64 and g["ncluster"] == 1, (g["ncluster_peak"], g["ncluster"])
    _same_run(g, o)


@pytest.mark.parametrize("shape,max_ndead", [("A", 22000), ("B", -1)], ids=["A-22000", "B-whole"])
def test_three_kernels_agree_above_64_clusters(engine, shape, max_ndead):
    """the assertions of test_gpu_parity.py's test_clustered_contraction_kernels_agree, where each of the three kernels keeps two clusters a lane:
    the default run (k_consume_clp), bit 10 (k_consume_cl), bit 5 (the general kernel, whose wide code is its own).  (equal_nan: the NaN rows
    of _same_run's note are the same rows in every run, as in test_clustered_contraction_with_a_chain_that_has_no_number; every number is
    still compared bit for bit)"""
    api = engine
    a, c, b = (_engine(api, shape, 21, max_ndead, ab) for ab in (0, SERIAL, GENERAL))
    assert a["path"]["consume_general"] == 0 and a["path"]["consume_cl"] > 0 and a["path"]["consume_cl_serial"] == 0, a["path"]
    assert c["path"]["consume_cl_serial"] > 0 and c["path"]["consume_cl"] == 0 and c["path"]["consume_general"] == 0, c["path"]
    assert b["path"]["consume_general"] > 0 and b["path"]["consume_cl"] == 0 and b["path"]["consume_cl_serial"] == 0, b["path"]
    assert a["ncluster_peak"] >= 2 and a["ncluster_dead"] >= 2
    assert a["ncluster_peak"] > 64, a["ncluster_peak"]
    for b in (c, b):
        for k in ("ndead", "nlike", "niter", "ncluster", "ncluster_dead", "nupdates", "ncluster_peak", "nlike_failed"):
            assert a[k] == b[k], (k, a[k], b[k])
        assert abs(a["logZ"] - b["logZ"]) < 1e-10 and abs(a["logZerr"] - b["logZerr"]) < 1e-10
        assert np.array_equal(a["dead"][:, :-2], b["dead"][:, :-2], equal_nan=True) and np.array_equal(a["dead"][:, -1], b["dead"][:, -1], equal_nan=True)
        assert np.abs(a["logweights"] - b["logweights"]).max() < 1e-9
        assert np.allclose(a["logZp"], b["logZp"], atol=1e-9) and np.allclose(a["varlogZp"], b["varlogZp"], atol=1e-9)
        assert np.array_equal(a["live"], b["live"])
    # with settings.ablate bit 8 -- a pass ends at a cluster's death -- the parallel and the serial kernel are bit for bit the same run
    a8, c8 = (_engine(api, shape, 21, max_ndead, ab) for ab in (END_AT_DEATH, END_AT_DEATH | SERIAL))
    assert a8["path"]["consume_cl"] > 0 and a8["path"]["consume_cl_serial"] == 0 and a8["path"]["consume_general"] == 0, a8["path"]
    assert c8["path"]["consume_cl_serial"] > 0 and c8["path"]["consume_cl"] == 0 and c8["path"]["consume_general"] == 0, c8["path"]
    assert a8["ncluster_peak"] > 64 and c8["ncluster_peak"] > 64
    assert np.array_equal(a8["dead"], c8["dead"], equal_nan=True) and np.array_equal(a8["live"], c8["live"])
    if a8["path"]["nn_fallbacks"] == 0:      # (a baby for the full search ends k_consume_clp's pass -- new references -- where k_consume_cl searches on the spot)
        assert a8["logZ"] == c8["logZ"] and np.array_equal(a8["logweights"], c8["logweights"])
    else:
        assert abs(a8["logZ"] - c8["logZ"]) < 1e-12 and np.abs(a8["logweights"] - c8["logweights"]).max() < 1e-10
    assert a8["ndead"] == a["ndead"] and abs(a8["logZ"] - a["logZ"]) < 1e-10


def test_three_seeds_in_step_above_64_clusters_equal_their_solo_runs(engine, monkeypatch):
    """k_consume_clp_many<2>: shape A to 22000 deaths, seeds 21, 22, 23 round by round together.  The three cross 64 clusters at different
    rounds, so the cohort groups them by the width of their per-cluster registers and both widths of the shared launch occur.
    (pchip_run_repeats deals clustered runs to min(4, max_in_flight) groups that go side by side, pc_merge.hip: three runs would be three
    groups of one and share no launch -- slice_step 0.  PC_REPEATS_SCHED=1, read at every call, keeps them in one group.)"""
    from polychordlite_amd import repeats
    seeds = [21, 22, 23]
    s, (L, P, keep) = _settings(engine, "A", 0, 22000)
    monkeypatch.setenv("PC_REPEATS_SCHED", "1")
    merged, runs = repeats.run_repeats(s, L, P, seeds, max_in_flight=3)
    for seed, step in zip(seeds, runs):
        own = _engine(engine, "A", seed, 22000)
        for k in ("ndead", "nlike", "niter", "nupdates", "ncluster", "ncluster_dead", "ncluster_peak", "logZ", "varlogZ"):
            assert own[k] == step[k], (seed, k, own[k], step[k])
        for k in ("dead", "logweights", "entry", "live"):
            assert np.asarray(own[k]).tobytes() == np.asarray(step[k]).tobytes(), (seed, k)
        assert own["ncluster_peak"] > 64 and step["ncluster_peak"] > 64, (seed, own["ncluster_peak"], step["ncluster_peak"])
        assert step["path"]["slice_step"] > 0, (seed, step["path"])          # (the runs really were in step)
        assert step["path"]["consume_cl"] > 0 and step["path"]["consume_general"] == 0 and step["path"]["consume_cl_serial"] == 0, (seed, step["path"])


def test_one_wave_kill_off_beyond_32_clusters(engine):
    """k_killoff_cl with clusters in lanes 32 and up: shape A, seed 21, stopped at 19000 deaths with 45 clusters alive -- bit for bit the
    general kernel's kill-off (settings.ablate bit 9), as test_gpu_parity.py's test_clustered_kill_off_kernels_agree asks, and the oracle's run"""
    a, b = (_engine(engine, "A", 21, 19000, ab) for ab in (0, KILLOFF_GENERAL))
    o = _oracle("A", 21, 19000)
    assert 32 < o["ncluster"] <= KO_MAXC, o["ncluster"]                   # (clusters alive when the run stopped: the kill-off's)
    assert a["path"]["killoff_cl"] == 1 and a["path"]["killoff_general"] == 0, a["path"]
    assert b["path"]["killoff_general"] == 1 and b["path"]["killoff_cl"] == 0, b["path"]
    assert a["ncluster"] >= 2
    for k in ("ndead", "nlike", "niter", "ncluster", "ncluster_dead", "nupdates", "ncluster_peak"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["logZ"] == b["logZ"] and a["logZerr"] == b["logZerr"], (a["logZ"], b["logZ"])
    assert np.array_equal(a["dead"], b["dead"], equal_nan=True)
    assert np.array_equal(a["logweights"], b["logweights"])
    assert np.array_equal(a["logZp"], b["logZp"]) and np.array_equal(a["varlogZp"], b["varlogZp"])
    assert np.array_equal(a["post_mean"], b["post_mean"])
    _same_run(a, o)                                                       # (ncluster: the engine's count at the stop is the oracle's)
