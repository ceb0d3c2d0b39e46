"""GPU (-m gpu): where the dead rows of a run's tail are copied and who moves the kill-off's rows, held against the path that does neither.

A run on its own (pchip_run) ends through k_final_par without its row loop plus k_final_rows (pc_par.hip), and requests the loop's
last dead rows and the live rows on the copy stream before the kill-off, beside it (Engine::end_a).  The same seed as one of two runs
in step (repeats.run_repeats -> pc_run_many) keeps the row loop inside k_final_par_many and every tail copy behind the kill-off.
Both must hand back the same run, bit for bit: only copies and their order differ.

Shapes, the smallest at which the new code can go wrong:
  kill-off rows   live counts 20 (less than a wavefront of rows), 64 / 65 (a workgroup boundary of k_final_rows; 16 and 17
                  workgroups of four rows), 1024 / 1025 (one pass / two passes of final_par_body, whose second pass has one row),
                  at nDims 2, num_repeats 2; and live count 65 at nDims 40, nDerived 3: a row of 85 doubles, longer than a
                  wavefront's 64 lanes.
  copies          nDims 4, num_repeats 8, nlive 50 and 51 (odd row offsets).  A copy leaves at the first update behind
                  4 nlive new dead rows.  The loop of a run has about nlive (H + log(1 / precision_criterion)) deaths; for
                  the 0.1-wide Gaussian in four dimensions H = 4 log(1 / (0.1 sqrt(2 pi e))) = 3.5, so precision_criterion
                  1e-6 (13.8) makes about 17 nlive: more than the 12 nlive that three copies in the loop need whatever the
                  updates' spacing.  path[] has no free slot that the Python mirror's pinned length lets through, so the
                  loop's deaths are asserted, not a counter.
  grow_dead       the dead array's first estimate is 64 nlive + 4 batch + 1024 rows and doubles when a nursery might not fit
                  (Engine::ensure_capacity).  nDims 8, nlive 40, the 1e-6-wide Gaussian: H = 8 log(1 / (1e-6 sqrt(2 pi e)))
                  = 99, so the run makes about 107 nlive = 4300 dead rows against an estimate of 3664: the array and its pinned
                  mirror move between two copies, after twenty of them.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#         nDims nDer nlive num_repeats  more settings, more of make_problem
KILLOFF = [(2, 0, 20, 2), (2, 0, 64, 2), (2, 0, 65, 2), (2, 0, 1024, 2), (2, 0, 1025, 2), (40, 3, 65, 2)]
COPIES = [(4, 0, 50, 8), (4, 0, 51, 8)]
SEED = 7


def _both(api, D, nDer, nlive, nr, sigma=0.1, **kw):
    """the run on its own and the same seed as the first of two runs in step"""
    from polychordlite_amd import repeats
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    s.nlive, s.num_repeats, s.seed = nlive, nr, SEED
    for k, v in kw.items():
        setattr(s, k, v)
    L, P, keep = api.make_problem("gaussian", D, nDer, sigma=sigma)
    own = api.run(s, L, P)
    merged, runs = repeats.run_repeats(s, L, P, [SEED, SEED + 1], max_in_flight=2)
    return own, runs[0]


def _same_run(own, step):
    assert own["path"]["killoff_par"] == 1 and step["path"]["killoff_par"] == 1, (own["path"], step["path"])
    for k in ("ndead", "nlike", "niter", "nupdates", "logZ", "varlogZ"):
        assert own[k] == step[k], (k, own[k], step[k])
    for k in ("dead", "logweights", "entry", "live"):
        assert own[k].shape == step[k].shape and np.array_equal(own[k], step[k]), k


def _killoff_rows_are_the_sorted_live_set(r):
    n, logL = r["live"].shape[0], r["nTotal"] - 1
    tail = np.asarray(r["dead"])[r["ndead"] - n:]
    assert n > 0 and np.all(np.diff(tail[:, logL]) >= 0)
    live = np.asarray(r["live"])
    assert np.array_equal(tail, live[np.argsort(live[:, logL], kind="stable")])


@pytest.mark.parametrize("D,nDer,nlive,nr", KILLOFF)
def test_killoff_rows_by_their_own_kernel(engine, D, nDer, nlive, nr):
    own, step = _both(engine, D, nDer, nlive, nr)
    assert own["live"].shape[0] == nlive
    _same_run(own, step)
    _killoff_rows_are_the_sorted_live_set(own)
    _killoff_rows_are_the_sorted_live_set(step)


@pytest.mark.parametrize("D,nDer,nlive,nr", COPIES)
def test_copies_of_the_loop_and_of_the_tail(engine, D, nDer, nlive, nr):
    own, step = _both(engine, D, nDer, nlive, nr, precision_criterion=1e-6)
    assert own["ndead"] - own["live"].shape[0] > 12 * nlive, (own["ndead"], nlive)      # three copies in the loop at the least
    _same_run(own, step)
    _killoff_rows_are_the_sorted_live_set(own)


def test_the_dead_array_grows_between_two_copies(engine):
    D, nlive, batch = 8, 40, 20
    own, step = _both(engine, D, 0, nlive, 4, sigma=1e-6, batch=batch)
    assert own["batch"] == batch and own["ndead"] + batch + nlive + 16 > 64 * nlive + 4 * batch + 1024, own["ndead"]      # (ensure_capacity's test at the last nursery)
    _same_run(own, step)
    _killoff_rows_are_the_sorted_live_set(own)
