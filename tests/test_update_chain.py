"""GPU (-m gpu): the one-cluster update by its five launches (pc_update.hip: k_upd_flag, k_upd_index_self, k_upd_gather, k_upd_fold,
k_upd_final) against the same stages as a chain of two launches (settings.ablate bit 16: k_upd_flag_scan, k_upd_chain), which shares the
row loads, the moment tiles and the final stage with them but finds its rows, folds and finishes by itself.  The chain finds the same rows
in the same order, puts them into the same tile rows, flushes at the same places and adds the records in the same groups, so the two are
the same run bit for bit -- counters, evidence, every dead and live row.

What the cases cover:
  * nlive 2000, num_repeats 40, a whole run: the nursery's launch is nlive / 2 = 1000 steps, a mark falls anywhere in it, so most of the
    run's ~30 updates leave more than 256 deaths behind the mark (two or more dead-after-mark workgroups with full pieces);
  * nlive 400 a second time with batch = 1: a launch of the contraction is then ONE step, so the death that passes the trigger is its
    last -- every update falls on a launch with no deaths after the mark (the dead-after-mark workgroup finds nothing to add);
  * nDims 5 (one tile), 24 (two tiles, the 24-bound of the factorisation), 70 (five tiles: locate + gather in the chain, fold, final and
    factorisation by the launches behind it)."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_api as orc

pytestmark = pytest.mark.gpu

CHAIN = 1 << 16


def _settings(api, D, nDer, **kw):
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _problem(api, kind, D, nDer):
    if kind == "gaussian":
        return api.make_problem("gaussian", D, nDer)
    olib = orc.load()
    ic = np.zeros((D, D)); ld = C.c_double()
    olib.pc_random_invcov(12345, D, C.c_double(0.1), orc.dptr(ic), C.byref(ld))
    return api.make_problem("corr_gaussian", D, nDer, invcov=ic, mean=np.full(D, 0.5), logdet=ld.value)


def _same_run(a, b):
    for k in ("ndead", "nlike", "niter", "nupdates"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["logZ"] == b["logZ"] and a["logZerr"] == b["logZerr"], (a["logZ"], b["logZ"], a["logZerr"], b["logZerr"])
    assert np.array_equal(a["dead"], b["dead"], equal_nan=True)
    assert np.array_equal(a["live"], b["live"], equal_nan=True)
    assert a["path"]["update_fused"] == b["path"]["update_fused"]


@pytest.mark.parametrize("D,nDer,nlive,nr,kind,whole", [(20, 2, 2000, 40, "gaussian", True), (20, 2, 400, 20, "gaussian", False), (5, 1, 200, 10, "gaussian", False),
                                                        (24, 0, 256, 48, "gaussian", False), (70, 0, 150, 8, "corr_gaussian", False)])
def test_two_launches_are_the_five_launches(engine, D, nDer, nlive, nr, kind, whole):
    api = engine
    L, P, keep = _problem(api, kind, D, nDer)
    batches = (0, 1) if (D, nlive) == (20, 400) else (0,)
    for batch in batches:
        runs = []
        for ab in (0, CHAIN):
            kw = dict(nlive=nlive, num_repeats=nr, seed=11, batch=batch)
            if not whole: kw["max_ndead"] = 8 * nlive
            s = _settings(api, D, nDer, **kw)
            s.ablate = ab
            runs.append(api.run(s, L, P))
        a, b = runs
        assert a["nupdates"] >= 3, a["nupdates"]
        # (the chain is pool mode's, and pool mode comes with the deferred update: without them both runs would be the five launches)
        assert a["path"]["update_fused"] >= 3 and a["path"]["pool_mode"] == 1 and a["path"]["defer_update"] == 1, a["path"]
        _same_run(a, b)
