"""k_nhats_w<DMAX, NW> (pc_bases.hip): part 1 of the split launch of a run on its own at nDims <= 24, one grade, by a workgroup of NW = 4
wavefronts for the same 64 / nDims bases -- all 256 threads deal the workgroup's stream calls, wavefronts 1 ... 3 make the decks of the chains
that start in the workgroup (the s-th start by wavefront 1 + s % 3) and end, wavefront 0 orthogonalises and stores -- against NW = 1
(settings.ablate bit 20: one wavefront does all of it, the kernel as it was) and against k_nhats<.., 64, 1> (bit 19: a wavefront a basis).
Everything BYTE FOR BYTE: a deviate is a function of its stream position, a deck of (keys, nursery, chain), whichever lane or wavefront makes it.

  CPU   the shapes below, from their arithmetic: some workgroup's stream calls are no multiple of 256 (fewer than 256, and more than 256),
        some workgroup holds two chain starts, some more than three (the dealing of decks to wavefronts wraps), some nursery ends in a short
        workgroup, some workgroup holds the end of one chain and the start of the next
  GPU   pchip_directions path 1 (raw bases, directions, widths) and pchip_deck_records (the 66 ints a chain, tags included): default against
        bit 20 and against bit 19; a whole run (nDims 5, nlive 50, num_repeats 10) under the three: every array and counter of the result
"""
import ctypes as C

import numpy as np
import pytest

NW = 4
DIMS = (1, 2, 7, 9, 10, 16, 17, 20, 24)
CHAINS = (1, 2, 65)
BASES = (1, 2, 3)
BIT_WAVE1, BIT_BASIS = 1 << 20, 1 << 19


def _repeats(D, nb):
    """num_repeats for nb bases a chain, at most 64: the last basis truncated to one vector (nb = 2 also full)"""
    nr = [(nb - 1) * D + 1] + ([2 * D] if nb == 2 else [])
    assert all(n <= 64 and -(-n // D) == nb for n in nr)
    return nr


def _workgroups(D, nb, nchains):
    """per workgroup of k_nhats_w: (bases, stream calls, chain starts, chains touched)"""
    per, nbases, NC = 64 // D, nchains * nb, (D * D + 1) // 2
    out = []
    for g0 in range(0, nbases, per):
        gs = range(g0, min(g0 + per, nbases))
        out.append((len(gs), len(gs) * NC, sum(1 for g in gs if g % nb == 0), len({g // nb for g in gs})))
    return per, out


def test_the_shapes_reach_every_case_of_the_workgroup():
    calls_under = calls_over = two_starts = starts_wrap = short_last = straddle = False
    for D in DIMS:
        for nb in BASES:
            for nchains in CHAINS:
                per, wgs = _workgroups(D, nb, nchains)
                assert sum(w[0] for w in wgs) == nchains * nb and sum(w[2] for w in wgs) == nchains
                for nbw, calls, starts, chains in wgs:
                    calls_under |= calls < 64 * NW and calls % 64 != 0
                    calls_over |= calls > 64 * NW and calls % (64 * NW) != 0
                    two_starts |= starts == 2
                    starts_wrap |= starts > NW - 1
                    straddle |= nb > 1 and chains > 1
                short_last |= len(wgs) > 1 and wgs[-1][0] < per
    assert calls_under and calls_over and two_starts and starts_wrap and short_last and straddle
    # nDims 1: NC = 1, a workgroup of a single chain has fewer stream calls than one wavefront has lanes
    assert _workgroups(1, 3, 1)[1] == [(3, 3, 1, 1)]
    # the metric configuration's shape: three bases, 600 stream calls = 2 x 256 + 88
    assert _workgroups(20, 2, 65)[1][0][:2] == (3, 600)


def _settings(api, D, nDer=0, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _rows_and_factor(D, nchains):
    rng = np.random.default_rng(1000 * D + nchains)
    rows = np.zeros((nchains, 2 * D + 2))
    rows[:, :D] = rng.uniform(0.2, 0.8, (nchains, D)); rows[:, D:2 * D] = rows[:, :D]
    rows[:, -1] = -rng.uniform(1.0, 2.0, nchains)
    Lh = np.tril(rng.uniform(-0.3, 0.3, (D, D)), -1) + np.diag(rng.uniform(0.5, 1.5, D))
    return rows, Lh


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
def test_directions_and_decks_byte_for_byte(engine, D):
    """default (four wavefronts a workgroup) against bit 20 (one) and bit 19 (k_nhats, a wavefront a basis): raw bases, directions and widths
    through path 1 of pchip_directions, the deck records with their tags through pchip_deck_records"""
    api = engine
    L, P, keep = api.make_problem("gaussian", D, 0)
    for nchains in CHAINS:
        rows, Lh = _rows_and_factor(D, nchains)
        for nb in BASES:
            for nr in _repeats(D, nb):
                new, one, basis = (api.directions(_settings(api, D, num_repeats=nr, seed=57 + D, ablate=ab), L, P, 6, rows, Lh, 1)
                                   for ab in (0, BIT_WAVE1, BIT_BASIS))
                assert new is not None and one is not None and basis is not None
                assert new["raw"].shape == (nchains, nb, D, D) and np.all(np.isfinite(new["raw"])) and np.all(np.isfinite(new["nhat"]))
                for what, other in (("bit 20", one), ("bit 19", basis)):
                    for k in ("raw", "nhat", "nhat_w"):
                        assert new[k].tobytes() == other[k].tobytes(), (D, nchains, nr, what, k)
                recs = [api.deck_records(_settings(api, D, num_repeats=nr, seed=57 + D, ablate=ab), L, P, 6, nchains, fill=-7)
                        for ab in (0, BIT_WAVE1, BIT_BASIS)]
                assert all(r is not None and r.shape == (nchains, 66) for r in recs)
                for what, other in (("bit 20", recs[1]), ("bit 19", recs[2])):
                    assert recs[0].tobytes() == other.tobytes(), (D, nchains, nr, what)
                # what a record is (pc_deck_keyed): an odd tag of its own, the first direction stays, the others a permutation, the rest themselves
                rec = recs[0]
                assert np.all(rec[:, 0] & 1 == 1) and len({(int(a), int(b)) for a, b in rec[:, :2]}) == nchains
                deck = rec[:, 2:]
                assert np.all(deck[:, 0] == 0) and np.all(np.sort(deck[:, :nr], axis=1) == np.arange(nr)) and np.all(deck[:, nr:] == np.arange(nr, 64))


NOT_RESULTS = ("t_generate", "t_loop", "t_final", "t_total", "t_setup", "t_results", "t_teardown", "kernel_time", "_owner")


@pytest.mark.gpu
def test_a_whole_run_is_the_same_under_the_three_bases_kernels(engine):
    """nDims 5, nlive 50, num_repeats 10, one seed, to termination: every array and counter of the result (all but the clocks)"""
    api = engine
    D = 5
    L, P, keep = api.make_problem("gaussian", D, 0)
    runs = [api.run(_settings(api, D, nlive=50, num_repeats=10, seed=29, ablate=ab), L, P) for ab in (0, BIT_WAVE1, BIT_BASIS)]
    assert runs[0]["ndead"] >= 8 * 50
    checked = 0
    for what, r in zip(("bit 20", "bit 19"), runs[1:]):
        assert set(r) == set(runs[0])
        for k, a in runs[0].items():
            if k in NOT_RESULTS:
                continue
            b = r[k]
            if isinstance(a, np.ndarray):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, k)
            else:
                assert a == b, (what, k, a, b)
            checked += 1
    assert checked >= 2 * 20
