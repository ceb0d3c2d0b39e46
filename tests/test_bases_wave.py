"""k_nhats_w (pc_bases.hip): part 1 of the split launch of a run on its own at nDims <= 24, one grade -- 64 / nDims bases a wavefront, bases
numbered flat over the nursery, the deviates made in place, the chains' deck records written by the wavefront that holds a chain's first basis
-- against k_nhats<.., 64, 1> (settings.ablate bit 19: a wavefront a basis), which it replaces, and against the packed bases of the runs in
step (path 2 of pchip_directions, bit 7 of a run).  Everything BYTE FOR BYTE: per vector the operations and their order are k_nhats'.

  CPU   the flat numbering restated in numpy as the kernel computes it (block, lane -> basis, vector; which wavefront writes which deck)
        against brute force over nDims 1 ... 24, 1 ... 3 bases a chain, 1 ... 70 chains
  GPU   pchip_directions path 1: raw bases, directions and widths, bit 19 against default (and against path 2 where it exists)
        pchip_deck_records: the 66 ints a chain as they lie behind the bases, tags included; num_repeats 65 leaves the block as it was
        whole runs: default, bit 19 and bit 7 agree on every array and counter; three seeds in step are their solo runs
"""
import ctypes as C

import numpy as np
import pytest

DIMS = (1, 2, 7, 8, 9, 16, 17, 20, 21, 22, 24)
PER = (64, 32, 9, 8, 7, 4, 3, 3, 3, 2, 2)
CHAINS = (1, 2, 5, 64, 65)
BIT_WAVE, BIT_PACKED = 1 << 19, 1 << 7


# ---------------------------------------------------------------------------------------------------------------- the numbering
def wave_layout(D, nb, nchains):
    """as k_nhats_w computes it, wavefront by wavefront and lane by lane: -> (owner [nwaves][64][3] = (chain, basis, vector) or -1 for a lane
    that only keeps the barriers, decks [nwaves] = the chains whose record the wavefront writes)"""
    per, nbases = 64 // D, nchains * nb
    nwaves = (nbases + per - 1) // per
    tid = np.arange(64)
    sub = tid // D
    i = tid - sub * D
    owner = np.full((nwaves, 64, 3), -1)
    decks = []
    for w in range(nwaves):
        g = w * per + sub
        active = (sub < per) & (g < nbases)
        chain = g // nb
        owner[w, active] = np.stack([chain, g - chain * nb, i], axis=1)[active]
        nbw = min(per, nbases - w * per)
        decks.append([(w * per + s) // nb for s in range(nbw) if (w * per + s) % nb == 0])
    return owner, decks


def test_flat_numbering_covers_every_vector_once_and_every_deck_once():
    assert tuple(64 // D for D in DIMS) == PER
    single_last = straddle = False
    for D in range(1, 25):
        per = 64 // D
        for nb in (1, 2, 3):
            for nchains in range(1, 71):
                owner, decks = wave_layout(D, nb, nchains)
                # brute force, the other way round: where must vector (chain, basis, vector) be
                want = np.full(owner.shape, -1)
                for chain in range(nchains):
                    for basis in range(nb):
                        g = chain * nb + basis
                        want[g // per, (g % per) * D:(g % per) * D + D] = [(chain, basis, v) for v in range(D)]
                assert np.array_equal(owner, want), (D, nb, nchains)
                assert np.all(owner[:, per * D:] == -1)
                # every chain's record by exactly one wavefront: the one that holds vector 0 of its basis 0
                assert sorted(c for d in decks for c in d) == list(range(nchains))
                first = {int(owner[w, l, 0]): int(w) for w, l in np.argwhere((owner[:, :, 1] == 0) & (owner[:, :, 2] == 0))}
                assert first == {c: w for w, d in enumerate(decks) for c in d}
                single_last |= (nchains * nb) % per == 1 and per > 1
                ch = owner[:, :, 0]
                straddle |= nb > 1 and bool(np.any(ch.max(1) != np.where(ch >= 0, ch, nchains).min(1)))
    assert single_last and straddle


# ---------------------------------------------------------------------------------------------------------------- the kernels
def _settings(api, D, nDer=0, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _rows_and_factor(D, nchains):
    rng = np.random.default_rng(100 * D + nchains)
    rows = np.zeros((nchains, 2 * D + 2))
    rows[:, :D] = rng.uniform(0.2, 0.8, (nchains, D)); rows[:, D:2 * D] = rows[:, :D]
    rows[:, -1] = -rng.uniform(1.0, 2.0, nchains)
    Lh = np.tril(rng.uniform(-0.3, 0.3, (D, D)), -1) + np.diag(rng.uniform(0.5, 1.5, D))
    return rows, Lh


def _repeats(D):
    """num_repeats for 1, 2 and 3 bases a chain: a truncated last basis, full bases, a truncated third -- and where no number of CHAINS times
    1, 2 or 3 is a multiple of per = 64 / nDims (nDims 7 and 9), for per bases a chain, so that some nursery fills its last wavefront"""
    per = 64 // D
    reps = [1, 2 * D, 2 * D + 1]
    if not any((n * nb) % per == 0 for n in CHAINS for nb in (1, 2, 3)):
        reps.append((per - 1) * D + 1)
    return reps


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
def test_bases_of_the_split_launch_byte_for_byte(engine, D):
    """bit 19 (k_nhats<.., 64, 1>) against default (k_nhats_w) through path 1 of pchip_directions, and against path 2 (k_deviates_t +
    k_bases_packed) where it exists: raw bases, directions, widths.  With 2 chains of 2 bases at per = 3 the last wavefront holds a single
    basis and the first one the end of chain 0 and the start of chain 1; per divides the number of bases in some cases and not in others."""
    api = engine
    per = 64 // D
    L, P, keep = api.make_problem("gaussian", D, 0)
    divides = set()
    for nchains in CHAINS:
        rows, Lh = _rows_and_factor(D, nchains)
        for nr in _repeats(D):
            nb = -(-nr // D)
            divides.add((nchains * nb) % per == 0)
            outs = []
            for ablate, path in ((0, 1), (BIT_WAVE, 1), (0, 2)):
                outs.append(api.directions(_settings(api, D, num_repeats=nr, seed=31 + D, ablate=ablate), L, P, 9, rows, Lh, path))
            new, old, packed = outs
            assert new is not None and old is not None and (packed is not None) == (D >= 2)
            assert new["raw"].shape == (nchains, nb, D, D) and np.all(np.isfinite(new["raw"])) and np.all(np.isfinite(new["nhat"]))
            for other in (old, packed):
                if other is None:
                    continue
                for k in ("raw", "nhat", "nhat_w"):
                    assert new[k].tobytes() == other[k].tobytes(), (D, nchains, nr, k)
    assert divides == {True, False}


@pytest.mark.gpu
@pytest.mark.parametrize("D", (20, 7))
def test_deck_records_byte_for_byte(engine, D):
    """the records as they lie behind the bases, tags included: bit 19 against default; num_repeats 65: neither kernel writes one, and the
    block comes back as it went in"""
    api = engine
    L, P, keep = api.make_problem("gaussian", D, 0)
    for nr in (2, 40, 64, 65):
        for nchains in (1, 5, 65):
            new = api.deck_records(_settings(api, D, num_repeats=nr, seed=77), L, P, 4, nchains, fill=-7)
            old = api.deck_records(_settings(api, D, num_repeats=nr, seed=77, ablate=BIT_WAVE), L, P, 4, nchains, fill=-7)
            assert new is not None and old is not None and new.shape == (nchains, 66)
            assert new.tobytes() == old.tobytes(), (D, nr, nchains)
            if nr > 64:
                assert np.all(new == -7)
                continue
            # what a record is (pc_deck_keyed): the first direction stays, the others are a permutation, lanes past num_repeats hold themselves
            assert np.all(new[:, 0] & 1 == 1) and len({(int(a), int(b)) for a, b in new[:, :2]}) == nchains
            deck = new[:, 2:]
            assert np.all(deck[:, 0] == 0) and np.all(np.sort(deck[:, :nr], axis=1) == np.arange(nr)) and np.all(deck[:, nr:] == np.arange(nr, 64))


RUN_KEYS = ("ndead", "nlike", "niter", "nupdates", "nbatches")
RUN_ARRAYS = ("dead", "logweights", "live", "post_mean")
RUN_SHAPES = [(20, 2, 32, 16, 20), (24, 0, 40, 20, 48), (10, 1, 50, 0, 30)]      # nDims, nDerived, nlive, batch, num_repeats


def _same_run(a, b, what):
    for k in RUN_KEYS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["logZ"] == b["logZ"] and a["logZerr"] == b["logZerr"], what
    for k in RUN_ARRAYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("D,nDer,nlive,batch,nr", RUN_SHAPES)
def test_whole_runs_agree_under_the_three_bases_kernels(engine, D, nDer, nlive, batch, nr):
    """default (k_nhats_w), bit 19 (k_nhats) and bit 7 (the packed kernels, no deck records) -- cut by max_ndead and run to termination"""
    api = engine
    L, P, keep = api.make_problem("gaussian", D, nDer)
    for extra in (dict(max_ndead=5 * nlive), {}):
        runs = [api.run(_settings(api, D, nDer, nlive=nlive, num_repeats=nr, seed=13, batch=batch, ablate=ab, **extra), L, P)
                for ab in (0, BIT_WAVE, BIT_PACKED)]
        assert runs[0]["ndead"] >= (5 * nlive if extra else 8 * nlive)
        for ab, r in zip(("bit 19", "bit 7"), runs[1:]):
            _same_run(runs[0], r, (D, ab, bool(extra)))


@pytest.mark.gpu
def test_three_seeds_in_step_are_their_solo_runs(engine):
    """in step the bases come from the packed kernels, alone from k_nhats_w"""
    from polychordlite_amd.repeats import run_repeats
    api = engine
    D, nDer, nlive, batch, nr = RUN_SHAPES[0]
    L, P, keep = api.make_problem("gaussian", D, nDer)
    seeds = [41, 42, 43]
    solo = [api.run(_settings(api, D, nDer, nlive=nlive, num_repeats=nr, seed=sd, batch=batch), L, P) for sd in seeds]
    merged, runs = run_repeats(_settings(api, D, nDer, nlive=nlive, num_repeats=nr, seed=0, batch=batch), L, P, seeds, max_in_flight=len(seeds))
    for sd, one, r in zip(seeds, solo, runs):
        _same_run(one, r, sd)
