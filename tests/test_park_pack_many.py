"""The pack of a group of runs in step alone (pchip_park_pack_many: k_park_index_many and k_park_rows_many, pc_park.hip) against numpy, exactly.

One workgroup a run makes the run's local ranks -- the ballot / LDS / carry scheme of k_park_index, so every run's size sits on its edges: one
chain, one wavefront less and more one, one chunk of 1024 and more one --; one wavefront per (run, chain) forms the run's base, the sum of the
counts of the runs before it (one wave reduction: up to 64 runs), writes the global rank and copies the row into the ONE block.  The runs of a
call have different sizes, so the row kernel's grid is wider than most runs are long."""
import ctypes as C

import numpy as np
import pytest

SIZES = (1, 63, 64, 65, 1024, 1025)
NDIMS = (1, 64, 65)
SENTINEL = -7.25


def _flags(kind, n, salt=0):
    if kind == "none":
        return np.zeros(n, dtype=np.int32)
    if kind == "all":
        return np.ones(n, dtype=np.int32)
    if kind == "alternating":
        return (np.arange(n) % 2).astype(np.int32)
    return (np.random.default_rng(1234 + n + 7919 * salt).random(n) < 0.37).astype(np.int32) * (3 + salt)      # (any non-zero value is a flag)


def _sizes(nruns):
    """nruns sizes that go through all of SIZES, starting somewhere else for every nruns"""
    return [SIZES[(r + nruns) % len(SIZES)] for r in range(nruns)]


def _check(engine, nchains, need, D):
    nchains = np.asarray(nchains)
    off = np.concatenate([[0], np.cumsum(nchains)])
    prop = np.random.default_rng(D * 10007 + int(off[-1])).random((int(off[-1]), D))
    cube = np.full_like(prop, SENTINEL)
    rank, counts, total, out = engine.park_pack_many(nchains, need, prop, cube=cube)
    flag = need != 0
    want_counts = np.array([np.count_nonzero(flag[off[r]:off[r + 1]]) for r in range(len(nchains))])
    # the global rank is the ascending enumeration of ALL flagged chains, run after run: the solo order, concatenated
    want_rank = np.where(flag, np.cumsum(flag) - 1, -1).astype(np.int32)
    assert np.array_equal(counts, want_counts), (list(nchains), D, counts, want_counts)
    assert total == int(want_counts.sum()), (list(nchains), D, total)
    assert np.array_equal(rank, want_rank), (list(nchains), D)
    assert np.array_equal(out[:total].view(np.uint64), prop[flag].view(np.uint64)), (list(nchains), D)
    assert np.all(out[total:] == SENTINEL), (list(nchains), D)      # nothing behind the total was written


@pytest.mark.gpu
@pytest.mark.parametrize("nruns", [1, 2, 3, 64])
def test_group_pack_is_the_concatenated_enumeration(engine, nruns):
    for nchains in ([[n] for n in SIZES] if nruns == 1 else [_sizes(nruns)]):      # (one run: every size in a call of its own)
        for kind in ("all", "alternating", "random"):
            need = np.concatenate([_flags(kind, n, salt=r) for r, n in enumerate(nchains)])
            for D in NDIMS:
                _check(engine, nchains, need, D)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["front", "middle", "end", "everywhere"])
def test_runs_without_a_flag(engine, where):
    """a run that is through with its nursery while the others go on -- the first of the group, one in the middle, the last -- adds nothing
    to the bases behind it; and a tick that finds nothing at all: total 0, no row written"""
    nchains = [65, 1025, 1, 64, 1024, 63]
    empty = {"front": [0], "middle": [1, 3], "end": [5], "everywhere": range(6)}[where]
    need = np.concatenate([_flags("none" if r in empty else "random", n, salt=r) for r, n in enumerate(nchains)])
    for D in NDIMS:
        _check(engine, nchains, need, D)


@pytest.mark.gpu
def test_group_pack_refuses_what_it_cannot_take(engine):
    lib = engine.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    lib.pchip_park_pack_many.argtypes = [C.c_int, ip, C.c_int, ip, dp, ip, ip, ip, dp, C.c_int]
    lib.pchip_park_pack_many.restype = C.c_int
    n65 = np.ones(65, dtype=np.int32)
    flags, rank, counts = np.zeros(65, dtype=np.int32), np.zeros(65, dtype=np.int32), np.zeros(65, dtype=np.int32)
    rows = np.zeros((65, 1))
    tot = C.c_int(0)
    p = lambda a: a.ctypes.data_as(ip)      # noqa: E731

    def call(nruns, nch=p(n65), need=p(flags), prop=engine.dptr(rows), rk=p(rank), cnt=p(counts), total=C.byref(tot), cube=engine.dptr(rows)):
        return lib.pchip_park_pack_many(nruns, nch, 1, need, prop, rk, cnt, total, cube, -1)
    assert call(0) == 1 and call(-1) == 1 and call(65) == 1
    assert call(1, nch=None) == 1 and call(1, need=None) == 1 and call(1, prop=None) == 1 and call(1, rk=None) == 1
    assert call(1, cnt=None) == 1 and call(1, total=None) == 1 and call(1, cube=None) == 1
    assert call(64) == 0 and tot.value == 0
