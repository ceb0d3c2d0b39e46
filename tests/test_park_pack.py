"""The pack of the device batch callback alone (pchip_park_pack: k_park_index and k_park_rows, pc_park.hip) against numpy, exactly.

The index kernel is one workgroup of 1024 threads: ballot / popcount prefixes inside a wavefront, the wavefronts' counts through LDS, a carry
from chunk to chunk.  The sizes sit on those edges -- one chain, one wavefront less and more one, one chunk and more one, several chunks with
a ragged tail -- and the rows on the row kernel's (one coordinate, less than a wavefront, exactly one, one more, four a lane)."""
import numpy as np
import pytest

NCHAINS = (1, 63, 64, 65, 1024, 1025, 2500)
NDIMS = (1, 20, 64, 65, 256)
SENTINEL = -7.25


def _flags(kind, n):
    if kind == "none":
        return np.zeros(n, dtype=np.int32)
    if kind == "all":
        return np.ones(n, dtype=np.int32)
    if kind == "alternating":
        return (np.arange(n) % 2).astype(np.int32)
    return (np.random.default_rng(1234 + n).random(n) < 0.37).astype(np.int32) * 3      # (any non-zero value is a flag)


@pytest.mark.gpu
@pytest.mark.parametrize("nchains", NCHAINS)
def test_pack_is_the_ascending_enumeration(engine, nchains):
    for kind in ("none", "all", "alternating", "random"):
        need = _flags(kind, nchains)
        want_rank = np.where(need != 0, np.cumsum(need != 0) - 1, -1).astype(np.int32)
        n = int(np.count_nonzero(need))
        for D in NDIMS:
            prop = np.random.default_rng(D * 10007 + nchains).random((nchains, D))
            cube = np.full((nchains, D), SENTINEL)
            rank, count, out = engine.park_pack(need, prop, cube=cube)
            assert count == n, (kind, D, count, n)
            assert np.array_equal(rank, want_rank), (kind, D)
            # row rank[c] is chain c's proposal, bit for bit: the needed chains in ascending order
            assert np.array_equal(out[:n].view(np.uint64), prop[need != 0].view(np.uint64)), (kind, D)
            # nothing behind the count was written
            assert np.all(out[n:] == SENTINEL), (kind, D)


@pytest.mark.gpu
def test_pack_refuses_what_it_cannot_take(engine):
    import ctypes as C
    lib = engine.load()
    one = np.zeros(1, dtype=np.int32); row = np.zeros((1, 1))
    ip = C.POINTER(C.c_int)
    lib.pchip_park_pack.argtypes = [C.c_int, C.c_int, ip, C.POINTER(C.c_double), ip, ip, C.POINTER(C.c_double), C.c_int]
    lib.pchip_park_pack.restype = C.c_int
    cnt = C.c_int(0)
    assert lib.pchip_park_pack(0, 1, one.ctypes.data_as(ip), engine.dptr(row), one.ctypes.data_as(ip), C.byref(cnt), engine.dptr(row), -1) == 1
    assert lib.pchip_park_pack(1, 1, None, engine.dptr(row), one.ctypes.data_as(ip), C.byref(cnt), engine.dptr(row), -1) == 1
