"""GPU (-m gpu): the straight-line stepping out of k_slice (pc_slice_body.inc: the first pc_step_spec candidates of each side of a
closed-form slice evaluated at once, the reference's loop only behind them) where it can go wrong -- a side that ends exactly at the
last straight-line candidate, a side that needs the loop behind the candidates, one side that does and the other that does not.

The parity tests of test_gpu_parity.py run shapes where a slice rarely steps out more than once.  Deep stepping out comes up when the
step w is small against the slice, i.e. when the covariance comes from barely more live points than dimensions: the shapes here.  Each
is the built-in Gaussian, seed 11, with nurseries a multiple of four chains so that the helped LEAN = 1 kernel is the one launched.

The default run must be, bit for bit, the run under settings.ablate 64 (pc_slice_t.hip: a lane per chain, the independent restatement
of the kernel's arithmetic with the reference's loop), 8192 (no helper wavefront) and both.

Measured once on the histogram build (tools/dev/gpu_slice_hist.py, profiles/slice_stepping.json; every chain, whole run),
the share of slices whose loop was entered behind the straight-line candidates -- on the right only / on the left only / on both sides:
    nDims 20, nDer 2, nlive 32, num_repeats 20, batch 16              12.3 % / 12.7 % / 0.11 % (27 of 24960 slices)
    nDims 24, nDer 2, nlive 40, num_repeats 48, batch 20              11.9 % / 11.8 % / 0.13 % (113 of 87360)
    nDims  8, nDer 0, nlive 16, num_repeats 16, batch 8               11.0 % / 10.9 % / 0.02 % (1 of 5376)
    nDims  5, nDer 2, nlive 24, num_repeats 25, batch 12, box (-0.5, 1.5)   9.7 % /  9.5 % / never
    nDims 12, nDer 2, nlive 24, num_repeats 25, batch 12, box (-0.5, 1.5)  11.7 % / 11.7 % / 0.04 % (8 of 21900)
In five dimensions no side of any slice takes a third iteration and no slice has the loop on both sides, with nlive 24, 20, 16 or 12
alike: the chord through a five-dimensional contour is too short against the step.  The same box with twelve dimensions reaches it, so
that shape stands next to the five-dimensional one (kept: it is the one with the right-only and left-only cases in a box that is not
the unit cube at the smallest nDims).  A side that ends exactly at the last straight-line candidate is a third of all sides everywhere.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(20, 2, 32, 20, 16, None), (24, 2, 40, 48, 20, None), (8, 0, 16, 16, 8, None), (5, 2, 24, 25, 12, (-0.5, 1.5)),
          (12, 2, 24, 25, 12, (-0.5, 1.5))]


def _run(api, D, nDer, nlive, nr, batch, box, ablate):
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    s.nlive, s.num_repeats, s.seed, s.batch, s.ablate = nlive, nr, 11, batch, ablate
    L, P, keep = api.make_problem("gaussian", D, nDer, *box) if box is not None else api.make_problem("gaussian", D, nDer)
    return api.run(s, L, P)


@pytest.mark.parametrize("D,nDer,nlive,nr,batch,box", SHAPES)
def test_deep_stepping_out_is_the_same_run_in_every_kernel(engine, D, nDer, nlive, nr, batch, box):
    a = _run(engine, D, nDer, nlive, nr, batch, box, 0)
    assert a["ndead"] > nlive and a["batch"] % 4 == 0
    for ab in (64, 8192, 64 | 8192):
        b = _run(engine, D, nDer, nlive, nr, batch, box, ab)
        for k in ("ndead", "nlike", "niter", "nupdates", "nbatches"):
            assert a[k] == b[k], (ab, k, a[k], b[k])
        assert a["logZ"] == b["logZ"] and a["logZerr"] == b["logZerr"], ab
        for k in ("dead", "logweights", "live", "post_mean"):
            assert np.array_equal(a[k], b[k]), (ab, k)
