"""Handles for the likelihoods / prior that run fused inside the slice-sampling kernel.

Passing one of these objects as `loglikelihood` (or `prior`) to `run` / `run_polychord` makes the
engine evaluate it on the GPU instead of calling back into Python for every proposal; they are also
ordinary callables (the formula is evaluated by the library's host function), so the same script runs
unchanged against the reference `pypolychord`.
"""
import ctypes as C

import numpy as np

from .. import _ctypes_api as api


class _Builtin:
    symbol = None

    def _fn(self):
        lib = api.load()
        f = getattr(lib, self.symbol)
        f.restype = C.c_double
        f.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int]
        return f

    def configure(self, nDims):
        pass

    def __call__(self, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        self.configure(theta.size)
        phi = np.zeros(max(self.nDerived, 1))
        logL = self._fn()(api.dptr(theta), theta.size, api.dptr(phi), self.nDerived)
        return (logL, phi[:self.nDerived]) if self.nDerived else logL


class Gaussian(_Builtin):
    """likelihoods/examples/gaussian.f90: N(mu, sigma^2 I); phi = (radius, log volume)"""
    symbol = "polychord_hip_gaussian"

    def __init__(self, mu=0.5, sigma=0.1, nDerived=0):
        self.mu, self.sigma, self.nDerived = mu, sigma, nDerived

    def configure(self, nDims):
        api.load().polychord_hip_set_gaussian(self.mu, self.sigma)


class Rastrigin(_Builtin):
    """likelihoods/examples/rastrigin.f90"""
    symbol = "polychord_hip_rastrigin"
    nDerived = 0


class TwinGaussian(_Builtin):
    """likelihoods/examples/twin_gaussian.f90; phi = (+-1 by theta_1 > 0.5)"""
    symbol = "polychord_hip_twin_gaussian"

    def __init__(self, sigma=0.1, nDerived=0):
        self.sigma, self.nDerived = sigma, nDerived

    def configure(self, nDims):
        api.load().polychord_hip_set_gaussian(0.0, self.sigma)


class CorrelatedGaussian(_Builtin):
    """likelihoods/examples/random_gaussian.f90 with an explicit inverse covariance"""
    symbol = "polychord_hip_corr_gaussian"
    nDerived = 0

    def __init__(self, invcov, mean, logdetcov):
        self.invcov = np.ascontiguousarray(invcov, dtype=np.float64)
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.logdetcov = float(logdetcov)

    def configure(self, nDims):
        api.load().polychord_hip_set_corr_gaussian(nDims, api.dptr(self.invcov), api.dptr(self.mean), self.logdetcov)


class Source(_Builtin):
    """The user's own likelihood as HIP device source (include/polychord_hip.h: pchip_source_create and its kin), compiled at run time and
    evaluated inside the sampling kernels.  The arguments are those of `_ctypes_api.source_create`: `source` the text; `data` its data
    block; `nterms` the terms form, `nsums` with it several sums per evaluation; `residuals` / `precision` the quadratic form;
    `shared` that many shared values beside any of these three (pchip_source_create_shared: the text defines pchip_shared_value);
    `batched=True` with `residuals` / `precision`: the batched quadratic form (pchip_source_create_quad_batch), up to 4096 residuals, a
    round's proposals evaluated at once on the matrix cores -- under `UniformPrior` or `TablePrior` only, and `maximise=True` is skipped with a message;
    `prior=True`: the text defines pchip_prior_param as well (pass `SourcePrior(this)` as the prior); `options`: -D / -U compiler options.
    The handle is made on first use (RuntimeError with the compiler's log if the text does not compile).  Under `UniformPrior`,
    `TablePrior` or `SourcePrior` the whole run stays on the device; under any other prior callable the prior is called on the host and
    the likelihood is evaluated on the device, a round's proposals in one launch.  Called like a function it is the library's host function
    (polychord_hip_source_loglike: one kernel launch a call, for single evaluations).  `close()` destroys the handle."""
    symbol = "polychord_hip_source_loglike"

    def __init__(self, source, nDerived=0, data=None, nterms=None, nsums=None, residuals=None, precision=None, prior=False, options=None, shared=None,
                 batched=False):
        if batched and residuals is None:
            raise ValueError("batched=True is the batched quadratic form: it needs residuals (and precision)")
        self.batched = bool(batched)
        self.source, self.nDerived, self.data, self.nterms, self.nsums = source, nDerived, data, nterms, nsums
        self.residuals, self.precision, self.prior, self.options = residuals, precision, prior, options
        self.shared = shared
        self._handle = None

    @property
    def handle(self):
        if self._handle is None:
            self._handle = api.source_create(self.source, options=self.options or (), data=self.data, nterms=self.nterms, prior=self.prior,
                                             nsums=self.nsums, residuals=self.residuals, precision=self.precision, shared=self.shared,
                                             **({"batched": True} if self.batched else {}))
        return self._handle

    def configure(self, nDims):
        api.set_source(self.handle)

    def __call__(self, theta):
        lib = api.load()
        lib.polychord_hip_set_option(b"halt_returns", 1.0)      # a failure comes back as an exception, not as `stop 1`
        out = super().__call__(theta)
        msg = lib.polychord_hip_last_error()
        if msg:
            raise RuntimeError(msg.decode(errors="replace"))
        return out

    def close(self):
        if self._handle is not None:
            lib = api.load()
            lib.pchip_source_destroy(self._handle)
            self._handle = None


class SourcePrior:
    """The prior of a `Source(..., prior=True)`: the handle's own pchip_prior_param inside the sampling kernels; only with that Source as
    the likelihood.  Called like a function it is the library's host function (polychord_hip_source_prior, one launch a call)."""
    symbol = "polychord_hip_source_prior"

    def __init__(self, source_obj):
        self.source_obj = source_obj

    def configure(self, nDims):
        self.source_obj.configure(nDims)

    def __call__(self, cube):
        lib = api.load()
        lib.polychord_hip_set_option(b"halt_returns", 1.0)
        cube = np.ascontiguousarray(cube, dtype=np.float64)
        self.configure(cube.size)
        theta = np.empty_like(cube)
        lib.polychord_hip_source_prior(api.dptr(cube), api.dptr(theta), int(cube.size))
        msg = lib.polychord_hip_last_error()
        if msg:
            raise RuntimeError(msg.decode(errors="replace"))
        return theta


class UniformPrior:
    """priors.f90:40-55 uniform box; evaluated on the device when the likelihood is a built-in"""
    symbol = "polychord_hip_uniform_prior"

    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def configure(self, nDims):
        lo = np.ascontiguousarray(np.broadcast_to(self.lo, (nDims,)), dtype=np.float64)
        hi = np.ascontiguousarray(np.broadcast_to(self.hi, (nDims,)), dtype=np.float64)
        api.load().polychord_hip_set_uniform_prior(nDims, api.dptr(lo), api.dptr(hi))

    def __call__(self, cube):
        cube = np.asarray(cube, dtype=np.float64)
        return np.broadcast_to(self.lo, cube.shape) + (np.broadcast_to(self.hi, cube.shape) - np.broadcast_to(self.lo, cube.shape)) * cube


class TablePrior:
    """The reference's prior types (priors.f90: uniform, log_uniform, power_uniform, gaussian, half_gaussian, exponential and the
    sorted_ forms of uniform / gaussian / half_gaussian / exponential) as a table, one entry per parameter: (type, params) or
    (type, block, params), e.g. [("gaussian", [0.5, 1.0])] * 4 + [("sorted_uniform", 1, [0, 1])] * 2.  `hyper`: the hypercube index
    of every parameter (None: identity).  The adaptive types -- adaptive_sorted_uniform, adaptive_sorted_gaussian,
    adaptive_sorted_half_gaussian, adaptive_sorted_exponential, nn_adaptive_layer_gaussian -- are blocks of consecutive entries of one
    type and block: the first entry is the count (behind the layer number, for nn_adaptive_layer_gaussian) and decides per point how
    many of the following members are sorted; every entry of the block, the count included, gives exactly the base type's number of
    prior parameters, e.g. [("adaptive_sorted_uniform", 1, [0, 1])] * 5.  Evaluated inside the sampling kernels when the likelihood is a built-in; called like a
    function it is the library's host function (polychord_hip_table_prior).  ValueError if the library refuses the table."""
    symbol = "polychord_hip_table_prior"

    def __init__(self, entries, hyper=None):
        self.entries, self.hyper = list(entries), hyper

    def configure(self, nDims):
        if nDims != len(self.entries):
            raise ValueError(f"TablePrior has {len(self.entries)} entries, the run {nDims} parameters")
        api.set_table_prior(self.entries, self.hyper)

    def __call__(self, cube):
        cube = np.ascontiguousarray(cube, dtype=np.float64)
        self.configure(cube.size)
        return api.table_prior(cube)
