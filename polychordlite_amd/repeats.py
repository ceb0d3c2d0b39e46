"""Independent repeats of one problem -- on one GPU, or spread over several (BASELINE's repeat-sharded mode).

A single run keeps about one wavefront per SIMD busy (B <= 1024 chains per nursery, the contraction on one CU), so
independent repeats overlap on one device; and they shard across devices with nothing to exchange until the end.
`run_repeats` is the front door: the library runs the repeats on host threads of its own (pchip_run_repeats: one engine
per run in flight, each on its own stream of its device) and merges their dead points on the first device
(pchip_merge_records): evidence with an error ~ 1/sqrt(repeats), posterior moments, the merged dead points and,
on request, <root>.stats / <root>_dead-birth.txt / <root>.txt of the union in the reference's formats.
"""
import ctypes as C

import numpy as np

from . import _ctypes_api as api
from . import merge as mg


def run_repeats(settings, like, prior, seeds, max_in_flight=4, devices=None, want_rows=False, write=None, comm=None, agree=None):
    """One nested-sampling run per seed, at most `max_in_flight` at a time per device, on `devices` (HIP ordinals of this
    process; None = the device of `settings`), merged.  comm (merge.Comm, one rank per GPU): every rank makes its own seeds' runs and
    the union of ALL ranks' runs is merged on every rank (pchip_comm_merge_many: one RCCL all-gather of the lived records).

    Returns (merged, runs): merged = {"n_runs", "logZ", "logZerr", "evidence_rule", "logZ_replay", "post_mean", "post_var", "logweights",
    "nlive", "records", "nlike", "nlike_local", "t_runs_s", "t_merge_s"[, "rows"]}; runs = the per-seed result dicts of `_ctypes_api.run`
    (this rank's).

    agree (with comm): `agree(ok) -> bool`, a collective of the caller's (e.g. an all-reduce of a failure flag over torch.distributed) that
    EVERY rank calls exactly once between its local runs and the exchange.  A rank whose runs failed must not leave the others waiting in
    the all-gather: when any rank reports a failure every rank raises here, before the exchange, and the collectives stay matched."""
    return _run("pchip_run_repeats_ex", settings, like, prior, seeds, max_in_flight, devices, want_rows, write, comm, agree)


def run_in_step(settings, like, prior, seeds, max_in_flight=4, devices=None, want_rows=False, write=None, comm=None, agree=None, maximise=False):
    """`run_repeats` for any problem that is wholly on the device (pchip_run_in_step): a built-in or a device source likelihood, plain or
    terms form, under the uniform box, a prior table or the handle's own source prior, and settings.ablate bit 15.  Up to `max_in_flight`
    runs of a device go round by round together, every kernel launched once for all of them; each run is bit for bit `_ctypes_api.run` of
    its seed (runs[k]["path"]["slice_step"] counts its nurseries whose sampling launch was shared).  A callback likelihood is taken while
    `_ctypes_api.set_device_batch_callback` holds a function (one call a tick for the rows of all runs of a group, on this thread; one
    device; `run_in_step_callable` does this for a torch callable); otherwise it raises, as a host prior does.  Arguments and return value as `run_repeats`.  maximise=True: every run's dict gains "maximum" (`_ctypes_api.maximum_dict`), the
    maximum-likelihood and maximum-posterior points polished from its final live set on the device, two launches for all runs
    (pchip_maximise_device_many); each is bit for bit `_ctypes_api.maximise_device` of that run alone."""
    merged, runs = _run("pchip_run_in_step", settings, like, prior, seeds, max_in_flight, devices, want_rows, write, comm, agree)
    if maximise:
        lib = mg._lib()
        n = len(runs)
        res = (api.Result * n)()
        for k, r in enumerate(runs):
            C.memmove(C.byref(res[k]), C.byref(r["_owner"].res), C.sizeof(api.Result))      # (borrowed: the dicts keep owning their blocks)
        mx = (api.Maximum * n)()
        rc = lib.pchip_maximise_device_many(C.byref(settings), C.byref(like), C.byref(prior), n, res, 0, mx)
        try:
            if rc != 0 and not (rc == 1 and all(bool(m.max_point) for m in mx)):
                msg = lib.polychord_hip_last_error()
                raise RuntimeError(f"pchip_maximise_device_many failed with code {rc}" + (": " + msg.decode(errors="replace") if msg else ""))
            for r, m in zip(runs, mx):
                r["maximum"] = api.maximum_dict(m, settings.nDims, settings.nDerived)
        finally:
            for m in mx:
                lib.pchip_maximum_free(C.byref(m))
    return merged, runs


def callable_problem(loglikelihood, prior, settings):
    """(like, prior, evaluator, keep) for a torch callable marked `device_batch` and its prior, as `run_in_step_callable` hands them to the
    library: an `_ctypes_api.Like` of kind callback, the `_ctypes_api.Prior` of UniformPrior / TablePrior (box / table: the engine's transform
    on the block) or of kind 0 for a callable marked `prior.device_batch`, the `_DeviceBatchEvaluator` to register around the runs, and the
    objects the structs point at.  With the evaluator registered, `_ctypes_api.run(settings, like, prior)` is the solo run of one seed."""
    from .pypolychord import polychord as pc
    if not pc._device_batch_pair(loglikelihood, prior):
        raise ValueError("a likelihood marked loglikelihood.device_batch = True is needed")
    nd, nder = int(settings.nDims), int(settings.nDerived)

    def scalar(theta_p, n, phi_p, m):      # (like.fn must be a function; no run in step calls it)
        out = pc._call_like(loglikelihood, np.ctypeslib.as_array(theta_p, shape=(n,)).copy())
        if isinstance(out, tuple):
            if m > 0:
                np.ctypeslib.as_array(phi_p, shape=(m,))[:] = out[1]
            out = out[0]
        return float(out)
    fl = api.LOGLIKE_FN(scalar)
    like = api.Like(); like.kind = api.LIKE_CALLBACK; like.fn = C.cast(fl, C.c_void_p)
    pr = api.Prior()
    keep = [fl]
    symbol = getattr(prior, "symbol", None)
    if symbol == "polychord_hip_uniform_prior":
        lo = np.ascontiguousarray(np.broadcast_to(prior.lo, (nd,)), dtype=np.float64)
        hi = np.ascontiguousarray(np.broadcast_to(prior.hi, (nd,)), dtype=np.float64)
        pr.kind, pr.lo, pr.hi = api.PRIOR_BOX, api.dptr(lo), api.dptr(hi)
        keep += [lo, hi]
    elif symbol == "polychord_hip_table_prior":
        if nd != len(prior.entries):
            raise ValueError(f"TablePrior has {len(prior.entries)} entries, the run {nd} parameters")
        arr, hy = api.prior_table(prior.entries, prior.hyper)
        pr.kind, pr.table = api.PRIOR_TABLE, arr
        if hy is not None:
            pr.hyper = hy.ctypes.data_as(C.POINTER(C.c_int))
        keep += [arr, hy]
    else:
        pr.kind = api.PRIOR_CALLBACK          # the callable's own prior, on the device: the evaluator calls it on the cube block
    return like, pr, pc._DeviceBatchEvaluator(loglikelihood, prior, nd, nder, settings.logzero), keep


def run_in_step_callable(loglikelihood, prior, settings, seeds, max_in_flight=4, want_rows=False, write=None):
    """`run_in_step` for a likelihood that is a torch callable on the device: `loglikelihood.device_batch = True`, theta tensor (n, nDims)
    -> logL (n,) or (logL, phi), as `pypolychord.run` takes it.  prior: `UniformPrior` / `TablePrior` of pypolychord.device_likelihoods (the
    engine evaluates it on the whole block) or a callable marked `prior.device_batch = True` (cube tensor -> theta tensor).  settings: an
    `_ctypes_api.Settings`.  The seeds go in step, up to `max_in_flight` of them a group, and the callable is called ONCE a tick with the
    parked proposals of all runs of the group, run after run in the order of `seeds` -- each run is its solo run if the callable's answer
    for a row depends neither on the row's place in the block nor on n.  Returns (merged, runs) like `run_in_step`; what the callable raises
    is raised here once the runs have wound down."""
    like, pr, ev, keep = callable_problem(loglikelihood, prior, settings)
    lib = ev.register()
    try:
        out = run_in_step(settings, like, pr, seeds, max_in_flight=max_in_flight, want_rows=want_rows, write=write)
    except RuntimeError:
        if ev.error is not None:
            raise ev.error
        raise
    finally:
        ev.unregister(lib)
    if ev.error is not None:
        raise ev.error
    del keep
    return out


def _run(symbol, settings, like, prior, seeds, max_in_flight, devices, want_rows, write, comm, agree):
    """the body of both doors: `symbol` is pchip_run_repeats_ex or pchip_run_in_step, which share their arguments"""
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError("run_repeats needs at least one seed")
    lib = mg._lib()
    f = getattr(lib, symbol)
    f.restype = C.c_int
    f.argtypes = [C.POINTER(api.Settings), C.POINTER(api.Like), C.POINTER(api.Prior), C.c_int, C.POINTER(C.c_int), C.c_int,
                  C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(api.Result), C.POINTER(mg.Merged)]
    n = len(seeds)
    sd = (C.c_int * n)(*seeds)
    devs = list(devices) if devices else []
    dv = (C.c_int * max(len(devs), 1))(*devs) if devs else None
    res = (api.Result * n)()
    m = mg.Merged()
    import time
    t0 = time.perf_counter()
    if comm is not None and not settings.device_records:
        # (the runs leave their lived records on the device for the exchange: no second trip over the host link)
        s2 = api.Settings(); C.memmove(C.byref(s2), C.byref(settings), C.sizeof(settings)); s2.device_records = 1
        settings = s2
    rc = f(C.byref(settings), C.byref(like), C.byref(prior), n, sd, len(devs), dv, int(max_in_flight), 1 if (want_rows or write) else 0, res,
           C.byref(m) if comm is None else None)
    if comm is not None and agree is not None:
        if not agree(rc == 0):
            if rc == 0:                                               # (a failed call has freed its results itself)
                for k in range(n):
                    lib.pchip_result_free(C.byref(res[k]))
            raise RuntimeError(f"run_repeats: the runs of at least one rank failed (this rank: code {rc}); the exchange was skipped on every rank")
    if rc != 0:
        raise RuntimeError(f"{symbol[:-3] if symbol.endswith('_ex') else symbol} failed with code {rc}")
    t_runs = time.perf_counter() - t0
    runs = []
    for k in range(n):
        r = api.Result()
        C.memmove(C.byref(r), C.byref(res[k]), C.sizeof(r))          # each dict owns (and frees) its own result block
        runs.append(api.result_dict(r, settings))
    if comm is None:
        try:
            if write:
                if lib.pchip_merged_write(C.byref(m), settings.nDims, settings.nDerived, str(write[0]).encode(), str(write[1]).encode()) != 0:
                    raise RuntimeError("pchip_merged_write failed")
            merged = mg.merged_dict(m, settings.nDims, settings.nDerived, want_rows)
        finally:
            lib.pchip_merged_free(C.byref(m))
    else:
        merged = mg.comm_merge_many(runs, comm, settings.nDims, settings.nDerived, want_rows=want_rows, write=write)
        merged["t_runs_s"] = t_runs
    merged["nlike_local"] = int(sum(r["nlike"] for r in runs))
    merged["runs_logZ"] = [r["logZ"] for r in runs]      # (their mean and its error: merged["runs_logZ_mean"], ["runs_logZ_sem"], from the library)
    return merged, runs
