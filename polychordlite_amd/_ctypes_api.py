"""ctypes view of libpolychord_hip.so (include/polychord_hip.h) -- plumbing only.

The product path is the HIP library; there is no Python/NumPy fallback.  Importing this module
loads the shared object and fails loudly if it has not been built (`python -m polychordlite_amd.build`).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCHIP_LIB") or os.path.join(_HERE, "libpolychord_hip.so")     # (PCHIP_LIB: A/B runs of two builds on one GPU box)

LOGLIKE_FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int)
PRIOR_FN = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int)
DUMPER_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                        C.POINTER(C.c_double), C.c_double, C.c_double)

LIKE_CALLBACK, LIKE_GAUSSIAN, LIKE_RASTRIGIN, LIKE_TWIN_GAUSSIAN, LIKE_CORR_GAUSSIAN, LIKE_SOURCE = range(6)
KERNEL_CLASSES = ("k_nhats", "k_slice", "k_consume", "k_apply", "k_clean", "k_covmats", "k_bases_side")
LIKE_KINDS = {"gaussian": LIKE_GAUSSIAN, "rastrigin": LIKE_RASTRIGIN, "twin_gaussian": LIKE_TWIN_GAUSSIAN,
              "corr_gaussian": LIKE_CORR_GAUSSIAN, "source": LIKE_SOURCE}


class Settings(C.Structure):
    _fields_ = [("nDims", C.c_int), ("nDerived", C.c_int), ("nlive", C.c_int), ("num_repeats", C.c_int),
                ("nprior", C.c_int), ("nfail", C.c_int), ("do_clustering", C.c_int),
                ("precision_criterion", C.c_double), ("logzero", C.c_double), ("max_ndead", C.c_int),
                ("boost_posterior", C.c_double), ("posteriors", C.c_int), ("equals", C.c_int),
                ("cluster_posteriors", C.c_int), ("compression_factor", C.c_double), ("n_nlives", C.c_int),
                ("loglikes", C.POINTER(C.c_double)), ("nlives", C.POINTER(C.c_int)), ("seed", C.c_int),
                ("batch", C.c_int), ("device", C.c_int), ("feedback", C.c_int), ("profile", C.c_int),
                ("force_general", C.c_int), ("ablate", C.c_int),
                ("resume_write", C.c_char_p), ("sequential_rng", C.c_int), ("resume_read", C.c_char_p),
                ("nGrade", C.c_int), ("grade_dims", C.POINTER(C.c_int)), ("grade_repeats", C.POINTER(C.c_int)),
                ("epoch_discard", C.c_int), ("device_records", C.c_int),
                ("n_sub_cluster", C.c_int), ("sub_cluster_dims", C.POINTER(C.c_int))]


class Like(C.Structure):
    _fields_ = [("kind", C.c_int), ("mu", C.c_double), ("sigma", C.c_double), ("invcov", C.POINTER(C.c_double)),
                ("mean", C.POINTER(C.c_double)), ("logdetcov", C.c_double), ("fn", C.c_void_p),
                ("source", C.c_int)]


class PriorEntry(C.Structure):
    """pchip_prior_entry: one parameter of a prior table (type number of PRIOR_TYPES / ADAPTIVE_PRIOR_TYPES, prior block, prior parameters)"""
    _fields_ = [("type", C.c_int), ("block", C.c_int), ("npar", C.c_int), ("par", C.c_double * 3)]


class Prior(C.Structure):
    _fields_ = [("kind", C.c_int), ("lo", C.POINTER(C.c_double)), ("hi", C.POINTER(C.c_double)), ("fn", C.c_void_p),
                ("table", C.POINTER(PriorEntry)), ("hyper", C.POINTER(C.c_int))]


# pchip_prior.kind
PRIOR_CALLBACK, PRIOR_BOX, PRIOR_TABLE, PRIOR_SOURCE = 0, 1, 2, 3
# the reference's prior type numbers (priors.f90:5-15) a table takes
PRIOR_TYPES = {"uniform": 1, "log_uniform": 2, "power_uniform": 3, "gaussian": 4, "half_gaussian": 5, "exponential": 6,
               "sorted_uniform": 7, "sorted_gaussian": 8, "sorted_half_gaussian": 9, "sorted_exponential": 10}
# ... and its adaptive types (priors.f90:16-20): blocks whose first parameter decides, per point, how many of the others are sorted
ADAPTIVE_PRIOR_TYPES = {"adaptive_sorted_uniform": 11, "adaptive_sorted_gaussian": 12, "adaptive_sorted_half_gaussian": 13,
                        "adaptive_sorted_exponential": 14, "nn_adaptive_layer_gaussian": 15}


class Result(C.Structure):
    _fields_ = [("logZ", C.c_double), ("varlogZ", C.c_double), ("ndead", C.c_long), ("nlike", C.c_long),
                ("niter", C.c_long), ("nbatches", C.c_long), ("nrounds", C.c_long), ("nupdates", C.c_long),
                ("ncluster", C.c_int), ("ncluster_dead", C.c_int), ("nTotal", C.c_int), ("batch", C.c_int),
                ("t_generate", C.c_double), ("t_loop", C.c_double), ("t_final", C.c_double), ("t_total", C.c_double),
                ("t_setup", C.c_double), ("t_results", C.c_double), ("t_teardown", C.c_double),
                ("k_time_s", C.c_double * 8), ("k_launches", C.c_long * 8),
                ("dead", C.POINTER(C.c_double)), ("logweights", C.POINTER(C.c_double)), ("entry", C.POINTER(C.c_double)),
                ("live", C.POINTER(C.c_double)), ("nlive_final", C.c_int),
                ("logZp", C.POINTER(C.c_double)), ("varlogZp", C.POINTER(C.c_double)), ("nZp", C.c_int),
                ("post_mean", C.POINTER(C.c_double)), ("post_var", C.POINTER(C.c_double)),
                ("nlike_grade", C.c_long * 8), ("live_cluster", C.POINTER(C.c_int)),
                ("nlike_failed", C.c_long), ("ncluster_peak", C.c_int), ("epoch_discard", C.c_int),
                ("d_records", C.c_void_p), ("n_records", C.c_long), ("records_cap", C.c_long), ("records_device", C.c_int),
                ("path", C.c_long * 24)]


class Maximum(C.Structure):
    """pchip_maximum: the maximiser's result as values; index 0 = the likelihood leg, 1 = the posterior leg"""
    _fields_ = [("status", C.c_int * 2), ("cluster", C.c_int * 2), ("niter", C.c_long * 2), ("neval", C.c_long * 2),
                ("max_logl", C.c_double), ("max_point", C.POINTER(C.c_double)),
                ("max_post", C.c_double), ("logl_at_post", C.c_double), ("post_point", C.POINTER(C.c_double)),
                ("has_mean", C.c_int), ("logl_mean", C.c_double), ("mean_point", C.POINTER(C.c_double))]


# pchip_result.path[]: launches per kernel variant (include/polychord_hip.h PCHIP_PATH_*)
PATH_NAMES = ("consume_par", "consume_cl", "consume_general", "consume_fast", "killoff_par", "killoff_cl", "killoff_general",
              "killoff_fast", "update_fused", "update_steps", "slice_wave", "slice_lane", "nn_lists", "nn_fallbacks", "pool_mode",
              "defer_update", "consume_cl_serial", "subcluster_passes", "subcluster_splits", "source_kernels", "device_prior", "source_terms", "slice_step")
# ... and the counter behind them, kept beside the tuple (tests pin the tuple's length to the kernel variants): calls of the device batch
# callback, PCHIP_PATH_DEVICE_BATCH; result_dict puts it into the same `path` dict as "device_batch"
PATH_DEVICE_BATCH = 23

# polychord_device_batch_fn (include/polychord_hip.h): user, n, nDims, nDerived, d_cube, d_theta, d_phi, d_logL, flags, stream -> 0 / stop.
# The pointers are DEVICE memory: plain addresses here.
DEVICE_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
_device_batch_cb = None


def set_device_batch_callback(fn):
    """polychord_hip_set_device_batch_callback: fn(user, n, nDims, nDerived, d_cube, d_theta, d_phi, d_logL, flags, stream) -> int, called
    with device addresses (see DeviceBlock) once per round of a callback-likelihood run; None removes it.  Process-global and sticky; the
    ctypes thunk is kept alive here until the next call.  A DEVICE_BATCH_FN is taken as it is."""
    global _device_batch_cb
    lib = load()
    cb = None if fn is None else (fn if isinstance(fn, DEVICE_BATCH_FN) else DEVICE_BATCH_FN(fn))
    lib.polychord_hip_set_device_batch_callback.argtypes = [C.c_void_p, C.c_void_p]
    lib.polychord_hip_set_device_batch_callback.restype = None
    lib.polychord_hip_set_device_batch_callback(C.cast(cb, C.c_void_p) if cb is not None else None, None)
    _device_batch_cb = cb
    return cb


class DeviceBlock:
    """A dense row-major float64 block of device memory the library handed out, for consumers of `__cuda_array_interface__` (version 3:
    torch.as_tensor, cupy.asarray -- zero copy).  ptr: the device address; shape: a tuple of ints; stream: the hipStream_t the block is valid
    on (None or 0: no `stream` entry, the consumer synchronises nothing)."""

    def __init__(self, ptr, shape, stream=None, readonly=False):
        self.ptr, self.shape, self.stream, self.readonly = int(ptr or 0), tuple(int(v) for v in shape), (int(stream) if stream else None), readonly

    @property
    def __cuda_array_interface__(self):
        d = {"shape": self.shape, "typestr": "<f8", "data": (self.ptr, bool(self.readonly)), "version": 3, "strides": None}
        if self.stream:
            d["stream"] = self.stream
        return d


def park_pack(need, prop, cube=None, device=-1):
    """pchip_park_pack: the pack of the device batch callback alone.  need [nchains] ints, prop [nchains][nDims]; cube: the block the rows are
    written into ([nchains][nDims], changed in place; None: zeros).  Returns rank [nchains], count, cube."""
    lib = load()
    nd = np.ascontiguousarray(need, dtype=np.int32)
    pr = np.ascontiguousarray(prop, dtype=np.float64)
    out = np.zeros_like(pr) if cube is None else cube
    assert out.flags.c_contiguous and out.dtype == np.float64 and out.shape == pr.shape
    rank = np.empty(nd.size, dtype=np.int32)
    cnt = C.c_int(-1)
    ip = C.POINTER(C.c_int)
    lib.pchip_park_pack.argtypes = [C.c_int, C.c_int, ip, C.POINTER(C.c_double), ip, ip, C.POINTER(C.c_double), C.c_int]
    lib.pchip_park_pack.restype = C.c_int
    rc = lib.pchip_park_pack(pr.shape[0], pr.shape[1], nd.ctypes.data_as(ip), dptr(pr), rank.ctypes.data_as(ip), C.byref(cnt), dptr(out), device)
    if rc:
        raise RuntimeError(f"pchip_park_pack failed with code {rc}")
    return rank, cnt.value, out


def park_pack_many(nchains, need, prop, cube=None, device=-1):
    """pchip_park_pack_many: the pack of a group of runs in step alone.  nchains [nruns] ints; need [sum nchains] ints and prop
    [sum nchains][nDims], the runs one behind the other; cube: the ONE block the rows are written into ([sum nchains][nDims], changed in
    place; None: zeros).  Returns rank [sum nchains] (rows of the block), counts [nruns], total, cube."""
    lib = load()
    nc = np.ascontiguousarray(nchains, dtype=np.int32)
    nd = np.ascontiguousarray(need, dtype=np.int32)
    pr = np.ascontiguousarray(prop, dtype=np.float64)
    out = np.zeros_like(pr) if cube is None else cube
    assert out.flags.c_contiguous and out.dtype == np.float64 and out.shape == pr.shape
    assert nc.ndim == 1 and pr.ndim == 2 and nd.size == pr.shape[0] == int(nc.sum())
    rank = np.empty(nd.size, dtype=np.int32)
    counts = np.full(nc.size, -1, dtype=np.int32)
    tot = C.c_int(-1)
    ip = C.POINTER(C.c_int)
    lib.pchip_park_pack_many.argtypes = [C.c_int, ip, C.c_int, ip, C.POINTER(C.c_double), ip, ip, ip, C.POINTER(C.c_double), C.c_int]
    lib.pchip_park_pack_many.restype = C.c_int
    rc = lib.pchip_park_pack_many(nc.size, nc.ctypes.data_as(ip), pr.shape[1], nd.ctypes.data_as(ip), dptr(pr), rank.ctypes.data_as(ip),
                                  counts.ctypes.data_as(ip), C.byref(tot), dptr(out), device)
    if rc:
        raise RuntimeError(f"pchip_park_pack_many failed with code {rc}")
    return rank, counts, tot.value, out


def par_accept(snapshot_logL, cand_logL, valid=None, serial=False, device=-1):
    """pchip_par_accept: the acceptance of the one-cluster parallel contraction alone.  snapshot_logL [n] ascending, cand_logL [T] by step,
    valid [T] (None: every step); serial: by the serial recurrence (settings.ablate bit 18).  Returns accept [T] as bools."""
    lib = load()
    sn = np.ascontiguousarray(snapshot_logL, dtype=np.float64)
    cd = np.ascontiguousarray(cand_logL, dtype=np.float64)
    vl = np.ones(cd.size, dtype=np.uint8) if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
    assert sn.ndim == 1 and cd.ndim == 1 and vl.shape == cd.shape
    acc = np.full(cd.size, 0xEE, dtype=np.uint8)
    bp = C.POINTER(C.c_ubyte)
    lib.pchip_par_accept.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), bp, C.c_int, bp, C.c_int]
    lib.pchip_par_accept.restype = C.c_int
    rc = lib.pchip_par_accept(sn.size, dptr(sn), cd.size, dptr(cd), vl.ctypes.data_as(bp), 1 if serial else 0, acc.ctypes.data_as(bp), device)
    if rc:
        raise RuntimeError(f"pchip_par_accept failed with code {rc}")
    assert np.all(acc <= 1)
    return acc.astype(bool)


_lib = None


def load():
    """dlopen libpolychord_hip.so (RTLD_GLOBAL so that the HIP runtime is shared with torch)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m polychordlite_amd.build` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    lib.pchip_settings_default.argtypes = [C.POINTER(Settings), C.c_int, C.c_int]
    lib.pchip_settings_default.restype = None
    lib.pchip_device_count.restype = C.c_int
    lib.pchip_run.argtypes = [C.POINTER(Settings), C.POINTER(Like), C.POINTER(Prior), C.POINTER(Result)]
    lib.pchip_run.restype = C.c_int
    lib.pchip_result_free.argtypes = [C.POINTER(Result)]
    lib.pchip_result_free.restype = None
    lib.pchip_slice_chains.argtypes = [C.POINTER(Settings), C.POINTER(Like), C.POINTER(Prior), C.c_uint, C.c_int,
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.pchip_slice_chains.restype = C.c_int
    lib.pchip_directions.argtypes = [C.POINTER(Settings), C.POINTER(Like), C.POINTER(Prior), C.c_uint, C.c_int, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_int]
    lib.pchip_directions.restype = C.c_int
    lib.polychord_hip_set_gaussian.argtypes = [C.c_double, C.c_double]
    lib.polychord_hip_set_uniform_prior.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.polychord_hip_set_corr_gaussian.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double]
    lib.polychord_hip_set_option.argtypes = [C.c_char_p, C.c_double]
    lib.polychord_hip_set_sub_clustering.argtypes = [C.c_int, C.POINTER(C.c_int)]
    lib.polychord_hip_set_sub_clustering.restype = None
    lib.polychord_hip_ini_sub_clustering.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int]
    lib.polychord_hip_ini_sub_clustering.restype = C.c_int
    lib.pchip_source_create.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_long]
    lib.pchip_source_create.restype = C.c_int
    lib.pchip_source_create_terms.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_long, C.c_long]
    lib.pchip_source_create_terms.restype = C.c_int
    lib.pchip_source_create_prior.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_long, C.c_long]
    lib.pchip_source_create_prior.restype = C.c_int
    lib.pchip_source_create_sums.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_long, C.c_long, C.c_int, C.c_int]
    lib.pchip_source_create_sums.restype = C.c_int
    lib.pchip_source_create_quad.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_long, C.c_long, C.POINTER(C.c_double), C.c_int]
    lib.pchip_source_create_quad.restype = C.c_int
    lib.pchip_source_create_quad_batch.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_long, C.c_long, C.POINTER(C.c_double)]
    lib.pchip_source_create_quad_batch.restype = C.c_int
    lib.pchip_source_create_shared.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_long, C.c_long, C.c_long, C.c_int, C.c_long,
                                               C.POINTER(C.c_double), C.c_int]
    lib.pchip_source_create_shared.restype = C.c_int
    lib.pchip_source_prior_eval.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_long, C.c_int, C.POINTER(C.c_double)]
    lib.pchip_source_prior_eval.restype = C.c_int
    lib.pchip_source_eval.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_long, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.pchip_source_eval.restype = C.c_int
    lib.pchip_source_destroy.argtypes = [C.c_int]
    lib.pchip_source_destroy.restype = None
    lib.polychord_hip_set_source.argtypes = [C.c_int]
    lib.polychord_hip_set_source.restype = C.c_int
    lib.polychord_hip_source_loglike.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int]
    lib.polychord_hip_source_loglike.restype = C.c_double
    lib.polychord_hip_source_prior.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
    lib.polychord_hip_source_prior.restype = None
    lib.pchip_rtc_embedded_source.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    lib.pchip_rtc_embedded_source.restype = C.c_char_p
    lib.pchip_rtc_compile_check.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_double)]
    lib.pchip_rtc_compile_check.restype = C.c_int
    lib.pchip_rtc_stats.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_double)]
    lib.pchip_rtc_stats.restype = None
    lib.polychord_hip_last_error.restype = C.c_char_p
    lib.polychord_hip_set_table_prior.argtypes = [C.c_int, C.POINTER(PriorEntry), C.POINTER(C.c_int)]
    lib.polychord_hip_set_table_prior.restype = C.c_int
    lib.polychord_hip_table_prior.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
    lib.polychord_hip_table_prior.restype = None
    lib.pchip_prior_transform.argtypes = [C.POINTER(Prior), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
    lib.pchip_prior_transform.restype = C.c_int
    pi = C.POINTER(C.c_int); pd = C.POINTER(C.c_double)
    lib.pchip_update_factors.argtypes = [C.POINTER(Settings), C.c_int, C.c_int, pd, pi, C.c_int, pd, pd, pi, pd, pd, C.c_int, pd, pd, pi, pd, pi]
    lib.pchip_update_factors.restype = C.c_int
    lib.pchip_cluster_update.argtypes = [C.POINTER(Settings), C.c_int, C.POINTER(ClusterIn), C.POINTER(ClusterOut), C.c_int]
    lib.pchip_cluster_update.restype = C.c_int
    lib.pchip_maximise_values.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, pd, pi, C.c_int, pd, C.POINTER(Maximum)]
    lib.pchip_maximise_values.restype = C.c_int
    lib.pchip_maximise_device.argtypes = [C.POINTER(Settings), C.POINTER(Like), C.POINTER(Prior), pd, pi, C.c_int, pd, C.c_long, C.POINTER(Maximum)]
    lib.pchip_maximise_device.restype = C.c_int
    lib.pchip_maximise_device_many.argtypes = [C.POINTER(Settings), C.POINTER(Like), C.POINTER(Prior), C.c_int, C.POINTER(Result), C.c_long, C.POINTER(Maximum)]
    lib.pchip_maximise_device_many.restype = C.c_int
    lib.pchip_maximum_write.argtypes = [C.POINTER(Maximum), C.c_int, C.c_int, C.c_char_p]
    lib.pchip_maximum_write.restype = C.c_int
    lib.pchip_maximum_free.argtypes = [C.POINTER(Maximum)]
    lib.pchip_maximum_free.restype = None
    # this mirror against the library that was loaded (the structs grow at their end: include/polychord_hip.h PCHIP_ABI_VERSION)
    lib.pchip_sizeof.argtypes = [C.c_char_p]
    lib.pchip_sizeof.restype = C.c_ulong
    for name, cls in (("settings", Settings), ("result", Result), ("like", Like), ("prior", Prior), ("maximum", Maximum)):
        if lib.pchip_sizeof(name.encode()) != C.sizeof(cls):
            raise ImportError(f"{LIB_PATH}: pchip_{name} is {lib.pchip_sizeof(name.encode())} bytes, this binding's mirror {C.sizeof(cls)} "
                              f"(library ABI version {lib.pchip_abi_version()}): rebuild with `python -m polychordlite_amd.build`")
    _lib = lib
    return lib


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def source_create(source, options=(), data=None, nterms=None, prior=False, nsums=None, residuals=None, precision=None, shared=None, batched=False):
    """handle of a likelihood written as HIP device source (pchip_source_create); RuntimeError with the compiler's log if it does not compile.
    nterms given: the terms form (pchip_source_create_terms) -- the source defines pchip_logl_term and pchip_logl_finish, the sum has nterms terms.
    nsums given (with nterms): several sums per evaluation (pchip_source_create_sums) -- the source defines pchip_logl_terms and
    pchip_logl_finish_sums, every sum has nterms terms; nsums=None: the calls above, unchanged.
    residuals given: the quadratic form (pchip_source_create_quad) -- the source defines pchip_residual and pchip_logl_finish, chi2 = r^T P r
    of that many residuals; precision: P, a 2-D float64 array of shape (residuals, residuals), used exactly as given (ValueError on another shape).
    shared given: that many shared values beside the form the other keywords name (pchip_source_create_shared) -- the source defines
    pchip_shared_value and its form's functions with `const double *shared` behind theta; nterms alone one sum, nsums with it several,
    residuals / precision the quadratic form.  shared=None: the calls above, unchanged.
    batched=True (with residuals / precision): the batched quadratic form (pchip_source_create_quad_batch) -- the same two functions, up to 4096
    residuals, evaluated for all parked proposals of a round at once on the matrix cores; no prior of its own, no shared values (ValueError
    without residuals, or with prior / shared / nterms / nsums).  batched=False: the calls above, unchanged.
    prior=True: the source defines pchip_prior_param as well (pchip_source_create_prior; with nsums, pchip_source_create_sums' with_prior),
    for runs with prior.kind = PRIOR_SOURCE"""
    if batched and residuals is None:
        raise ValueError("batched=True is the batched quadratic form: it needs residuals (and precision)")
    if batched and (prior or shared is not None or nterms is not None or nsums is not None):
        raise ValueError("batched=True takes residuals and precision alone: no prior of its own, no shared values, no terms or sums")
    lib = load()
    d = None if data is None else np.ascontiguousarray(np.ravel(data), dtype=np.float64)
    opts = " ".join(options) if not isinstance(options, str) else options
    args = (source.encode(), opts.encode(), dptr(d) if d is not None and d.size else None, 0 if d is None else int(d.size))
    p = None
    if residuals is not None:
        n = int(residuals)
        p = None if precision is None else np.ascontiguousarray(precision, dtype=np.float64)
        if p is not None and n >= 1 and p.shape != (n, n):
            raise ValueError(f"precision has shape {p.shape}: the quadratic form of {n} residuals takes a 2-D array of shape ({n}, {n})")
    if batched:
        h = lib.pchip_source_create_quad_batch(*args, n, dptr(p) if p is not None and p.size else None)
    elif shared is not None:
        h = lib.pchip_source_create_shared(*args, int(shared), 0 if nterms is None else int(nterms), 0 if nsums is None else int(nsums),
                                           0 if residuals is None else int(residuals), dptr(p) if p is not None and p.size else None, 1 if prior else 0)
    elif residuals is not None:
        h = lib.pchip_source_create_quad(*args, n, dptr(p) if p is not None and p.size else None, 1 if prior else 0)
    elif nsums is not None:
        h = lib.pchip_source_create_sums(*args, 0 if nterms is None else int(nterms), int(nsums), 1 if prior else 0)
    elif prior:
        h = lib.pchip_source_create_prior(*args, 0 if nterms is None else int(nterms))
    else:
        h = lib.pchip_source_create(*args) if nterms is None else lib.pchip_source_create_terms(*args, int(nterms))
    if h <= 0:
        log = lib.polychord_hip_last_error()
        raise RuntimeError("device source does not compile:\n" + (log.decode(errors="replace") if log else "(no log)"))
    return h


def set_source(handle):
    """polychord_hip_set_source: the handle behind polychord_hip_source_loglike / polychord_hip_source_prior for the next calls of the
    PolyChord-interface doors (0 clears it); RuntimeError with the library's message for a handle that does not exist"""
    lib = load()
    if lib.polychord_hip_set_source(int(handle)) != 0:
        msg = lib.polychord_hip_last_error()
        raise RuntimeError(msg.decode(errors="replace") if msg else f"polychord_hip_set_source({handle}) failed")


def source_eval(handle, thetas, nDerived=0):
    """pchip_source_eval: a source likelihood (either form) at the rows of `thetas` ([n][nDims]), on the device; (logL [n], phi [n][nDerived])"""
    lib = load()
    t = np.ascontiguousarray(np.atleast_2d(thetas), dtype=np.float64)
    logL = np.empty(t.shape[0])
    phi = np.empty((t.shape[0], nDerived))
    rc = lib.pchip_source_eval(handle, dptr(t), t.shape[0], t.shape[1], nDerived, dptr(logL), dptr(phi) if nDerived > 0 else None)
    if rc != 0:
        msg = lib.polychord_hip_last_error()
        raise RuntimeError(f"pchip_source_eval failed with code {rc}" + (": " + msg.decode(errors="replace") if rc == 1 and msg else ""))
    return logL, phi


def source_prior_eval(handle, cubes):
    """pchip_source_prior_eval: the prior of a source handle (source_create(..., prior=True)) at the rows of `cubes` ([n][nDims]), on the
    device; theta rows"""
    lib = load()
    c = np.ascontiguousarray(np.atleast_2d(cubes), dtype=np.float64)
    th = np.empty_like(c)
    rc = lib.pchip_source_prior_eval(handle, dptr(c), c.shape[0], c.shape[1], dptr(th))
    if rc != 0:
        msg = lib.polychord_hip_last_error()
        raise RuntimeError(f"pchip_source_prior_eval failed with code {rc}" + (": " + msg.decode(errors="replace") if rc == 1 and msg else ""))
    return th


def prior_table(entries, hyper=None):
    """(PriorEntry array, hypercube-order array or None) of a prior table: entries = one (type, block, params) or (type, params) per
    PARAMETER, type a name of PRIOR_TYPES or ADAPTIVE_PRIOR_TYPES or its number; hyper = hypercube index of every parameter (None: identity)"""
    arr = (PriorEntry * len(entries))()
    for i, e in enumerate(entries):
        t, block, pars = (e[0], 1, e[1]) if len(e) == 2 else e
        pars = [float(v) for v in np.atleast_1d(pars)]
        arr[i].type = (PRIOR_TYPES[t] if t in PRIOR_TYPES else ADAPTIVE_PRIOR_TYPES[t]) if isinstance(t, str) else int(t)
        arr[i].block, arr[i].npar = int(block), len(pars)
        for k, v in enumerate(pars[:3]):
            arr[i].par[k] = v
    hy = None if hyper is None else np.ascontiguousarray(hyper, dtype=np.int32)
    return arr, hy


def set_table_prior(entries, hyper=None):
    """polychord_hip_set_table_prior: the table behind polychord_hip_table_prior; ValueError with the library's message if it is refused"""
    lib = load()
    arr, hy = prior_table(entries, hyper)
    if lib.polychord_hip_set_table_prior(len(arr), arr, hy.ctypes.data_as(C.POINTER(C.c_int)) if hy is not None else None) != 0:
        msg = lib.polychord_hip_last_error()
        raise ValueError(msg.decode(errors="replace") if msg else "prior table refused")


def table_prior(cube):
    """polychord_hip_table_prior (the HOST function) at one hypercube point"""
    lib = load()
    c = np.ascontiguousarray(cube, dtype=np.float64)
    th = np.empty_like(c)
    lib.polychord_hip_table_prior(dptr(c), dptr(th), int(c.size))
    return th


def prior_transform(entries, cubes, hyper=None, device=-1):
    """pchip_prior_transform: the DEVICE transform of a table at the rows of `cubes` ([n][nDims]); theta rows"""
    lib = load()
    c = np.ascontiguousarray(np.atleast_2d(cubes), dtype=np.float64)
    th = np.empty_like(c)
    arr, hy = prior_table(entries, hyper)
    P = Prior()
    P.kind, P.table = PRIOR_TABLE, arr
    if hy is not None:
        P.hyper = hy.ctypes.data_as(C.POINTER(C.c_int))
    rc = lib.pchip_prior_transform(C.byref(P), c.shape[1], c.shape[0], dptr(c), dptr(th), device)
    if rc != 0:
        msg = lib.polychord_hip_last_error()
        raise RuntimeError(f"pchip_prior_transform failed with code {rc}" + (": " + msg.decode(errors="replace") if rc == 1 and msg else ""))
    return th


def update_factors(live, live_cluster, phantom, ph_logL, ph_cluster, threshold, path, shift=None, ablate=0, device=-1):
    """pchip_update_factors: covariance and Cholesky factor of an update of the given rows, by the run's own launchers (path 1: the fused
    update, path 0: clean + covmats).  live [nlive][nDims] with a 0-based cluster per row; phantom [nph][nDims] with logL and cluster
    per row (-1: the row holds no phantom); threshold per cluster; shift [nDims] or None (the cube centre).
    dict: cov, chol [ncluster][nDims][nDims], count [ncluster], shift [nDims], chol_suspect"""
    lib = load()
    x = np.ascontiguousarray(np.atleast_2d(live), dtype=np.float64)
    D = x.shape[1]
    ph = np.ascontiguousarray(np.reshape(phantom, (-1, D)), dtype=np.float64)
    lc = np.ascontiguousarray(live_cluster, dtype=np.int32)
    pl = np.ascontiguousarray(ph_logL, dtype=np.float64)
    pc = np.ascontiguousarray(ph_cluster, dtype=np.int32)
    thr = np.ascontiguousarray(np.atleast_1d(threshold), dtype=np.float64)
    nc = thr.size
    assert lc.shape == (x.shape[0],) and pl.shape == (ph.shape[0],) and pc.shape == (ph.shape[0],)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    assert sh is None or sh.shape == (D,)
    s = Settings(); lib.pchip_settings_default(C.byref(s), D, 0)
    s.ablate, s.device = ablate, device
    cov = np.full((nc, D, D), np.nan); chol = np.full((nc, D, D), np.nan)
    count = np.full(nc, -1, dtype=np.int32); sho = np.full(D, np.nan); sus = C.c_int(-1)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    rc = lib.pchip_update_factors(C.byref(s), nc, x.shape[0], dptr(x), ip(lc), ph.shape[0], dptr(ph), dptr(pl), ip(pc), dptr(thr),
                                  dptr(sh) if sh is not None else None, path, dptr(cov), dptr(chol), ip(count), dptr(sho), C.byref(sus))
    if rc != 0:
        msg = lib.polychord_hip_last_error()
        raise RuntimeError(f"pchip_update_factors failed with code {rc}" + (": " + msg.decode(errors="replace") if rc == 1 and msg else ""))
    return dict(cov=cov, chol=chol, count=count, shift=sho, chol_suspect=sus.value)


NO_SUCH_PATH = 64      # PCHIP_NO_SUCH_PATH


class ClusterIn(C.Structure):
    """pchip_cluster_in"""
    _fields_ = [("ncluster", C.c_int), ("nlive", C.c_int), ("nph", C.c_int),
                ("live", C.POINTER(C.c_double)), ("live_logL", C.POINTER(C.c_double)), ("live_cluster", C.POINTER(C.c_int)),
                ("phantom", C.POINTER(C.c_double)), ("ph_logL", C.POINTER(C.c_double)), ("ph_cluster", C.POINTER(C.c_int))]


class ClusterOut(C.Structure):
    """pchip_cluster_out"""
    _fields_ = ([(k, C.c_int) for k in ("maxc", "nsplit_cap", "scratch_cap", "ncluster", "nsplit", "levels", "scratch_n")]
                + [(k, C.POINTER(C.c_int)) for k in ("live_cluster", "live_pos", "cl_list", "cl_n", "imin_slot", "ph_count")]
                + [("cl_uid", C.POINTER(C.c_uint))]
                + [(k, C.POINTER(C.c_double)) for k in ("logLp", "lse_ref", "lse_sum", "logXp", "logZp", "logZXp", "logZp2", "logZpXp", "XpXq")]
                + [("ph_cluster", C.POINTER(C.c_int)), ("split_child", C.POINTER(C.c_uint)), ("split_parent", C.POINTER(C.c_uint)),
                   ("split_logfrac", C.POINTER(C.c_double)), ("init", C.POINTER(C.c_double)),
                   ("scratch_Sm", C.POINTER(C.c_double)), ("scratch_knn", C.POINTER(C.c_int)), ("scratch_lab", C.POINTER(C.c_int))])


class ClusterUpdateError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def cluster_update(sets, path=0, device=-1):
    """pchip_cluster_update: the clustering of an update on given point sets, by the run's own launchers.  sets: dicts with live [nlive][nDims],
    cluster [nlive] (0-based, -1: a dead slot) and optionally logL [nlive], ncluster, phantom [nph][nDims], ph_logL, ph_cluster, sub_dims,
    scratch (points the first cluster's scratch is asked for; 0: not).  None where the path does not exist; ClusterUpdateError (code) on
    failure; else one dict per set: the state after the update (include/polychord_hip.h), the per-cluster arrays cut to ncluster entries.
    path 0: one set, the one-run launchers.  path 1: the sets at once by the launchers of the runs in step; of a set's dict then live_cluster
    (as given), live_pos (a slot's part within its cluster, 1-based), cl_n (the parts of each cluster), levels and the scratch are meaningful."""
    lib = load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
    R = len(sets)
    S = (Settings * R)(); I = (ClusterIn * R)(); O = (ClusterOut * R)()
    keep, outs = [], []
    for r, st in enumerate(sets):
        x = np.ascontiguousarray(np.atleast_2d(st["live"]), dtype=np.float64)
        n, D = x.shape
        lc = np.ascontiguousarray(st["cluster"], dtype=np.int32)
        ll = np.ascontiguousarray(st.get("logL", np.zeros(n)), dtype=np.float64)
        ph = np.ascontiguousarray(np.reshape(st.get("phantom", np.zeros((0, D))), (-1, D)), dtype=np.float64)
        nph = ph.shape[0]
        pl = np.ascontiguousarray(st.get("ph_logL", np.zeros(nph)), dtype=np.float64)
        pc = np.ascontiguousarray(st.get("ph_cluster", np.zeros(nph)), dtype=np.int32)
        assert lc.shape == (n,) and ll.shape == (n,) and pl.shape == (nph,) and pc.shape == (nph,)
        nc = int(st.get("ncluster", lc.max() + 1))
        lib.pchip_settings_default(C.byref(S[r]), D, 0)
        S[r].device = device
        sd = np.ascontiguousarray(st.get("sub_dims", ()), dtype=np.int32)
        if sd.size:
            S[r].n_sub_cluster, S[r].sub_cluster_dims = int(sd.size), ip(sd)
        I[r].ncluster, I[r].nlive, I[r].nph = nc, n, nph
        I[r].live, I[r].live_logL, I[r].live_cluster = dptr(x), dptr(ll), ip(lc)
        if nph:
            I[r].phantom, I[r].ph_logL, I[r].ph_cluster = dptr(ph), dptr(pl), ip(pc)
        maxc, cap = min(nc + n, max(nc, int(st.get("maxc", 2048)))), int(st.get("scratch", 0))      # (room for that many clusters after the update)
        o = dict(live_cluster=np.full(n, -9, np.int32), live_pos=np.full(n, -9, np.int32), cl_list=np.full(n, -9, np.int32),
                 cl_n=np.full(maxc, -9, np.int32), imin_slot=np.full(maxc, -9, np.int32), ph_count=np.full(maxc, -9, np.int32),
                 cl_uid=np.zeros(maxc, np.uint32), XpXq=np.full((maxc, maxc), np.nan),
                 ph_cluster=np.full(max(nph, 1), -9, np.int32), split_child=np.zeros(maxc, np.uint32), split_parent=np.zeros(maxc, np.uint32),
                 split_logfrac=np.full(maxc, np.nan), init=np.full(5 * nc + nc * nc, np.nan))
        for k in ("logLp", "lse_ref", "lse_sum", "logXp", "logZp", "logZXp", "logZp2", "logZpXp"):
            o[k] = np.full(maxc, np.nan)
        if cap:
            o.update(Sm=np.full((cap, cap), np.nan), knn=np.full((cap, cap), -9, np.int32), lab=np.full(cap, -9, np.int32))
            O[r].scratch_Sm, O[r].scratch_knn, O[r].scratch_lab, O[r].scratch_cap = dptr(o["Sm"]), ip(o["knn"]), ip(o["lab"]), cap
        O[r].maxc, O[r].nsplit_cap = maxc, maxc
        for k in ("live_cluster", "live_pos", "cl_list", "cl_n", "imin_slot", "ph_count", "ph_cluster"):
            setattr(O[r], k, ip(o[k]))
        for k in ("cl_uid", "split_child", "split_parent"):
            setattr(O[r], k, up(o[k]))
        for k in ("logLp", "lse_ref", "lse_sum", "logXp", "logZp", "logZXp", "logZp2", "logZpXp", "XpXq", "split_logfrac", "init"):
            setattr(O[r], k, dptr(o[k]))
        keep.append((x, lc, ll, ph, pl, pc, sd))
        outs.append((o, n, nc, nph, cap, maxc))
    rc = lib.pchip_cluster_update(S, R, I, O, path)
    if rc == NO_SUCH_PATH:
        return None
    if rc != 0:
        msg = lib.polychord_hip_last_error()
        raise ClusterUpdateError(rc, f"pchip_cluster_update failed with code {rc}" + (": " + msg.decode(errors="replace") if rc == 1 and msg else ""))
    res = []
    for r, (o, n, nc0, nph, cap, maxc) in enumerate(outs):
        nc, nsp = O[r].ncluster, O[r].nsplit
        d = dict(ncluster=nc, nsplit=nsp, levels=O[r].levels, live_cluster=o["live_cluster"], live_pos=o["live_pos"],
                 ph_cluster=o["ph_cluster"][:nph], XpXq=o["XpXq"][:nc, :nc].copy(), init=o["init"][:5 * nc0].reshape(5, nc0),
                 XpXq0=o["init"][5 * nc0:].reshape(nc0, nc0))
        for k in ("cl_n", "imin_slot", "ph_count", "cl_uid", "logLp", "lse_ref", "lse_sum", "logXp", "logZp", "logZXp", "logZp2", "logZpXp"):
            d[k] = o[k][:nc]
        for k in ("split_child", "split_parent", "split_logfrac"):
            d[k] = o[k][:nsp]
        ends = np.cumsum(d["cl_n"])
        d["cl_list"] = [o["cl_list"][e - m:e] for e, m in zip(ends, d["cl_n"])]
        if cap:
            m = O[r].scratch_n
            d.update(scratch_n=m, Sm=o["Sm"].ravel()[:m * m].reshape(m, m), knn=o["knn"].ravel()[:m * m].reshape(m, m), lab=o["lab"][:m])
        res.append(d)
    return res


def directions(settings, like, prior, batch, seeds, chol, path):
    """pchip_directions: the directions of `len(seeds)` chains by the launcher a run takes (path 0: the whole kernels, 1: the split launch,
    2: the split launch with the packed bases); seeds [nchains][nTotal], chol [nDims][nDims].  None where the state has no such path.
    dict: nhat [nchains][nr][D] (generation order), nhat_w [nchains][nr], nhat_Ms / ch_My (None unless the run forms them), raw
    [nchains][bases][D][D] (paths 1 and 2: the orthonormal bases before whitening; NaN where nothing was copied)"""
    lib = load()
    D = settings.nDims
    sd = np.ascontiguousarray(np.atleast_2d(seeds), dtype=np.float64)
    ch = np.ascontiguousarray(chol, dtype=np.float64)
    assert ch.shape == (D, D) and sd.shape[1] == 2 * D + settings.nDerived + 2
    nch = sd.shape[0]
    if settings.nGrade > 1:
        off = np.concatenate([[0], np.cumsum([settings.grade_dims[g] for g in range(settings.nGrade)])[:-1]])
        reps = [settings.grade_repeats[g] for g in range(settings.nGrade)]
    else:
        off, reps = [0], [settings.num_repeats]
    nr = int(sum(reps))
    nb = int(sum(-(-r // (D - o)) for r, o in zip(reps, off)))
    nhat = np.full((nch, nr, D), np.nan); w = np.full((nch, nr), np.nan)
    Ms = np.full((nch, nr, D), np.nan); My = np.full((nch, D), np.nan); raw = np.full((nch, nb, D, D), np.nan)
    has = C.c_int(0)
    rc = lib.pchip_directions(C.byref(settings), C.byref(like), C.byref(prior), batch, nch, dptr(sd), dptr(ch), path, dptr(nhat), dptr(w),
                              dptr(Ms), dptr(My), C.byref(has), dptr(raw), nr, nb)
    if rc == NO_SUCH_PATH:
        return None
    if rc != 0:
        msg = lib.polychord_hip_last_error()
        raise RuntimeError(f"pchip_directions failed with code {rc}" + (": " + msg.decode(errors="replace") if rc == 1 and msg else ""))
    return dict(nhat=nhat, nhat_w=w, nhat_Ms=Ms if has.value else None, ch_My=My if has.value else None, raw=raw if path else None)


def deck_records(settings, like, prior, batch, nchains, fill=-1):
    """pchip_deck_records: the deck records the first half of the split launch leaves behind the bases of `nchains` chains, int32
    [nchains][66] = [tag lo, tag hi, deck[64]] exactly as they lie there; every int is `fill` where the kernel wrote nothing.  None where
    the state has no such path."""
    lib = load()
    # (bound here, not in load(): PCHIP_LIB may name an older build that has no such door)
    lib.pchip_deck_records.argtypes = [C.POINTER(Settings), C.POINTER(Like), C.POINTER(Prior), C.c_uint, C.c_int, C.POINTER(C.c_int)]
    lib.pchip_deck_records.restype = C.c_int
    rec = np.full((nchains, 66), fill, dtype=np.int32)
    rc = lib.pchip_deck_records(C.byref(settings), C.byref(like), C.byref(prior), batch, nchains, rec.ctypes.data_as(C.POINTER(C.c_int)))
    if rc == NO_SUCH_PATH:
        return None
    if rc != 0:
        msg = lib.polychord_hip_last_error()
        raise RuntimeError(f"pchip_deck_records failed with code {rc}" + (": " + msg.decode(errors="replace") if rc == 1 and msg else ""))
    return rec


def maximum_dict(m, nDims, nDerived):
    """dict copy of a filled pchip_maximum (the struct stays the caller's to free): status, cluster, niter, neval per leg ([0] likelihood,
    [1] posterior), max_logl / max_point, max_post / logl_at_post / post_point, logl_mean / mean_point (None without a mean)"""
    n = nDims + nDerived
    pt = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if p else None
    return dict(status=[int(v) for v in m.status], cluster=[int(v) for v in m.cluster], niter=[int(v) for v in m.niter], neval=[int(v) for v in m.neval],
                max_logl=m.max_logl, max_point=pt(m.max_point), max_post=m.max_post, logl_at_post=m.logl_at_post, post_point=pt(m.post_point),
                logl_mean=m.logl_mean if m.has_mean else None, mean_point=pt(m.mean_point) if m.has_mean else None)


def _maximum_out(lib, m, rc, who, nDims, nDerived, write):
    """the dict of `m` (freed here); a leg without a simplex (code 1, status set) is a result, any other failure raises"""
    try:
        if rc != 0 and not (rc == 1 and m.max_point and (m.status[0] or m.status[1])):
            msg = lib.polychord_hip_last_error()
            raise RuntimeError(f"{who} failed with code {rc}" + (": " + msg.decode(errors="replace") if msg else ""))
        if write is not None and lib.pchip_maximum_write(C.byref(m), nDims, nDerived, str(write).encode()) != 0:
            raise RuntimeError(f"pchip_maximum_write({write}) failed")
        return maximum_dict(m, nDims, nDerived)
    finally:
        lib.pchip_maximum_free(C.byref(m))


def maximise_device(settings, like, prior, run, max_iter=0, write=None):
    """pchip_maximise_device on the final live set of `run` (a dict of run(): live, live_cluster, post_mean): the maximum-likelihood and the
    maximum-posterior point of a problem that lives wholly on the device, one wavefront per leg; dict of maximum_dict.  max_iter 0: the
    host's cap of 200000 iterations; write: path of a <root>.maximum file to write as well"""
    lib = load()
    live = np.ascontiguousarray(run["live"], dtype=np.float64)
    cl = np.ascontiguousarray(run["live_cluster"], dtype=np.int32)
    mean = run.get("post_mean")
    mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
    m = Maximum()
    rc = lib.pchip_maximise_device(C.byref(settings), C.byref(like), C.byref(prior), dptr(live), cl.ctypes.data_as(C.POINTER(C.c_int)), live.shape[0],
                                   dptr(mean) if mean is not None else None, int(max_iter), C.byref(m))
    return _maximum_out(lib, m, rc, "pchip_maximise_device", settings.nDims, settings.nDerived, write)


def maximise_values(loglike, prior_fn, nDims, nDerived, logzero, live, live_cluster, post_mean=None, write=None):
    """pchip_maximise_values: the HOST maximiser through host function pointers (ctypes function objects or addresses); dict of maximum_dict"""
    lib = load()
    x = np.ascontiguousarray(live, dtype=np.float64)
    cl = np.ascontiguousarray(live_cluster, dtype=np.int32)
    mean = None if post_mean is None else np.ascontiguousarray(post_mean, dtype=np.float64)
    m = Maximum()
    rc = lib.pchip_maximise_values(C.cast(loglike, C.c_void_p), C.cast(prior_fn, C.c_void_p), nDims, nDerived, logzero, dptr(x),
                                   cl.ctypes.data_as(C.POINTER(C.c_int)), x.shape[0], dptr(mean) if mean is not None else None, C.byref(m))
    return _maximum_out(lib, m, rc, "pchip_maximise_values", nDims, nDerived, write)


def make_problem(kind, nDims, nDerived=0, lo=None, hi=None, mu=0.5, sigma=0.1, invcov=None, mean=None, logdet=0.0, source=0,
                 prior_table=None, hyper=None, prior_source=False):
    """(Like, Prior, keepalive) for a built-in device likelihood, or a device source ("source", source=handle), and a uniform box prior
    -- or, with prior_table = [(type, block, params) | (type, params), ...] (and hyper, the parameters' hypercube indices), a prior table
    evaluated inside the sampling kernels (pchip_prior.kind = 2) -- or, with prior_source=True, the source handle's own pchip_prior_param
    (pchip_prior.kind = 3; the handle from source_create(..., prior=True))."""
    keep = []
    L = Like()
    L.kind = LIKE_KINDS[kind]
    L.source = source
    L.mu, L.sigma, L.logdetcov = mu, sigma, logdet
    if invcov is not None:
        ic = np.ascontiguousarray(invcov, dtype=np.float64)
        mn = np.ascontiguousarray(mean, dtype=np.float64)
        keep += [ic, mn]
        L.invcov, L.mean = dptr(ic), dptr(mn)
    P = Prior()
    P.kind = 1
    if prior_source:
        P.kind = PRIOR_SOURCE
        return L, P, keep
    if prior_table is not None:
        arr, hy = globals()["prior_table"](prior_table, hyper)
        keep += [arr, hy]
        P.kind, P.table = PRIOR_TABLE, arr
        if hy is not None:
            P.hyper = hy.ctypes.data_as(C.POINTER(C.c_int))
        return L, P, keep
    if lo is not None:
        lo_a = np.ascontiguousarray(np.broadcast_to(lo, (nDims,)), dtype=np.float64)
        hi_a = np.ascontiguousarray(np.broadcast_to(hi, (nDims,)), dtype=np.float64)
        keep += [lo_a, hi_a]
        P.lo, P.hi = dptr(lo_a), dptr(hi_a)
    return L, P, keep


def set_grades(settings, dims, repeats):
    """fast/slow parameter grades with explicit repeats per grade; returns the arrays to keep alive"""
    gd = np.array(dims, dtype=np.int32)
    gr = np.array(repeats, dtype=np.int32)
    settings.nGrade = len(dims)
    settings.grade_dims = gd.ctypes.data_as(C.POINTER(C.c_int))
    settings.grade_repeats = gr.ctypes.data_as(C.POINTER(C.c_int))
    return gd, gr


def set_sub_clustering(settings, dims):
    """sub-dimension clustering on the 0-based cube coordinates `dims` (in this order); returns the array to keep alive"""
    sd = np.array(list(dims), dtype=np.int32)
    settings.n_sub_cluster = len(sd)
    settings.sub_cluster_dims = sd.ctypes.data_as(C.POINTER(C.c_int)) if len(sd) else None
    return sd


class _Owner:
    """Keeps a pchip_result alive for the numpy views handed out by run(); frees it when the last view dies."""

    def __init__(self, lib, res):
        self.lib, self.res = lib, res

    def __del__(self):
        try:
            self.lib.pchip_result_free(C.byref(self.res))
        except Exception:
            pass


class _View:
    """array-interface shim: numpy keeps this object (and through it the owner) as the array's base"""

    def __init__(self, owner, ptr, shape):
        self.owner = owner
        addr = C.cast(ptr, C.c_void_p).value or 0
        self.__array_interface__ = {"data": (addr, False), "shape": tuple(shape), "typestr": "<f8", "version": 3}


def _view(owner, ptr, shape):
    if int(np.prod(shape)) == 0:
        return np.zeros(shape)
    return np.asarray(_View(owner, ptr, shape))


def run(settings, like, prior):
    """pchip_run -> dict; the big arrays (dead points, weights, live points) are zero-copy views of the
    engine's pinned result buffers, released when the last view is garbage collected."""
    lib = load()
    r = Result()
    rc = lib.pchip_run(C.byref(settings), C.byref(like), C.byref(prior), C.byref(r))
    if rc != 0:
        raise RuntimeError(f"pchip_run failed with code {rc}")
    return result_dict(r, settings)


def result_dict(r, settings):
    """dict view of a filled pchip_result; takes ownership (the block is freed when the last array view dies)"""
    lib = load()
    own = _Owner(lib, r)
    nT, nd, D = r.nTotal, r.ndead, settings.nDims
    out = dict(logZ=r.logZ, logZerr=float(np.sqrt(abs(r.varlogZ))), varlogZ=r.varlogZ, ndead=nd, nlike=r.nlike,
               niter=r.niter, nbatches=r.nbatches, nrounds=r.nrounds, nupdates=r.nupdates, ncluster=r.ncluster,
               ncluster_dead=r.ncluster_dead, nTotal=nT, batch=r.batch, t_generate=r.t_generate, t_loop=r.t_loop,
               t_final=r.t_final, t_total=r.t_total, t_setup=r.t_setup, t_results=r.t_results, t_teardown=r.t_teardown,
               kernel_time={n: {"total_s": r.k_time_s[i], "launches": r.k_launches[i]}
                            for i, n in enumerate(KERNEL_CLASSES) if r.k_launches[i] > 0},
               dead=_view(own, r.dead, (nd, nT)),
               logweights=_view(own, r.logweights, (nd,)),
               entry=_view(own, r.entry, (nd,)),
               live=_view(own, r.live, (r.nlive_final, nT)),
               live_cluster=(np.ctypeslib.as_array(r.live_cluster, shape=(r.nlive_final,)).copy() if r.live_cluster and r.nlive_final > 0
                             else np.zeros(max(r.nlive_final, 0), dtype=np.int32)),
               logZp=np.ctypeslib.as_array(r.logZp, shape=(max(r.nZp, 1),))[:r.nZp].copy(),
               post_mean=np.ctypeslib.as_array(r.post_mean, shape=(D + settings.nDerived,)).copy(),
               post_var=np.ctypeslib.as_array(r.post_var, shape=(D + settings.nDerived,)).copy(),
               nlike_grade=[int(v) for v in r.nlike_grade], nlike_failed=r.nlike_failed, ncluster_peak=r.ncluster_peak, epoch_discard=r.epoch_discard, n_records=int(r.n_records) if r.d_records else None,
               path=dict({n: int(r.path[i]) for i, n in enumerate(PATH_NAMES)}, device_batch=int(r.path[PATH_DEVICE_BATCH])),
               varlogZp=np.ctypeslib.as_array(r.varlogZp, shape=(max(r.nZp, 1),))[:r.nZp].copy(),
               logzero=settings.logzero,
               _owner=own)          # the pchip_result itself (merge.comm_merge hands it back to the library)
    return out
