"""A device-source handle is one form record (PcSourceForm, pc_launch.h) that outlives the handle: pc_rtc_source_form answers the same after
pchip_source_destroy as before it, with alive = 0, so that a run in flight keeps its launch shapes, while whatever starts work on the handle
refuses it as one that does not exist.  The data block is handed out as a hold: tools/dev/source_hold_record.hip checks, as a stand-alone
program under the host sanitizers, that a hold taken before the destroy still reads the doubles that went in.  All on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polychordlite_amd", "csrc")


class Form(C.Structure):
    """PcSourceForm (pc_launch.h)"""
    _fields_ = [("nterms", C.c_long), ("nsums", C.c_int), ("nquad", C.c_long), ("nshared", C.c_long), ("has_prior", C.c_int),
                ("ndata", C.c_longlong), ("ntail", C.c_longlong), ("alive", C.c_int)]

    def fields(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


PRIOR = "__device__ double pchip_prior_param(const double *c, int i, int, const double *, long) { return c[i]; }\n"
PLAIN = "__device__ double pchip_loglikelihood(const double *t, double *, int, int, const double *d, long) { return t[0] * d[0]; }\n"
TERMS = ("__device__ double pchip_logl_term(const double *t, int, const double *d, long, long i) { return t[0] * d[i]; }\n"
         "__device__ double pchip_logl_finish(double s, const double *, double *, int, int, const double *, long) { return s; }\n")
SUMS = ("__device__ void pchip_logl_terms(const double *t, int, const double *d, long, long i, double *o) { for (int k = 0; k < PCHIP_SRC_NSUMS; ++k) o[k] = t[0] * d[i]; }\n"
        "__device__ double pchip_logl_finish_sums(const double *s, const double *, double *, int, int, const double *, long) { return s[0]; }\n")
QUAD = ("__device__ double pchip_residual(const double *t, int, const double *d, long, long i) { return t[0] - d[i]; }\n"
        "__device__ double pchip_logl_finish(double c, const double *, double *, int, int, const double *, long) { return -0.5 * c; }\n")
SHARED_TERMS = ("__device__ double pchip_shared_value(const double *t, int, const double *, long, long k) { return t[0] + k; }\n"
                "__device__ double pchip_logl_term(const double *t, const double *s, int, const double *d, long, long i) { return s[0] * d[i]; }\n"
                "__device__ double pchip_logl_finish(double s, const double *, const double *, double *, int, int, const double *, long) { return s; }\n")
SHARED_QUAD = ("__device__ double pchip_shared_value(const double *t, int, const double *, long, long k) { return t[0] + k; }\n"
               "__device__ double pchip_residual(const double *t, const double *s, int, const double *d, long, long i) { return s[0] - d[i]; }\n"
               "__device__ double pchip_logl_finish(double c, const double *, const double *, double *, int, int, const double *, long) { return -0.5 * c; }\n")
ND, NRES = 7, 3
# (keywords of api.source_create, the form it must make): one handle of each form
HANDLES = {
    "plain": (PLAIN, {}, dict(nterms=0, nsums=0, nquad=0, nshared=0, has_prior=0, ntail=0)),
    "terms": (TERMS, dict(nterms=ND), dict(nterms=ND, nsums=0, nquad=0, nshared=0, has_prior=0, ntail=0)),
    "plain with prior": (PLAIN + PRIOR, dict(prior=True), dict(nterms=0, nsums=0, nquad=0, nshared=0, has_prior=1, ntail=0)),
    "sums": (SUMS, dict(nterms=ND, nsums=5), dict(nterms=ND, nsums=5, nquad=0, nshared=0, has_prior=0, ntail=0)),
    "quadratic": (QUAD + PRIOR, dict(residuals=NRES, precision=np.eye(NRES), prior=True), dict(nterms=NRES, nsums=0, nquad=NRES, nshared=0, has_prior=1, ntail=NRES * NRES)),
    "terms with shared": (SHARED_TERMS, dict(nterms=ND, shared=4), dict(nterms=ND, nsums=0, nquad=0, nshared=4, has_prior=0, ntail=0)),
    "quadratic with shared": (SHARED_QUAD, dict(residuals=NRES, precision=np.eye(NRES), shared=2), dict(nterms=NRES, nsums=0, nquad=NRES, nshared=2, has_prior=0, ntail=NRES * NRES)),
}


def _lib():
    from polychordlite_amd import _ctypes_api as api
    lib = api.load()
    lib.pc_rtc_source_form.argtypes = [C.c_int, C.POINTER(Form)]
    lib.pc_rtc_source_form.restype = C.c_int
    return api, lib


@pytest.mark.parametrize("name", sorted(HANDLES))
def test_the_form_outlives_the_handle(name):
    api, lib = _lib()
    src, kw, want = HANDLES[name]
    h = api.source_create(src, data=np.arange(ND) + 0.5, **kw)
    want = dict(want, ndata=ND, alive=1)
    f = Form()
    assert lib.pc_rtc_source_form(h, C.byref(f)) == 0 and f.fields() == want
    lib.pchip_source_destroy(h)
    g = Form()
    assert lib.pc_rtc_source_form(h, C.byref(g)) == 0 and g.fields() == dict(want, alive=0)
    # whatever starts work refuses it, in the words for a handle that never existed
    assert lib.polychord_hip_set_source(h) != 0
    assert (b"device source handle %d does not exist" % h) in lib.polychord_hip_last_error()
    log = C.create_string_buffer(1 << 12)
    assert lib.pchip_rtc_compile_check(h, b"gfx950", b"k_source_eval<1>", log, len(log), None) != 0
    assert (b"device source handle %d does not exist" % h) in log.value
    with pytest.raises(RuntimeError, match="device source handle %d does not exist" % h):
        api.source_eval(h, np.full((1, 2), 0.5))
    lib.pchip_source_destroy(h)      # (a second time: nothing happens)
    assert lib.pc_rtc_source_form(h, C.byref(g)) == 0 and g.fields() == dict(want, alive=0)


def test_an_id_that_never_existed_has_no_form():
    _, lib = _lib()
    f = Form(nterms=3, alive=1)
    assert lib.pc_rtc_source_form(987654, C.byref(f)) != 0
    assert not any(f.fields().values())


def test_a_hold_outlives_the_destroy():
    """the stand-alone program (host sanitizers; a missing hipcc fails the test, it does not skip it)"""
    subprocess.run(["make", "-C", CSRC, "source_hold_record"], check=True, capture_output=True, text=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "dev", "source_hold_record")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "6 handles, 0 disagreements"
