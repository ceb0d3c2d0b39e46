"""The batched quadratic form of a device source (pchip_source_create_quad_batch): chi2 = r^T P r of all parked proposals of a round at once
on the fp64 matrix cores, up to 4096 residuals (polychordlite_amd/csrc/pc_quad_mm.hip; the two run-time kernels around it, k_quad_residuals
and k_quad_finish, in pc_sample.hip under PCHIP_USER_QUAD_BATCH).  The fixture is test_source_quad.py's: the line a + b x_i under AR(1) noise,
derived parameters chi2 and the first residual.

The kernel's condition is DERIVED, not measured.  q_j = sum_i P_ij r_i by nres accumulations in any order, fused or not, errs by at most
gamma_nres sum_i |P_ij r_i|; the product with r_j and the sum over j add gamma_(nres + 1); so
    |chi2_dev - chi2_ref| <= (2 nres + 4) 2^-53 S,      S = sum_ij |r_i| |P_ij| |r_j|,
with chi2_ref and S formed in long double from the residuals as the source forms them.  The matrices are the dense AR(1) inverse and a dense
NON-symmetric one with entries +-uniform(0.5, 1.5): every entry carries about 1 / nres^2 of S, so a dropped edge element or a transposed
read misses the bound by many orders (a matrix over six decades could hide a lost small entry under it: not used here).

CPU: the surface, the refusals, the two kernels compile for gfx950 from handles of 17, 1025 and 4096 residuals.  GPU: the kernel against
long double at the tile edges of both indices; a row's bits do not depend on the other rows, on the row's place, on n or on where a long block is cut; agreement with the
in-kernel form; a run at nres = 1040 (dead rows are pchip_source_eval's bits, the posterior against generalised least squares, logZ against
the closed form); two seeds in step are their solo runs; the refusals; the pypolychord door."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_source_quad import QUAD, LO, HI, _line_data, _precision, _residuals, _box_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _door(lib):
    """the door this file is about: a library without the feature fails here, at the missing symbol"""
    assert hasattr(lib, "pchip_source_create_quad_batch"), "the library does not export pchip_source_create_quad_batch"
    return lib.pchip_source_create_quad_batch


def _create(api, text, **kw):
    _door(api.load())
    return api.source_create(text, batched=True, **kw)


def _settings(api, D, nDer, **kw):
    s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _matrix(kind, n):
    """ar1: the dense inverse of the AR(1) covariance; nonsym: dense, NOT symmetric, entries +-uniform(0.5, 1.5)"""
    if kind == "ar1":
        return _precision("ar1", n)
    rng = np.random.default_rng(1000 + n)
    return np.ascontiguousarray(rng.choice([-1.0, 1.0], (n, n)) * rng.uniform(0.5, 1.5, (n, n)))


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_the_symbol_is_exported_and_the_abi_is_still_9():
    api, lib = _lib()
    _door(lib)
    assert lib.pchip_abi_version() == 9
    hdr = open(os.path.join(ROOT, "include", "polychord_hip.h")).read()
    assert "#define PCHIP_SOURCE_MAX_RES_BATCH 4096" in hdr and "#define PCHIP_SOURCE_MAX_RES 1024" in hdr
    assert "int  pchip_source_create_quad_batch(" in hdr


@pytest.mark.parametrize("nres", [0, -1, 4097])
def test_nres_out_of_range_is_refused_with_the_range(nres):
    api, lib = _lib()
    one = np.ones(1)
    h = _door(lib)(QUAD.encode(), b"-DNRES=4", None, 0, nres, api.dptr(one))
    msg = lib.polychord_hip_last_error().decode()
    assert h == -1 and "pchip_source_create_quad_batch" in msg and "nres" in msg and "1 <= nres <= 4096" in msg


def test_no_precision_is_refused():
    api, lib = _lib()
    h = _door(lib)(QUAD.encode(), b"-DNRES=4", None, 0, 4, None)
    assert h == -1 and "precision == NULL" in lib.polychord_hip_last_error().decode()
    with pytest.raises(RuntimeError) as e:
        _create(api, QUAD, options=("-DNRES=4",), data=_line_data(4), residuals=4, precision=None)
    assert "precision == NULL" in str(e.value)


def test_a_source_that_lacks_one_of_its_functions_is_refused_by_name():
    api, _ = _lib()
    kw = dict(options=("-DNRES=8",), data=_line_data(8), residuals=8, precision=_precision("ar1", 8))
    cut = QUAD.index("__device__ double pchip_logl_finish")
    with pytest.raises(RuntimeError) as e:
        _create(api, "#pragma clang fp contract(off)\n" + QUAD[cut:], **kw)
    assert "pchip_residual" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        _create(api, QUAD[:cut], **kw)
    assert "pchip_logl_finish" in str(e.value)


@pytest.mark.parametrize("nres", [17, 1025, 4096])
def test_the_two_kernels_compile_for_gfx950(nres):
    api, lib = _lib()
    P = np.eye(nres)
    h = _create(api, QUAD, options=(f"-DNRES={nres}",), data=_line_data(nres), residuals=nres, precision=P)
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", b"k_quad_residuals;k_quad_finish", log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")
    lib.pchip_source_destroy(h)


def test_the_embedded_text_is_still_five_files():
    api, lib = _lib()
    _door(lib)
    seen, i = [], 0
    while True:
        name = C.c_char_p()
        if lib.pchip_rtc_embedded_source(i, C.byref(name)) is None:
            break
        seen.append(name.value.decode())
        i += 1
    assert sorted(seen) == sorted(["pc_dev.h", "pc_state.h", "pc_seed.h", "pc_sample.hip", "pc_slice_body.inc"])


def test_a_precision_of_another_shape_is_a_value_error():
    api, lib = _lib()
    _door(lib)
    for bad in (np.eye(5), np.ones(16), np.ones((2, 8))):
        with pytest.raises(ValueError):
            _create(api, QUAD, options=("-DNRES=4",), data=_line_data(4), residuals=4, precision=bad)


def test_batched_without_residuals_is_a_value_error():
    api, lib = _lib()
    _door(lib)
    with pytest.raises(ValueError):
        api.source_create(QUAD, batched=True)
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    with pytest.raises(ValueError):
        dl.Source(QUAD, batched=True)


def test_the_form_says_batched_and_nothing_in_kernel():
    """the launchers' record of the handle: no terms, no quadratic form in the kernels (their LDS helpers answer 0), the matrix in the tail"""
    api, lib = _lib()

    class Form(C.Structure):
        _fields_ = [("nterms", C.c_long), ("nsums", C.c_int), ("nquad", C.c_long), ("nshared", C.c_long), ("has_prior", C.c_int),
                    ("ndata", C.c_longlong), ("ntail", C.c_longlong), ("alive", C.c_int), ("nbatch", C.c_int)]
    h = _create(api, QUAD, options=("-DNRES=9",), data=_line_data(9), residuals=9, precision=np.eye(9))
    f = Form()
    lib.pc_rtc_source_form.argtypes = [C.c_int, C.POINTER(Form)]
    lib.pc_rtc_source_form.restype = C.c_int
    assert lib.pc_rtc_source_form(h, C.byref(f)) == 0
    assert (f.nterms, f.nsums, f.nquad, f.nshared, f.has_prior, f.ndata, f.ntail, f.alive, f.nbatch) == (0, 0, 0, 0, 0, 18, 81, 1, 9)
    lib.pchip_source_destroy(h)
    assert lib.pc_rtc_source_form(h, C.byref(f)) == 0 and f.alive == 0 and f.nbatch == 9


# ---------------------------------------------------------------------------------------------------------------------------- GPU
_HANDLES, _REFS = {}, {}
NPTS = 130


@pytest.fixture(scope="module", autouse=True)
def _destroy_handles():
    yield
    api, lib = _lib()
    for h in _HANDLES.values():
        lib.pchip_source_destroy(h)
    _HANDLES.clear(); _REFS.clear()


def _problem(api, kind, nres):
    """(handle, data, P) for a matrix and a size, made once for the module: its two kernels compile once"""
    data, P = _line_data(nres, seed=100 + nres), _matrix(kind, nres)
    if (kind, nres) not in _HANDLES:
        _HANDLES[(kind, nres)] = _create(api, QUAD, options=(f"-DNRES={nres}",), data=data, residuals=nres, precision=P)
    return _HANDLES[(kind, nres)], data, P


def _long_double(r, P):
    """chi2_ref and S of every row of r in long double (P in slabs of rows: 4096^2 long doubles at once would be 256 MB)"""
    rl, ra = r.astype(np.longdouble), np.abs(r).astype(np.longdouble)
    q, qa = np.zeros(r.shape, np.longdouble), np.zeros(r.shape, np.longdouble)
    for i0 in range(0, P.shape[0], 256):
        Pl = P[i0:i0 + 256].astype(np.longdouble)
        q += rl[:, i0:i0 + 256] @ Pl
        qa += ra[:, i0:i0 + 256] @ np.abs(Pl)
    return (q * rl).sum(axis=1), (qa * ra).sum(axis=1)


def _reference(api, kind, nres, npts=NPTS):
    """the points, chi2_ref and S of a problem, computed once and shared: _box_points(n, seed) is the first n rows of _box_points(130, seed)"""
    key = (kind, nres, npts)
    if key not in _REFS:
        h, data, P = _problem(api, kind, nres)
        th = _box_points(npts, nres)
        ref, S = _long_double(_residuals(th, data), P)
        th.setflags(write=False); ref.setflags(write=False); S.setflags(write=False)
        _REFS[key] = (th, ref, S)
    return _REFS[key]


def _check_against_long_double(api, kind, nres, n, npts=NPTS):
    h, data, P = _problem(api, kind, nres)
    th_all, ref, S = _reference(api, kind, nres, npts)
    th = np.ascontiguousarray(th_all[:n])
    assert np.array_equal(th, _box_points(n, nres))
    logL, phi = api.source_eval(h, th, 2)
    err = np.abs(phi[:, 0].astype(np.longdouble) - ref[:n])
    bound = (2 * nres + 4) * EPS * S[:n]
    print(f"{kind} nres {nres} n {n}: max |chi2 - ref| / bound = {float(np.max(err / bound)):.4f}")
    assert np.all(np.isfinite(phi)) and np.all(err <= bound)
    assert np.array_equal(logL, -phi[:, 0] / 2.0)
    assert np.array_equal(phi[:, 1], _residuals(th, data)[:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 130])
@pytest.mark.parametrize("nres", [1, 3, 15, 16, 17, 67, 1025])
@pytest.mark.parametrize("kind", ["ar1", "nonsym"])
def test_the_kernel_against_long_double(engine, kind, nres, n):
    _check_against_long_double(engine, kind, nres, n)


@pytest.mark.gpu
def test_the_kernel_against_long_double_at_the_largest_nres(engine):
    _check_against_long_double(engine, "nonsym", 4096, 3, npts=3)


@pytest.mark.gpu
@pytest.mark.parametrize("nres", [67, 1025])
def test_a_rows_bits_depend_on_that_row_alone(engine, nres):
    """the same 130 points in another order, the first 17 alone, and with the other rows replaced by huge values: every common row the same bits"""
    api = engine
    h, data, P = _problem(api, "nonsym", nres)
    th = np.array(_reference(api, "nonsym", nres)[0])
    l0, p0 = api.source_eval(h, th, 2)
    perm = np.random.default_rng(5).permutation(NPTS)
    l1, p1 = api.source_eval(h, np.ascontiguousarray(th[perm]), 2)
    assert np.array_equal(l1.view(np.uint64), l0[perm].view(np.uint64)) and np.array_equal(p1.view(np.uint64), p0[perm].view(np.uint64))
    l2, p2 = api.source_eval(h, np.ascontiguousarray(th[:17]), 2)
    assert np.array_equal(l2.view(np.uint64), l0[:17].view(np.uint64)) and np.array_equal(p2.view(np.uint64), p0[:17].view(np.uint64))
    keep = np.arange(NPTS) % 7 == 3                      # (rows in every row tile and both halves of the 64-row block)
    huge = th.copy()
    huge[~keep] = [1e300, 0.0]                           # residuals of -1e300 in every other row
    l3, p3 = api.source_eval(h, huge, 2)
    assert np.array_equal(l3[keep].view(np.uint64), l0[keep].view(np.uint64)) and np.array_equal(p3[keep].view(np.uint64), p0[keep].view(np.uint64))
    assert not np.any(np.isfinite(l3[~keep]))


@pytest.mark.gpu
def test_a_block_longer_than_a_slab_is_cut_invisibly(engine):
    """more rows than one evaluation takes (PC_QUAD_BATCH_SLAB = 8192, pc_launch.h): the block goes slab by slab through the same scratch,
    and a row has the bits it has alone -- on either side of the cut"""
    api = engine
    nres = 3
    h, data, P = _problem(api, "nonsym", nres)
    th = _box_points(8192 + 70, 77)
    l0, p0 = api.source_eval(h, th, 2)
    for rows in (slice(0, 17), slice(8180, 8192 + 70)):
        l1, p1 = api.source_eval(h, np.ascontiguousarray(th[rows]), 2)
        assert np.array_equal(l1.view(np.uint64), l0[rows].view(np.uint64)) and np.array_equal(p1.view(np.uint64), p0[rows].view(np.uint64))
    ref, S = _long_double(_residuals(th, data), P)
    assert np.all(np.abs(p0[:, 0].astype(np.longdouble) - ref) <= (2 * nres + 4) * EPS * S)


@pytest.mark.gpu
def test_agreement_with_the_in_kernel_form(engine):
    """nres = 256, the same text, data and P: chi2 within the sum of the two derived bounds (the in-kernel form's: test_source_quad.py,
    nres 2^-52 S)"""
    api = engine
    nres = 256
    hb, data, P = _problem(api, "ar1", nres)
    hq = api.source_create(QUAD, options=(f"-DNRES={nres}",), data=data, residuals=nres, precision=P)
    try:
        th = _box_points(40, 9)
        _, S = _long_double(_residuals(th, data), P)
        lq, pq = api.source_eval(hq, th, 2)
        lb, pb = api.source_eval(hb, th, 2)
        bound = ((2 * nres + 4) * EPS + nres * 2.0 * EPS) * S
        diff = np.abs(pq[:, 0].astype(np.longdouble) - pb[:, 0].astype(np.longdouble))
        print(f"max |chi2_quad - chi2_batch| / bound = {float(np.max(diff / bound)):.4f}")
        assert np.all(diff <= bound)
        assert np.array_equal(pq[:, 1], pb[:, 1])
    finally:
        api.load().pchip_source_destroy(hq)


def _gls(data, P, nres):
    """(theta_hat, Fisher matrix, chi2 at theta_hat) of the line under P's symmetric part"""
    x, d = data[:nres], data[nres:]
    A, Ps = np.stack([np.ones(nres), x], axis=1), (P + P.T) / 2.0
    F = A.T @ Ps @ A
    hat = np.linalg.solve(F, A.T @ Ps @ d)
    rr = d - A @ hat
    return hat, F, float(rr @ Ps @ rr)


RUN_KW = dict(nlive=100, num_repeats=4)
TABLE = [("uniform", [-1.0, 2.0]), ("uniform", [-1.0, 2.0])]


@pytest.mark.gpu
@pytest.mark.parametrize("prior", ["box", "table"])
def test_a_run_at_1040_residuals(engine, prior):
    api = engine
    nres = 1040
    h, data, P = _problem(api, "ar1", nres)
    kw = dict(prior_table=TABLE) if prior == "table" else dict(lo=LO, hi=HI)
    L, Pr, keep = api.make_problem("source", 2, 2, source=h, **kw)
    r = api.run(_settings(api, 2, 2, seed=7, **RUN_KW), L, Pr)
    assert r["path"]["device_batch"] > 0 and r["path"]["source_kernels"] > 0 and r["ndead"] > 500
    dead = np.array(r["dead"])
    ok = dead[:, -1] > -1e29
    assert ok.sum() > 500
    # every dead row's logL (and chi2) is pchip_source_eval of its theta, bit for bit
    le, pe = api.source_eval(h, np.ascontiguousarray(dead[ok, 2:4]), 2)
    assert np.array_equal(le.view(np.uint64), dead[ok, -1].view(np.uint64))
    assert np.array_equal(pe.view(np.uint64), np.ascontiguousarray(dead[ok, 4:6]).view(np.uint64))
    # the posterior mean against generalised least squares, the evidence against the closed form of the linear-Gaussian model under the box
    hat, F, chi2_min = _gls(data, P, nres)
    sd = np.sqrt(r["post_var"][:2])
    logZ = -chi2_min / 2.0 + np.log(2.0 * np.pi) - 0.5 * np.log(np.linalg.det(F)) - np.log((HI[0] - LO[0]) * (HI[1] - LO[1]))
    cov = np.linalg.inv(F)
    assert np.all(hat - 8.0 * np.sqrt(np.diag(cov)) > LO[0]) and np.all(hat + 8.0 * np.sqrt(np.diag(cov)) < HI[0])      # (the box holds the posterior)
    print(f"{prior}: post mean {r['post_mean'][:2]} +/- {sd}, gls {hat}; logZ {r['logZ']:.4f} +/- {r['logZerr']:.4f}, closed form {logZ:.4f}")
    assert np.all(np.abs(r["post_mean"][:2] - hat) <= 5.0 * sd)
    assert abs(r["logZ"] - logZ) <= 5.0 * r["logZerr"]


@pytest.mark.gpu
def test_runs_in_step_are_their_solo_runs(engine):
    api = engine
    from polychordlite_amd import repeats
    h, data, P = _problem(api, "ar1", 67)
    L, Pr, keep = api.make_problem("source", 2, 2, source=h, lo=LO, hi=HI)
    # (40 chains a nursery: the group's ticks carry up to 80 rows, more than the 64 the first run's scratch holds -- two slabs)
    kw = dict(nlive=50, num_repeats=5, batch=40)
    seeds = [21, 22]
    merged, runs = repeats.run_in_step(_settings(api, 2, 2, **kw), L, Pr, seeds, max_in_flight=4)
    assert len(runs) == 2
    for seed, r in zip(seeds, runs):
        solo = api.run(_settings(api, 2, 2, seed=seed, **kw), L, Pr)
        for k in ("ndead", "nlike", "niter"):
            assert r[k] == solo[k], (seed, k, r[k], solo[k])
        assert r["ndead"] > 0 and r["logZ"] == solo["logZ"] and np.array_equal(r["dead"], solo["dead"]), seed
        assert r["path"]["device_batch"] > 0 and r["path"]["device_batch"] == solo["path"]["device_batch"], r["path"]


@pytest.mark.gpu
def test_refusals_on_a_live_device(engine):
    api = engine
    lib = api.load()
    h, data, P = _problem(api, "ar1", 67)
    s = _settings(api, 2, 2, seed=7, nlive=50, num_repeats=5, batch=10)
    # the handle has no prior of its own
    L, Pr, keep = api.make_problem("source", 2, 2, source=h, prior_source=True)
    r = api.Result()
    assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(Pr), C.byref(r)) == 1
    msg = lib.polychord_hip_last_error().decode()
    assert "batched quadratic form" in msg and "prior.kind = 3" in msg
    # a host prior
    L, Pr, keep = api.make_problem("source", 2, 2, source=h, lo=LO, hi=HI)
    Pr.kind = 0
    assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(Pr), C.byref(r)) == 1
    msg = lib.polychord_hip_last_error().decode()
    assert "batched quadratic form" in msg and "host prior" in msg
    # the device maximiser: not covered
    L, Pr, keep = api.make_problem("source", 2, 2, source=h, lo=LO, hi=HI)
    g = api.run(s, L, Pr)
    with pytest.raises(RuntimeError) as e:
        api.maximise_device(s, L, Pr, g)
    assert "batched quadratic form" in str(e.value) and "not covered" in str(e.value)


@pytest.mark.gpu
def test_through_pypolychord_run(engine, tmp_path, capfd):
    """Source(..., batched=True) under UniformPrior writes .stats; the same logZ as through _ctypes_api.run (the kernels a run with hooks
    takes: tests/test_source_doors.py, HOOKS_MODES); maximise=True prints that it is not covered and the run stands"""
    api = engine
    lib = api.load()
    from polychordlite_amd import pypolychord
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    nres = 64
    data, P = _line_data(nres, seed=100 + nres), _matrix("ar1", nres)
    src = dl.Source(QUAD, nDerived=2, data=data, residuals=nres, precision=P, options=(f"-DNRES={nres}",), batched=True)
    try:
        lib.polychord_hip_set_option(b"batch", 20.0)
        try:
            pypolychord.run(src, 2, nDerived=2, prior=dl.UniformPrior(LO[0], HI[0]), nlive=50, num_repeats=5, seed=7, do_clustering=False, feedback=1,
                            base_dir=str(tmp_path), file_root="qb", read_resume=False, write_resume=False, posteriors=False, equals=False,
                            cluster_posteriors=False, write_live=False, write_prior=False, write_dead=True, write_stats=True, maximise=True)
        finally:
            lib.polychord_hip_set_option(b"batch", 0.0)
        out = capfd.readouterr().out
        assert "in batches on the matrix cores" in out and "not covered" in out
        assert not (tmp_path / "qb.maximum").exists()
        text = open(tmp_path / "qb.stats").read()
        m = re.search(r"log\(Z\)\s*=\s*([-+0-9.Ee]+)\s*\+/-\s*([-+0-9.Ee]+)", text)
        L, Pr, keep = api.make_problem("source", 2, 2, source=src.handle, lo=LO, hi=HI)
        g = api.run(_settings(api, 2, 2, seed=7, nlive=50, num_repeats=5, batch=20, do_clustering=0, ablate=2 | 4), L, Pr)
        assert g["path"]["device_batch"] > 0
        assert float(m.group(1)) == float("%.14E" % g["logZ"]) and float(m.group(2)) == float("%.14E" % g["logZerr"])
    finally:
        lib.polychord_hip_set_source(0)
        src.close()
