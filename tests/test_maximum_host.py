"""The maximiser's three parts on the host (pc_maximise.hip): the choice of simplex, the values (pchip_maximise_values), the writer
(pchip_maximum_write) -- and the device door's refusals, which need no device.  The device side: tests/test_maximum_device.py."""
import ctypes as C

import numpy as np
import pytest


def _api():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _gauss_rows(live_cube, nDer, mu=0.5, sigma=0.1):
    """live rows [cube | theta | phi | birth | logL] of the built-in Gaussian under the unit box"""
    n, D = live_cube.shape
    rows = np.zeros((n, 2 * D + nDer + 2))
    rows[:, :D] = live_cube
    rows[:, D:2 * D] = live_cube
    rows[:, -1] = -D * (np.log(sigma) + 0.5 * np.log(2 * np.pi)) - 0.5 * np.sum(((live_cube - mu) / sigma) ** 2, axis=1)
    return rows


def _host_fns(lib, D, mu=0.5, sigma=0.1):
    lib.polychord_hip_set_gaussian(mu, sigma)
    lo, hi = np.zeros(D), np.ones(D)
    lib.polychord_hip_set_uniform_prior(D, lo.ctypes.data_as(C.POINTER(C.c_double)), hi.ctypes.data_as(C.POINTER(C.c_double)))
    return C.cast(lib.polychord_hip_gaussian, C.c_void_p), C.cast(lib.polychord_hip_uniform_prior, C.c_void_p)


def test_the_struct_mirror_and_the_symbols():
    api, lib = _api()
    assert lib.pchip_sizeof(b"maximum") == C.sizeof(api.Maximum) > 0
    assert lib.pchip_abi_version() == 9
    for sym in ("pchip_maximise_values", "pchip_maximise_device", "pchip_maximise_device_many", "pchip_maximum_write", "pchip_maximum_free"):
        assert hasattr(lib, sym), sym


def test_values_and_writer_are_the_file_of_pchip_maximise(tmp_path):
    """the live set of test_maximiser_on_the_host: pchip_maximise_values written out by pchip_maximum_write is, byte for byte, the file
    pchip_maximise writes"""
    api, lib = _api()
    D, nDer, n = 4, 1, 60
    like, prior = _host_fns(lib, D)
    rng = np.random.default_rng(5)
    live = _gauss_rows(0.5 + 0.03 * rng.standard_normal((n, D)), nDer)
    cl = np.zeros(n, dtype=np.int32)
    mean = np.array([0.5, 0.5, 0.5, 0.5, 0.0])
    f = lib.pchip_maximise
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.c_char_p]
    for k, mn in enumerate((mean, None)):
        a, b = tmp_path / f"a{k}.maximum", tmp_path / f"b{k}.maximum"
        assert f(like, prior, D, nDer, -1e30, api.dptr(live), cl.ctypes.data_as(C.POINTER(C.c_int)), n, api.dptr(mn) if mn is not None else None, str(a).encode()) == 0
        m = api.maximise_values(like, prior, D, nDer, -1e30, live, cl, post_mean=mn, write=b)
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 200
        assert m["status"] == [0, 0] and m["cluster"] == [0, 0] and min(m["niter"]) > 0 and min(m["neval"]) >= min(m["niter"])
        assert (m["logl_mean"] is None) == (mn is None)
        norm = -D * (np.log(0.1) + 0.5 * np.log(2 * np.pi))
        assert abs(m["max_logl"] - norm) < 1e-4 and np.all(np.abs(m["max_point"][:D] - 0.5) < 2e-3)
        assert abs(m["max_post"] - m["logl_at_post"]) < 1e-9          # the unit box: dX/dtheta = 1


def test_the_file_of_pchip_maximise_is_the_one_it_wrote_before_the_split(tmp_path):
    """tests/golden/maximise_host_d4.maximum is what pchip_maximise wrote for this live set (the one above, with the mean) when it was still
    one function with its own writer.  Every label, blank line and field width byte for byte; every number to a relative 1e-13.  On the
    machine that made the golden the new file is the same bytes; the numbers are not held to their last printed digit because dXdtheta is
    D log(dx) - log(det), a difference of two values near 46 whose rounding -- one ulp of the C library's log, which its builds for
    different CPUs do not share -- is 7e-15 in a max_post of 5.5 printed to fifteen digits."""
    import pathlib
    import re
    api, lib = _api()
    D, nDer, n = 4, 1, 60
    like, prior = _host_fns(lib, D)
    live = _gauss_rows(0.5 + 0.03 * np.random.default_rng(5).standard_normal((n, D)), nDer)
    cl = np.zeros(n, dtype=np.int32)
    mean = np.array([0.5, 0.5, 0.5, 0.5, 0.0])
    f = lib.pchip_maximise
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.c_char_p]
    out = tmp_path / "now.maximum"
    assert f(like, prior, D, nDer, -1e30, api.dptr(live), cl.ctypes.data_as(C.POINTER(C.c_int)), n, api.dptr(mean), str(out).encode()) == 0
    want = (pathlib.Path(__file__).parent / "golden" / "maximise_host_d4.maximum").read_text().split("\n")
    got = out.read_text().split("\n")
    assert len(got) == len(want) == 17
    numbers = 0
    for g, w in zip(got, want):
        if w.endswith(":") or not w:
            assert g == w
            continue
        assert len(g) == len(w) and re.sub(r"\S+", "#", g) == re.sub(r"\S+", "#", w)      # the same columns
        for a, b in zip(map(float, g.split()), map(float, w.split())):
            assert abs(a - b) <= 1e-13 * abs(b), (g, w)
            numbers += 1
    assert numbers == 4 + 3 * (D + nDer)


def test_a_refusal_leaves_a_result_that_can_be_freed():
    """the documented use is `pchip_maximum m; door(..., &m); pchip_maximum_free(&m);` whatever the door returns: every refusal (null
    arguments, a callback likelihood, nDims < 1, nDims > 64), of the door and of the _many door, zeroes the structs it was given first"""
    api, lib = _api()
    D = 3
    rows = _gauss_rows(np.full((8, D), 0.5), 0)
    cl = np.zeros(8, dtype=np.int32)
    clp = cl.ctypes.data_as(C.POINTER(C.c_int))

    def garbage(k):
        ms = (api.Maximum * k)()
        C.memset(ms, 0x5a, C.sizeof(ms))
        return ms

    def empty(ms):
        return bytes(ms) == bytes(C.sizeof(ms))

    raw = C.CDLL(lib._name)                       # a handle of its own: the prototypes set here stay here
    dev = raw.pchip_maximise_device
    dev.restype = C.c_int
    dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.c_long, C.c_void_p]
    many = raw.pchip_maximise_device_many
    many.restype = C.c_int
    many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    cb = api.LOGLIKE_FN(lambda th, n, phi, nd: 0.0)
    cases = []
    for what in ("null settings", "callback", "nDims 0", "nDims 65"):
        d = {"nDims 0": 0, "nDims 65": 65}.get(what, D)
        s = api.Settings(); lib.pchip_settings_default(C.byref(s), max(d, 1), 0)
        s.nDims = d
        L, P, keep = api.make_problem("gaussian", D)
        if what == "callback":
            L.kind, L.fn = api.LIKE_CALLBACK, C.cast(cb, C.c_void_p)
        cases.append((what, None if what == "null settings" else C.addressof(s), L, P, 3 if what == "nDims 65" else 1, (s, keep)))
    for what, sp, L, P, code, keep in cases:
        m = garbage(1)
        assert dev(sp, C.addressof(L), C.addressof(P), api.dptr(rows), clp, 8, None, 0, C.addressof(m)) == code, what
        assert empty(m), what
        lib.pchip_maximum_free(C.byref(m[0]))
        runs = (api.Result * 2)()
        for r in runs:
            r.live, r.live_cluster, r.nlive_final = api.dptr(rows), clp, 8
        m = garbage(2)
        assert many(sp, C.addressof(L), C.addressof(P), 2, C.addressof(runs), 0, C.addressof(m)) == code, what
        assert empty(m), what
        for k in range(2):
            lib.pchip_maximum_free(C.byref(m[k]))
    m = garbage(2)
    assert many(None, None, None, 2, None, 0, C.addressof(m)) == 1 and empty(m)


def test_the_better_peaked_cluster_is_chosen_and_a_small_one_skipped():
    """two clusters around the peak: cluster 0 holds the single best row but fewer than D + 1 rows (skipped); of the two eligible ones
    cluster 2 lies nearer the peak than cluster 1 and wins both legs"""
    api, lib = _api()
    D, nDer = 3, 0
    like, prior = _host_fns(lib, D)
    rng = np.random.default_rng(11)
    c0 = 0.5 + 0.001 * rng.standard_normal((D, D))                  # D rows: one short of a simplex
    c1 = 0.56 + 0.01 * rng.standard_normal((12, D))
    c2 = 0.52 + 0.01 * rng.standard_normal((9, D))
    live = _gauss_rows(np.vstack([c0, c1, c2]), nDer)
    cl = np.array([0] * D + [1] * 12 + [2] * 9, dtype=np.int32)
    assert live[:D, -1].max() > live[D:, -1].max()
    m = api.maximise_values(like, prior, D, nDer, -1e30, live, cl)
    assert m["status"] == [0, 0] and m["cluster"] == [2, 2]
    assert np.all(np.abs(m["max_point"] - 0.5) < 2e-3)
    # ... in index order a later cluster must be STRICTLY better: the same rows twice, the first copy is taken
    live2 = np.vstack([live[D:D + 12], live[D:D + 12]])
    m2 = api.maximise_values(like, prior, D, nDer, -1e30, live2, np.array([0] * 12 + [1] * 12, dtype=np.int32))
    assert m2["cluster"] == [0, 0]


def test_no_eligible_cluster_is_status_one():
    api, lib = _api()
    D = 3
    like, prior = _host_fns(lib, D)
    rng = np.random.default_rng(2)
    live = _gauss_rows(0.5 + 0.01 * rng.standard_normal((6, D)), 0)
    m = api.maximise_values(like, prior, D, 0, -1e30, live, np.array([0, 0, 0, 1, 1, 1], dtype=np.int32))      # two clusters of D rows
    assert m["status"] == [1, 1] and m["cluster"] == [-1, -1] and m["niter"] == [0, 0] and m["neval"] == [0, 0]
    # rows at logzero build no simplex either
    live[:, -1] = -1e30
    m = api.maximise_values(like, prior, D, 0, -1e30, live, np.zeros(6, dtype=np.int32))
    assert m["status"] == [1, 1]
    # ... and such a result has no file
    mx = api.Maximum()
    assert lib.pchip_maximise_values(like, prior, D, 0, -1e30, api.dptr(live), np.zeros(6, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int)), 6, None, C.byref(mx)) == 1
    assert lib.pchip_maximum_write(C.byref(mx), D, 0, b"/nonexistent-dir/x.maximum") == 1
    lib.pchip_maximum_free(C.byref(mx))


def test_the_device_door_refuses_host_callbacks_before_any_device_call():
    """a callback likelihood or a callback prior has no device code: code 1 and a message, on a machine without a device too (a device call
    would have answered 2)"""
    api, lib = _api()
    D = 3
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, 0)
    rng = np.random.default_rng(3)
    run = dict(live=_gauss_rows(0.5 + 0.01 * rng.standard_normal((8, D)), 0), live_cluster=np.zeros(8, dtype=np.int32), post_mean=None)
    L, P, keep = api.make_problem("gaussian", D)
    cb = api.LOGLIKE_FN(lambda th, n, phi, nd: 0.0)
    L.kind, L.fn = api.LIKE_CALLBACK, C.cast(cb, C.c_void_p)
    with pytest.raises(RuntimeError) as e:
        api.maximise_device(s, L, P, run)
    assert "code 1" in str(e.value) and "callback" in str(e.value)
    L, P, keep = api.make_problem("gaussian", D)
    P.kind = api.PRIOR_CALLBACK
    with pytest.raises(RuntimeError) as e:
        api.maximise_device(s, L, P, run)
    assert "code 1" in str(e.value) and "callback" in str(e.value)
    # nDims > 64: code 3, the host maximiser remains
    D = 65
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, 0)
    L, P, keep = api.make_problem("gaussian", D)
    run = dict(live=_gauss_rows(np.full((70, D), 0.5), 0), live_cluster=np.zeros(70, dtype=np.int32), post_mean=None)
    with pytest.raises(RuntimeError) as e:
        api.maximise_device(s, L, P, run)
    assert "code 3" in str(e.value) and "64" in str(e.value)
