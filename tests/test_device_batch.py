"""The device batch callback (polychord_hip_set_device_batch_callback): the parked proposals of a round as one dense block in device memory.

The reference in every comparison is the same functions behind the HOST batch callback: the proposals come from the same kernels, the live
points from the same Philox coordinates, the answers are the same bits -- so the two runs agree in every counter, in log Z and in every dead
row, or something between the pack and the next tick is out of order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NDER = 6, 1
H2D, D2H = 1, 2
COUNTERS = ("logZ", "varlogZ", "ndead", "nlike", "niter", "nbatches", "nrounds", "nupdates", "ncluster", "ncluster_dead", "nlike_failed")
HOST_BATCH_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                            C.POINTER(C.c_double))


# ---- the numpy functions of test_vectorised_and_farmed_likelihoods (the sums taken column by column: one order whatever the block) ----
def np_prior(cube):
    return -1.0 + 2.0 * cube


def _r2(z):
    s = np.zeros(z.shape[0])
    for d in range(z.shape[1]):
        s = s + z[:, d] * z[:, d]
    return s


def np_gauss(theta):
    r2 = _r2(theta)
    return -np.log(2 * np.pi * 0.01) * theta.shape[1] / 2.0 - r2 / 0.02, r2[:, None]


def np_twin(theta):
    """two Gaussians of width 0.08 at -+0.5 along the first coordinate: two clusters"""
    a = theta.copy(); a[:, 0] -= 0.5
    b = theta.copy(); b[:, 0] += 0.5
    la, lb = -_r2(a) / (2 * 0.08 ** 2), -_r2(b) / (2 * 0.08 ** 2)
    return np.logaddexp(la, lb), (theta[:, 0] > 0).astype(float)[:, None]


def _settings(api, lib, batch, clustering=False, max_ndead=-1, seed=7):
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, NDER)
    s.nlive, s.num_repeats, s.seed, s.batch, s.do_clustering, s.max_ndead = 80, 8, seed, batch, int(clustering), max_ndead
    return s


def _scalars(api, like, prior):
    """the scalar callbacks a run still needs, from the block functions"""
    def fl(theta_p, nd, phi_p, nder):
        logL, phi = like(np.ctypeslib.as_array(theta_p, shape=(nd,))[None, :].copy())
        if nder > 0:
            np.ctypeslib.as_array(phi_p, shape=(nder,))[:] = phi[0]
        return float(logL[0])

    def fp(cube_p, theta_p, nd):
        np.ctypeslib.as_array(theta_p, shape=(nd,))[:] = prior(np.ctypeslib.as_array(cube_p, shape=(nd,)).copy())
    return api.LOGLIKE_FN(fl), api.PRIOR_FN(fp)


def _problem(api, like_fn, prior_fn=None, kind=0, **pk):
    L = api.Like(); L.kind = api.LIKE_CALLBACK; L.fn = C.cast(like_fn, C.c_void_p)
    P = api.Prior(); P.kind = kind
    if prior_fn is not None:
        P.fn = C.cast(prior_fn, C.c_void_p)
    for k, v in pk.items():
        setattr(P, k, v)
    return L, P


def _host_cb(like, prior, calls):
    def cb(_user, n, nd, nder, cube_p, theta_p, phi_p, logL_p):
        calls.append(n)
        theta = prior(np.ctypeslib.as_array(cube_p, shape=(n, nd)).copy())
        logL, phi = like(theta)
        np.ctypeslib.as_array(theta_p, shape=(n, nd))[:] = theta
        np.ctypeslib.as_array(phi_p, shape=(n, max(1, nder)))[:, :nder] = phi
        np.ctypeslib.as_array(logL_p, shape=(n,))[:] = logL
    return HOST_BATCH_FN(cb)


def _hip():
    from polychordlite_amd import merge
    hip = merge.hip_runtime()
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.restype = C.c_int
    return hip


def _down(hip, ptr, shape):
    a = np.empty(shape)
    assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes, D2H) == 0
    return a


def _up(hip, ptr, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert hip.hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0


def _device_cb(api, like, prior, calls, rc=0, want_flags=0, seen=None):
    """a device callback in Python: waits for the engine's stream (its copies are blocking, on no stream), brings the cubes -- or, behind the
    engine's prior, the thetas -- down with the library's runtime, evaluates the numpy functions, puts the answers back"""
    hip = _hip()

    def cb(_user, n, nd, nder, cube_p, theta_p, phi_p, logL_p, flags, stream):
        try:
            calls.append(n)
            if seen is not None:
                seen.append(flags)
            assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
            if flags & 1:
                theta = _down(hip, theta_p, (n, nd))
            else:
                theta = prior(_down(hip, cube_p, (n, nd)))
                _up(hip, theta_p, theta)
            logL, phi = like(theta)
            if nder > 0:
                _up(hip, phi_p, phi)
            _up(hip, logL_p, logL)
            return rc if flags == want_flags else 3
        except BaseException:       # noqa: BLE001 -- nothing may cross the C frames: the run ends and the test sees it
            return 4
    return api.DEVICE_BATCH_FN(cb)


def _blocks(lib):
    d, p = C.c_long(), C.c_long()
    lib.pchip_blocks_in_use(C.byref(d), C.byref(p))
    return d.value, p.value


def _run(api, s, L, P):
    """api.run with the result's arrays copied and its pinned blocks given back: pchip_blocks_in_use then counts what a RUN left behind"""
    import gc
    r = api.run(s, L, P)
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items() if k != "_owner"}
    del r
    gc.collect()
    return out


def _same_run(a, b):
    for k in COUNTERS:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ("dead", "logweights", "entry", "live"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _pair(api, lib, like, prior, s):
    """the run through the host batch callback and the run through the device callback, of the same functions"""
    fl, fp = _scalars(api, like, prior)
    L, P = _problem(api, fl, fp)
    hcalls, dcalls = [], []
    hcb = _host_cb(like, prior, hcalls)
    lib.polychord_hip_set_batch_callback.argtypes = [C.c_void_p, C.c_void_p]
    lib.polychord_hip_set_batch_callback(C.cast(hcb, C.c_void_p), None)
    before = _blocks(lib)
    try:
        host = _run(api, s, L, P)
        assert _blocks(lib) == before
        api.set_device_batch_callback(_device_cb(api, like, prior, dcalls))       # both registered: the device one wins
        try:
            dev = _run(api, s, L, P)
        finally:
            api.set_device_batch_callback(None)
        assert _blocks(lib) == before
    finally:
        lib.polychord_hip_set_batch_callback(None, None)
    assert host["path"]["device_batch"] == 0 and dev["path"]["device_batch"] == len(dcalls) > 0
    assert dcalls == hcalls                                     # the same blocks, round for round
    _same_run(host, dev)
    return host, dev


# ---- 1. the same run, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("batch", [32, 1, 65])
def test_device_callback_run_is_the_host_batch_run(engine, batch):
    """nDims 6, nDerived 1, nlive 80, num_repeats 8, one cluster, to the end of the run (batch 1: one proposal a round, tens of thousands of
    Python calls to the end -- held to the first 400 dead points, for the suite's sake; the rounds are the same rounds)"""
    lib = engine.load()
    host, dev = _pair(engine, lib, np_gauss, np_prior, _settings(engine, lib, batch, max_ndead=400 if batch == 1 else -1))
    assert dev["ndead"] >= 400 and dev["batch"] == batch


@pytest.mark.gpu
def test_device_callback_run_with_clustering(engine):
    """a twin Gaussian under do_clustering: clusters split, chains of a nursery in flight are lost mid-round, the blocks shrink and grow"""
    lib = engine.load()
    host, dev = _pair(engine, lib, np_twin, np_prior, _settings(engine, lib, 32, clustering=True))
    assert dev["ncluster_peak"] >= 2


# ---- 2. nothing leaves the device -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss_so(tmp_path_factory):
    """tools/dev/device_batch_gauss.hip as a shared object: a device callback that launches one kernel on the engine's stream and does not
    wait, and its host twin -- one formula, contraction off on both sides.  A missing hipcc fails the test, it does not skip it"""
    so = tmp_path_factory.mktemp("dbgauss") / "libdbgauss.so"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(ROOT, "tools", "dev", "device_batch_gauss.hip"), "-o", str(so)])
    g = C.CDLL(str(so))
    g.gauss_set_scalar.argtypes = [C.c_double, C.c_double, C.c_double]
    return g


class GaussCtx(C.Structure):
    _fields_ = [("mu", C.c_double), ("sigma", C.c_double), ("c", C.c_double), ("inner", C.c_int), ("calls", C.c_int)]


@pytest.mark.gpu
def test_kernel_likelihood_never_synchronises(engine, gauss_so):
    """the stream contract: the callback enqueues its kernel behind the pack and returns; the next tick reads the answers in stream order"""
    lib = engine.load()
    c0 = -D * (np.log(0.1) + 0.5 * np.log(2 * np.pi))
    gauss_so.gauss_set_scalar(0.5, 0.1, c0)
    L, P = _problem(engine, gauss_so.gauss_loglike, gauss_so.gauss_prior)
    s = _settings(engine, lib, 32)
    lib.polychord_hip_set_batch_callback.argtypes = [C.c_void_p, C.c_void_p]
    lib.polychord_hip_set_device_batch_callback.argtypes = [C.c_void_p, C.c_void_p]
    hctx, dctx = GaussCtx(0.5, 0.1, c0, 0, 0), GaussCtx(0.5, 0.1, c0, 0, 0)
    lib.polychord_hip_set_batch_callback(C.cast(gauss_so.gauss_host_batch, C.c_void_p), C.byref(hctx))
    try:
        host = _run(engine, s, L, P)
    finally:
        lib.polychord_hip_set_batch_callback(None, None)
    before = _blocks(lib)
    lib.polychord_hip_set_device_batch_callback(C.cast(gauss_so.gauss_device_batch, C.c_void_p), C.byref(dctx))
    try:
        dev = _run(engine, s, L, P)
    finally:
        lib.polychord_hip_set_device_batch_callback(None, None)
    assert _blocks(lib) == before
    assert dctx.calls == hctx.calls == dev["path"]["device_batch"] > 100 and host["path"]["device_batch"] == 0
    _same_run(host, dev)
    # the kernel's values are the formula's: logL of every dead row from its theta, the derived parameter the sum
    th = dev["dead"][:, D:2 * D]
    z = (th - 0.5) / 0.1
    assert np.array_equal(dev["dead"][:, 2 * D], _r2(z)) and np.array_equal(dev["dead"][:, -1], -0.5 * _r2(z) + c0)
    assert np.array_equal(th, dev["dead"][:, :D])              # the callback's own prior: the unit box


# ---- 3. the engine's prior on the block (flags bit 0) ------------------------------------------------------------------------------
TABLE = [("gaussian", [0.0, 0.4])] * 3 + [("sorted_uniform", 1, [-1.0, 1.0])] * 3
LO, HI = np.array([-1.0, -0.5, 0.0, -2.0, -1.0, 0.25]), np.array([1.0, 0.5, 3.0, 1.0, 1.5, 0.75])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["box", "table"])
def test_engine_prior_fills_theta_on_the_device(engine, which):
    lib = engine.load()

    def like(theta):
        r2 = _r2(theta)
        return -r2 / 0.5, r2[:, None]
    fl, fp = _scalars(engine, like, lambda c: c)
    if which == "box":
        lo, hi = LO.copy(), HI.copy()
        L, P = _problem(engine, fl, None, kind=engine.PRIOR_BOX, lo=engine.dptr(lo), hi=engine.dptr(hi))
        entries = [("uniform", [float(a), float(b)]) for a, b in zip(LO, HI)]       # the same box as a table: the device's box transform
    else:
        entries = TABLE
        arr, _ = engine.prior_table(entries)
        L, P = _problem(engine, fl, None, kind=engine.PRIOR_TABLE, table=arr)
    calls, seen = [], []
    before = _blocks(lib)
    engine.set_device_batch_callback(_device_cb(engine, like, None, calls, want_flags=1, seen=seen))      # (prior None: calling it would fail the run)
    try:
        r = _run(engine, _settings(engine, lib, 32), L, P)
    finally:
        engine.set_device_batch_callback(None)
    assert _blocks(lib) == before
    assert len(calls) > 100 and set(seen) == {1} and r["path"]["device_batch"] == len(calls)
    cube, theta = np.ascontiguousarray(r["dead"][:, :D]), r["dead"][:, D:2 * D]
    assert np.array_equal(np.ascontiguousarray(theta).view(np.uint64), engine.prior_transform(entries, cube).view(np.uint64))
    logL, phi = like(np.ascontiguousarray(theta))
    assert np.array_equal(r["dead"][:, -1], logL) and np.array_equal(r["dead"][:, 2 * D], phi[:, 0])


# ---- 4. refusals and endings -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_endings(engine, capfd):
    lib = engine.load()
    fl, fp = _scalars(engine, np_gauss, np_prior)
    s = _settings(engine, lib, 32)
    L, P = _problem(engine, fl, fp)
    lib.polychord_hip_set_batch_callback.argtypes = [C.c_void_p, C.c_void_p]
    hcb = _host_cb(np_gauss, np_prior, [])
    lib.polychord_hip_set_batch_callback(C.cast(hcb, C.c_void_p), None)
    try:
        first = _run(engine, s, L, P)
        before = _blocks(lib)
        # a source prior with a callback likelihood: refused as ever, with its message
        L3, P3 = _problem(engine, fl, fp, kind=engine.PRIOR_SOURCE)
        calls = []
        engine.set_device_batch_callback(_device_cb(engine, np_gauss, np_prior, calls))
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            _run(engine, s, L3, P3)
        assert "prior.kind = 3 (source prior) needs a device source likelihood of the same handle" in capfd.readouterr().err
        assert calls == [] and _blocks(lib) == before
        # a callback that returns non-zero ends the run by the stop path: among the live points, and in the middle of a nursery
        for after in (0, 40):
            calls = []
            inner = _device_cb(engine, np_gauss, np_prior, calls)
            ender = engine.DEVICE_BATCH_FN(lambda *a: 1 if len(calls) >= after else inner(*a))
            engine.set_device_batch_callback(ender)
            with pytest.raises(RuntimeError, match="code 5"):
                _run(engine, s, L, P)
            assert len(calls) == after and _blocks(lib) == before
        # NULL gives the host path back: the run from before the registration
        engine.set_device_batch_callback(None)
        again = _run(engine, s, L, P)
        assert again["path"]["device_batch"] == 0
        _same_run(first, again)
    finally:
        engine.set_device_batch_callback(None)
        lib.polychord_hip_set_batch_callback(None, None)


# ---- 5. torch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_torch_likelihood_on_the_library_blocks(engine, tmp_path, monkeypatch):
    """pypolychord.run with a `device_batch` Gaussian in torch under UniformPrior: the callable sees the library's own theta block as a float64
    tensor on the device.  torch reduces in another order than numpy, so log Z is held against the numpy `vectorised` run of the same
    settings statistically: within 5 times the two reported errors in quadrature (the run's own error is the measured scatter of one-cluster
    runs -- README: 0.092 against 0.092 --; five and not three because this is one fixed seed, not a distribution)."""
    import torch
    from polychordlite_amd import pypolychord
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    from polychordlite_amd.pypolychord import polychord as pc
    lib = engine.load()
    kw = dict(nDerived=1, nlive=80, num_repeats=8, seed=7, do_clustering=False, read_resume=False, write_resume=False, write_dead=False,
              write_live=False, write_stats=True, posteriors=False, equals=False, write_prior=False, feedback=0)
    seen, handed = [], []

    def t_like(theta):
        seen.append((theta.is_cuda, theta.dtype, tuple(theta.shape), theta.data_ptr()))
        r2 = (theta * theta).sum(dim=1)
        return -np.log(2 * np.pi * 0.01) * theta.shape[1] / 2.0 - r2 / 0.02, r2[:, None]
    t_like.device_batch = True

    def v_like(theta):
        return np_gauss(theta)
    v_like.vectorised = True
    orig = pc._DeviceBatchEvaluator

    class Spy(orig):
        def evaluate(self, n, nd, nder, cube_p, theta_p, phi_p, logL_p, flags, stream):
            handed.append((theta_p, flags, n))
            return super().evaluate(n, nd, nder, cube_p, theta_p, phi_p, logL_p, flags, stream)
    monkeypatch.setattr(pc, "_DeviceBatchEvaluator", Spy)
    before = _blocks(lib)
    try:
        pypolychord.run(t_like, D, prior=dl.UniformPrior(-1.0, 1.0), base_dir=str(tmp_path), file_root="torch", **kw)
    except RuntimeError as e:
        if "torch and libpolychord_hip do not share a HIP runtime" in str(e):
            pytest.skip(str(e))
        raise
    assert _blocks(lib) == before
    assert len(seen) > 100 and len(seen) == len(handed)
    assert all(c and t == torch.float64 and sh[1] == D for c, t, sh, _ in seen) and max(sh[0] for _, _, sh, _ in seen) > 8
    assert all(p == h[0] and h[1] == 1 and sh[0] == h[2] for (_, _, sh, p), h in zip(seen, handed))      # the library's own block, no copy
    pypolychord.run(v_like, D, prior=dl.UniformPrior(-1.0, 1.0), base_dir=str(tmp_path), file_root="numpy", **kw)

    def logz(root):
        import re
        m = re.search(r"^log\(Z\)\s*=\s*(\S+)\s*\+/-\s*(\S+)", open(tmp_path / (root + ".stats")).read(), flags=re.M)
        return float(m.group(1)), float(m.group(2))
    (zt, et), (zn, en) = logz("torch"), logz("numpy")
    print(f"torch logZ = {zt} +- {et}; numpy logZ = {zn} +- {en}")
    assert et > 0 and en > 0 and abs(zt - zn) < 5.0 * np.hypot(et, en)

    def bad(theta):
        raise KeyError("device boom")
    bad.device_batch = True
    with pytest.raises(KeyError):
        pypolychord.run(bad, D, prior=dl.UniformPrior(-1.0, 1.0), base_dir=str(tmp_path), file_root="bad", **dict(kw, nDerived=0))
    assert _blocks(lib) == before
