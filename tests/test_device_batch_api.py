"""CPU: the surface of the device batch callback -- the setter's symbol and its declarations in the three bindings, DeviceBlock's
`__cuda_array_interface__`, and the pairing rule of `device_batch` callables, which is checked before anything is loaded."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_setter_is_exported_and_declared():
    from polychordlite_amd import _ctypes_api as api
    lib = api.load()
    assert hasattr(lib, "polychord_hip_set_device_batch_callback") and hasattr(lib, "pchip_park_pack")
    h = _read("include", "polychord_hip.h")
    m = re.search(r"typedef int \(\*polychord_device_batch_fn\)\((.*?)\);", h, flags=re.S)
    args = [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]
    assert len(args) == 10 and args[0] == "void *user" and args[-2] == "int flags" and args[-1] == "void *stream"
    assert re.search(r"^void polychord_hip_set_device_batch_callback\(polychord_device_batch_fn fn, void \*user\);", h, flags=re.M)
    assert "PCHIP_PATH_DEVICE_BATCH = 23" in h and "PCHIP_PATH_COUNT = 24" in h and "#define PCHIP_ABI_VERSION 9" in h
    assert "polychord_hip_set_device_batch_callback(fn, user)" in _read("include", "polychord_hip.hpp")
    f90 = _read("bindings", "fortran", "polychord_hip.f90")
    assert 'bind(c, name="polychord_hip_set_device_batch_callback")' in f90
    assert re.search(r"public ::.*?polychord_hip_set_device_batch_callback", f90, flags=re.S)
    # the ctypes mirror: the path counter's name at its index, the callback's ten arguments
    assert api.PATH_DEVICE_BATCH == 23 and "device_batch" not in api.PATH_NAMES and C.sizeof(api.Result().path) == 24 * C.sizeof(C.c_long)
    assert len(api.DEVICE_BATCH_FN._argtypes_) == 10 and api.DEVICE_BATCH_FN._restype_ is C.c_int
    # no struct changed
    assert lib.pchip_sizeof(b"prior") == 48 == C.sizeof(api.Prior)


def test_registration_is_sticky_and_null_removes_it():
    from polychordlite_amd import _ctypes_api as api
    lib = api.load()
    lib.pc_device_batch_registered.restype = C.c_int
    assert lib.pc_device_batch_registered() == 0
    cb = api.set_device_batch_callback(lambda *a: 0)
    try:
        assert isinstance(cb, api.DEVICE_BATCH_FN) and lib.pc_device_batch_registered() == 1
    finally:
        assert api.set_device_batch_callback(None) is None
    assert lib.pc_device_batch_registered() == 0


def test_device_block_interface():
    from polychordlite_amd._ctypes_api import DeviceBlock
    b = DeviceBlock(0x7F0000001000, (5, 3), stream=0xABC0)
    i = b.__cuda_array_interface__
    assert set(i) == {"shape", "typestr", "data", "version", "strides", "stream"}
    assert i["shape"] == (5, 3) and i["typestr"] == "<f8" and i["version"] == 3 and i["data"] == (0x7F0000001000, False)
    assert i["strides"] is None                                # dense, row-major: the interface's word for C-contiguous
    assert i["stream"] == 0xABC0 and b.ptr == 0x7F0000001000
    v = DeviceBlock(C.c_void_p(4096).value, [7]).__cuda_array_interface__
    assert v["shape"] == (7,) and "stream" not in v            # (0 is no stream in version 3: the key is left out)


def test_host_prior_under_a_device_likelihood_is_refused_before_the_library(tmp_path, monkeypatch):
    from polychordlite_amd import _ctypes_api as api
    from polychordlite_amd.pypolychord import device_likelihoods as dl
    from polychordlite_amd.pypolychord import polychord as pc

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(api, "load", touched)
    monkeypatch.setattr(pc._pypolychord, "run", touched)

    def like(theta):
        return theta.sum(dim=1)
    like.device_batch = True

    def host_prior(cube):
        return cube
    for run in (lambda: pc.run(like, 3, prior=host_prior, base_dir=str(tmp_path / "a")),
                lambda: pc.run(like, 3, base_dir=str(tmp_path / "b")),
                lambda: pc.run_polychord(like, 3, 0, pc.PolyChordSettings(3, 0, base_dir=str(tmp_path / "c")), host_prior)):
        with pytest.raises(ValueError) as e:
            run()
        assert "UniformPrior / TablePrior" in str(e.value) and "prior.device_batch = True" in str(e.value)
    assert not any((tmp_path / d).exists() for d in "abc")     # ... and before a directory was made

    def dev_prior(cube):
        return cube
    dev_prior.device_batch = True
    with pytest.raises(ValueError, match="loglikelihood.device_batch = True"):
        pc.run(lambda theta: 0.0, 3, prior=dev_prior, base_dir=str(tmp_path / "d"))
    # the two pairings that exist pass the check
    assert pc._device_batch_pair(like, dl.UniformPrior(0.0, 1.0)) and pc._device_batch_pair(like, dev_prior)
    assert pc._device_batch_pair(like, dl.TablePrior([("uniform", [0, 1])] * 3)) and not pc._device_batch_pair(host_prior, host_prior)
