#!/usr/bin/env python3
"""Registers of the run-time kernels of a device source, without a device: composes the unit pc_rtc.hip's kernel_unit() composes for a
handle (the form's #defines, pc_sample.hip with pc_seed.h and pc_slice_body.inc from the library's embedded text -- the evaluation kernels;
the direction kernels of pc_bases.hip are no part of it --, the user's text behind its -D options), compiles it with
hiprtc for gfx950 and prints, per kernel, what the code object's metadata note says: VGPRs, AGPRs, spilled vector and scalar registers,
scratch bytes a lane.

    python tools/dev/rtc_registers.py            # the shared-values fixture of tests/test_source_shared.py, with and without shared values

The #define lines below mirror kernel_unit() (polychordlite_amd/csrc/pc_rtc.hip): keep them in step with it."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from polychordlite_amd import _ctypes_api as api      # noqa: E402

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
KERNELS = ["k_slice<1, 1, false>", "k_slice<1, 1, false, 1, 0, 0, 1>", "k_source_eval<1>"]


def unit(nterms, nsums=0, quad=False, nshared=0):
    u = ""
    if nsums:
        u += f"#define PCHIP_USER_SUMS 1\n#define PCHIP_SRC_NSUMS {nsums}\n"
    if quad:
        u += "#define PCHIP_USER_QUAD 1\n"
    if nshared:
        u += f"#define PCHIP_USER_SHARED 1\n#define PCHIP_SRC_NSHARED {nshared}\n"
    return u + f'#define PCHIP_USER_SOURCE 1\n#define PCHIP_USER_TERMS 1\n#define PCHIP_SRC_NTERMS {nterms}L\n#include "pc_sample.hip"\n#include "pchip_user_source.h"\n'


def user_text(source, options):
    defs = ""
    for o in options:
        name, _, val = o[2:].partition("=")
        defs += f"#define {name} {val or 1}\n"
    return defs + "#line 1\n" + source


def compile_unit(unit_text, user, kernels, arch="gfx950"):
    lib, rtc = api.load(), C.CDLL("libhiprtc.so")
    names, texts, i = [], [], 0
    while True:
        name = C.c_char_p()
        t = lib.pchip_rtc_embedded_source(i, C.byref(name))
        if t is None:
            break
        names.append(name.value); texts.append(t); i += 1
    names.append(b"pchip_user_source.h"); texts.append(user.encode())
    prog = C.c_void_p()
    n = len(names)
    assert rtc.hiprtcCreateProgram(C.byref(prog), unit_text.encode(), b"pchip_rtc_unit.hip", n, (C.c_char_p * n)(*texts), (C.c_char_p * n)(*names)) == 0
    for k in kernels:
        rtc.hiprtcAddNameExpression(prog, k.encode())
    opts = [f"--offload-arch={arch}".encode(), b"-O3", b"-std=c++17", b"-Wno-unused-value"]          # (compile()'s options)
    rc = rtc.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*opts))
    if rc != 0:
        sz = C.c_size_t(); rtc.hiprtcGetProgramLogSize(prog, C.byref(sz))
        log = C.create_string_buffer(sz.value + 1); rtc.hiprtcGetProgramLog(prog, log)
        raise RuntimeError(log.value.decode(errors="replace"))
    lowered = {}
    for k in kernels:
        ln = C.c_char_p(); rtc.hiprtcGetLoweredName(prog, k.encode(), C.byref(ln)); lowered[ln.value.decode()] = k
    sz = C.c_size_t(); rtc.hiprtcGetCodeSize(prog, C.byref(sz))
    code = C.create_string_buffer(sz.value); rtc.hiprtcGetCode(prog, code)
    rtc.hiprtcDestroyProgram(C.byref(prog))
    return code.raw, lowered


def registers(code, lowered):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code); f.flush()
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], text=True)
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        get = lambda key: int(re.search(r"\." + key + r":\s*(\d+)", block).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", block).group(1)
        if name in lowered:
            out[lowered[name]] = dict(vgpr=get("vgpr_count"), agpr=get("agpr_count"), vgpr_spill=get("vgpr_spill_count"),
                                      sgpr_spill=get("sgpr_spill_count"), scratch=get("private_segment_fixed_size"))
    return out


# the line of tests/test_source_quad.py with its two coefficients as shared values: the smallest text that uses the machinery
LINE_SHARED = r"""
#pragma clang fp contract(off)
__device__ double pchip_shared_value(const double *theta, int nDims, const double *data, long ndata, long k) { return theta[k]; }
__device__ double pchip_residual(const double *theta, const double *shared, int nDims, const double *data, long ndata, long i)
{
    return data[NRES + i] - (shared[0] + shared[1] * data[i]);
}
__device__ double pchip_logl_finish(double chi2, const double *theta, const double *shared, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    if (nDerived > 0) phi[0] = chi2;
    if (nDerived > 1) phi[1] = data[NRES] - (shared[0] + shared[1] * data[0]);
    for (int e = 2; e < nDerived; ++e) phi[e] = 0.0;
    return -chi2 / 2.0;
}
"""


def report(label, u, user):
    code, lowered = compile_unit(u, user, KERNELS)
    for k, r in registers(code, lowered).items():
        print(f"{label:28s} {k:34s} VGPRs {r['vgpr']:3d}  AGPRs {r['agpr']:3d}  spilled VGPRs {r['vgpr_spill']:3d}  "
              f"spilled SGPRs {r['sgpr_spill']:3d}  scratch {r['scratch']:4d} B", flush=True)


def main():
    from tests.test_source_shared import GRID, OLD_SIGNATURES, _options
    from tests.test_source_quad import QUAD
    nsh, n = 130, 256
    # GRID serves both sides: with the signatures without `shared` it is a terms / quad source as it stands (the block behind theta is
    # then whatever follows theta -- nothing is run here)
    for form in ("terms", "quad"):
        for shared in (nsh, 0):
            report(f"GRID {form} nshared {shared}", unit(n, quad=form == "quad", nshared=shared), user_text(GRID + OLD_SIGNATURES, _options(form, nsh, n)))
    report("line quad nshared 2", unit(n, quad=True, nshared=2), user_text(LINE_SHARED, [f"-DNRES={n}"]))
    report("line quad nshared 0", unit(n, quad=True), user_text(QUAD, [f"-DNRES={n}"]))


if __name__ == "__main__":
    main()
