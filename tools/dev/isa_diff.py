#!/usr/bin/env python3
"""Compare the gfx950 instruction text of the kernels two builds of an object file have in common.

    python3 tools/dev/isa_diff.py OLD.o NEW.o [NEW2.o ...] [--arch gfx950] [--drop-trailing-zero NAME ...]

Unbundles the device code object of the files, disassembles them, and compares kernel by kernel (demangled names) the instruction
text with addresses and encodings removed.  Several NEW objects -- a translation unit that was split -- count as the union of their
kernels, so that "only in OLD" means a kernel was lost, not that it moved; a name that occurs in two of them is an error.
A template that gained a defaulted trailing parameter keeps its instruction stream but not
its name: `--drop-trailing-zero k_slice` compares NEW's `k_slice<..., 0>` with OLD's `k_slice<...>`.  Prints one line per kernel that
differs or exists on one side only, then a summary; exit status 1 if a common kernel differs.

Two things that change when a function gets other neighbours in its object are layout, not instructions, and are taken out of both sides
before the comparison (normalise_layout):
  * the run of `s_nop`s behind a function's LAST `s_endpgm` (with no `s_endpgm`, the trailing run): padding up to the alignment of whatever
    follows.  An `s_nop` inside the body, or behind an `s_endpgm` that is not the last, is an instruction and stays.
  * the literal of an `s_add_u32` (and of the `s_addc_u32` behind it) that directly follows an `s_getpc_b64` naming the same register pair:
    the pc-relative distance to a constant or a function, which is where the linker put it.  Any other literal stays.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def disassemble(obj, arch, tmp):
    stem = os.path.join(tmp, os.path.basename(obj) + "." + str(len(os.listdir(tmp))))
    fat, co = stem + ".fatbin", stem + ".co"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.devnull])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat, "--output=" + co,
                           "--targets=hipv4-amdgcn-amd-amdhsa--" + arch])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--demangle", co], text=True)
    funcs, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            name = m.group(1)
            funcs[name] = []
            continue
        if name is None or not line.startswith("\t"):
            continue
        ins = line.split("//")[0].strip()
        ins = re.sub(r"<[^>]*>", "<sym>", ins)          # branch targets are printed as <symbol+offset>
        if ins and ins != "...":
            funcs[name].append(ins)
    return {n: normalise_layout(body) for n, body in funcs.items()}


def normalise_layout(lines):
    """The instruction lines of one function without what only its place in the object decides (see the module's docstring)."""
    lines = list(lines)
    op = [l.split()[0] for l in lines]
    if "s_endpgm" in op:
        first = len(op) - op[::-1].index("s_endpgm")          # behind the last s_endpgm
        last = first
        while last < len(op) and op[last] == "s_nop":
            last += 1
    else:
        first = last = len(op)
        while first > 0 and op[first - 1] == "s_nop":
            first -= 1
    del lines[first:last]
    for i, l in enumerate(lines):
        m = re.match(r"^s_getpc_b64 s\[(\d+):(\d+)\]$", l)
        if not m or i + 1 >= len(lines):
            continue
        lo, hi = "s" + m.group(1), "s" + m.group(2)
        a = re.match(r"^s_add_u32 %s, %s, (\S+)$" % (lo, lo), lines[i + 1])
        if not a:
            continue
        lines[i + 1] = "s_add_u32 %s, %s, <pcrel>" % (lo, lo)
        if i + 2 < len(lines) and re.match(r"^s_addc_u32 %s, %s, (\S+)$" % (hi, hi), lines[i + 2]):
            lines[i + 2] = "s_addc_u32 %s, %s, <pcrel>" % (hi, hi)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"); ap.add_argument("new", nargs="+")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--drop-trailing-zero", nargs="*", default=[])
    ap.add_argument("--show", type=int, default=0, help="print up to this many lines of the diff of every kernel that differs")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = disassemble(a.old, a.arch, tmp), {}
        for obj in a.new:
            funcs = disassemble(obj, a.arch, tmp)
            twice = sorted(set(funcs) & set(new))
            if twice:
                sys.exit("in two NEW objects (the second: %s): %s" % (obj, ", ".join(twice)))
            new.update(funcs)
    renamed = {}
    for n, body in new.items():
        k = n
        for t in a.drop_trailing_zero:
            m = re.match(r"^(.*\b" + re.escape(t) + r"<.*), 0>(\(.*)$", n)
            if m and (m.group(1) + ">" + m.group(2)) in old:
                k = m.group(1) + ">" + m.group(2)
        renamed[k] = body
    same = diff = lost = 0
    for n in sorted(old):
        if n not in renamed:
            print("only in OLD:", n)
            lost += 1
            continue
        if old[n] == renamed[n]:
            same += 1
        else:
            diff += 1
            first = next((i for i, (x, y) in enumerate(zip(old[n], renamed[n])) if x != y), min(len(old[n]), len(renamed[n])))
            print("DIFFERS: %s (%d / %d instructions, first difference at %d)" % (n, len(old[n]), len(renamed[n]), first))
            if a.show:
                import difflib
                for l in list(difflib.unified_diff(old[n], renamed[n], "OLD", "NEW", n=1, lineterm=""))[:a.show]:
                    print("    " + l)
    only_new = [n for n in sorted(renamed) if n not in old]
    for n in only_new:
        print("only in NEW:", n)
    print("%d kernels / functions identical, %d differ, %d only in OLD, %d only in NEW" % (same, diff, lost, len(only_new)))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
