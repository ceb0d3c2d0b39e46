"""CPU: what tools/dev/isa_diff.py takes out of a function's instruction lines before it compares them (normalise_layout) -- the padding behind
the last s_endpgm and the pc-relative literal behind an s_getpc_b64, both decided by a function's neighbours in its object -- and, as much,
what it leaves in.  Literal lines, no compiler."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "dev", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)
norm = isa_diff.normalise_layout

BODY = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v0, 0", "global_store_dword v0, v0, s[0:1]"]


def test_nop_inside_a_body_is_kept():
    lines = BODY[:2] + ["s_nop 0"] + BODY[2:] + ["s_endpgm"]
    assert norm(lines) == lines
    assert norm(lines) != norm(BODY + ["s_endpgm"])


def test_nops_behind_the_last_endpgm_are_dropped():
    assert norm(BODY + ["s_endpgm", "s_nop 0", "s_nop 0", "s_nop 0"]) == BODY + ["s_endpgm"]
    assert norm(BODY + ["s_endpgm", "s_nop 0"]) == norm(BODY + ["s_endpgm"] + ["s_nop 0"] * 5)


def test_nops_behind_an_endpgm_that_is_not_the_last_are_kept():
    lines = BODY[:2] + ["s_cbranch_scc1 <sym>", "s_endpgm", "s_nop 0", "s_nop 0"] + BODY[2:] + ["s_endpgm", "s_nop 0"]
    assert norm(lines) == lines[:-1]
    assert norm(lines) != norm(BODY[:2] + ["s_cbranch_scc1 <sym>", "s_endpgm"] + BODY[2:] + ["s_endpgm"])


def test_trailing_nops_of_a_function_without_endpgm_are_dropped():
    f = BODY + ["s_setpc_b64 s[30:31]"]
    assert norm(f + ["s_nop 0", "s_nop 0"]) == f
    assert norm(BODY[:2] + ["s_nop 0"] + BODY[2:] + ["s_setpc_b64 s[30:31]", "s_nop 0"]) == BODY[:2] + ["s_nop 0"] + BODY[2:] + ["s_setpc_b64 s[30:31]"]


def _pcrel(lit, pair=(4, 5), add=(4, 5), hi_lit="0"):
    return (BODY[:2] + ["s_getpc_b64 s[%d:%d]" % pair, "s_add_u32 s%d, s%d, %s" % (add[0], add[0], lit),
                        "s_addc_u32 s%d, s%d, %s" % (add[1], add[1], hi_lit)] + BODY[2:] + ["s_endpgm"])


def test_pc_relative_literal_behind_getpc_compares_equal():
    assert norm(_pcrel("0x1f4c")) == norm(_pcrel("0x2a90"))
    assert norm(_pcrel("0x1f4c", hi_lit="0")) == norm(_pcrel("0xfffff000", hi_lit="-1"))
    assert len(norm(_pcrel("0x1f4c"))) == len(_pcrel("0x1f4c"))


def test_add_literal_not_behind_getpc_is_kept():
    a = BODY[:2] + ["s_add_u32 s4, s4, 0x1f4c", "s_addc_u32 s5, s5, 0"] + BODY[2:] + ["s_endpgm"]
    b = BODY[:2] + ["s_add_u32 s4, s4, 0x2a90", "s_addc_u32 s5, s5, 0"] + BODY[2:] + ["s_endpgm"]
    assert norm(a) == a and norm(b) == b and norm(a) != norm(b)
    # an instruction between the two: not "directly behind"
    a = BODY[:2] + ["s_getpc_b64 s[4:5]", "s_mov_b32 s6, 0", "s_add_u32 s4, s4, 0x1f4c"] + BODY[2:] + ["s_endpgm"]
    b = BODY[:2] + ["s_getpc_b64 s[4:5]", "s_mov_b32 s6, 0", "s_add_u32 s4, s4, 0x2a90"] + BODY[2:] + ["s_endpgm"]
    assert norm(a) == a and norm(a) != norm(b)


def test_add_literal_behind_getpc_of_another_pair_is_kept():
    a, b = _pcrel("0x1f4c", pair=(4, 5), add=(6, 7)), _pcrel("0x2a90", pair=(4, 5), add=(6, 7))
    assert norm(a) == a and norm(b) == b and norm(a) != norm(b)
    # the low half names the pair, the carry another register: only the low literal is the pc-relative one
    a = BODY[:2] + ["s_getpc_b64 s[4:5]", "s_add_u32 s4, s4, 0x1f4c", "s_addc_u32 s7, s7, 1"] + BODY[2:] + ["s_endpgm"]
    b = BODY[:2] + ["s_getpc_b64 s[4:5]", "s_add_u32 s4, s4, 0x2a90", "s_addc_u32 s7, s7, 2"] + BODY[2:] + ["s_endpgm"]
    assert norm(a) != norm(b)


def test_the_two_layout_cases_together_and_nothing_else():
    old = _pcrel("0x1f4c") + ["s_nop 0"] * 3
    new = _pcrel("0x2a90") + ["s_nop 0"] * 11
    assert norm(old) == norm(new)
    changed = list(new)
    changed[changed.index("s_endpgm") - 1] = "global_store_dword v0, v0, s[2:3]"      # (the store in front of s_endpgm)
    assert norm(old) != norm(changed)
