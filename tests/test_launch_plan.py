"""The sampling launchers choose the kernels, grids, blocks and LDS sizes they chose before they were rewritten around one plan
(pc_slice_plan and the variant table of pc_sample.hip, launch_t of pc_slice_t.hip): tools/dev/launch_record.hip walks a grid of
fabricated states through them on the CPU, under no developer switch and under each of seven, and the digest of every launcher's
record is compared with the one taken from the commit before the rewrite (69220c3).  A second sweep, `launch_record --forms`, walks the
same launchers over the same grid for source handles of every form (several sums, quadratic, shared values): what pins the LDS sizes the
launchers take from a handle's form record on the CPU, against the commit before that record (e2f1bd3)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polychordlite_amd", "csrc")
SWITCHES = ["", "PC_SLICE_LEAN_OFF", "PC_SLICE_HELPER_OFF", "PC_SLICE_WPB_OFF", "PC_SLICE_FUSED_OFF", "PC_SLICE_T_HELP_OFF", "PC_BASES_T_OFF",
            "PC_SLICE_T_OFF"]

# launch_record / launch_record_t built against 69220c3's pc_sample.hip / pc_slice_t.hip, no switch set: {launcher: (digest, calls)}
PARENT = {'slice': ('fcdd23aa9e930bbf', 716800),
 'slice_fused': ('4ef919ac9d7197c5', 716800),
 'slice_many0': ('3f92b004f6a8bafb', 716800),
 'slice_many1': ('8b61ed18699f572d', 716800),
 'nhats': ('32e0e22ea1cd0d63', 716800),
 'nhats_part1': ('ecaa399402a1b4c3', 716800),
 'nhats_part2': ('07dd67a199643493', 716800),
 'nhats_part1_packed': ('971067fcee908493', 716800),
 'nhats_many': ('30a84a1f6bf133d3', 716800),
 'generate_live': ('97254d6634035c63', 716800),
 'prior_transform': ('c6f6006297f53f03', 716800),
 'source_eval': ('c68249adb44ca9c3', 716800),
 'slice_t': ('f64966acb1583d4b', 358400),
 'slice_t_many': ('656859e6a3ff4dbb', 1433600),
 'slice_t_ok': ('bb315de8f3d07823', 179200),
 'bases_t': ('cc3fa7f178163d53', 358400),
 'bases_t_many': ('1a5d33c1d41c0b13', 1433600)}
# ... and the launchers that choose differently under each developer switch
PARENT_UNDER = {'PC_SLICE_LEAN_OFF': {'slice': ('fdb1beeffeb0da6f', 716800),
                       'slice_fused': ('a00908d5786f014b', 716800),
                       'slice_many0': ('c0fa7f34481df6af', 716800),
                       'slice_many1': ('6224950099455703', 716800)},
 'PC_SLICE_HELPER_OFF': {'slice_fused': ('8e6aea1168826943', 716800)},
 'PC_SLICE_WPB_OFF': {'slice': ('40798779d482662b', 716800)},
 'PC_SLICE_FUSED_OFF': {'slice_fused': ('069b3b502f55b103', 716800), 'slice_many1': ('069b3b502f55b103', 716800)},
 'PC_SLICE_T_HELP_OFF': {'slice_t_many': ('a83dca273b6276a3', 1433600)},
 'PC_BASES_T_OFF': {'bases_t': ('0a131b6bc49e2f13', 358400), 'bases_t_many': ('730a16dd293b47e3', 1433600)},
 'PC_SLICE_T_OFF': {'slice_t_ok': ('1f32a1b3e67b3903', 179200)}}

# launch_record --forms built against e2f1bd3's pc_sample.hip and pc_launch.h, with that commit's one accessor per field stubbed from the same
# table of handles, no switch set: {launcher: (digest, calls)}
PARENT_FORMS = {'slice': ('c5aa8f1ec4e4a77b', 921600),
 'slice_fused': ('6bf493219f1523eb', 921600),
 'slice_many0': ('1cf45aefe825d845', 921600),
 'slice_many1': ('af6b9727ea093f3f', 921600),
 'nhats': ('318a554bd2e1df53', 921600),
 'nhats_part1': ('b0857b6c5a881f33', 921600),
 'nhats_part2': ('6aa2ac09c37ab1c3', 921600),
 'nhats_part1_packed': ('9dccc37170a43143', 921600),
 'nhats_many': ('e8aced6c7605c633', 921600),
 'generate_live': ('ddb0789792c4a823', 921600),
 'prior_transform': ('9d8afbda98ddf71b', 921600),
 'source_eval': ('24cfff098d184613', 921600)}


def record(binary, switch, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PC_")}
    if switch:
        env[switch] = "1"
    out = subprocess.run([binary, *args], env=env, check=True, capture_output=True, text=True).stdout
    return {name: (digest, int(calls)) for name, digest, calls in (line.split() for line in out.splitlines())}


@pytest.fixture(scope="module")
def recorders():
    """built host-only (no device pass: seconds); a missing hipcc fails the test, it does not skip it"""
    subprocess.run(["make", "-C", CSRC, "launch_record"], check=True, capture_output=True, text=True)
    return [os.path.join(ROOT, "tools", "dev", n) for n in ("launch_record", "launch_record_t")]


@pytest.mark.parametrize("switch", SWITCHES)
def test_launches_are_those_of_the_parent(recorders, switch):
    got = {}
    for b in recorders:
        got.update(record(b, switch))
    want = dict(PARENT, **PARENT_UNDER.get(switch, {}))
    assert set(got) == set(want)
    differ = sorted(n for n in want if got[n] != want[n])
    assert not differ, (
        "launchers %s choose differently from 69220c3%s.  For the two texts: build tools/dev/launch_record.hip against both trees "
        "(make -C polychordlite_amd/csrc launch_record; in a checkout of 69220c3 the same two hipcc lines with -I set to its csrc), run "
        "each as `%slaunch_record --dump DIR` and diff DIR/<launcher>.txt" % (differ, " under " + switch if switch else "", switch + "=1 " if switch else ""))


def test_launches_of_every_source_form_are_those_of_the_parent(recorders):
    """the recorder itself exits 1 unless the handles with several sums and the quadratic form of 1024 residuals have states on both sides of
    pc_slice_phi_lds's 48 KB limit"""
    got = record(recorders[0], "", "--forms")
    assert set(got) == set(PARENT_FORMS)
    differ = sorted(n for n in PARENT_FORMS if got[n] != PARENT_FORMS[n])
    assert not differ, "launchers %s choose differently from e2f1bd3 for a source handle of some form (`launch_record --forms --dump DIR` of both trees, as above)" % differ


def test_every_sampling_kernel_is_reached(recorders):
    """every k_slice / k_slice_many row of the variant table is chosen by some state of the sweep, except the three the launchers cannot
    reach: four chains a workgroup with the twin Gaussian's functor (the helper wavefronts exist for LEAN = 1, 3, 5 only)"""
    import re
    src = open(os.path.join(CSRC, "pc_sample.hip")).read()
    one = src[src.index("#define PC_SLICE_VARIANTS(X)"):src.index("#define PC_SLICE_MANY_VARIANTS(X)")]
    many = src[src.index("#define PC_SLICE_MANY_VARIANTS(X)"):src.index("static int pc_slice_launch(")]
    rows = ["k_slice<%s>" % r for r in re.findall(r"\bX\(([^)]*)\)", one)] + ["k_slice_many<%s>" % r for r in re.findall(r"\bX\(([^)]*)\)", many)]
    table = set(rows)
    assert len(table) == len(rows) == 61 + 18      # (a row written twice would compile: the first one wins)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PC_")}
    reached = set(subprocess.run([recorders[0], "--kernels"], env=env, check=True, capture_output=True, text=True).stdout.split("\n"))
    missing = sorted(table - reached)
    assert missing == ["k_slice<1, 1, false, 4, 16, 4, 0>", "k_slice<1, 1, false, 4, 8, 4, 0>", "k_slice<1, 2, false, 4, 24, 4, 0>"], missing
    assert not [k for k in reached if k.startswith(("k_slice<", "k_slice_many<")) and k not in table]
    # lane = chain: every nDims 1 .. 24, the unit box or not, one run / runs in step without and with the helping wavefronts
    reached_t = set(subprocess.run([recorders[1], "--kernels"], env=env, check=True, capture_output=True, text=True).stdout.split("\n"))
    want_t = {"k_slice_t<%d, %s>" % (d, u) for d in range(1, 25) for u in ("true", "false")}
    want_t |= {"k_slice_t_many<%d, %s, %s>" % (d, u, h) for d in range(1, 25) for u in ("true", "false") for h in ("true", "false")}
    assert {k for k in reached_t if k.startswith("k_slice_t")} == want_t
