"""Which kernels a run, a nursery, a contraction and an update take is decided by pc_plan.h; before that header the host loop decided inline,
in seven functions of pc_engine.hip.  tools/dev/plan_record.hip holds those conditions (commit ba2108c) transcribed, one function per decision,
and walks them and the header's functions over the full grid of their facts on the CPU: every boolean both ways, ncluster 0 / 1 / 2 / 64 / 65,
nDims 8 / 24 / 25 / 64 / 65 / 128 / 129, nursery_left 0 / 1 / 2, phantom rows 0 / 1, settings.ablate 0 and each of the plan's bits alone.  An
answer is the choice, what goes with it and its pchip_result.path[] increments."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polychordlite_amd", "csrc")

# the transcribed parent's answers over the grid: {decision: (digest, grid points)}
PARENT = {"run": ("0ca53294d8fac383", 688128),
          "update": ("d5a10ce3c6526f83", 13762560),
          "nursery": ("e041eb2005795343", 1605632),
          "contract": ("48ab1f80dfbda2e3", 2580480)}
ENUMERATORS = ["PC_BASES_READY", "PC_BASES_PART1", "PC_BASES_PART1_STEP", "PC_BASES_NHATS_G", "PC_BASES_WHOLE",
               "PC_SAMPLER_CALLBACK", "PC_SAMPLER_LANE", "PC_SAMPLER_WAVE_STEP", "PC_SAMPLER_WAVE",
               "PC_AHEAD_NONE", "PC_AHEAD_STEP", "PC_AHEAD_SIDE",
               "PC_CONTRACT_PAR", "PC_CONTRACT_FAST", "PC_CONTRACT_CL_STEP", "PC_CONTRACT_CL", "PC_CONTRACT_GENERAL",
               "PC_UPDATE_FUSED", "PC_UPDATE_STEPS", "PC_CTL_NONE", "PC_CTL_EARLY", "PC_CTL_LATE",
               "defer", "no_defer", "pool", "no_pool"]


@pytest.fixture(scope="module")
def record():
    """built host-only (seconds, no device pass); a missing hipcc fails the test, it does not skip it.  One walk of the grid for all tests."""
    subprocess.run(["make", "-C", CSRC, "plan_record"], check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PC_")}
    out = subprocess.run([os.path.join(ROOT, "tools", "dev", "plan_record")], env=env, capture_output=True, text=True).stdout
    decisions, reached = {}, {}
    for line in out.splitlines():
        w = line.split()
        if w[0] == "reached":
            reached[w[1]] = int(w[2])
        else:
            decisions[w[0]] = {"new": w[1], "old": w[2], "points": int(w[3]), "differ": int(w[4])}
    return decisions, reached


@pytest.mark.parametrize("decision", sorted(PARENT))
def test_choices_are_those_of_the_parent(record, decision):
    """the choice, what goes with it and the path[] slots it adds to, at every grid point"""
    d = record[0][decision]
    assert (d["old"], d["points"]) == PARENT[decision], "the transcribed conditions of ba2108c (or the grid) in tools/dev/plan_record.hip changed"
    assert d["differ"] == 0 and d["new"] == d["old"], (
        "pc_plan.h decides differently from ba2108c at %d of %d grid points: tools/dev/plan_record --dump lists them" % (d["differ"], d["points"]))


def test_every_enumerator_is_reached(record):
    reached = record[1]
    assert sorted(reached) == sorted(ENUMERATORS)
    assert not [n for n in ENUMERATORS if reached[n] <= 0]


def test_every_enumerator_of_the_header_is_walked():
    """an enumerator added to a choice of pc_plan.h must be added to the recorder (and to the list above)"""
    import re
    src = open(os.path.join(CSRC, "pc_plan.h")).read()
    names = set()
    for body in re.findall(r"\benum Pc\w+ \{(.*?)\};", src, re.S):
        body = re.sub(r"//[^\n]*", "", body)
        names |= set(re.findall(r"\b(PC_[A-Z0-9_]+)\b", body))
    assert names == {n for n in ENUMERATORS if n.startswith("PC_")}
