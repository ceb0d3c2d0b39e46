"""The host's half of a clustering update (polychordlite_amd/csrc/pc_split.h: the first pass' descriptors, NN_clustering's recursion level by level,
add_cluster in two pure steps around its one wait, the cluster map; and ClusterUpdate, which owns the scratch and does the traffic) does what lines
1292-1604 of pc_engine.hip did before they were moved out: tools/dev/split_record.hip drives it on the CPU with a scripted engine and a scripted
device -- no cluster above two points, one cluster not split, split in two, in five, a refinement three levels deep with parts of one point, three
clusters of which the first and the last split, the split cluster first, in the middle and last among one and seven, a split that outgrows the
list of clusters (the mirror asked for again), the two passes of a sub-dimension update with a split in the first, the second and both,
epoch_discard 0 and 1 with an empty and a filled nursery, the injected cluster-limit fault; each on its own and in step with other runs -- and the
digest of every scenario's record (every send with its destination, size and bytes, every launch or cohort record with its arguments, every
fetch and wait, in order; the cluster count, the next id, the genealogy, the map, the device's arrays at the end) is compared with the one the
same tool took from the code of the commit before (9f0f34b).

The parent also kept the recursion one cluster at a time, depth first, as a second path that no run took.  What that path was good for -- holding
the level-by-level order against the reference's -- is the tool's --order mode, run here; and the pure steps of add_cluster are held against the
oracle's formulas to the last bit."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from tests import oracle_api as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polychordlite_amd", "csrc")
BINARY = os.path.join(ROOT, "tools", "dev", "split_record")

# split_record_parent (make split_record_parent SPLIT_PARENT = lines 1292-1604 of 9f0f34b's pc_engine.hip): {scenario: (digest, lines)}
PARENT = {
 'nothing_above_two_points': ('742c9bd61c0534e6', 5),
 'nothing_above_two_points_in_step': ('4f77f266ea535c70', 6),
 'one_cluster_not_split': ('c0cdf72d96440cfc', 20),
 'one_cluster_not_split_in_step': ('b2b029d11571c48e', 22),
 'one_cluster_in_two': ('0e1baa9fdc5a7687', 44),
 'one_cluster_in_two_in_step': ('b9dfdfd52510a480', 62),
 'one_cluster_in_five': ('4a9b3dfe2f9cc93d', 44),
 'one_cluster_in_five_in_step': ('51763961842f477c', 62),
 'three_levels_single_points': ('b903cdcd0ebd49a2', 50),
 'three_levels_single_points_in_step': ('aa963f6a2c623de1', 69),
 'three_levels_uneven': ('cde4d76c9d9d6850', 56),
 'three_levels_uneven_in_step': ('43cc1d9213b7e5f3', 76),
 'first_and_last_of_three_split': ('8a02e32848853ceb', 67),
 'first_and_last_of_three_split_in_step': ('50a3275920352cf3', 100),
 'sizes_asked_for': ('e2e12d40a811410d', 69),
 'sizes_asked_for_in_step': ('63436c3b09ce99cd', 103),
 'split_at_0_of_1': ('444fcbff95720248', 44),
 'split_at_0_of_1_in_step': ('5023560641e5443f', 62),
 'split_at_0_of_7': ('571c62428f976691', 44),
 'split_at_0_of_7_in_step': ('5093d994a07a71e9', 62),
 'split_at_3_of_7': ('3f8af1b8572a41c1', 44),
 'split_at_3_of_7_in_step': ('ddb134f4f856c741', 62),
 'split_at_6_of_7': ('3e59c1d757343b87', 44),
 'split_at_6_of_7_in_step': ('64cd1f19f09a137d', 62),
 'the_list_grows': ('fd6094a3dda46df0', 93),
 'the_list_grows_in_step': ('7d0fa92f37f5efa3', 130),
 'the_list_grows_at_the_first_split': ('b3120f58c3c7e4d3', 57),
 'the_list_grows_at_the_first_split_in_step': ('e47d12619c6bfe48', 77),
 'two_passes_split_in_the_first': ('160817b57fc05c89', 64),
 'two_passes_split_in_the_first_in_step': ('0a17d2c68d025a2d', 86),
 'two_passes_split_in_the_second': ('11ed8a36fcd34f02', 79),
 'two_passes_split_in_the_second_in_step': ('65aa17a0b6a3ddb1', 114),
 'two_passes_split_in_both': ('e6913c5ad8d3cfe6', 122),
 'two_passes_split_in_both_in_step': ('5f3c06aa0df38d7f', 188),
 'two_passes_no_split': ('ab9f9c13b54302f2', 36),
 'two_passes_no_split_in_step': ('ff58356030cd42a0', 39),
 'two_passes_epoch_discard': ('c22e672fb056fadd', 103),
 'two_passes_epoch_discard_in_step': ('88b1a79e2cdfdad7', 153),
 'epoch_discard_0_nursery_0': ('bf87da90b29f1f51', 61),
 'epoch_discard_0_nursery_0_in_step': ('b6bb3848e4e35d44', 93),
 'epoch_discard_0_nursery_9': ('bb035666f57a837e', 63),
 'epoch_discard_0_nursery_9_in_step': ('db7acabb8157590b', 97),
 'epoch_discard_1_nursery_0': ('a4ccb6648e543f94', 61),
 'epoch_discard_1_nursery_0_in_step': ('26d49a736a9f2771', 93),
 'epoch_discard_1_nursery_9': ('53781dc905a708ba', 61),
 'epoch_discard_1_nursery_9_in_step': ('467cfe71d7b110af', 93),
 'injected_cluster_limit': ('c3fbe6d70f9b3bf3', 26),
 'injected_cluster_limit_in_step': ('724c3d65f220f2a8', 29)
}

REBUILD = ("For the two texts: CHANGELOG.md (the entry of pc_split.h) has the recipe for FILE; make -C polychordlite_amd/csrc split_record "
           "split_record_parent SPLIT_PARENT='\"FILE\"'; tools/dev/split_record_parent --dump > parent.txt (its lines without --dump are the PARENT "
           "table of this file); tools/dev/split_record --dump > new.txt; diff parent.txt new.txt")


def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PC_")}


def _run(*args):
    """the recorder's output.  Built host-only (seconds) from the headers alone; a missing hipcc fails the test, it does not skip it"""
    subprocess.run(["make", "-C", CSRC, "split_record"], check=True, capture_output=True, text=True)
    return subprocess.run([BINARY, *args], check=True, capture_output=True, text=True, env=_env()).stdout.splitlines()


@pytest.fixture(scope="module")
def recorded():
    digests = {name: (digest, int(lines)) for name, digest, lines in (line.split() for line in _run())}
    texts, name = {}, None
    for line in _run("--dump"):
        w = line.split()
        if len(w) == 3 and w[0] in digests and digests[w[0]] == (w[1], int(w[2])):
            name = w[0]; texts[name] = []
        else:
            texts[name].append(line)
    assert set(texts) == set(digests) and all(len(texts[n]) == digests[n][1] for n in texts)
    return digests, texts


def test_an_update_does_what_the_parent_did(recorded):
    digests, _ = recorded
    assert set(digests) == set(PARENT)
    differ = sorted(n for n in PARENT if digests[n] != PARENT[n])
    assert not differ, "scenarios %s differ from 9f0f34b.  %s" % (differ, REBUILD)


def test_the_scenarios_reach_every_path_of_an_update(recorded):
    """what the scenarios are there for does occur in their records"""
    _, texts = recorded
    def has(name, *whats):
        text = "\n".join(texts[name])
        for what in whats:
            assert re.search(what, text, re.M), (name, what)
    def count(name, what):
        return sum(1 for l in texts[name] if re.search(what, l))
    assert set(n for n in texts if not n.endswith("_in_step")) == set(n[:-8] for n in texts if n.endswith("_in_step"))
    assert count("nothing_above_two_points", r"^(launch|send|fetch)") == 0
    has("nothing_above_two_points", r"^found: no$", r"^clusters 3 peak 3 room 16 splits 0 ")
    has("one_cluster_not_split", r"^launch first pass: .* clusters 1 coordinates 0 ", r"^found: no$")
    assert count("one_cluster_not_split", r"^launch (level|rebuild)") == 0
    has("one_cluster_in_two", r"^clusters 2 peak 2 .* splits 1 next id 103 ")
    has("one_cluster_in_five", r"^clusters 5 peak 5 .* splits 1 next id 106 ")
    assert count("one_cluster_in_two", r"^launch level") == 1      # (the parts are looked at once more, and stay)
    assert count("three_levels_single_points", r"^launch level") == 2
    has("three_levels_single_points", r"^launch level: .* parts 3 largest 2$", r"^clusters 7 ")
    has("three_levels_single_points_in_step", r"^written down: level: .* parts 3 largest 2$", r"^left written down: 0$")
    assert count("three_levels_single_points_in_step", r"^launch (level|first pass)") == 0
    # the first and the last of three: the first split takes place 0, the untouched cluster moves up to 0, the last is split at 1
    has("first_and_last_of_three_split", r"^launch shift_mats: cluster 0 of 3$", r"^launch shift_mats: cluster 1 of 4$", r"^clusters 9 .* splits 2 ")
    assert count("first_and_last_of_three_split", r"^wait$") == 1 + 2 + 2      # (the first pass, two levels for both clusters at once, a wait a split)
    has("sizes_asked_for", r"^fetch cl_n\+0 12 bytes$")
    for p, nc in ((0, 1), (0, 7), (3, 7), (6, 7)):
        has("split_at_%d_of_%d" % (p, nc), r"^launch shift_mats: cluster %d of %d$" % (p, nc), r"^clusters %d " % (nc + 2))
    has("the_list_grows", r"^the list of clusters grows from 4 to 8$", r"^the list of clusters grows from 8 to 16$", r"^clusters 9 peak 9 room 16 splits 2 ")
    # (the mirror of the first pass is for another leading dimension: asked for again, in a wait of its own)
    assert count("the_list_grows", r"^fetch XpXq") == 3 and count("one_cluster_in_five", r"^fetch XpXq") == 1
    has("the_list_grows_at_the_first_split", r"^the list of clusters grows from 2 to 6$", r"^clusters 6 ")
    has("two_passes_split_in_the_first", r"^launch first pass: .* dims c_subdims\+0 .* coordinates 2 ", r"^sub-dimension pass found: yes$", r"^fetch cl_n\+0 16 bytes$",
        r"^map: -1 0 1$", r"^launch remap_chains: map c_map\+0 clusters 3 chains 5$")
    has("two_passes_split_in_the_second", r"^sub-dimension pass found: no$", r"^found: yes$", r"^map: -1 0 -1$")
    assert count("two_passes_split_in_the_second", r"^fetch cl_n\+0 12 bytes$") == 0
    has("two_passes_split_in_both", r"^sub-dimension pass found: yes$", r"^map: -1 0 -1$", r"^launch remap_chains: ")
    assert count("two_passes_split_in_both", r"^launch remap_chains") == 1
    has("two_passes_no_split", r"^found: no$", r"^map: 0 1$")
    assert count("two_passes_no_split", r"^(send ctl|launch remap_chains)") == 0
    has("two_passes_epoch_discard", r" epoch 5 ")
    assert count("two_passes_epoch_discard", r"^launch remap_chains") == 0
    has("epoch_discard_0_nursery_9", r"^launch remap_chains: map c_map\+0 clusters 3 chains 9$", r" epoch 3 ")
    assert count("epoch_discard_0_nursery_0", r"^launch remap_chains") == 0 and count("epoch_discard_1_nursery_9", r"^launch remap_chains") == 0
    has("epoch_discard_1_nursery_9", r" epoch 4 ", r"^send ctl\+0 ")
    has("injected_cluster_limit", r"^failed with code 8: more than 2 clusters \(injected\)$", r"^clusters 2 .* splits 0 ")
    assert count("injected_cluster_limit", r"^(send live_cluster|launch rebuild)") == 0
    for name, lines in texts.items():
        assert not any("outside every block" in l for l in lines), name


def test_the_order_of_the_recursion_does_not_matter():
    """PartRefiner, level by level over all clusters of an update at once, against the reference's order -- one cluster after the other, depth
    first, relabelled by first appearance after every step (clustering.f90:80-95, utils.F90:713-749; restated in the tool) -- with a rule that depends
    on a part's point set only, over 300 seeded updates of one to four clusters of 3 ... 200 points: the same final labels and counts"""
    out = _run("--order")
    m = re.fullmatch(r"order: (\d+) clusters, 0 mismatches", out[-1])
    assert m and int(m.group(1)) >= 300 and len(out) == 1, out[-5:]


def _oracle_split(logni, logni1, par, rowpq):
    """run_time_info.f90:458-503 with the oracle's pc_logsumexp / pc_logaddexp (oracle/pc_oracle.c, add_cluster)"""
    lib = orc.load()
    v = (C.c_double * len(logni))(*logni)
    logn = lib.pc_logsumexp(v, len(logni)); logn1 = lib.pc_logaddexp(logn, 0.0)
    new = {"Xp": [par["Xp"] + l - logn for l in logni], "ZXp": [par["ZXp"] + l - logn for l in logni], "Zp": [par["Zp"] + l - logn for l in logni],
           "Zp2": [par["Zp2"] + l + l1 - logn - logn1 for l, l1 in zip(logni, logni1)], "ZpXp": [par["ZpXp"] + l + l1 - logn - logn1 for l, l1 in zip(logni, logni1)]}
    rows = [[r + l - logn for r in rowpq] for l in logni]
    block = [[par["Xp2"] + logni[a] + (logni1[a] if a == b else logni[b]) - logn - logn1 for b in range(len(logni))] for a in range(len(logni))]
    return new, rows, block, [l - logn for l in logni]


@pytest.mark.parametrize("counts", [(2, 11, 3, 0, 1, 40), (1, 0, 1, 0, 1, 0), (150, 20000, 1, 3, 7, 7)])
def test_add_cluster_steps_match_the_oracle_formulas(counts):
    """cluster 1 of 4 splits into 3 (the live and phantom points of the new clusters: counts): the labels, ids and thresholds of the step before
    the wait by hand; the evidences, volumes, cross volumes and the genealogy of the step behind it equal to the last bit to the oracle's"""
    out = _run("--split", *[str(c) for c in counts])
    f = float.fromhex
    got = {}
    for line in out[1:]:
        w = line.split()
        if w[0] in ("in", "out") and w[1] == "XQ":
            got.setdefault(w[0] + " XQ", []).append([f(x) for x in w[3:]])
        elif w[0] in ("in", "out"):
            got[w[0] + " " + w[1]] = [f(x) for x in w[2:]]
        else:
            got[w[0]] = w[1:]
    nc, p, nnew = 4, 1, 3
    keep = [c for c in range(nc) if c != p]
    # before the wait: the parent's points (slots 1 2 5 7 8 10 in its order, labels 2 1 2 3 1 2) take the new clusters 3 4 5 and their ranks there;
    # the clusters behind the parent move up
    assert [int(x) for x in got["lc"]] == [0, 4, 3, 1, -1, 4, 2, 5, 3, 0, 4, 2]
    assert [int(x) for x in got["lp"]] == [0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 2, 1]
    assert got["uid"] == ["10", "12", "13", "50", "51", "52", "next", "53"]
    assert [f(x) for x in got["thr"]][3:] == [-1.7976931348623157e308] * 3
    assert [int(x) for x in got["nlv"]] == list(counts[0::2]) and [int(x) for x in got["nph"]] == list(counts[1::2])
    n = [a + b for a, b in zip(counts[0::2], counts[1::2])]
    logni, logni1 = [math.log(float(x) + 0.0) for x in n], [math.log(float(x) + 1.0) for x in n]
    par = {k: got["in " + k][p] for k in ("Xp", "ZXp", "Zp", "Zp2", "ZpXp")}
    par["Xp2"] = got["in XQ"][p][p]
    rowpq = [got["in XQ"][p][q] for q in keep]
    new, rows, block, frac = _oracle_split(logni, logni1, par, rowpq)
    for k in ("Xp", "ZXp", "Zp", "Zp2", "ZpXp"):
        assert got["out " + k] == [got["in " + k][c] for c in keep] + new[k], k
    xq = got["out XQ"]
    nold = nc - 1
    for a in range(nold):
        assert xq[a][:nold] == [got["in XQ"][keep[a]][q] for q in keep]
    for k in range(nnew):
        assert xq[nold + k][:nold] == rows[k] and [xq[q][nold + k] for q in range(nold)] == rows[k]
        assert xq[nold + k][nold:] == block[k]
    g = got["genealogy"]
    assert g[0::3] == ["50", "51", "52"] and g[1::3] == ["11"] * 3 and [f(x) for x in g[2::3]] == frac
