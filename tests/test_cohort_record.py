"""The cohort of the runs in step (polychordlite_amd/csrc/pc_cohort.h: the table of stages, the constructors of its records, flush) makes
the launches, waits and uploads that the Cohort inside pc_engine.hip made before it was moved out and rewritten around one table:
tools/dev/cohort_record.hip drives it on the CPU with fabricated records -- every kind in groups of 1, 2, 5 and 64 runs, runs that differ in
each key of the launch order, every launcher for several runs declining, with and without the second stream, every case of the numbered
wait for the bases, a block outgrown, more flushes than the ring has slots, flushes with nothing written down -- and the digest of every
scenario's record is compared with the one the same driver took from the Cohort of the commit before (abd2406)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polychordlite_amd", "csrc")

# cohort_record_parent (make cohort_record_parent COHORT_PARENT = lines 493-676 of abd2406's pc_engine.hip): {scenario: (digest, lines)}
PARENT = {'group_compact': ('e9f4c72d9b7c1886', 80),
 'group_reset': ('0fd7edaf70fdfeff', 80),
 'group_clus1': ('949d18766e96309e', 80),
 'group_clusg': ('b6dda128a2c15438', 80),
 'group_bases': ('7400070fba8a63a3', 80),
 'group_nhats_g': ('b757a8ec13ea9d4f', 80),
 'group_slice': ('e00ba5c33d2a18f7', 80),
 'group_slice_g': ('4364acb929dcd981', 80),
 'group_bases_next': ('7400070fba8a63a3', 80),
 'group_sort': ('c98137a08d971b69', 80),
 'group_nn': ('b557696fcdede336', 80),
 'group_consume': ('d624b4898089c7dd', 80),
 'group_consume_cl': ('cecd80d5688ae297', 80),
 'group_apply': ('ecb768abee7e5507', 80),
 'group_update': ('c1dcb59dbe14c2be', 80),
 'group_final': ('4852903acd9872e7', 80),
 'group_compact_st2': ('dafc8458e77be53a', 88),
 'group_reset_st2': ('6e7166b7fa384045', 88),
 'group_clus1_st2': ('420e54de681bc007', 88),
 'group_clusg_st2': ('ab0c06e0d0cdeec3', 88),
 'group_bases_st2': ('596f27ea83e32169', 88),
 'group_nhats_g_st2': ('ade15a73dcaea355', 88),
 'group_slice_st2': ('f967509bc09d2ddd', 88),
 'group_slice_g_st2': ('780bb1b56dd64b4f', 88),
 'group_bases_next_st2': ('154dab9876f3607d', 120),
 'group_sort_st2': ('37529153c056d257', 88),
 'group_nn_st2': ('16425a11ecf56844', 88),
 'group_consume_st2': ('864402212253761b', 88),
 'group_consume_cl_st2': ('3ab7713241754afd', 88),
 'group_apply_st2': ('b786e56294e3346d', 88),
 'group_update_st2': ('a6cb5bbe1420bc3f', 88),
 'group_final_st2': ('3f68a96529c0974d', 88),
 'keys_compact': ('ba70985926fae702', 62),
 'keys_reset': ('c06c0c1cc3f8b738', 62),
 'keys_clus1': ('bd595f0f63f60156', 62),
 'keys_clusg': ('5a1977cf9feb55dc', 62),
 'keys_bases': ('b0eb76e054b9aa48', 65),
 'keys_nhats_g': ('0c13903619bc7966', 65),
 'keys_slice': ('33293926657505c2', 65),
 'keys_slice_g': ('7eaa85fa44dab93c', 68),
 'keys_bases_next': ('b166c2b6139c9d0b', 134),
 'keys_sort': ('df14daf7afbe40ca', 62),
 'keys_nn': ('7fcb1ad7bf13d9a8', 62),
 'keys_consume': ('0ba2deac7b19fe64', 62),
 'keys_consume_cl': ('5230f32764401738', 65),
 'keys_apply': ('f4a623499af37d45', 65),
 'keys_update': ('258506f32e78b7b8', 68),
 'keys_final': ('bdd8d10cfcef2559', 62),
 'declines_compact': ('407ac865ee8f26f6', 34),
 'declines_reset': ('66d9d84322710014', 34),
 'declines_clus1': ('56e538f21a79b6f5', 34),
 'declines_clusg': ('7b354b10c3fbc0a0', 34),
 'declines_bases': ('1025c0523b53f5be', 34),
 'declines_nhats_g': ('41d69eb7beb489dc', 34),
 'declines_slice': ('9b70896b5d181f0e', 34),
 'declines_slice_g': ('cfb8337682cb2691', 35),
 'declines_bases_next': ('a2f62e667387fb20', 34),
 'declines_sort': ('2e3fdb5c52f9873f', 34),
 'declines_nn': ('b5e69b3c78214c92', 34),
 'declines_consume': ('f2425ee6adfb34ee', 34),
 'declines_consume_cl': ('029421ee00f14ecd', 35),
 'declines_apply': ('43c7ff09e45ebf6a', 34),
 'declines_update': ('656c5f5aad976d5e', 35),
 'declines_final': ('8f3bd358909434c7', 34),
 'declines_compact_st2': ('5406bc053275ac1d', 42),
 'declines_reset_st2': ('ffbf42f9980eab16', 42),
 'declines_clus1_st2': ('19a7a81fd3e1b283', 42),
 'declines_clusg_st2': ('8b8ad9609a5a0e41', 42),
 'declines_bases_st2': ('0e8d8a21459a002e', 42),
 'declines_nhats_g_st2': ('72b470afb33e9a3c', 42),
 'declines_slice_st2': ('85835beba598a32e', 42),
 'declines_slice_g_st2': ('afe28c6f5641bee1', 51),
 'declines_bases_next_st2': ('2d1372484c8178d5', 50),
 'declines_sort_st2': ('2638848779496332', 42),
 'declines_nn_st2': ('4eaeb23e1d13713c', 42),
 'declines_consume_st2': ('b91634e9e03ffcde', 42),
 'declines_consume_cl_st2': ('d6d7647944be6335', 43),
 'declines_apply_st2': ('6a90068ec2a1c22c', 42),
 'declines_update_st2': ('d83d8286291c765e', 43),
 'declines_final_st2': ('c44c1a35d43ee101', 42),
 'rounds': ('27e3f360a1192127', 358),
 'rounds_declined': ('f2bd0b94117ff987', 773),
 'rounds_st2': ('5211281674bd20aa', 438),
 'rounds_st2_declined': ('e9d9b3c9a7f1e73e', 893),
 'bases_number_slice': ('56cba459209495eb', 116),
 'bases_number_slice_g': ('61c4be2e6c03906f', 116),
 'bases_number_slice_st2': ('2aa7bf48dff931c2', 181),
 'bases_number_slice_g_st2': ('f9c7e7f8e6a1fdd6', 181),
 'empty_flush': ('d7e29c61e4753d82', 45),
 'empty_flush_st2': ('32e6c5dc4169ee5a', 53)}

REBUILD = ("For the two texts: git show abd2406:polychordlite_amd/csrc/pc_engine.hip | sed -n 493,676p > /tmp/parent_cohort.inc; "
           "make -C polychordlite_amd/csrc cohort_record cohort_record_parent COHORT_PARENT='\"/tmp/parent_cohort.inc\"'; "
           "tools/dev/cohort_record_parent --dump > parent.txt (its lines without --dump are the PARENT table of this file); "
           "tools/dev/cohort_record --dump > new.txt; diff parent.txt new.txt")
KINDS = {"compact": ("clean_many", "clean"), "reset": ("reset_thresholds_many", "reset_thresholds"), "clus1": ("knn_cluster_batch_many", "knn_cluster_batch_dev"),
         "clusg": ("knn_cluster_sub_many", "knn_cluster_sub"), "bases": ("bases_t_many", "nhats_part"), "nhats_g": ("nhats_many", "nhats"),
         "slice": ("slice_t_many", "slice_t"), "slice_g": ("slice_many", "slice"), "bases_next": ("bases_t_many", "nhats_part"),
         "sort": ("sort_live_many", "sort_live"), "nn": ("nn_lists_many", "nn_lists"), "consume": ("consume_par_many", "consume_par"),
         "consume_cl": ("consume_cl_many", "consume_cl"), "apply": ("apply_many", "apply"), "update": ("update_fused_many", "update_fused"),
         "final": ("final_par_many", "final_par")}


@pytest.fixture(scope="module")
def recorded():
    """the recorder's digests and its records by scenario.  Built host-only (seconds) from pc_cohort.h alone -- the variant that drives an older
    Cohort is another binary --; a missing hipcc fails the test, it does not skip it"""
    subprocess.run(["make", "-C", CSRC, "cohort_record"], check=True, capture_output=True, text=True)
    binary = os.path.join(ROOT, "tools", "dev", "cohort_record")
    out = subprocess.run([binary], check=True, capture_output=True, text=True).stdout
    digests = {name: (digest, int(lines)) for name, digest, lines in (line.split() for line in out.splitlines())}
    texts, name = {}, None
    for line in subprocess.run([binary, "--dump"], check=True, capture_output=True, text=True).stdout.splitlines():
        w = line.split()
        if len(w) == 3 and w[0] in digests and digests[w[0]] == (w[1], int(w[2])):
            name = w[0]; texts[name] = []
        else:
            texts[name].append(line)
    assert set(texts) == set(digests) and all(len(texts[n]) == digests[n][1] for n in texts)
    return digests, texts


def test_the_cohort_launches_what_the_parent_launched(recorded):
    digests, _ = recorded
    assert set(digests) == set(PARENT)
    differ = sorted(n for n in PARENT if digests[n] != PARENT[n])
    assert not differ, "scenarios %s differ from abd2406.  %s" % (differ, REBUILD)


@pytest.mark.parametrize("second", ["", "_st2"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_declining_launcher_sends_its_runs_one_by_one(recorded, kind, second):
    """the scenario of a kind: its own launcher for several runs declines and its three runs are launched one by one, behind the declined
    launch of their group and on its stream; the two runs of the other kind in the same flush are launched together"""
    lines = recorded[1]["declines_" + kind + second]
    many, one = KINDS[kind]
    launches = [l for l in lines if l.startswith("launch ")]
    # (the three runs of slice_g, consume_cl and update differ in a word the runs of a launch must share: more than one group, each declined)
    declined = [i for i, l in enumerate(launches) if l.endswith("-> declines")]
    assert declined and sum(int(launches[i].split("+")[1].split()[0]) for i in declined) == 3
    for i in declined:
        assert launches[i].startswith("launch %s records " % many), launches[i]
        n = int(launches[i].split("+")[1].split()[0])
        stream = launches[i].split(" on ")[1].split()[0]
        assert stream == ("second" if kind == "bases_next" and second else "main")
        singles = launches[i + 1:i + 1 + n]
        assert len(singles) == n and all(l.split()[1] in (one, "slice_fused") and " records " not in l and l.endswith(" on " + stream) for l in singles), singles
    assert sum(1 for l in launches if " records " in l and "+2 run" in l and not l.endswith("declines")) == 1
    counters = [l for l in lines if l.startswith("fused ")]
    assert len(counters) == 1 and counters[0].startswith("fused 2 single 3 ")


def test_the_sweep_reaches_every_stage_both_ways(recorded):
    """every row of the table is launched for a group and run by run; the waits of every role occur"""
    text = "\n".join(l for lines in recorded[1].values() for l in lines)
    for many, one in KINDS.values():
        assert "launch %s records" % many in text, many
        assert "launch %s run" % one in text, one
    assert "launch slice_fused run" in text
    for what in ["wait upload on second", "wait next on main", "wait ev_seq[0] on main", "wait ev_seq[1] on main", "wait ev_seq[2] on main", "wait ev_seq[3] on main",
                 "host waits slot[3]", "host waits slot2[", "device block freed", "closure in front 2", "closure behind 2", "copies on main"]:
        assert what in text, what
