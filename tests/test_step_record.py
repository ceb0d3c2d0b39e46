"""The driver of the runs in step (polychordlite_amd/csrc/pc_step.h: pc_run_many and the phases of StepGroup -- streams picked, runs set up, full
phantom arrays compacted, the round enqueued, awaited and finished, finished runs ended by a thread, endings joined, everything released) asks of
its engines, its streams and the device what the 285-line pc_run_many inside pc_engine.hip asked before it was moved out: tools/dev/step_record.hip
drives it on the CPU with a scripted engine -- groups of 1, 2, 5 and 64 runs ending in different rounds, more seeds than fit (several groups,
the last one short), another group busy on the device, compactions in some rounds, updates that wait one to three times as fibers next to
runs that finish at once, an update throwing in the first, a middle and the last fiber while others are suspended, set-up without memory at
run 0 and at a later run, set-up failing otherwise, begin returning a code, a run's own code in a round, results failing in an ending batch;
all of it with and without the second stream, the copy streams and the fibers -- and the digest of every scenario's record is compared with
the one the same tool took from the driver of the commit before (b330d9b).

One scenario is new with the header: the event pool fails while the streams are picked, which used to leave pc_run_many as an exception through
its C interface.  It is a return code now, and everything taken by then is given back."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polychordlite_amd", "csrc")
BINARY = os.path.join(ROOT, "tools", "dev", "step_record")
# (a process each: the switches are read once.  PC_COHORT_SETUP_THREADS stays at its default, one)
VARIANTS = {"": {}, "_noside": {"PC_COHORT_SIDE": "0"}, "_nocopystreams": {"PC_COHORT_COPY_STREAMS": "0"}, "_nofibers": {"PC_COHORT_FIBERS": "0"}}

# step_record_parent (make step_record_parent STEP_PARENT = lines 2715-2999 of b330d9b's pc_engine.hip), once per variant: {scenario: (digest, lines)}
PARENT = {
 'group_1': ('a40ba5b3a4708876', 91),
 'group_2': ('cb80420b25319414', 122),
 'group_5': ('5cc01d70361e97b6', 220),
 'group_64': ('8f70e083d5289a9d', 1161),
 'groups_3_3_1': ('506e72643f63025a', 414),
 'groups_2_2_1': ('a1e304ace7637db3', 364),
 'device_busy': ('8806195ab594a12c', 165),
 'device_busy_four': ('77333c6b0e04dcc0', 166),
 'device_busy_all_main': ('8b92689fda9a1b9f', 125),
 'compactions': ('1364bf4a8a50f7f8', 245),
 'waits_1': ('bbd453d62a97efba', 118),
 'waits_6': ('2e85ad87de9722b2', 358),
 'waits_16': ('af33518b342ea87d', 622),
 'waits_compactions_groups': ('2e3b39f51b35ceee', 505),
 'update_throws_run_0_after_0': ('db71cb7117ddf253', 123),
 'update_throws_run_0_after_1': ('633b5daf339dcb25', 140),
 'update_throws_run_2_after_0': ('3fc23eabd05c61d1', 123),
 'update_throws_run_2_after_1': ('fffaadadc2a6bc13', 140),
 'update_throws_run_4_after_0': ('ae0bdef0836381ab', 123),
 'update_throws_run_4_after_1': ('e3a2f0e85491929d', 140),
 'update_throws_outside_a_fiber': ('67a85e44e1ace349', 136),
 'update_throws_with_an_ending_under_way': ('9bf8dd91c0a3c719', 163),
 'setup_fails_run_0_how_1': ('18a8d2ef6276aeb9', 32),
 'setup_fails_run_0_how_2': ('cdbd1052c21adb00', 32),
 'setup_fails_run_0_how_3': ('18a8d2ef6276aeb9', 32),
 'setup_no_memory_run_3': ('c6d789855c0ac960', 319),
 'setup_no_memory_twice': ('9d644f72d3f2f2a9', 416),
 'setup_fails_run_2_how_2': ('a66aafe57a6b1e9e', 40),
 'setup_fails_run_2_how_3': ('8ba9645143521ba3', 293),
 'begin_returns_0': ('66a9041a54fc6d83', 44),
 'begin_returns_5': ('0bfe6c0f08825ac1', 44),
 'a_run_fails_in_a_round': ('1374f5b72643cf4f', 127),
 'a_run_fails_as_another_ends': ('8e3179a659f9fdc9', 137),
 'results_fail_code': ('0ed46f718ba3de72', 185),
 'results_fail_thrown': ('32758982542d0de6', 185),
 'ending_batch_of_12': ('145d277bd35edec6', 236),
 'group_1_noside': ('1e81cb4587078917', 65),
 'group_2_noside': ('c1cf9e43bbb1777e', 94),
 'group_5_noside': ('58783836f1cb5e3a', 180),
 'group_64_noside': ('5f702c8018c8fc59', 1121),
 'groups_3_3_1_noside': ('c21d269d0cbb87fc', 326),
 'groups_2_2_1_noside': ('d143b482415f10ed', 284),
 'device_busy_noside': ('51f86d31f77b1da3', 134),
 'device_busy_four_noside': ('f18ce2e8056ceab2', 135),
 'device_busy_all_main_noside': ('c3128150512dfeee', 98),
 'compactions_noside': ('c100931ba7bfdeef', 217),
 'waits_1_noside': ('5074c10e85642324', 94),
 'waits_6_noside': ('0acc8a5b032290ba', 318),
 'waits_16_noside': ('e78950e7642a700f', 582),
 'waits_compactions_groups_noside': ('a95030cdb3ecf38c', 441),
 'update_throws_run_0_after_0_noside': ('46f0b05beea40cea', 103),
 'update_throws_run_0_after_1_noside': ('ca495963cc534f46', 120),
 'update_throws_run_2_after_0_noside': ('52a1ab207f385ea0', 103),
 'update_throws_run_2_after_1_noside': ('98c6eba8bd7dc75c', 120),
 'update_throws_run_4_after_0_noside': ('4d0512f8f3dc0a12', 103),
 'update_throws_run_4_after_1_noside': ('72baa52627fd32ee', 120),
 'update_throws_outside_a_fiber_noside': ('ad9404d7e7d557b6', 116),
 'update_throws_with_an_ending_under_way_noside': ('3bb6c861c0aae609', 139),
 'setup_fails_run_0_how_1_noside': ('d36c0d1e3d7a0d82', 20),
 'setup_fails_run_0_how_2_noside': ('cabee76a398ebfb1', 20),
 'setup_fails_run_0_how_3_noside': ('d36c0d1e3d7a0d82', 20),
 'setup_no_memory_run_3_noside': ('3b5318bf9ef22b44', 255),
 'setup_no_memory_twice_noside': ('1ba7739f0cfbf98b', 328),
 'setup_fails_run_2_how_2_noside': ('c7b03d435d281ea9', 28),
 'setup_fails_run_2_how_3_noside': ('c834c0a9166d8e50', 233),
 'begin_returns_0_noside': ('d6c987cc4a3dbdf2', 32),
 'begin_returns_5_noside': ('240c45f52fe586a8', 32),
 'a_run_fails_in_a_round_noside': ('b09e8fead66a9cd3', 103),
 'a_run_fails_as_another_ends_noside': ('9adf721680587ef5', 113),
 'results_fail_code_noside': ('a1b506585498bb7d', 157),
 'results_fail_thrown_noside': ('59aebc5f8427fac7', 157),
 'ending_batch_of_12_noside': ('7a984e18c1112400', 212),
 'group_1_nocopystreams': ('94a72fcf67e84e92', 79),
 'group_2_nocopystreams': ('7a9541ca2baf6b14', 112),
 'group_5_nocopystreams': ('9ebfaa1774ffe886', 210),
 'group_64_nocopystreams': ('9af9dd760908bc6d', 1151),
 'groups_3_3_1_nocopystreams': ('1c4ad358cf306d74', 384),
 'groups_2_2_1_nocopystreams': ('7e4cffc48da81813', 334),
 'device_busy_nocopystreams': ('b61717e83b289b30', 155),
 'device_busy_four_nocopystreams': ('920575110e016be2', 156),
 'device_busy_all_main_nocopystreams': ('cb23c6416133ffb6', 115),
 'compactions_nocopystreams': ('8a3a3c37383f5b43', 235),
 'waits_1_nocopystreams': ('4a3319e161331838', 108),
 'waits_6_nocopystreams': ('73129bceb30ab122', 348),
 'waits_16_nocopystreams': ('bb2d217b4c617a1b', 612),
 'waits_compactions_groups_nocopystreams': ('9dc242fbc734fa48', 485),
 'update_throws_run_0_after_0_nocopystreams': ('0c9f4b8a57081de2', 113),
 'update_throws_run_0_after_1_nocopystreams': ('8369e4332d70d58a', 130),
 'update_throws_run_2_after_0_nocopystreams': ('405a9c15de723e3c', 113),
 'update_throws_run_2_after_1_nocopystreams': ('d64ef10b11813934', 130),
 'update_throws_run_4_after_0_nocopystreams': ('9f1df2b727d9f52a', 113),
 'update_throws_run_4_after_1_nocopystreams': ('f3ee07e9e8cfb902', 130),
 'update_throws_outside_a_fiber_nocopystreams': ('88ac06b5631102bc', 126),
 'update_throws_with_an_ending_under_way_nocopystreams': ('2447e6a41b5f1c5b', 153),
 'setup_fails_run_0_how_1_nocopystreams': ('3b19638008858c1e', 22),
 'setup_fails_run_0_how_2_nocopystreams': ('9f4ff8c2c8c25167', 22),
 'setup_fails_run_0_how_3_nocopystreams': ('3b19638008858c1e', 22),
 'setup_no_memory_run_3_nocopystreams': ('8e768577cf0adbaa', 299),
 'setup_no_memory_twice_nocopystreams': ('c2b23c4be4e5e899', 386),
 'setup_fails_run_2_how_2_nocopystreams': ('e6c7bd1c91f43c95', 30),
 'setup_fails_run_2_how_3_nocopystreams': ('8d490ad566fa3126', 273),
 'begin_returns_0_nocopystreams': ('9d5a743e4054e71a', 34),
 'begin_returns_5_nocopystreams': ('9a3292d99032ff0c', 34),
 'a_run_fails_in_a_round_nocopystreams': ('f127d8e0db2af39f', 117),
 'a_run_fails_as_another_ends_nocopystreams': ('ef5adac3a818369b', 127),
 'results_fail_code_nocopystreams': ('6e6dd92e604cf2c1', 175),
 'results_fail_thrown_nocopystreams': ('2b0f2b12a28cd6cb', 175),
 'ending_batch_of_12_nocopystreams': ('139f63b4d7fdbcc4', 226),
 'group_1_nofibers': ('a40ba5b3a4708876', 91),
 'group_2_nofibers': ('cb80420b25319414', 122),
 'group_5_nofibers': ('5cc01d70361e97b6', 220),
 'group_64_nofibers': ('8f70e083d5289a9d', 1161),
 'groups_3_3_1_nofibers': ('506e72643f63025a', 414),
 'groups_2_2_1_nofibers': ('a1e304ace7637db3', 364),
 'device_busy_nofibers': ('8806195ab594a12c', 165),
 'device_busy_four_nofibers': ('77333c6b0e04dcc0', 166),
 'device_busy_all_main_nofibers': ('8b92689fda9a1b9f', 125),
 'compactions_nofibers': ('1364bf4a8a50f7f8', 245),
 'waits_1_nofibers': ('bbd453d62a97efba', 118),
 'waits_6_nofibers': ('abcfc267ed4dc751', 400),
 'waits_16_nofibers': ('a61f7a1825812859', 818),
 'waits_compactions_groups_nofibers': ('a614c669e10ec2d9', 526),
 'update_throws_run_0_after_0_nofibers': ('4bc64031240742df', 115),
 'update_throws_run_0_after_1_nofibers': ('209ca2c7f271f63d', 124),
 'update_throws_run_2_after_0_nofibers': ('d094ad732a10b09a', 153),
 'update_throws_run_2_after_1_nofibers': ('e70cf52f0924c1c2', 162),
 'update_throws_run_4_after_0_nofibers': ('80e0d93f78f082db', 191),
 'update_throws_run_4_after_1_nofibers': ('60c7248521521e75', 200),
 'update_throws_outside_a_fiber_nofibers': ('80b57c81cd4e1643', 153),
 'update_throws_with_an_ending_under_way_nofibers': ('bd82fde93f19a3a4', 170),
 'setup_fails_run_0_how_1_nofibers': ('18a8d2ef6276aeb9', 32),
 'setup_fails_run_0_how_2_nofibers': ('cdbd1052c21adb00', 32),
 'setup_fails_run_0_how_3_nofibers': ('18a8d2ef6276aeb9', 32),
 'setup_no_memory_run_3_nofibers': ('c6d789855c0ac960', 319),
 'setup_no_memory_twice_nofibers': ('9d644f72d3f2f2a9', 416),
 'setup_fails_run_2_how_2_nofibers': ('a66aafe57a6b1e9e', 40),
 'setup_fails_run_2_how_3_nofibers': ('8ba9645143521ba3', 293),
 'begin_returns_0_nofibers': ('66a9041a54fc6d83', 44),
 'begin_returns_5_nofibers': ('0bfe6c0f08825ac1', 44),
 'a_run_fails_in_a_round_nofibers': ('1374f5b72643cf4f', 127),
 'a_run_fails_as_another_ends_nofibers': ('8e3179a659f9fdc9', 137),
 'results_fail_code_nofibers': ('0ed46f718ba3de72', 185),
 'results_fail_thrown_nofibers': ('32758982542d0de6', 185),
 'ending_batch_of_12_nofibers': ('145d277bd35edec6', 236)
}

REBUILD = ("For the two texts: git show b330d9b:polychordlite_amd/csrc/pc_engine.hip | sed -n 2715,2999p > /tmp/parent_step.inc; "
           "make -C polychordlite_amd/csrc step_record step_record_parent STEP_PARENT='\"/tmp/parent_step.inc\"'; "
           "tools/dev/step_record_parent --dump > parent.txt (its lines without --dump are the PARENT table of this file, with the variant's "
           "switch in the environment); tools/dev/step_record --dump > new.txt; diff parent.txt new.txt")


def _env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PC_")}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def recorded():
    """the recorder's digests and its records by scenario, all variants.  Built host-only (seconds) from the headers alone -- the variant that
    drives an older pc_run_many is another binary --; a missing hipcc fails the test, it does not skip it"""
    subprocess.run(["make", "-C", CSRC, "step_record"], check=True, capture_output=True, text=True)
    digests, texts = {}, {}
    for extra in VARIANTS.values():
        out = subprocess.run([BINARY], check=True, capture_output=True, text=True, env=_env(extra)).stdout
        mine = {name: (digest, int(lines)) for name, digest, lines in (line.split() for line in out.splitlines())}
        name = None
        for line in subprocess.run([BINARY, "--dump"], check=True, capture_output=True, text=True, env=_env(extra)).stdout.splitlines():
            w = line.split()
            if len(w) == 3 and w[0] in mine and mine[w[0]] == (w[1], int(w[2])):
                name = w[0]; texts[name] = []
            else:
                texts[name].append(line)
        digests.update(mine)
    assert set(texts) == set(digests) and all(len(texts[n]) == digests[n][1] for n in texts)
    return digests, texts


def test_the_driver_does_what_the_parent_did(recorded):
    digests, _ = recorded
    assert set(digests) == set(PARENT)
    differ = sorted(n for n in PARENT if digests[n] != PARENT[n])
    assert not differ, "scenarios %s differ from b330d9b.  %s" % (differ, REBUILD)


def test_the_sweep_reaches_every_path_of_the_driver(recorded):
    """what the scenarios are there for does occur in their records"""
    _, texts = recorded
    def has(name, *whats):
        text = "\n".join(texts[name])
        for what in whats:
            assert re.search(what, text, re.M), (name, what)
    has("group_64", r"^launch apply_many records 0\+64 ", r"^ending thread waits e", r"^run 63 destroyed")
    has("groups_3_3_1", r"^run 6 set up", r"^the call returns 0; results: 1 2 3 4 5 6 7$")
    assert sum(1 for l in texts["groups_3_3_1"] if l.startswith("classes held on the device:")) == 3
    has("device_busy", r"^classes held on the device: 1 2$", r"^a stream avoiding classes 1 2 0 \(known ones only\)$")
    has("device_busy_four", r"^classes held on the device by main streams: 1 3$")
    has("compactions", r"^launch clean_many records 0\+3 ", r"^rows in use 1004 to the host", r"^run 3 compacted to 1003 rows$")
    has("waits_6", r"^run 3 reads back what wait 0 was for$", r"^query s\d+$", r"^run 4 resumed$")
    has("waits_6_nofibers", r"^run 3 reads back what wait 0 was for$", r"^query s\d+$")
    for who in (0, 2, 4):
        has("update_throws_run_%d_after_1" % who, r"^run %d throws$" % who, r"^run %d cancelled$" % (who - 1 if who else 1), r"^the call returns 2; results: 0 0 0 0 0$")
        assert not any("cancelled" in l for l in texts["update_throws_run_%d_after_1_nofibers" % who])
    # (nothing a cancelled fiber had written down is left for a later flush)
    assert all(l.endswith("written down: 0 records, 0 closures, 0 copies") for n in texts if n.startswith("update_throws") for l in texts[n] if " destroyed" in l and "written down" in l)
    has("setup_fails_run_0_how_1", r"^the call returns 7; ")
    has("setup_no_memory_run_3", r"^run 3 set-up fails$", r"^the call returns 0; results: 1 2 3 4 5 6$")
    has("setup_fails_run_2_how_2", r"^the call returns 2; results: 0 0 0 0 0$")
    has("begin_returns_5", r"^the call returns 5; ")
    has("begin_returns_0", r"^the call returns 2; ")
    has("a_run_fails_in_a_round", r"^run 2 fails with its own code$", r"^the call returns 8; ")
    has("results_fail_code", r"^result of run 1 freed$", r"^the call returns 7; results: 1 0 3 4 5 6$")
    has("results_fail_thrown", r"^the call returns 2; results: 1 0 3 4 5 6$")
    for name, lines in texts.items():
        assert lines[-1] == "not given back: 0 streams, 0 events, 0 classes", name


def test_a_failing_event_pool_while_the_streams_are_picked_is_a_return_code():
    """the event pool throws at its Nth request inside pick_streams(), for each N that phase makes (two: the second stream's events): the call
    returns PC_RC_DEVICE (2), every stream and event taken by then is given back, the lease on the hardware-queue classes released.  (The parent
    had this stretch outside its handlers: the exception left through extern "C" and ended the process.)"""
    subprocess.run(["make", "-C", CSRC, "step_record"], check=True, capture_output=True, text=True)
    out = subprocess.run([BINARY, "--gap"], check=True, capture_output=True, text=True, env=_env({})).stdout.splitlines()
    assert out == ["gap %d of 2: rc 2, not given back: 0 streams, 0 events, 0 classes" % n for n in (1, 2)], out
    out = subprocess.run([BINARY, "--gap"], check=True, capture_output=True, text=True, env=_env({"PC_COHORT_COPY_STREAMS": "0"})).stdout.splitlines()
    assert out == ["gap %d of 2: rc 2, not given back: 0 streams, 0 events, 0 classes" % n for n in (1, 2)], out
