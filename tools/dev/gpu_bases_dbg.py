"""dev: one run of the metric configuration on the NHATS_W_DBG build (PCHIP_LIB = libpolychord_hip_basesdbg.so, `make -C polychordlite_amd/csrc
../libpolychord_hip_basesdbg.so [BASES_DBG=1]`), the section counters of k_nhats_w read from the engine's PC_DEBUG=4 lines -> JSON on stdout.
Argument: settings.ablate (0: four wavefronts a workgroup, 1048576 = bit 20: one).  Sections (pc_bases.hip, k_nhats_w): 0 decks (one
wavefront a workgroup: wavefront 0, in front of everything; four: wavefront 1, behind the deviates), then wavefront 0's 1 deviates loop up to
its barrier, 2 tail pass, 3 loading v[], 4 PC_GS_PACKED, 5 stores; 6 wavefront 0 from start to end; 7 the workgroups counted (BASES_DBG=1:
workgroup 0 of every launch; 2: all of them)."""
import ctypes as C, json, os, re, subprocess, sys
sys.path.insert(0, ".")
if os.environ.get("BASES_DBG_CHILD") != "1":
    env = dict(os.environ, BASES_DBG_CHILD="1", PC_DEBUG="4")
    p = subprocess.run([sys.executable, __file__] + sys.argv[1:], env=env, capture_output=True, text=True)
    line = [l for l in p.stderr.splitlines() if "dbg par: stage+search" in l][-1]
    v = [int(x) for x in re.findall(r"(\d+)", line.split("stage+search")[1])][:7]
    n = int(re.findall(r"dbg par: (\d+) evidence scans", p.stderr)[-1])
    res = json.loads(p.stdout.strip().splitlines()[-1])
    names = ["decks", "deviates_loop", "tail_pass", "load_v", "gram_schmidt", "stores"]
    whole = v[6] / n
    out = {"workload": "BASELINE configs[1]: 20-D Gaussian, nlive 2000, num_repeats 40, B 1000", "ablate": res["ablate"], "workgroups_counted": n,
           "nurseries": res["nbatches"], "cycles_per_workgroup": {k: v[i] / n for i, k in enumerate(names)}, "cycles_per_workgroup_start_to_end": whole,
           "share_of_wavefront_0": {k: round(v[i] / v[6], 4) for i, k in enumerate(names)},
           "note": "clock64 (s_memtime) at the section boundaries; a section ends where the compiler leaves the read, so read the shares"}
    print(json.dumps(out, indent=1))
    sys.exit(0)
from polychordlite_amd import _ctypes_api as api
lib = api.load()
s = api.Settings(); lib.pchip_settings_default(C.byref(s), 20, 2)
s.nlive, s.num_repeats, s.seed = 2000, 40, 1002
s.ablate = int(sys.argv[1]) if len(sys.argv) > 1 else 0
L, P, keep = api.make_problem("gaussian", 20, 2)
r = api.run(s, L, P)
print(json.dumps({"nbatches": r["nbatches"], "ablate": s.ablate}))
