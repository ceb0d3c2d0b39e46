# where the dead rows' copies lie against k_slice and the update in a rocprofv3 trace of bench.py (profiles/dead_rows.json):
#   rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -o p --output-format csv -- python bench.py --steps 4 --warmup 1
# usage: trace_dead_rows.py DIR   (finds *kernel_trace.csv and *memory_copy_trace.csv below DIR; prints one JSON object)
import csv, glob, json, os, re, sys

d = sys.argv[1]
find = lambda pat: sorted(glob.glob(os.path.join(d, "**", pat), recursive=True))[0]
short = lambda n: re.sub(r"\(.*", "", re.sub(r"^void ", "", n))
K = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in csv.DictReader(open(find("*kernel_trace.csv"))))
# (copies to pinned memory are the runtime's own kernel __amd_rocclr_copyBuffer in the kernel trace, the others rows of the copy trace; neither
#  has byte counts, so a copy is told by its length -- the loop's dead rows, 3 MB and more, last 40 us and more; the live rows, the weights
#  and the birth contours of the tail, 0.5 - 0.7 MB, 12 - 25 us; control blocks 2 - 6 us)
C = sorted([(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Direction"]) for r in csv.DictReader(open(find("*memory_copy_trace.csv")))]
           + [(s, e, "KERNEL_DEVICE_TO_HOST") for s, e, n in K if n == "__amd_rocclr_copyBuffer"])
K = [k for k in K if not k[2].startswith("__amd_rocclr")]
LONG, MID = 40000, 8000      # ns
us = lambda ns: round(ns / 1e3, 2)
stat = lambda v: {"n": len(v), "mean": round(sum(v) / len(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} if v else {"n": 0}
is_slice = lambda n: n.startswith("k_slice")
sl = [(s, e) for s, e, n in K if is_slice(n)]
dur = [us(e - s) for s, e in sl]
out = {"k_slice": {"launches": len(dur), "over_80us": stat([x for x in dur if x > 80.0]), "others": stat([x for x in dur if x <= 80.0]),
                   "sum_ms": round(sum(dur) / 1e3, 3)}}
# copies of the loop's dead rows to the host: the kernels that run while each is on its way
big = [c for c in C if c[1] - c[0] > LONG and c[2].endswith("DEVICE_TO_HOST")]
beside = {}
rows = []
for cs, ce, _ in big:
    ov = {}
    for s, e, n in K:
        if e <= cs or s >= ce: continue
        ov[n] = ov.get(n, 0) + min(e, ce) - max(s, cs)
    rows.append({"us": us(ce - cs), "beside_us": {n: us(t) for n, t in ov.items()}})
    for n in ov: beside[n] = beside.get(n, 0) + 1
out["d2h_over_40us"] = {"n": len(big), "us": stat([us(ce - cs) for cs, ce, *_ in big]), "copies_that_overlap_a_launch_of": beside, "each": rows}
# the update's span: its first kernel's start to the next k_slice's start, with and without a big copy inside
# (an update starts at k_upd_flag, or at k_upd_index_self where the flags came with the row kernel's launch: k_apply_pool_flag)
upd_first = [s for i, (s, e, n) in enumerate(K) if n.startswith("k_upd_flag") or (n.startswith("k_upd_index_self") and not (i and K[i - 1][2].startswith("k_upd_flag")))]
spans = {"copy_beside": [], "no_copy": []}
for u in upd_first:
    nxt = next((s for s, e in sl if s > u), None)
    if nxt is None: continue
    spans["copy_beside" if any(cs < nxt and ce > u for cs, ce, *_ in big) else "no_copy"].append(us(nxt - u))
out["update_span_us"] = {k: stat(v) for k, v in spans.items()}
# the k_slice behind each update, by whether a big copy overlaps it
ks = {"copy_beside": [], "no_copy": []}
for u in upd_first:
    nx = next(((s, e) for s, e in sl if s > u), None)
    if nx: ks["copy_beside" if any(cs < nx[1] and ce > nx[0] for cs, ce, *_ in big) else "no_copy"].append(us(nx[1] - nx[0]))
out["k_slice_behind_an_update_us"] = {k: stat(v) for k, v in ks.items()}
# the row kernel (with or without the flag pass in its launch), and the update: launches from its first kernel up to the next k_slice
out["row_kernel_us"] = {nm: stat([us(e - s) for s, e, n in K if n == nm]) for nm in sorted({n for s, e, n in K if n.startswith("k_apply_pool")})}
per_upd = []
for u in upd_first:
    nxt = next((s for s, e in sl if s > u), None)
    if nxt is not None: per_upd.append(sum(1 for s, e, n in K if u <= s < nxt))
out["launches_per_update"] = stat(per_upd)
out["d2h_over_40us_not_behind_a_killoff"] = sum(1 for cs, ce, _ in big if not any(fs <= cs < fs + 500000 for fs, fe, n in K if n.startswith("k_final_par")))
for name in ("k_final_par", "k_final_par_whole", "k_final_rows"):
    out[name + "_us"] = stat([us(e - s) for s, e, n in K if n == name])
# the tail: the kill-off's start to the end of the last copy of the chain of copies to the host behind it (rows, weights, birth contours: 8 us
# or more each, none starting more than 150 us behind the end of what came before; the merge of the run's records follows much later)
fin = [(s, e) for s, e, n in K if n.startswith("k_final_par")]
tail = []
for fs, fe in fin:
    t = fe
    for cs, ce, dr in C:
        if cs < fs or ce - cs <= MID or not dr.endswith("DEVICE_TO_HOST"): continue
        if cs > t + 150000: break
        t = max(t, ce)
    tail.append(us(t - fs))
out["killoff_start_to_last_copy_end_us"] = stat(tail)
print(json.dumps(out, indent=1))
