"""dev: a rocprofv3 kernel trace of `bench.py --gpus 1 --steps 4 --warmup 1` (`rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
python bench.py ...`) read for the side-stream bases launch of a run on its own -> JSON on stdout (profiles/bases_wave.json, bases_wave4.json):
the bases launch, k_slice, k_consume_par and k_apply_pool_flag (calls, average, min, max, median in us), the bases launches that have not ended
when the next k_slice starts and by how much, and k_consume_par / k_slice by whether a bases launch ran beside them, with a straight-line fit
of duration against microseconds of overlap.      python tools/dev/trace_bases.py DIR"""
import csv, glob, json, statistics, sys

BASES = ("k_nhats_w<", "k_nhats<")


def stats(d):
    return {"calls": len(d), "avg_us": round(sum(d) / len(d), 2), "min_us": round(min(d), 2), "max_us": round(max(d), 2),
            "median_us": round(statistics.median(d), 2)} if d else {"calls": 0}


def fit(xs, ys):
    n = len(xs)
    if n < 2 or max(xs) == min(xs):
        return None, None
    mx, my = sum(xs) / n, sum(ys) / n
    b = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    return round(b, 3), round(my - b * mx, 2)


def against(rows, bases):
    """rows of one kernel against the bases launches: overlap in us per launch"""
    ov = []
    for s, e in rows:
        ov.append(sum(max(0.0, min(e, be) - max(s, bs)) for bs, be in bases if bs < e and be > s))
    dur = [e - s for s, e in rows]
    w = [(o, d) for o, d in zip(ov, dur) if o > 0]
    wo = [d for o, d in zip(ov, dur) if o == 0]
    b, a = fit([o for o, _ in w], [d for _, d in w])
    return {"with_overlap": len(w), "without": len(wo), "avg_us_with_overlap": round(sum(d for _, d in w) / len(w), 2) if w else None,
            "avg_overlap_us": round(sum(o for o, _ in w) / len(w), 2) if w else None,
            "avg_us_without_overlap": round(sum(wo) / len(wo), 2) if wo else None, "fit_us_per_us_of_overlap": b, "fit_us_at_zero_overlap": a}


def main(d):
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))
    rows = list(csv.DictReader(open(f[-1])))
    k = {}
    for r in rows:
        k.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3))
    pick = lambda pred: sorted(x for n, v in k.items() if pred(n) for x in v)
    bases = pick(lambda n: any(b in n for b in BASES) and ", 2>" not in n)
    sl = pick(lambda n: "k_slice" in n and "k_slice_t" not in n)
    cp, ap = pick(lambda n: "k_consume_par" in n), pick(lambda n: "k_apply_pool_flag" in n)
    out = {"bases": stats([e - s for s, e in bases]), "k_slice": stats([e - s for s, e in sl]), "k_consume_par": stats([e - s for s, e in cp]),
           "k_apply_pool_flag": stats([e - s for s, e in ap]),
           "bases_kernel_names": {n[:60]: len(v) for n, v in k.items() if any(b in n for b in BASES) and ", 2>" not in n}}
    over = []
    starts = [s for s, _ in sl]
    import bisect
    for bs, be in bases:
        j = bisect.bisect_right(starts, bs)
        if j < len(starts) and starts[j] < be:
            over.append(be - starts[j])
    out["bases_running_at_next_k_slice"] = {"count": len(over), "of": len(bases), "avg_overrun_us": round(sum(over) / len(over), 2) if over else 0.0,
                                            "max_overrun_us": round(max(over), 2) if over else 0.0}
    out["k_consume_par_against_bases_overlap"] = against(cp, bases)
    out["k_slice_against_bases_overlap"] = against(sl, bases)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
