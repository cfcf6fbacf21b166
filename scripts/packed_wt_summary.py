#!/usr/bin/env python3
"""The packed step's two kernels and the boundaries between them, from three rocprofv3 runs of their own over bench.py:
    --kernel-trace                      over  bench.py --gpus 1 --steps 200 --warmup 10 --profile --no-cpu-baseline --no-abi
    --pmc FETCH_SIZE                    over  bench.py --steps 3 --warmup 1 --profile --no-cpu-baseline --no-abi
    --pmc WRITE_SIZE GRBM_GUI_ACTIVE    over  the same
(csv output, in DIR/trace, DIR/fetch, DIR/write).  From the trace's begin and end timestamps: the duration of each kernel and the two gaps,
end of encode to begin of decode and end of decode to begin of the next encode, over the launches that directly follow one another.
FETCH_SIZE and WRITE_SIZE count kilobytes; FETCH_SIZE is doubled (it under-reports by a factor of two on gfx950).
    python scripts/packed_wt_summary.py DIR [RUNS NAME] > profiles/packed_wt_parent.json
RUNS: a file of lines "NAME ms_per_step", one per un-profiled run of a timing session; those of NAME are added with their median and max - min."""
import csv
import glob
import json
import os
import statistics
import sys


def short(name):
    for k in ("rirb1_encode_packed", "rirb1_decode_packed"):
        if k in name:
            return k
    return None


def stats(v):
    v = sorted(v)
    return {"n": len(v), "median_us": round(statistics.median(v) / 1e3, 3), "mean_us": round(sum(v) / len(v) / 1e3, 3),
            "p10_us": round(v[len(v) // 10] / 1e3, 3), "p90_us": round(v[(len(v) * 9) // 10] / 1e3, 3)}


def main():
    root = sys.argv[1]
    rows = []
    for f in glob.glob(os.path.join(root, "trace", "*", "*kernel_trace.csv")):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    dur = {"rirb1_encode_packed": [], "rirb1_decode_packed": []}
    gaps = {"encode_end_to_decode_begin": [], "decode_end_to_next_encode_begin": []}
    for i, (b, e, k) in enumerate(rows):
        if k:
            dur[k].append(e - b)
        if i + 1 < len(rows):
            b2, _, k2 = rows[i + 1]
            if k == "rirb1_encode_packed" and k2 == "rirb1_decode_packed":
                gaps["encode_end_to_decode_begin"].append(b2 - e)
            if k == "rirb1_decode_packed" and k2 == "rirb1_encode_packed" and b2 - e < 50000:  # (a host synchronisation in between is no boundary)
                gaps["decode_end_to_next_encode_begin"].append(b2 - e)
    out = {"kernel_trace": {k: stats(v) for k, v in dur.items() if v}, "gaps": {k: stats(v) for k, v in gaps.items() if v}}
    cnt = {}
    for sub in ("fetch", "write"):
        for f in glob.glob(os.path.join(root, sub, "*", "*counter_collection.csv")):
            for r in csv.DictReader(open(f)):
                k = short(r["Kernel_Name"])
                if k:
                    cnt.setdefault(k, {}).setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    out["counters_per_launch"] = {}
    for k, cs in sorted(cnt.items()):
        o = {c: sum(v) / len(v) for c, v in sorted(cs.items())}
        o["_dispatches"] = len(next(iter(cs.values())))
        if "FETCH_SIZE" in o:
            o["fetch_MB (FETCH_SIZE x 1024 x 2)"] = round(o["FETCH_SIZE"] * 2048 / 1e6, 2)
        if "WRITE_SIZE" in o:
            o["write_MB (WRITE_SIZE x 1024)"] = round(o["WRITE_SIZE"] * 1024 / 1e6, 2)
        out["counters_per_launch"][k] = o
    for name in ("trace", "fetch", "write"):
        p = os.path.join(root, name + ".json")
        if os.path.exists(p) and name == "trace":
            try:
                out["bench_line_under_the_trace"] = json.loads(open(p).read().strip().splitlines()[-1])
            except Exception:
                pass
    if len(sys.argv) > 3:  # RUNS NAME: the lines "NAME ms_per_step" of the un-profiled runs of a timing session
        v = [float(l.split()[1]) for l in open(sys.argv[2]) if l.split() and l.split()[0] == sys.argv[3]]
        out["step_ms (bench.py --gpus 1 --steps 200 --warmup 10, un-profiled)"] = {"runs": v, "median": round(statistics.median(v), 5),
                                                                                     "max_minus_min": round(max(v) - min(v), 5)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
