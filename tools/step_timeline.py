#!/usr/bin/env python3
"""Condense a rocprofv3 --kernel-trace --hip-runtime-trace run of bench.py into the headline step's timeline.

    rocprofv3 --kernel-trace --hip-runtime-trace --stats --output-format csv -d OUT -o trace -- python bench.py --full --quick --steps 20
    python tools/step_timeline.py OUT/trace [--steps 4]

A step is one rbs_frame_prep_kernel / rbs_prep_kernel dispatch and the raster and copy kernels after it.  Prints the medians
over the last 100 steps of the run (the timed ones), then a few consecutive steps in full: every kernel's queue, start and end
relative to the step's prep, and the HIP runtime calls the host made in between."""
import argparse
import csv
import glob
import os
import statistics as st


def short(name):
    for k in ("rbs_frame_prep_kernel", "rbs_prep_kernel", "rbs_raster_kernel", "rbs_copy_window_kernel", "rbs_copy_rows_kernel"):
        if k in name:
            if k == "rbs_raster_kernel":
                return name[name.index("rbs_raster_kernel"):].split("(")[0]
            return k
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", help="the -d/-o prefix of the run, e.g. OUT/trace (reads <prefix>_kernel_trace.csv, <prefix>_hip_api_trace.csv)")
    ap.add_argument("--steps", type=int, default=4, help="consecutive steps printed in full")
    ap.add_argument("--tail", type=int, default=100, help="steps the medians are taken over (the last ones of the run)")
    a = ap.parse_args()
    kt = a.trace + "_kernel_trace.csv"
    if not os.path.exists(kt):
        kt = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    ht = kt.replace("kernel_trace.csv", "hip_api_trace.csv")
    ks = []
    for r in csv.DictReader(open(kt)):
        s = short(r["Kernel_Name"])
        if s:
            ks.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), s, int(r["Queue_Id"]), int(r["Stream_Id"]), int(r["Correlation_Id"])))
    ks.sort()
    api = []
    if os.path.exists(ht):
        for r in csv.DictReader(open(ht)):
            api.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"], int(r["Correlation_Id"])))
        api.sort()
    launch = {c: t0 for t0, _, _, c in api}   # correlation id -> when the host called the launch
    steps, cur = [], None
    for k in ks:
        if "prep" in k[2]:
            cur = {"prep": k, "raster": None, "copy": None}
            steps.append(cur)
        elif cur is not None:
            cur["raster" if k[2].startswith("rbs_raster") else "copy"] = k
    steps = [s for s in steps if s["raster"]]
    tail = steps[-a.tail:]
    us = lambda ns: ns / 1000.0   # noqa: E731
    print(f"# {len(steps)} steps in the trace ({len([s for s in steps if s['copy']])} with a copy kernel); medians over the last {len(tail)}")
    rows = []
    for i, s in enumerate(tail[:-1]):
        nxt = tail[i + 1]
        p, r, c = s["prep"], s["raster"], s["copy"]
        d = {"period": us(nxt["prep"][0] - p[0]), "prep": us(p[1] - p[0]), "prep_end->raster_start": us(r[0] - p[1]),
             "raster": us(r[1] - r[0]), "raster_end->next_prep_start": us(nxt["prep"][0] - r[1])}
        if r[5] in launch:
            d["raster_launch_call->raster_start"] = us(r[0] - launch[r[5]])
        if nxt["prep"][5] in launch:
            d["next_prep_launch_call->its_start"] = us(nxt["prep"][0] - launch[nxt["prep"][5]])
        if c:
            d.update({"copy": us(c[1] - c[0]), "copy_start-raster_start": us(c[0] - r[0]), "copy_end-raster_end": us(c[1] - r[1]),
                      "copy_end->next_prep_start": us(nxt["prep"][0] - c[1])})
        rows.append(d)
    keys = list(dict.fromkeys(k for d in rows for k in d))
    for k in keys:
        v = [d[k] for d in rows if k in d]
        print(f"{k:36s} median {st.median(v):9.2f} us   min {min(v):9.2f}   max {max(v):9.2f}   (n={len(v)})")
    kernels = sorted({(s[x][2], s[x][3], s[x][4]) for s in tail for x in ("prep", "raster", "copy") if s[x]})
    print("# kernels of these steps (name, hardware queue id, stream id):")
    for k in kernels:
        print(f"#   {k[0]}  queue {k[1]}  stream {k[2]}")
    print()
    show = tail[-a.steps - 1:]
    t0_ = show[0]["prep"][0]
    print(f"# {len(show) - 1} consecutive steps in full, us from the first prep's start.  GPU: kernel execution (hardware queue).  "
          "API: the HIP runtime calls the host made from the launch of the step's prep to the launch of the next prep")
    for i, s in enumerate(show[:-1]):
        nxt = show[i + 1]
        print(f"step {i}:")
        ev = []
        for x in ("prep", "raster", "copy"):
            if s[x]:
                k = s[x]
                ev.append((k[0], f"  GPU  {us(k[0] - t0_):9.2f} .. {us(k[1] - t0_):9.2f}  {k[2]}  (queue {k[3]}, {us(k[1] - k[0]):.2f} us)"))
        a0, a1 = launch.get(s["prep"][5]), launch.get(nxt["prep"][5])
        if a0 is not None and a1 is not None:
            for t0, t1, f, _ in api:
                if a0 <= t0 < a1:
                    ev.append((t0, f"  API  {us(t0 - t0_):9.2f} .. {us(t1 - t0_):9.2f}  {f}"))
        ev.sort()
        for _, line in ev:
            print(line)
        print(f"  gap raster end -> next prep start: {us(nxt['prep'][0] - s['raster'][1]):.2f} us")


if __name__ == "__main__":
    main()
