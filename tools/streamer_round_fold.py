#!/usr/bin/env python3
"""Every run of tools/streamer_round.sh as a table: markers/s, ms per step, the sweep's device ms and us per round of each bench.py
line (<tag>_<config>_<i>.json), the medians, the criterion of DESIGN.md section 8 (this tree's median at c4 above the parent's best
run; c3 and c2 not below the parent's medians), and the stage anatomy of both builds (<tag>_c4_anatomy_<i>.json).
usage: streamer_round_fold.py OUT_DIR"""
import glob
import json
import os
import statistics
import sys

O = sys.argv[1]
val = {}
for c in ("c4", "c3", "c2"):
    for tag in ("parent", "result"):
        rows = []
        for f in sorted(glob.glob(os.path.join(O, "%s_%s_[0-9]*.json" % (tag, c)))):
            d = json.load(open(f))
            r = d["roofline"]
            rows.append((d["value"] / 1e6, d["ms_per_step"], r["sweep_ms_per_iter"], r["us_per_round"]))
        if not rows:
            continue
        val[(c, tag)] = [x[0] for x in rows]
        print("%s %-6s markers/s (M): %s | ms per step: %s | sweep, device ms: %s | us per round: %s | median %.3f M" % (
            c, tag, ", ".join("%.3f" % x[0] for x in rows), ", ".join("%.1f" % x[1] for x in rows), ", ".join("%.1f" % x[2] for x in rows),
            ", ".join("%.2f" % x[3] for x in rows), statistics.median(x[0] for x in rows)))
if ("c4", "parent") in val and ("c4", "result") in val:
    m, b = statistics.median(val[("c4", "result")]), max(val[("c4", "parent")])
    print("c4: this tree's median %.3f M %s the parent's best run %.3f M (%+.1f %% on the medians)" % (
        m, "above" if m > b else "NOT above", b, 100.0 * (m / statistics.median(val[("c4", "parent")]) - 1.0)))
for c in ("c3", "c2"):
    if (c, "parent") in val and (c, "result") in val:
        m, pm = statistics.median(val[(c, "result")]), statistics.median(val[(c, "parent")])
        print("%s: this tree's median %.3f M %s the parent's median %.3f M" % (c, m, "not below" if m >= pm else "BELOW", pm))
for tag in ("parent", "result"):
    for f in sorted(glob.glob(os.path.join(O, "%s_c4_anatomy_*.json" % tag))):
        a = json.load(open(f))["roofline"]["anatomy_us"]
        s, w = a["streaming_workgroup0_us"], a["walker_us"]
        print("anatomy %-6s %s: period %.2f us | streaming: gram_terms %.2f update %.2f refill_dots %.2f barrier %.2f wait_for_message %.2f | walker: wait_for_gram_terms %.2f wait_for_raw_dots %.2f" % (
            tag, os.path.basename(f), a["period_us"], s["gram_terms"], s["update"], s["refill_dots"], s["barrier"], s["wait_for_message"],
            w["wait_for_gram_terms"], w["wait_for_raw_dots"]))
