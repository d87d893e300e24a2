"""One line per run of tools/host_share.sh (value, ms per step, the sweep's device ms, the gap between the two, and with
HGIBBS_TIMING=1 the mean of every line of the breakdown over the timed iterations), then per figure the median and range of
the parent and of this tree.  usage: host_share_fold.py OUT_DIR [PAIRS]"""
import glob, json, os, re, statistics as st, sys
O = sys.argv[1]
PAIRS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
def runs(tag, c, timing):
    out = []
    for i in range(1, PAIRS + 1):
        p = os.path.join(O, "%s_%s_%s%d.json" % (tag, c, "t_" if timing else "", i))
        if not os.path.exists(p):
            continue
        d = json.load(open(p))
        row = {"value": d["value"], "ms": d["ms_per_step"], "sweep": d["roofline"]["sweep_ms_per_iter"]}
        row["gap"] = row["ms"] - row["sweep"]
        if timing:
            err = open(p[:-5] + ".err").read()
            keys = {}
            its = re.findall(r"iteration (\d+): mu ([\d.]+)  shuffle ([\d.]+)  sweep call ([\d.]+)  beta sqnorm ([\d.]+)  hyper-parameters \+ sigmaE ([\d.]+)", err)
            its = [t for t in its if int(t[0]) >= 2]  # the timed iterations
            for j, name in enumerate(["mu", "shuffle", "sweep call", "beta sqnorm", "hyper"]):
                keys[name] = st.mean(float(t[j + 1]) for t in its)
            prep = re.findall(r"sweep preparation.*?([\d.]+) ms(?:, wait for uploads, metadata gather and opening reduction ([\d.]+) ms)?", err)[2:]
            keys["prep"] = st.mean(float(a) + (float(b) if b else 0.0) for a, b in prep)
            old = re.findall(r"host until the kernel is back ([\d.]+) ms \(device ([\d.]+)\), results \+ drift ([\d.]+)", err)[2:]
            new = re.findall(r"launch preparation ([\d.]+) ms, kernel wait ([\d.]+) ms \(device ([\d.]+)\), results \+ drift ([\d.]+)", err)[2:]
            if old:
                keys["launch+wait-device"] = st.mean(float(a) - float(b) for a, b, c_ in old)
                keys["results+drift"] = st.mean(float(c_) for a, b, c_ in old)
            if new:
                keys["launch+wait-device"] = st.mean(float(a) + float(b) - float(c_) for a, b, c_, d_ in new)
                keys["results+drift"] = st.mean(float(d_) for a, b, c_, d_ in new)
            row.update(keys)
        out.append(row)
    return out
for c in ("c4", "c3", "c2"):
    for timing in (False, True):
        P, R = runs("parent", c, timing), runs("result", c, timing)
        if not P:
            continue
        print("== %s%s" % (c, " (HGIBBS_TIMING=1)" if timing else ""))
        for tag, rows in (("parent", P), ("result", R)):
            for i, r in enumerate(rows):
                print("  %s run %d: " % (tag, i + 1) + "  ".join("%s %.3f" % (k, v) if k != "value" else "value %.0f" % v for k, v in r.items()))
        for k in P[0]:
            p, r = [x[k] for x in P], [x[k] for x in R]
            print("  %-20s parent median %.3f (min %.3f max %.3f)   result median %.3f (min %.3f max %.3f)" % (k, st.median(p), min(p), max(p), st.median(r), min(r), max(r)))
