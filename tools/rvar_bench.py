"""Throughput of hgibbs_region_var on a synthetic cohort made in HBM (hgibbs_synth_bed), beside the same
job's score pass on the same handle.

For N individuals x M markers, S weight vectors, windows of W consecutive markers and the set of all markers: device time of one
hgibbs_region_var call with the windows and ALL, with the windows alone (the bytes of one score pass) and with ALL alone, and of one
hgibbs_score call for the same weights (every kernel of each call; HIP events); GB/s of BED read per pass over the codes and the
ratios to the score.  One JSON line per case, appended to --out when given.

    python tools/rvar_bench.py [--n 100000] [--m 1000000] [--samples 1,16,128] [--window 400] [--reps 3] [--out profiles/rvar_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--samples", default="1,16,128")
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--missing", default="0.01")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    rng = np.random.default_rng(1)
    windows = [np.arange(j, min(j + args.window, args.m)) for j in range(0, args.m, args.window)]
    everything = [np.arange(args.m)]
    bed_bytes = args.m * ((args.n + 3) // 4)
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(args.n, args.m, seed=5, missing_rate=miss)
        for S in [int(x) for x in args.samples.split(",")]:
            a = rng.standard_normal((S, args.m)) * 1e-3
            o = -a * 0.5
            dev.score(a[:1], o[:1])  # warm-up of the code objects
            dev.region_var(a[:1], o[:1], windows[:2])

            def timed(call, last):
                ms = []
                for _ in range(args.reps):
                    out = call()
                    ms.append(last())
                return float(np.median(ms)), out

            score_ms, _ = timed(lambda: dev.score(a, o), dev.last_score_ms)
            both_ms, both = timed(lambda: dev.region_var(a, o, windows + everything), dev.last_region_var_ms)
            win_ms, win = timed(lambda: dev.region_var(a, o, windows), dev.last_region_var_ms)
            all_ms, alone = timed(lambda: dev.region_var(a, o, everything), dev.last_region_var_ms)
            same = bool(np.array_equal(both[1][:-1], win[1]) and np.array_equal(both[1][-1:], alone[1]))
            passes = -(-S // 8)
            emit({"n": args.n, "m": args.m, "S": S, "missing": miss, "sets": len(windows), "window": args.window,
                  "score_ms": round(score_ms, 3), "rvar_windows_and_all_ms": round(both_ms, 3), "rvar_windows_ms": round(win_ms, 3),
                  "rvar_all_ms": round(all_ms, 3), "ratio_windows_and_all": round(both_ms / score_ms, 3),
                  "ratio_windows": round(win_ms / score_ms, 3), "ratio_all": round(all_ms / score_ms, 3),
                  "score_bed_read_gbps": round(passes * bed_bytes / (score_ms * 1e-3) / 1e9, 1),
                  "rvar_windows_bed_read_gbps": round(passes * bed_bytes / (win_ms * 1e-3) / 1e9, 1),
                  "ms_per_sample_windows_and_all": round(both_ms / S, 4), "same_in_parts": same})
        dev.close()


if __name__ == "__main__":
    main()
