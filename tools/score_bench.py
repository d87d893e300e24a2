"""Scoring throughput of hgibbs_score on a synthetic target made in HBM (hgibbs_synth_bed).

For N individuals x M markers, S weight vectors and missing-call rates 0 and 1 %: device time of one call (every kernel of it,
scales to rounded result; HIP events), GB/s of BED read (M x N / 4 bytes over that time), its fraction of the measured copy
ceiling (hgibbs_stream_ceiling: bytes read + written) and ms per sample.  --sp also times every samples-per-pass setting.
One JSON line per case.

    python tools/score_bench.py [--n 100000] [--m 1000000] [--samples 1,16,128] [--reps 3] [--sp]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--samples", default="1,16,128")
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sp", action="store_true", help="also time score_sp = 2, 4, 8, 16")
    args = ap.parse_args()
    probe = capi.Device(0)
    ceiling = probe.stream_ceiling(2 << 30, 10)
    probe.close()
    print(json.dumps({"copy_ceiling_gbps": round(ceiling, 1)}), flush=True)
    rng = np.random.default_rng(1)
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(args.n, args.m, seed=5, missing_rate=miss)
        bed_bytes = args.m * ((args.n + 3) // 4)
        for S in [int(x) for x in args.samples.split(",")]:
            a = rng.standard_normal((S, args.m)) * 1e-3
            o = -a * 0.5
            sps = [0] + ([2, 4, 8, 16] if args.sp else [])
            ref = None
            for sp in sps:
                dev.set_option("score_sp", sp)
                dev.score(a[:1], o[:1])  # warm-up of the code objects
                dev_ms, wall = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    out = dev.score(a, o)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    dev_ms.append(dev.last_score_ms())
                if ref is None:
                    ref = out
                ms = float(np.median(dev_ms))
                gbps = bed_bytes / (ms * 1e-3) / 1e9
                print(json.dumps({"n": args.n, "m": args.m, "S": S, "missing": miss, "score_sp": sp or "auto",
                                  "device_ms": round(ms, 3), "device_ms_all": [round(x, 3) for x in dev_ms],
                                  "call_ms": round(float(np.median(wall)), 1), "bed_read_gbps": round(gbps, 1),
                                  "frac_of_copy_ceiling": round(gbps / ceiling, 3), "ms_per_sample": round(ms / S, 4),
                                  "same_as_auto": bool(np.array_equal(out, ref))}), flush=True)
            dev.set_option("score_sp", 0)
        dev.close()


if __name__ == "__main__":
    main()
