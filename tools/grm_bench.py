"""Genomic relationship matrix throughput of hgibbs_grm on a synthetic BED made in HBM (hgibbs_synth_bed),
with hgibbs_king_pairs at the same shape in the same job as the yardstick.

For N individuals x M markers and missing-call rates 0 and 1 %: device time of the whole triangle (every kernel of the call: scale,
table, image, products, rounding; HIP events; the outputs stay on the device: both output pointers NULL), pair-markers per second
(N (N + 1) / 2 x M over the time; KING: N (N - 1) / 2 x M), and the fraction of the I8 MFMA rate (MI355X: 8192 i8 operations a clock
per CU, 256 CUs at 2.4 GHz: 2.52e15 multiply-adds/s) that the kernel issues: fifteen 16 x 16 x 64 products per tile pair ta >= tb and
k-step of 64 markers (KING: five), as section 15 computes it.  One JSON line per case and operator; --out appends them to a file.

    python tools/grm_bench.py [--n 40000] [--m 40000] [--missing 0,0.01] [--reps 2] [--ops grm,king] [--out profiles/grm_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402

I8_MACS = 256 * 2.4e9 * 8192 / 2  # multiply-adds per second at the I8 MFMA rate (2 operations each)
PRODUCTS = {"grm": 15, "king": 5}  # per tile pair and k-step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40000)
    ap.add_argument("--m", type=int, default=40000)
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--cutoff", type=float, default=0.0442)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ops", default="grm,king")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    N, M = args.n, args.m
    ntile = (N + 15) // 16
    nks = (M + 63) // 64
    tile_steps = ntile * (ntile + 1) // 2 * nks
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        dev.grm(0, 16)  # warm-up of the code objects
        dev.king(0, 16, 0, 16)
        for op in args.ops.split(","):
            times = []
            extra = {}
            for _ in range(args.reps):
                if op == "grm":
                    capi.check(dev.L.hgibbs_grm(dev.h, 0, N, None, None))
                    times.append(dev.last_grm_ms())
                    extra["m_used"], extra["E"] = dev.grm_info()
                else:
                    ab, _, _ = dev.king_pairs(args.cutoff)
                    times.append(dev.last_king_ms())
                    extra["pairs_listed"] = len(ab)
            ms = float(np.median(times))
            pairs = N * (N + 1) // 2 if op == "grm" else N * (N - 1) // 2
            issued = tile_steps * PRODUCTS[op] * 16 * 16 * 64  # multiply-adds of the products the kernel issues
            rec = {"op": op, "n": N, "m": M, "missing": miss, "device_ms": round(ms, 3), "device_ms_all": [round(x, 3) for x in times],
                   "pair_markers_per_s": float("%.4g" % (pairs * M / (ms * 1e-3))),
                   "issued_macs_per_s": float("%.4g" % (issued / (ms * 1e-3))),
                   "issued_frac_of_i8_mfma_rate": round(issued / (ms * 1e-3) / I8_MACS, 4)}
            rec.update(extra)
            emit(rec)
        dev.close()


if __name__ == "__main__":
    main()
