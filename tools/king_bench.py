"""KING-robust kinship throughput of hgibbs_king_pairs on a synthetic BED made in HBM (hgibbs_synth_bed).

For N individuals x M markers and missing-call rates 0 and 1 %: device time of the whole triangle (every kernel of the call: the
individual-major image, the products and the filter; HIP events), pair-markers per second (N (N - 1) / 2 x M over the time), and the
fraction of the I8 MFMA rate (MI355X: 8192 i8 operations a clock per CU, 256 CUs at 2.4 GHz: 2.52e15 multiply-adds/s) that the
kernel issues: five 16 x 16 x 64 products per tile pair ta <= tb and k-step of 64 markers.  One JSON line per case; --out appends
them to a file as well.

    python tools/king_bench.py [--n 100000] [--m 100000] [--missing 0,0.01] [--cutoff 0.0442] [--reps 2] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402

I8_MACS = 256 * 2.4e9 * 8192 / 2  # multiply-adds per second at the I8 MFMA rate (2 operations each)
PRODUCTS = 5  # c.c, h.c, c.h, h.h, u.u per tile pair and k-step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--cutoff", type=float, default=0.0442)
    ap.add_argument("--reps", type=int, default=2)
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
    issued = ntile * (ntile + 1) // 2 * nks * PRODUCTS * 16 * 16 * 64  # multiply-adds of the products the kernel issues
    pairs = N * (N - 1) // 2
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        dev.king(0, 16, 0, 16)  # warm-up of the code objects
        times, npairs = [], 0
        for _ in range(args.reps):
            ab, _, _ = dev.king_pairs(args.cutoff)
            npairs = len(ab)
            times.append(dev.last_king_ms())
        ms = float(np.median(times))
        emit({"n": N, "m": M, "missing": miss, "cutoff": args.cutoff, "pairs_listed": npairs, "device_ms": round(ms, 3),
              "device_ms_all": [round(x, 3) for x in times], "pair_markers_per_s": float("%.4g" % (pairs * M / (ms * 1e-3))),
              "issued_macs_per_s": float("%.4g" % (issued / (ms * 1e-3))),
              "issued_frac_of_i8_mfma_rate": round(issued / (ms * 1e-3) / I8_MACS, 4)})
        dev.close()


if __name__ == "__main__":
    main()
