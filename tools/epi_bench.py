"""Throughput of the epistasis screen hgibbs_epi_scan on a synthetic BED made in HBM (hgibbs_synth_bed) with
random classes.

For N individuals and one square scan over the first M markers (every pair a < b), at missing-call rates 0 and 1 %: device time of the
products (class image, marker counts, zeroing, tile products, tables) and of the screen (KSA and the list) over every block of the
scan (HIP events), pairs per second, and the tile products the kernel issues -- whole 16 x 16 x 64 products over whole slices of 512
individuals, 8 per tile pair and k-step in the clean build with classes, 18 in the missing-call build, over whole blocks of the pair
space, the diagonal blocks in full -- as a share of the I8 MFMA rate (MI355X: 8192 i8 multiply-add operations a clock per CU, 256 CUs at
2.4 GHz: 2.52e15 multiply-adds/s).  One JSON line per case; --out appends them to a file as well.

    python tools/epi_bench.py [--n 100000] [--m 8192] [--missing 0,0.01] [--threshold 30] [--reps 3] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402

I8_MACS = 256 * 2.4e9 * 8192 / 2  # multiply-adds per second at the I8 MFMA rate (2 operations each)
BLOCK = 1024                      # list positions a side of a block (the default of option epi_block)


def issued_macs(flag16, M, N, cls=True):
    """multiply-adds of the tile products a triangular scan over markers 0 .. M - 1 issues: per block of the pair space that holds a
    pair a < b, per (tile of A, group of two tiles of B), 2 x 4 (clean) or 2 x 9 (missing-call build) products, twice with classes"""
    n_slices = (N + 511) // 512
    flag32 = np.array([flag16[2 * g:2 * g + 2].any() for g in range((len(flag16) + 1) // 2)])
    total = 0
    for a0 in range(0, M, BLOCK):
        for b0 in range(0, M, BLOCK):
            ca, cb = min(BLOCK, M - a0), min(BLOCK, M - b0)
            if b0 + cb <= a0 + 1:
                continue
            fa = flag16[a0 // 16:(a0 + ca + 15) // 16]
            fb = flag32[b0 // 32:(b0 + cb + 31) // 32]
            miss = int(np.count_nonzero(fa[:, None] | fb[None, :]))
            total += (miss * 9 + (fa.size * fb.size - miss) * 4) * 2
    return total * (2 if cls else 1) * 256 * 64 * 8 * n_slices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--threshold", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=3)
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
    cls = (np.random.default_rng(3).random(N) < 0.5).astype(np.uint8)
    idx = np.arange(M, dtype=np.uint32)
    pairs = M * (M - 1) // 2
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        nm = dev.marker_stats()[4]
        flag16 = np.zeros((M + 15) // 16, dtype=bool)
        np.logical_or.at(flag16, np.arange(M) // 16, nm[:M] > 0)
        dev.epi_scan(idx[:64], None, cls, args.threshold)  # warm-up of the code objects
        times, listed = [], 0
        for _ in range(args.reps):
            ab, _, _ = dev.epi_scan(idx, None, cls, args.threshold)
            listed = int(ab.shape[0])
            times.append(dev.last_epi_ms())
        pm, sm = (float(np.median([t[k] for t in times])) for k in (0, 1))
        issued = issued_macs(flag16, M, N)
        emit({"n": N, "m": M, "missing": miss, "threshold": args.threshold, "pairs": pairs, "listed": listed,
              "products_ms": round(pm, 3), "screen_ms": round(sm, 3), "device_ms_all": [[round(a, 3), round(b, 3)] for a, b in times],
              "pairs_per_s": float("%.4g" % (pairs / ((pm + sm) * 1e-3))),
              "issued_macs_per_s": float("%.4g" % (issued / (pm * 1e-3))),
              "issued_frac_of_i8_mfma_rate": round(issued / (pm * 1e-3) / I8_MACS, 4)})
        dev.close()


if __name__ == "__main__":
    main()
