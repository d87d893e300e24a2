"""Throughput of hgibbs_marker_dots and of the --assoc LOCO pipeline on a synthetic BED made in HBM
(hgibbs_synth_bed).

For N individuals x M markers and missing-call rates 0 and 1 %:
  - hgibbs_marker_dots over all markers for each K: device time (every kernel of the call; HIP events), BED bytes per second
    (M x N / 4 over the time) against the copy ceiling that hgibbs_stream_ceiling measures, and the MFMAs the kernel issues over the
    I8 rate (MI355X: 8192 i8 operations a clock per CU, two per multiply-add, 256 CUs at 2.4 GHz);
  - the LOCO pipeline as the CLI runs it: hgibbs_score with one sample per chromosome, then one hgibbs_marker_dots per chromosome
    (K = 1 + q with q = 1 + covariates): total device ms.
One JSON line per case; --out appends them to a file as well.

    python tools/assoc_bench.py [--n 100000] [--m 1000000] [--ks 2,4,10] [--missing 0,0.01] [--chroms 22] [--covariates 2] [--reps 2] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402

I8_MACS = 256 * 2.4e9 * 8192 / 2  # multiply-adds per second at the I8 MFMA rate (2 operations each)
MFMA_MACS = 16 * 16 * 64          # multiply-adds of one v_mfma_i32_16x16x64_i8


def issued_mfmas(K, n, tile_miss):
    """products the kernel issues over all markers: per 16-marker tile, slice of 512 individuals (8 k-steps) and vector tile, one
    product, two in tiles with missing calls"""
    tiles = (K + 1) // 2
    slices = (n + 511) // 512
    return (len(tile_miss) + int(np.count_nonzero(tile_miss))) * slices * 8 * tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--ks", default="2,4,10")
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--chroms", type=int, default=22)
    ap.add_argument("--covariates", type=int, default=2)
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

    probe = capi.Device(0)
    ceiling = probe.stream_ceiling(2 << 30, 10)
    probe.close()
    emit({"copy_ceiling_gbps": round(ceiling, 1)})
    N, M = args.n, args.m
    bed_bytes = M * ((N + 3) // 4)
    rng = np.random.default_rng(3)
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        mave, mstd, _, _, nm = dev.marker_stats()
        tile_miss = np.zeros((M + 15) // 16, dtype=bool)
        np.logical_or.at(tile_miss, np.arange(M) // 16, nm > 0)
        for K in [int(x) for x in args.ks.split(",")]:
            U = rng.standard_normal((K, N))
            dev.marker_dots(U, m0=0, count=min(M, 256))  # warm-up of the code objects
            times = []
            for _ in range(args.reps):
                dev.marker_dots(U)
                times.append(dev.last_marker_dots_ms())
            ms = float(np.median(times))
            mf = issued_mfmas(K, N, tile_miss)
            emit({"n": N, "m": M, "K": K, "missing": miss, "device_ms": round(ms, 3), "device_ms_all": [round(x, 3) for x in times],
                  "bed_read_gbps": round(bed_bytes / (ms * 1e-3) / 1e9, 1),
                  "frac_of_copy_ceiling": round(bed_bytes / (ms * 1e-3) / 1e9 / ceiling, 3),
                  "bed_read_ms_at_ceiling": round(bed_bytes / (ceiling * 1e9) * 1e3, 3),
                  "issued_mfmas": mf, "issued_frac_of_i8_mfma_rate": round(mf * MFMA_MACS / (ms * 1e-3) / I8_MACS, 4)})

        # the LOCO pipeline: S = chroms samples through hgibbs_score, then one hgibbs_marker_dots per chromosome (contiguous runs)
        C = args.chroms
        K = 2 + args.covariates
        cuts = np.linspace(0, M, C + 1).astype(int)
        a = np.zeros((C, M))
        o = np.zeros((C, M))
        beta = rng.standard_normal(M) * 1e-3
        ok = np.isfinite(mstd)
        w = np.where(ok, beta * np.where(ok, mstd, 0.0), 0.0)
        for c in range(C):
            a[c, cuts[c]:cuts[c + 1]] = w[cuts[c]:cuts[c + 1]]
            o[c, cuts[c]:cuts[c + 1]] = -(w * np.where(ok, mave, 0.0))[cuts[c]:cuts[c + 1]]
        U = rng.standard_normal((K, N))
        totals = []
        for _ in range(args.reps):
            dev.score(a, o)
            t = dev.last_score_ms()
            for c in range(C):
                dev.marker_dots(U, m0=int(cuts[c]), count=int(cuts[c + 1] - cuts[c]))
                t += dev.last_marker_dots_ms()
            totals.append(t)
        emit({"n": N, "m": M, "pipeline": "loco", "chroms": C, "K": K, "missing": miss, "device_ms": round(float(np.median(totals)), 3),
              "device_ms_all": [round(x, 3) for x in totals]})
        dev.close()


if __name__ == "__main__":
    main()
