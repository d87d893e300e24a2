"""Windowed LD throughput of hgibbs_ld on a synthetic BED made in HBM (hgibbs_synth_bed).

For N individuals x M markers, windows W and missing-call rates 0 and 1 %: device time of the whole band (every kernel of every
call; HIP events), useful multiply-adds per second (pairs x N) and their fraction of the I8 MFMA rate (MI355X: 2x the dense BF16
rate, 8192 i8 multiply-add operations a clock per CU, 256 CUs at 2.4 GHz: 2.52e15 multiply-adds/s), the same for the products the
kernel issues (whole 16 x 16 tiles, four of them on tiles with missing calls), and BED bytes per second (M x N / 4 over the time)
against the copy ceiling that hgibbs_stream_ceiling measures.  One JSON line per case; --out appends them to a file as well.

    python tools/ld_bench.py [--n 100000] [--m 1000000] [--windows 10,128,1024] [--missing 0,0.01] [--reps 2] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402

I8_MACS = 256 * 2.4e9 * 8192 / 2  # multiply-adds per second at the I8 MFMA rate (2 operations each)


def band(dev, W, M, chunk_pairs=1 << 27):
    """r of the whole band in chunks of markers; device ms summed over the calls"""
    chunk = max(16, chunk_pairs // W)
    ms = 0.0
    for m0 in range(0, M, chunk):
        dev.ld(W, m0=m0, count=min(chunk, M - m0), sums=False)
        ms += dev.last_ld_ms()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--windows", default="10,128,1024")
    ap.add_argument("--missing", default="0,0.01")
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
    n_slices = (N + 511) // 512
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        _, _, _, _, nm = dev.marker_stats()
        tile_miss = np.zeros((M + 15) // 16, dtype=bool)
        np.logical_or.at(tile_miss, np.arange(M) // 16, nm > 0)
        for W in [int(x) for x in args.windows.split(",")]:
            dev.ld(W, m0=0, count=min(M, 64), sums=False)  # warm-up of the code objects
            times = [band(dev, W, M) for _ in range(args.reps)]
            ms = float(np.median(times))
            pairs = sum(min(W, M - 1 - j) for j in range(0, M)) if M < 100000 else W * M - W * (W + 1) // 2
            macs = pairs * N
            # products issued: A tile t against tiles t .. t + floor((W + 15) / 16) within M, whole slices of 512 individuals
            nt = len(tile_miss)
            nq = (W + 15) // 16 + 1
            forms = 0
            for d in range(nq):
                a, b = tile_miss[:nt - d], tile_miss[d:]
                forms += int(np.count_nonzero(a | b)) * 4 + int(np.count_nonzero(~(a | b)))
            issued = forms * 256 * n_slices * 512
            emit({"n": N, "m": M, "W": W, "missing": miss, "device_ms": round(ms, 3), "device_ms_all": [round(x, 3) for x in times],
                  "pairs": pairs, "macs_per_s": float("%.4g" % (macs / (ms * 1e-3))),
                  "frac_of_i8_mfma_rate": round(macs / (ms * 1e-3) / I8_MACS, 4),
                  "issued_macs_per_s": float("%.4g" % (issued / (ms * 1e-3))),
                  "issued_frac_of_i8_mfma_rate": round(issued / (ms * 1e-3) / I8_MACS, 4),
                  "bed_read_gbps": round(bed_bytes / (ms * 1e-3) / 1e9, 1),
                  "frac_of_copy_ceiling": round(bed_bytes / (ms * 1e-3) / 1e9 / ceiling, 3)})
        dev.close()


if __name__ == "__main__":
    main()
