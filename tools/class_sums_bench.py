"""Throughput of hgibbs_marker_class_sums beside hgibbs_marker_dots on a synthetic BED made in HBM
(hgibbs_synth_bed).

For N individuals x M markers, missing-call rates 0 and 1 % and each K, in ONE process and on the same handle and vectors: the device
time of each operator over all markers (every kernel of the call; HIP events, the median of --reps calls), their ratio, the BED bytes
per second (M x N / 4 over the time) against the copy ceiling that hgibbs_stream_ceiling measures, and the MFMAs the kernel issues
over the I8 rate (MI355X: 8192 i8 operations a clock per CU, two per multiply-add, 256 CUs at 2.4 GHz).
One JSON line per case; --out appends them to a file as well (default profiles/class_sums_bench.jsonl).

    python tools/class_sums_bench.py [--n 100000] [--m 1000000] [--ks 2,4,10] [--missing 0,0.01] [--reps 3] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hydra_amd import capi  # noqa: E402

I8_MACS = 256 * 2.4e9 * 8192 / 2  # multiply-adds per second at the I8 MFMA rate (2 operations each)
MFMA_MACS = 16 * 16 * 64          # multiply-adds of one v_mfma_i32_16x16x64_i8


def issued_mfmas(K, n, tile_miss, clean, missing):
    """products a kernel issues over all markers: per 16-marker tile, slice of 512 individuals (8 k-steps) and vector tile, `clean`
    products and `missing` more in tiles with missing calls"""
    tiles = (K + 1) // 2
    slices = (n + 511) // 512
    return (clean * len(tile_miss) + missing * int(np.count_nonzero(tile_miss))) * slices * 8 * tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--ks", default="2,4,10")
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_sums_bench.jsonl"))
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
        nm = dev.marker_stats()[4]
        tile_miss = np.zeros((M + 15) // 16, dtype=bool)
        np.logical_or.at(tile_miss, np.arange(M) // 16, nm > 0)
        for K in [int(x) for x in args.ks.split(",")]:
            U = rng.standard_normal((K, N))
            ops = {"class_sums": (dev.marker_class_sums, dev.last_marker_class_sums_ms, 2, 1),
                   "marker_dots": (dev.marker_dots, dev.last_marker_dots_ms, 1, 1)}
            rec = {"n": N, "m": M, "K": K, "missing": miss, "bed_read_ms_at_ceiling": round(bed_bytes / (ceiling * 1e9) * 1e3, 3)}
            for name, (call, last_ms, clean, missing) in ops.items():
                call(U, m0=0, count=min(M, 256))  # warm-up of the code objects
                times = []
                for _ in range(args.reps):
                    call(U)
                    times.append(last_ms())
                ms = float(np.median(times))
                mf = issued_mfmas(K, N, tile_miss, clean, missing)
                rec[name] = {"device_ms": round(ms, 3), "device_ms_all": [round(x, 3) for x in times],
                             "bed_read_gbps": round(bed_bytes / (ms * 1e-3) / 1e9, 1),
                             "frac_of_copy_ceiling": round(bed_bytes / (ms * 1e-3) / 1e9 / ceiling, 3),
                             "issued_mfmas": mf, "issued_frac_of_i8_mfma_rate": round(mf * MFMA_MACS / (ms * 1e-3) / I8_MACS, 4)}
            rec["class_sums_over_marker_dots"] = round(rec["class_sums"]["device_ms"] / rec["marker_dots"]["device_ms"], 3)
            emit(rec)
        dev.close()


if __name__ == "__main__":
    main()
