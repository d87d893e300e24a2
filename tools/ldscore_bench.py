"""LD score throughput of hgibbs_ld_scores on a synthetic BED made in HBM (hgibbs_synth_bed).

For N individuals x M markers, windows W, C annotation columns (about eight annotations per marker when C > 1) and one missing-call
rate: device time of the products (hgibbs_ld's product kernel and its zeroing, every piece) and of the reduce (the reduction kernel
of every piece, zeroing the accumulator, the final conversion), both from hgibbs_last_ld_scores_ms (HIP events), their ratio, and
pairs per second of the reduce.  With --host-route M2 the route this operator replaces is timed once for contrast at W = 1024
(--host-route-w): hgibbs_ld of M2 markers with r copied to the host and a NumPy reduction of r^2 forwards and backwards (wall clock).
One JSON line per case; --out appends them to a file as well.  One invocation is one GPU step: run it under `timeout`.

    python tools/ldscore_bench.py [--n 100000] [--m 1000000] [--windows 128,1024,4096] [--cols 1,64] [--missing 0] [--reps 2]
                                  [--host-route 0] [--host-route-w 1024] [--out F]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402


def annotations(M, C, seed=3, per_marker=8):
    """(M,) uint64: bit 0 everywhere and about per_marker - 1 of the other C - 1 bits"""
    rng = np.random.default_rng(seed)
    a = np.ones(M, dtype=np.uint64)
    for c in range(1, C):
        a |= (rng.random(M) < (per_marker - 1) / max(1, C - 1)).astype(np.uint64) << np.uint64(c)
    return a


def host_route(dev, W, M2, chunk_pairs=1 << 25):
    """hgibbs_ld with r to the host, then r^2 summed forwards and backwards in NumPy: wall seconds and the device's share"""
    l2 = np.ones(M2)
    chunk = max(16, chunk_pairs // W)
    dev_ms = 0.0
    t0 = time.perf_counter()
    for m0 in range(0, M2, chunk):
        cnt = min(chunk, M2 - m0)
        r, _ = dev.ld(W, m0=m0, count=cnt, sums=False)
        dev_ms += dev.last_ld_ms()
        t = np.nan_to_num(r * r)
        for jj in range(cnt):
            j = m0 + jj
            nd = min(W, M2 - 1 - j)
            l2[j] += t[jj, :nd].sum()
            l2[j + 1:j + 1 + nd] += t[jj, :nd]
    return time.perf_counter() - t0, dev_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--windows", default="128,1024,4096")
    ap.add_argument("--cols", default="1,64")
    ap.add_argument("--missing", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-route", type=int, default=0, help="markers of the host-route contrast (0: skip it)")
    ap.add_argument("--host-route-w", type=int, default=1024)
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
    windows = [int(x) for x in args.windows.split(",")]
    dev = capi.Device(0)
    dev.synth_bed(N, M, seed=5, missing_rate=args.missing)
    dev.marker_stats()
    for W in windows:
        pairs = W * M - W * (W + 1) // 2 if W < M else M * (M - 1) // 2
        for C in [int(x) for x in args.cols.split(",")]:
            annot = annotations(M, C) if C > 1 else None
            times = []
            for _ in range(args.reps + 1):  # the first run warms the code objects up
                dev.ld_scores(W, annot=annot, C=C)
                times.append(dev.last_ld_scores_ms())
            times = times[1:]
            prod = float(np.median([t[0] for t in times]))
            red = float(np.median([t[1] for t in times]))
            emit({"n": N, "m": M, "W": W, "C": C, "missing": args.missing, "pairs": pairs, "products_ms": round(prod, 3), "reduce_ms": round(red, 3),
                  "products_ms_all": [round(t[0], 3) for t in times], "reduce_ms_all": [round(t[1], 3) for t in times],
                  "reduce_over_products": round(red / prod, 4), "reduce_pairs_per_s": float("%.4g" % (pairs / (red * 1e-3)))})
    dev.close()
    if args.host_route:
        M2, W = min(args.host_route, M), args.host_route_w
        small = capi.Device(0)
        small.synth_bed(N, M2, seed=5, missing_rate=args.missing)
        small.marker_stats()
        small.ld(W, m0=0, count=min(M2, 64), sums=False)
        wall, dev_ms = host_route(small, W, M2)
        small.ld_scores(W, adjust=False)
        small.ld_scores(W, adjust=False)
        p, r = small.last_ld_scores_ms()
        emit({"host_route": True, "n": N, "m": M2, "W": W, "missing": args.missing, "wall_s": round(wall, 3), "hgibbs_ld_device_ms": round(dev_ms, 3),
              "ld_scores_products_ms": round(p, 3), "ld_scores_reduce_ms": round(r, 3)})
        small.close()


if __name__ == "__main__":
    main()
