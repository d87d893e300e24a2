"""Throughput of hgibbs_spa_roots on synthetic rare markers.

N individuals, nm markers of minor allele frequency --maf-lo .. --maf-hi (geometric), a null model of q columns (intercept and q - 1
normal covariates, about 5 % cases, fitted by hgibbs_logit_null), and per marker b, xv and a score s = z sqrt(V) with z spread over
2 .. 6: what --assoc-spa hands the operator for its flagged markers.  Per q, in one process: the device time of the call (every
kernel; HIP events, the median of --reps calls), the passes per marker (pass 0 and the passes of its longer tail), row-passes per second
(N times the passes of all markers over the time) and row-tail evaluations per second (one per row, pass and tail that took part:
one expm1 and one division each, a log1p more in a tail's closing pass).
One JSON line per case; --out appends them to a file as well (default profiles/spa_bench.jsonl).

    python tools/spa_bench.py [--n 100000] [--nm 4096] [--qs 4,12] [--maf-lo 0.001] [--maf-hi 0.05] [--reps 3] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hydra_amd import capi  # noqa: E402


def rare_bed(N, mafs, rng):
    """PLINK-packed columns (M, ceil(N / 4)) and, per marker, the rows and codes of its carriers: made from the carriers, not from a
    dense matrix"""
    nb = (N + 3) // 4
    bed = np.full((len(mafs), nb), 0xFF, dtype=np.uint8)  # code 0: two bits set per slot
    if N % 4:
        bed[:, -1] &= np.uint8(0xFF >> (2 * (4 - N % 4)))
        bed[:, -1] |= np.uint8((0x55 << (2 * (N % 4))) & 0xFF)  # padding slots read as missing
    carriers = []
    for j, p in enumerate(mafs):
        k = max(2, rng.binomial(N, 1 - (1 - p) ** 2))
        rows = rng.choice(N, size=k, replace=False)
        codes = 1 + (rng.random(k) < p / (2 - p)).astype(np.int64)  # P(2 copies | carrier)
        clear = np.where(codes == 1, 0b01, 0b11).astype(np.uint8) << (2 * (rows % 4)).astype(np.uint8)  # 1 -> 0b10, 2 -> 0b00
        np.bitwise_and.at(bed[j], rows // 4, ~clear)
        carriers.append((rows, codes))
    return bed, carriers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--nm", type=int, default=4096)
    ap.add_argument("--qs", default="4,12")
    ap.add_argument("--maf-lo", type=float, default=0.001)
    ap.add_argument("--maf-hi", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spa_bench.jsonl"))
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    N, M = args.n, args.nm
    rng = np.random.default_rng(7)
    bed, carriers = rare_bed(N, np.geomspace(args.maf_lo, args.maf_hi, M), rng)
    dev = capi.Device(0)
    dev.load_bed(bed, N)
    markers = np.arange(M, dtype=np.uint32)
    for q in [int(x) for x in args.qs.split(",")]:
        Z = np.column_stack([np.ones(N)] + [rng.standard_normal(N) for _ in range(q - 1)])
        eta = -3.2 + (Z[:, 1:] @ np.full(q - 1, 0.3 / np.sqrt(max(q - 1, 1))) if q > 1 else 0.0)
        d = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        fit = capi.logit_null(Z, d)
        mu, w = fit["mu"], fit["w"]
        info = Z.T @ (Z * w[:, None])
        zw1, sw = Z.T @ w, w.sum()
        B, xv, s = np.zeros((M, q)), np.zeros((M, 4)), np.zeros(M)
        for j, (rows, codes) in enumerate(carriers):
            m = codes.sum() / N
            sd = 1.0 / np.sqrt((np.sum((codes - m) ** 2) + (N - codes.size) * m * m) / (N - 1))
            xv[j] = ((0 - m) * sd, (1 - m) * sd, (2 - m) * sd, 0.0)
            dx = xv[j][codes] - xv[j][0]  # x = xv[0] + dx on the carriers
            t = xv[j][0] * zw1 + Z[rows].T @ (w[rows] * dx)
            B[j] = np.linalg.solve(info, t)
            xwx = xv[j][0] ** 2 * sw + np.sum(w[rows] * (xv[j][codes] ** 2 - xv[j][0] ** 2))
            s[j] = (2.0 + 4.0 * ((j * 0.6180339887) % 1.0)) * np.sqrt(xwx - t @ B[j]) * (1 if j % 2 else -1)
        dev.spa_roots(markers[:64], Z, mu, B[:64], xv[:64], s[:64])  # warm-up of the code object
        times = []
        for _ in range(args.reps):
            recs = dev.spa_roots(markers, Z, mu, B, xv, s)
            times.append(dev.last_spa_ms())
        ms = float(np.median(times))
        it = np.array([[r.iters[0], r.iters[1]] for r in recs])
        flags = np.array([r.flags for r in recs])
        passes = 1 + it.max(axis=1)
        rec = {"n": N, "nm": M, "q": q, "maf": [args.maf_lo, args.maf_hi], "cases": int(d.sum()),
               "device_ms": round(ms, 3), "device_ms_all": [round(x, 3) for x in times],
               "mean_passes_per_marker": round(float(passes.mean()), 3), "max_passes": int(passes.max()),
               "tails_converged": int(np.count_nonzero(flags & 1) + np.count_nonzero(flags & 2)),
               "tails_unreachable": int(np.count_nonzero(flags & 4) + np.count_nonzero(flags & 8)),
               "row_passes_per_s": round(N * float(passes.sum()) / (ms * 1e-3), 0),
               "row_tail_evals_per_s": round(N * float(it.sum()) / (ms * 1e-3), 0),
               "z_bytes_read_gbps": round(N * float(passes.sum()) * (q + 1) * 8 / (ms * 1e-3) / 1e9, 1)}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    dev.close()


if __name__ == "__main__":
    main()
