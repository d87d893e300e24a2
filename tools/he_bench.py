"""Device time of hgibbs_grm_rowsums on a synthetic BED made in HBM (hgibbs_synth_bed), with hgibbs_grm at the
same shape in the same job as the yardstick: the products of the two calls are the same kernels, the reduce is what the row sums add.

For N individuals x M markers, P vectors and missing-call rates 0 and 1 %: products ms and reduce ms of the row sums (HIP events; the
medians over the repeats), the device ms of hgibbs_grm with both output pointers NULL, the reduce as a share of the products, and the
pairs a second the reducer takes.  One JSON line per case; --out appends them to a file.

    python tools/he_bench.py [--n 40000] [--m 40000] [--p 2] [--missing 0,0.01] [--reps 2] [--out profiles/he_bench.jsonl]
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
    ap.add_argument("--n", type=int, default=40000)
    ap.add_argument("--m", type=int, default=40000)
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    N, M, P = args.n, args.m, args.p
    y = np.random.default_rng(1).standard_normal(N)
    y = (y - y.mean()) / y.std(ddof=1)
    Y = np.ascontiguousarray(np.stack([y ** (p + 1) for p in range(P)]))
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        small = capi.Device(0)  # warm-up of the code objects on a few rows
        small.synth_bed(64, 64, seed=5)
        small.grm_rowsums(np.ones((1, 64)))
        small.close()
        grm, prod, red = [], [], []
        for _ in range(args.reps):
            capi.check(dev.L.hgibbs_grm(dev.h, 0, N, None, None))
            grm.append(dev.last_grm_ms())
            ay, a1, a2, diag, partners = dev.grm_rowsums(Y)
            a, b = dev.last_grm_rowsums_ms()
            prod.append(a)
            red.append(b)
        m_used, E = dev.grm_info()
        g, pr, rd = float(np.median(grm)), float(np.median(prod)), float(np.median(red))
        rec = {"op": "grm_rowsums", "n": N, "m": M, "p": P, "missing": miss, "products_ms": round(pr, 3), "reduce_ms": round(rd, 3),
               "grm_device_ms": round(g, 3), "reduce_share_of_products": round(rd / pr, 5),
               "products_ms_all": [round(x, 3) for x in prod], "reduce_ms_all": [round(x, 3) for x in red], "grm_device_ms_all": [round(x, 3) for x in grm],
               "reduce_pairs_per_s": float("%.4g" % (N * (N - 1) // 2 / (rd * 1e-3))), "m_used": m_used, "E": E,
               "partners_min": int(partners.min()), "partners_max": int(partners.max()),
               "a_sum_mean": float("%.6g" % a1.mean()), "a_sqsum_mean": float("%.6g" % a2.mean()), "a_diag_mean": float("%.6g" % np.nanmean(diag))}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        dev.close()


if __name__ == "__main__":
    main()
