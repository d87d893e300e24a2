"""Where an iteration of hgibbs_pca spends its time, on a synthetic BED made in HBM (hgibbs_synth_bed).

For N individuals x M markers, K components on a panel of L vectors and missing-call rates 0 and 1 %, `--reps` times, alternating:
  - hgibbs_pca with a fixed number of iterations and tol = 0 (data without structure has no gap to converge on: no claim is made on
    convergence): device ms of the whole call and of its parts (hgibbs_last_pca_ms), per product and per iteration;
  - hgibbs_marker_dots and hgibbs_score called once each from host panels of the same L: their device ms and their wall time with
    the allocations and copies.  This pair is what a host-driven loop over the existing calls would pay per iteration.
Reported: (a) the products inside hgibbs_pca per call against the standalone device ms (the same kernels on the same sizes), with the
spread over the repeats; (b) the panel algebra per iteration against the wall-time overhead of the copies it replaces.  Plus the copy
ceiling of hgibbs_stream_ceiling, against which the kernel trace of k_pca_gram is read.  One JSON line per case; --out appends them.

    python tools/pca_bench.py [--n 100000] [--m 1000000] [--k 10] [--l 24] [--iters 5] [--missing 0,0.01] [--reps 3] [--out F]
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--l", type=int, default=24)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters < 2:
        ap.error("--iters must be at least 2: the X T products and the panel algebra are timed per iteration after the first X'Q")
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    N, M, K, L, P = args.n, args.m, args.k, args.l, args.iters
    rng = np.random.default_rng(1)
    U = rng.standard_normal((L, N))
    a = rng.standard_normal((L, M))
    o = rng.standard_normal((L, M))
    r3 = lambda v: [round(float(x), 3) for x in v]  # noqa: E731
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        dev.pca(K, L=L, iters=1, tol=0.0, seed=3)  # warm-up of the code objects
        dev.marker_dots(U[:1], 0, 1024)
        ceiling = dev.stream_ceiling()
        whole, xq, xt, alg, md_ms, md_wall, sc_ms, sc_wall = ([] for _ in range(8))
        for _ in range(args.reps):
            dev.pca(K, L=L, iters=P, tol=0.0, seed=3)
            ms = dev.last_pca_ms()
            whole.append(ms[0])
            xq.append(ms[1] / P)
            xt.append(ms[2] / (P - 1))
            alg.append(ms[3] / (P - 1))
            t0 = time.perf_counter()
            dev.marker_dots(U)
            md_wall.append(1e3 * (time.perf_counter() - t0))
            md_ms.append(dev.last_marker_dots_ms())
            t0 = time.perf_counter()
            dev.score(a, o)
            sc_wall.append(1e3 * (time.perf_counter() - t0))
            sc_ms.append(dev.last_score_ms())
        med = lambda v: float(np.median(v))  # noqa: E731
        it_ms = med(xq) + med(xt) + med(alg)
        emit({"n": N, "m": M, "k": K, "l": L, "iters": P, "missing": miss, "stream_ceiling_gbps": round(ceiling, 1),
              "pca_whole_ms": r3(whole), "pca_xq_ms_per_product": r3(xq), "pca_xt_ms_per_product": r3(xt), "pca_algebra_ms_per_iter": r3(alg),
              "pca_iter_ms": round(it_ms, 3), "algebra_share_of_iter": round(med(alg) / it_ms, 4),
              "marker_dots_device_ms": r3(md_ms), "marker_dots_wall_ms": r3(md_wall), "score_device_ms": r3(sc_ms), "score_wall_ms": r3(sc_wall),
              "xq_inside_over_standalone": round(med(xq) / med(md_ms), 4), "xt_inside_over_standalone": round(med(xt) / med(sc_ms), 4),
              "host_loop_copy_overhead_ms_per_iter": round(med(md_wall) - med(md_ms) + med(sc_wall) - med(sc_ms), 3)})
        dev.close()


if __name__ == "__main__":
    main()
