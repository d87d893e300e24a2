"""LD mask throughput of hgibbs_ld_mask and the cost of the walk of hgibbs_ld_greedy on a synthetic BED made in
HBM (hgibbs_synth_bed).

For N individuals x M markers, windows W, thresholds t (the synthetic markers are independent: next to no pair passes t = 0.5, every
pair passes t = 0, the most the reduce can write) and one missing-call rate: device time of the products (hgibbs_ld's product
kernel and its zeroing, every piece) and of the reduce (k_ldm_reduce of every piece and zeroing the masks), both from
hgibbs_last_ld_mask_ms (HIP events); the wall time of the call beyond them (the host's preparation and the copy of the two masks);
and the wall time of the single-threaded walk on those masks with every marker participating, in a random order of priority and in
.bim order (the longest chain of dependencies).  The yardstick of the reduce is hgibbs_ld_scores at C = 1 on the same handle, the calls
alternating: both kernels read the same 32 B per pair once.  One JSON line per window and threshold; --out appends them to a file as well.  One
invocation is one GPU step: run it under `timeout`.

    python tools/ldmask_bench.py [--n 100000] [--m 1000000] [--windows 128,1024,4096] [--t 0.5,0] [--missing 0] [--reps 2] [--out F]
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
    ap.add_argument("--windows", default="128,1024,4096")
    ap.add_argument("--t", default="0.5,0", help="thresholds on r^2 (0: every pair with a finite r passes, the most the reduce writes)")
    ap.add_argument("--missing", type=float, default=0.0)
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
    dev = capi.Device(0)
    dev.synth_bed(N, M, seed=5, missing_rate=args.missing)
    dev.marker_stats()
    for W in [int(x) for x in args.windows.split(",")]:
        pairs = W * M - W * (W + 1) // 2 if W < M else M * (M - 1) // 2
        for thr in [float(x) for x in args.t.split(",")]:
            mask, score, wall = [], [], []
            fwd = bwd = None
            npass = 0
            for _ in range(args.reps + 1):  # the first round warms the code objects up
                dev.ld_scores(W, adjust=False)
                score.append(dev.last_ld_scores_ms())
                fwd = bwd = None
                t0 = time.perf_counter()
                fwd, bwd, npass = dev.ld_mask(W, thr)
                wall.append(1e3 * (time.perf_counter() - t0))
                mask.append(dev.last_ld_mask_ms())
            mask, score, wall = mask[1:], score[1:], wall[1:]
            prod = float(np.median([t[0] for t in mask]))
            red = float(np.median([t[1] for t in mask]))
            sred = float(np.median([t[1] for t in score]))
            beyond = float(np.median([w - t[0] - t[1] for w, t in zip(wall, mask)]))
            walks = {}
            for name, order in (("random", np.random.default_rng(1).permutation(M).astype(np.uint32)), ("bim", np.arange(M, dtype=np.uint32))):
                t0 = time.perf_counter()
                owner = capi.ld_greedy(M, W, fwd, bwd, order)
                walks[name] = (1e3 * (time.perf_counter() - t0), int(np.count_nonzero(owner == np.arange(M))))
            emit({"n": N, "m": M, "W": W, "t": thr, "missing": args.missing, "pairs": pairs, "passing_pairs": npass, "products_ms": round(prod, 3),
                  "reduce_ms": round(red, 3), "products_ms_all": [round(t[0], 3) for t in mask], "reduce_ms_all": [round(t[1], 3) for t in mask],
                  "ld_scores_c1_reduce_ms": round(sred, 3), "ld_scores_c1_reduce_ms_all": [round(t[1], 3) for t in score],
                  "reduce_over_ld_scores_reduce": round(red / sred, 4), "reduce_pairs_per_s": float("%.4g" % (pairs / (red * 1e-3))),
                  "mask_mib": round(2 * fwd.nbytes / 1048576.0, 1), "host_and_copy_ms": round(beyond, 3),
                  "walk_random_ms": round(walks["random"][0], 3), "walk_random_leaders": walks["random"][1],
                  "walk_bim_ms": round(walks["bim"][0], 3), "walk_bim_leaders": walks["bim"][1]})
    dev.close()


if __name__ == "__main__":
    main()
