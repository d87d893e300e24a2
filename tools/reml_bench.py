"""Device time of hgibbs_reml on a synthetic BED made in HBM (hgibbs_synth_bed), with the public
hgibbs_marker_dots and hgibbs_score at K = 16 alone in the same job as the yardstick: the products inside the driver are those two
calls' kernels, so they should cost what the calls cost, and everything else (algebra_ms) is what the solver adds.

The phenotype comes from the score operator: g = X beta for standard normal effects scaled to h2, plus standard normal noise.
Per shape, after one warm-up run: evaluations, CG iterations per evaluation, products_ms, algebra_ms, the algebra's share, wall
time, and the two yardsticks.  One JSON line per case; --out appends them to a file.

    python tools/reml_bench.py [--shapes 100000x100000,500000x1000000] [--trials 15] [--h2 0.5] [--out profiles/reml_bench.jsonl]
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
    ap.add_argument("--shapes", default="100000x100000,500000x1000000")
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--h2", type=float, default=0.5)
    ap.add_argument("--missing", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    small = capi.Device(0)  # warm-up of the code objects on a few rows
    small.synth_bed(256, 256, seed=5)
    small.reml(np.random.default_rng(0).standard_normal(256), np.ones((256, 1)), trials=3)
    small.close()
    for shape in args.shapes.split(","):
        N, M = (int(v) for v in shape.split("x"))
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=args.missing)
        mave, mstd = dev.marker_stats()[:2]
        rng = np.random.default_rng(1)
        used = np.isfinite(mstd)
        a = np.where(used, rng.standard_normal(M) * np.sqrt(args.h2 / used.sum()) * np.where(used, mstd, 0.0), 0.0)
        g = dev.score(a, np.where(used, -a * mave, 0.0))[:, 0]
        y = g + rng.standard_normal(N) * np.sqrt(1.0 - args.h2)
        y = (y - y.mean()) / y.std(ddof=1)
        Z = np.ones((N, 1))
        dev.reml(y, Z, trials=args.trials, seed=7)  # the warm-up
        t0 = time.perf_counter()
        r = dev.reml(y, Z, trials=args.trials, seed=7)
        wall = time.perf_counter() - t0
        U = rng.standard_normal((16, N))
        dev.marker_dots(U)
        T = dev.marker_dots(U)
        md = dev.last_marker_dots_ms()
        w = np.where(used[None, :], T.T * np.where(used, mstd, 0.0)[None, :] / used.sum(), 0.0)
        o = np.where(used[None, :], -w * np.where(used, mave, 0.0)[None, :], 0.0)
        dev.score(w, o)
        dev.score(w, o)
        sc = dev.last_score_ms()
        pairs = int(np.sum(r["cg_iters"])) + r["steps"] + 1 + int(r["ai_cg_iters"])  # X'P products: per iteration, per evaluation (u), the AI step
        rec = {"op": "reml", "n": N, "m": M, "trials": args.trials, "missing": args.missing, "status": capi.REML_STATUS[r["status"]],
               "evaluations": r["steps"], "cg_iters": [int(v) for v in r["cg_iters"]], "ai_cg_iters": int(r["ai_cg_iters"]),
               "products_ms": round(r["products_ms"], 3), "algebra_ms": round(r["algebra_ms"], 3),
               "algebra_share": round(r["algebra_ms"] / (r["products_ms"] + r["algebra_ms"]), 5), "wall_s": round(wall, 3),
               "h2": float("%.6g" % r["h2"]), "se_h2": float("%.4g" % r["se_h2"]), "se_mc": float("%.4g" % r["se_mc"]), "logdelta": float("%.6g" % r["logdelta"]),
               "marker_dots_k16_ms": round(md, 3), "score_k16_ms": round(sc, 3), "product_pairs_upper": pairs, "m_used": r["m_used"]}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        dev.close()


if __name__ == "__main__":
    main()
