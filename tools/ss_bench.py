"""Sweep time of the summary-statistics engine (hgibbs_ss_sweep) on a synthetic panel made in HBM (hgibbs_synth_bed).

For a panel of N rows x M markers and a window of W markers: the band's build time (hgibbs_ss_begin: hgibbs_ld's products and the
scaling), then --iters iterations of hydra_ss_chain on synthetic summary statistics (noise of a GWAS of n_eff individuals plus a
fraction of signals), each with the device time of its sweep kernel (hgibbs_last_ss_ms, HIP events), markers per second, microseconds
per marker and the census of non-zero updates (markers whose effect changed: each costs two barriers and a pass over the window).
Before the chain, one sweep with every marker fixed (adaV = 0, every effect 0: no draw, no update) times the walk alone, in shuffled
and in marker order.  One JSON line per case; --out appends them to a file as well.  One invocation is one GPU step: run it under
`timeout`.

--chromosomes C cuts the window into C index intervals with the relative sizes of the first C human autosomes (chromosome 1 about
8 % of M at C = 22), as ld_window does per chromosome.  --streams S sweeps the independent blocks at the same time in at most S
streams (hgibbs_ss_sweep_streams); the record then names the streams used, the largest interval and the
ideal ratio M / largest against one stream.  Run the same cases without --streams for the single stream on the same band.

--chains R[,R...] times, after the single chain and in the same process, hydra_ss_multi with R chains from the seeds 11 + r on a band
of the same panel (hgibbs_ss_sweep_replicas; it composes with --chromosomes and --streams): per R one record
with the device time of every replica launch, its median against the single chain's median sweep of this run, and the wall time of
an iteration beside it (what the host adds: R shuffles, the uploads, the sums).  The records go to --chains-out as well
(profiles/ss_chains_bench.jsonl unless told otherwise).

--post (with --chains) folds every iteration of those runs into the per-marker posterior accumulators (hgibbs_ss_post_add, DESIGN.md
section 34) and downloads every chain's effects, components and acum as the command line does per record without
--sumstats-post-only (hydra_ss_multi_effects into buffers made once).  Per R one record in --post-out (profiles/ss_post_bench.jsonl
unless told otherwise): the device time of an add beside the replica launch of the same iteration, the bytes the add kernel moves and
the bandwidth that implies, the table's kernel, and the host's wall time of an iteration with the downloads and without them.

--cs (with --chains, not with --post) opens the inclusion history beside the posterior accumulators (hgibbs_cs_begin, DESIGN.md section
35) and folds every iteration into both, the calls alternating: per R one record in --cs-out (profiles/ss_cs_bench.jsonl unless told
otherwise) with the device time of one hgibbs_ss_cs_add beside one hgibbs_ss_post_add and beside the replica launch of the same
iteration.  Then, on the same handle, hgibbs_ld_mask at r^2 >= --cs-r2 (the synthetic markers are independent: the default 1e-4 is
about 1 / N, so that a third of the window's pairs pass and a lead has friends), and hgibbs_cs_sets for 10^4 random leads on a
history of 40 x 100 = 4000 records of random flags (each marker in 2 % of the records), need = 0.9 NREC, at most 64 members.

    python tools/ss_bench.py [--cases 10000x100000x128,20000x1000000x512] [--n-eff 4000000] [--signals 0.001] [--iters 6] [--out F]
                             [--chromosomes C] [--streams S] [--chains R[,R...]] [--chains-iters I] [--chains-out F] [--post] [--post-out F]
                             [--cs] [--cs-out F] [--cs-r2 T]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hydra_amd import capi  # noqa: E402


# lengths of the human autosomes in Mb, rounded
AUTOSOME_MB = [248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47, 51]


def chromosome_ahead(M, W, C):
    """(sizes, ahead): C intervals with the autosomes' relative sizes, ahead[j] = min(W, markers left in j's interval)"""
    mb = np.array(AUTOSOME_MB[:C], dtype=np.float64)
    ends = np.round(np.cumsum(mb) * (M / mb.sum())).astype(np.int64)
    sizes = np.diff(np.concatenate([[0], ends]))
    end_of = np.repeat(ends, sizes)
    return sizes, np.minimum(W, end_of - 1 - np.arange(M)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x100000x128,20000x1000000x512", help="NxMxW, comma-separated")
    ap.add_argument("--n-eff", type=float, default=4000000.0,
                    help="above M: independent synthetic markers carry no LD, so the noise of M markers must fit into y'y = n - 1")
    ap.add_argument("--signals", type=float, default=0.001, help="fraction of markers with an effect")
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--chromosomes", type=int, default=0, help="cut the window into this many intervals (1..22) sized like the human autosomes")
    ap.add_argument("--streams", type=int, default=0, help="sweep independent blocks in at most this many parallel streams (1..1024)")
    ap.add_argument("--chains", default="", help="numbers of chains (1..64), comma-separated: time the replica launch with each after the single chain")
    ap.add_argument("--chains-iters", type=int, default=0, help="iterations of every --chains run (default: --iters)")
    ap.add_argument("--chains-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ss_chains_bench.jsonl"))
    ap.add_argument("--post", action="store_true", help="with --chains: time hgibbs_ss_post_add and the per-record downloads it can replace (at least 4 iterations)")
    ap.add_argument("--post-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ss_post_bench.jsonl"))
    ap.add_argument("--cs", action="store_true", help="with --chains: time hgibbs_ss_cs_add beside hgibbs_ss_post_add, then hgibbs_ld_mask and hgibbs_cs_sets (at least 4 iterations)")
    ap.add_argument("--cs-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ss_cs_bench.jsonl"))
    ap.add_argument("--cs-r2", type=float, default=1e-4, help="the threshold of the mask the sets are timed on")
    ap.add_argument("--label", default=None, help="a word copied into every record (which build, which run)")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    chains = [int(x) for x in args.chains.split(",") if x]
    chains_out = open(args.chains_out, "a") if chains else None
    post_out = open(args.post_out, "a") if chains and args.post else None
    if args.cs and args.post:
        ap.error("--cs and --post each open the posterior accumulators: one at a time")
    cs_out = open(args.cs_out, "a") if chains and args.cs else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for case in args.cases.split(","):
        N, M, W = (int(x) for x in case.split("x"))
        n = args.n_eff
        rs = np.random.default_rng(7)
        # b_j = x_j'y of a y with y'y = n - 1: sqrt(n - 1) times a standard normal under the null, plus (n - 1) beta_j for the signals
        xty = np.sqrt(n - 1.0) * rs.standard_normal(M)
        sig = rs.random(M) < args.signals
        xty[sig] += (n - 1.0) * rs.normal(0.0, np.sqrt(0.5 / max(1, sig.sum())), int(sig.sum()))
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5)
        ahead = chromosome_ahead(M, W, args.chromosomes)[1] if args.chromosomes else None
        ch = capi.SsChain(dev, n, W, xty, ahead=ahead, seed=11, streams=args.streams or None)
        bounds, _ = ch.streams()
        band_ms = dev.last_ss_ms()[0]
        rec = {"n_panel": N, "m": M, "W": W, "n_eff": n, "signals": int(sig.sum()), "band_mib": round(M * W * 8 / 2.0**20, 1), "band_ms": round(band_ms, 3)}
        if args.label:
            rec["label"] = args.label
        if args.chromosomes:
            rec["chromosomes"] = args.chromosomes
        if args.streams:
            largest = int(np.diff(bounds.astype(np.int64)).max())
            rec.update({"streams_max": args.streams, "streams": len(bounds) - 1, "largest_interval": largest, "ideal_ratio": round(M / largest, 3)})

        # the walk alone: nothing adaptive, every effect 0 (the first launch warms the code object up)
        fixed = np.zeros(M, dtype=np.uint8)
        sG, pi = np.array([0.5]), np.array([[0.5, 0.25, 0.15, 0.10]])
        rng = capi.RngState()
        rng.idx = 624
        rngs = [capi.RngState() for _ in range(len(bounds) - 1)] if args.streams else []
        for r in rngs:
            r.idx = 624
        for name, order in (("warm", np.arange(M)), ("walk_marker_order", np.arange(M)), ("walk_shuffled", rs.permutation(M))):
            if args.streams:
                _, nnz = dev.ss_sweep_streams(order, 0.5, sG, pi, fixed, bounds, rngs)
            else:
                _, nnz = dev.ss_sweep(order, 0.5, sG, pi, fixed, rng)
            assert nnz == 0
            if name != "warm":
                ms = dev.last_ss_ms()[1]
                rec[name + "_ms"] = round(ms, 3)
                rec[name + "_us_per_marker"] = round(1e3 * ms / M, 4)

        sweeps = []
        for it in range(args.iters):
            t0 = time.perf_counter()
            ch.iterate()
            wall = 1e3 * (time.perf_counter() - t0)
            ms = dev.last_ss_ms()[1]
            st = ch.state()
            sweeps.append({"it": it, "sweep_ms": round(ms, 3), "wall_ms": round(wall, 3), "markers_per_s": float("%.4g" % (M / (ms * 1e-3))), "us_per_marker": round(1e3 * ms / M, 4),
                           "nnz_updates": ch.last_nnz(), "m0": int(st["m0"].sum()), "sigmaG": float("%.6g" % st["sigmaG"].sum()),
                           "sigmaE": float("%.6g" % st["sigmaE"])})
        rec["sweeps"] = sweeps
        # two unknowns from the sweeps: time = M t_marker + nnz t_update (least squares over the iterations)
        A = np.array([[M, s["nnz_updates"]] for s in sweeps], dtype=np.float64)
        t = np.array([s["sweep_ms"] for s in sweeps])
        if len(sweeps) >= 2 and np.linalg.matrix_rank(A) == 2:
            sol = np.linalg.lstsq(A, t, rcond=None)[0]
            rec["fit_us_per_marker"] = round(1e3 * sol[0], 4)
            rec["fit_us_per_update"] = round(1e3 * sol[1], 4)
        emit(rec)
        del ch

        single_ms = float(np.median([s["sweep_ms"] for s in sweeps])) if sweeps else None
        single_host = float(np.median([s["wall_ms"] - s["sweep_ms"] for s in sweeps])) if sweeps else None
        for R in chains:
            mc = capi.SsMultiChain(dev, n, W, xty, [11 + r for r in range(R)], ahead=ahead, streams=args.streams or None)
            its, pits = [], []
            T = args.chains_iters or args.iters
            if args.post:
                dev.ss_post_begin(R, T)
                beta, acum, comp = np.zeros(M), np.zeros(M), np.zeros(M, dtype=np.int32)
                added = 0.0
            if args.cs:
                dev.ss_post_begin(R, T)
                dev.cs_begin(R, T)
                cits = []
            for it in range(T):
                t0 = time.perf_counter()
                mc.iterate()
                wall = 1e3 * (time.perf_counter() - t0)
                its.append({"it": it, "launch_ms": round(dev.last_ss_ms()[1], 3), "wall_ms": round(wall, 3), "nnz_updates": [mc.last_nnz(r) for r in range(R)]})
                if args.post:
                    t1 = time.perf_counter()
                    dev.ss_post_add()
                    t2 = time.perf_counter()
                    for r in range(R):  # what a record costs the command line without --sumstats-post-only, but for the disk
                        capi.check(mc.L.hydra_ss_multi_effects(mc.h, r, capi._dp(beta), capi._ip(comp), capi._dp(acum), None))
                    t3 = time.perf_counter()
                    total = dev.last_ss_post_ms()[0]
                    pits.append({"it": it, "launch_ms": its[-1]["launch_ms"], "iterate_wall_ms": round(wall, 3), "add_ms": round(total - added, 4),
                                 "add_wall_ms": round(1e3 * (t2 - t1), 3), "download_wall_ms": round(1e3 * (t3 - t2), 3)})
                    added = total
                if args.cs:  # the two adds alternate on the one handle
                    p0, c0 = dev.last_ss_post_ms()[0], dev.last_cs_ms()[0]
                    dev.ss_post_add()
                    dev.ss_cs_add(R)
                    cits.append({"it": it, "launch_ms": its[-1]["launch_ms"], "post_add_ms": round(dev.last_ss_post_ms()[0] - p0, 4),
                                 "cs_add_ms": round(dev.last_cs_ms()[0] - c0, 4)})
            if args.cs:
                med = {k: float(np.median([x[k] for x in cits])) for k in ("launch_ms", "post_add_ms", "cs_add_ms")}
                in_model = dev.cs_counts()
                dev.ss_post_end()
                fwd, bwd, npass = dev.ld_mask(W, args.cs_r2, ahead=ahead)
                mask_ms = dev.last_ld_mask_ms()
                # the sets' kernel on a history of its own: 40 chains x 100 records, a block of random flags shifted from record to record
                CC, TT, nlead, max_size = 40, 100, min(10000, M), 64
                nrec = CC * TT
                dev.cs_begin(CC, TT)
                block = (rs.random((CC, M)) < 0.02).astype(np.uint8)
                for t in range(TT):
                    dev.cs_add_flags(np.roll(block, 9973 * t, axis=1))
                cnt = dev.cs_counts()
                leads = np.sort(rs.choice(M, nlead, replace=False)).astype(np.uint32)
                need = int(np.ceil(0.9 * nrec))
                status, size, total, pep, members = dev.cs_sets(W, fwd, bwd, leads, need, max_size)
                add_ms, counts_ms, sets_ms = dev.last_cs_ms()
                dev.cs_end()
                words = (R + 63) // 64 + 1  # at most: the words one record's R bits touch
                crec_cs = {"kind": "cs", "n_panel": N, "m": M, "W": W, "chains": R, "records": T, "launch_ms_median": round(med["launch_ms"], 3),
                           "post_add_ms_median": round(med["post_add_ms"], 4), "cs_add_ms_median": round(med["cs_add_ms"], 4),
                           "cs_add_to_post_add": round(med["cs_add_ms"] / med["post_add_ms"], 4), "cs_add_bytes_at_most": int(M * (4 * R + 16 * words)),
                           "history_bytes": int((R * T + 63) // 64 * 8 * M), "markers_ever_in_the_model": int(np.count_nonzero(in_model)),
                           "mask_r2": args.cs_r2, "mask_pairs_passing": int(npass), "mask_products_ms": round(mask_ms[0], 3), "mask_reduce_ms": round(mask_ms[1], 3),
                           "sets_nrec": nrec, "sets_leads": int(nlead), "sets_need": need, "sets_max_size": max_size, "sets_history_add_ms_mean": round(add_ms / TT, 4),
                           "sets_counts_ms": round(counts_ms, 4), "sets_ms": round(sets_ms, 3), "sets_reached": int(np.count_nonzero(status == 0)),
                           "sets_short": int(np.count_nonzero(status == 1)), "sets_capped": int(np.count_nonzero(status == 2)),
                           "sets_mean_size": round(float(size[status == 0].mean()), 2) if np.any(status == 0) else None,
                           "sets_mean_cnt": round(float(cnt.mean()), 2), "iterations": cits}
                for k in ("chromosomes", "streams_max", "streams", "largest_interval", "label"):
                    if k in rec:
                        crec_cs[k] = rec[k]
                emit(crec_cs)
                cs_out.write(json.dumps(crec_cs) + "\n")
                cs_out.flush()
            if args.post:
                t1 = time.perf_counter()
                mean, sd, pip, cnt, rhat = dev.ss_post_get()
                get_wall = 1e3 * (time.perf_counter() - t1)
                K = cnt.shape[0]
                med = {k: float(np.median([x[k] for x in pits])) for k in ("launch_ms", "iterate_wall_ms", "add_ms", "add_wall_ms", "download_wall_ms")}
                # a record inside a half (every record of an even T): per chain and marker the effect, the component and the half-chain's
                # pair read and written; per marker the pooled pair and the K counts read and written
                nbytes = M * (R * (8 + 4 + 32) + 32 + 8 * K)
                prec = {"kind": "post", "n_panel": N, "m": M, "W": W, "chains": R, "records": T, "K": int(K), "launch_ms_median": round(med["launch_ms"], 3),
                        "add_ms_median": round(med["add_ms"], 4), "add_to_launch": round(med["add_ms"] / med["launch_ms"], 6), "add_bytes": int(nbytes),
                        "add_gb_per_s": round(nbytes / (med["add_ms"] * 1e-3) / 1e9, 1), "final_ms": round(dev.last_ss_post_ms()[1], 4),
                        "get_wall_ms": round(get_wall, 3), "download_bytes_per_record": int(R * M * 20),
                        "host_s_per_iteration_with_downloads": round(1e-3 * (med["iterate_wall_ms"] + med["add_wall_ms"] + med["download_wall_ms"]), 6),
                        "host_s_per_iteration_post_only": round(1e-3 * (med["iterate_wall_ms"] + med["add_wall_ms"]), 6),
                        "pip_between_0_and_1": int(np.count_nonzero((pip > 0) & (pip < 1))), "rhat_finite": int(np.count_nonzero(np.isfinite(rhat))), "iterations": pits}
                for k in ("chromosomes", "streams_max", "streams", "largest_interval", "label"):
                    if k in rec:
                        prec[k] = rec[k]
                emit(prec)
                post_out.write(json.dumps(prec) + "\n")
                post_out.flush()
            launch = float(np.median([x["launch_ms"] for x in its]))
            host = float(np.median([x["wall_ms"] - x["launch_ms"] for x in its]))
            crec = {"kind": "chains", "n_panel": N, "m": M, "W": W, "chains": R, "workgroups": R * max(1, len(mc.streams()[0]) - 1),
                    "single_sweep_ms_median": single_ms, "single_host_ms_median": single_host, "launch_ms_median": round(launch, 3),
                    "ratio_to_single": round(launch / single_ms, 4) if single_ms else None, "host_ms_median": round(host, 3),
                    "host_ratio_to_R_singles": round(host / (R * single_host), 4) if single_host else None, "iterations": its}
            for k in ("chromosomes", "streams_max", "streams", "largest_interval", "label"):
                if k in rec:
                    crec[k] = rec[k]
            emit(crec)
            chains_out.write(json.dumps(crec) + "\n")
            chains_out.flush()
            del mc
        dev.close()


if __name__ == "__main__":
    main()
