"""Throughput of hgibbs_set_gram beside what the tree could do before it, on a synthetic BED made in HBM
(hgibbs_synth_bed).

For N individuals, missing-call rates 0 and 1 % and sets of 16, 64 and 256 contiguous markers, in ONE process and on the same handle
and weights: the device time of hgibbs_set_gram over all sets of a size (every kernel of the call; HIP events, the median of --reps
calls), the BED bytes its workgroups read per second against the copy ceiling that hgibbs_stream_ceiling measures, and the MFMAs the
kernel issues over the I8 rate (MI355X: 8192 i8 operations a clock per CU, two per multiply-add, 256 CUs at 2.4 GHz).  Beside it
the route through hgibbs_marker_class_sums: the BED of a set decoded on the host, the vectors w o g_k formed there, at most 32 of
them a pass against the set's markers, GG = S1 + 2 S2 (its asymmetry, the roundings of two different vectors, is recorded as a
check of the route); its device time and the host's wall time for the vectors and the copies.
One JSON line per case; --out appends them to a file as well (default profiles/set_gram_bench.jsonl).

    python tools/set_gram_bench.py [--n 100000] [--m 4096] [--sizes 16,64,256] [--missing 0,0.01] [--reps 3] [--out F]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hydra_amd import capi, synth  # noqa: E402

I8_MACS = 256 * 2.4e9 * 8192 / 2  # multiply-adds per second at the I8 MFMA rate (2 operations each)
MFMA_MACS = 16 * 16 * 64          # multiply-adds of one v_mfma_i32_16x16x64_i8


def issued_mfmas(sets, n, gran_miss):
    """products k_sgram issues: per job (tile pair) and k-step of 64 individuals 14 for GG, 28 more where a tile of the pair lies in
    a granule with missing calls (21 on a diagonal job), one more on every diagonal job; and the jobs' number"""
    steps = ((n + 511) // 512) * 8
    total = jobs = 0
    for idx in sets:
        nt = (len(idx) + 15) // 16
        flag = [bool(gran_miss[np.asarray(idx[16 * t:16 * t + 16]) // 16].any()) for t in range(nt)]
        for a in range(nt):
            for b in range(a, nt):
                jobs += 1
                total += steps * (14 + (1 if a == b else 0) + ((14 if a == b else 28) if flag[a] or flag[b] else 0))
    return total, jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_gram_bench.jsonl"))
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
    rng = np.random.default_rng(3)
    mu = rng.uniform(0.02, 0.98, N)
    w = mu * (1.0 - mu)
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        nm = dev.marker_stats()[4]
        gran_miss = np.zeros((M + 15) // 16, dtype=bool)
        np.logical_or.at(gran_miss, np.arange(M) // 16, nm > 0)
        for size in [int(x) for x in args.sizes.split(",")]:
            sets = [np.arange(s, s + size, dtype=np.uint32) for s in range(0, M - size + 1, size)]
            mf, jobs = issued_mfmas(sets, N, gran_miss)
            read = jobs * 32 * ((N + 3) // 4)  # two tiles of sixteen columns a job
            dev.set_gram(sets[:1], w)  # warm-up of the code objects
            times = []
            for _ in range(args.reps):
                dev.set_gram(sets, w)
                times.append(dev.last_set_gram_ms())
            ms = float(np.median(times))
            rec = {"n": N, "m": M, "set_size": size, "sets": len(sets), "missing": miss, "jobs": jobs,
                   "set_gram": {"device_ms": round(ms, 3), "device_ms_all": [round(x, 3) for x in times],
                                "us_per_set": round(1e3 * ms / len(sets), 2), "bed_read_gbps": round(read / (ms * 1e-3) / 1e9, 1),
                                "frac_of_copy_ceiling": round(read / (ms * 1e-3) / 1e9 / ceiling, 3), "issued_mfmas": mf,
                                "issued_frac_of_i8_mfma_rate": round(mf * MFMA_MACS / (ms * 1e-3) / I8_MACS, 4)}}
            # before: the set's codes to the host, w o g_k there, class sums of at most 32 vectors a pass (timed on the first sets only)
            nb = min(len(sets), 4)
            dev_ms, t0, worst = 0.0, time.perf_counter(), 0.0
            for idx in sets[:nb]:
                m0 = int(idx[0])
                codes = synth.unpack_bed_columns(dev.get_bed(m0, size), N)
                g = np.where(codes == 3, 0, codes).astype(np.float64)
                GG = np.zeros((size, size))
                for k0 in range(0, size, 32):
                    S = dev.marker_class_sums(w * g[k0:k0 + 32], m0=m0, count=size)
                    dev_ms += dev.last_marker_class_sums_ms()
                    GG[:, k0:k0 + 32] = S[:, :, 1] + 2.0 * S[:, :, 2]
                worst = max(worst, float(np.max(np.abs(GG - GG.T)) / np.max(np.abs(GG))))
            wall = time.perf_counter() - t0
            rec["class_sums_route"] = {"sets_timed": nb, "device_ms_per_set": round(dev_ms / nb, 3), "wall_ms_per_set": round(1e3 * wall / nb, 3),
                                       "device_ms_all_sets": round(dev_ms / nb * len(sets), 3), "gg_asymmetry": worst}
            rec["set_gram_over_class_sums_device"] = round(ms / (dev_ms / nb * len(sets)), 4)
            emit(rec)
        dev.close()


if __name__ == "__main__":
    main()
