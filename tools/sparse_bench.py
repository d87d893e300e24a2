"""Device time of hgibbs_sparse_get (ordered compaction of the 2-bit image into hydra's three index lists) and of feeding those lists
back through hgibbs_sparse_begin / _put / _end, on a synthetic shard made in HBM (hgibbs_synth_bed).

For N individuals x M markers and missing-call rates 0 and 1 %: get_ms and put_ms (HIP events around the kernels; medians over the
repeats), each as bytes moved -- 2 bits a genotype on the image's side and 4 bytes an entry on the lists' side -- over the
device-to-device copy rate hgibbs_stream_ceiling measures in the same job, and beside them the wall time of the numpy restatement
(tests/sparse_restate.py) on the host for the first --host-cols of the same columns, with its extrapolation to M columns.  One JSON
line per case; --out appends them to a file.

    python tools/sparse_bench.py [--n 500000] [--m 4096] [--missing 0,0.01] [--reps 3] [--host-cols 128] [--out profiles/sparse_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sparse_restate as sr  # noqa: E402
from hydra_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--missing", default="0,0.01")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-cols", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    N, M = args.n, args.m
    small = capi.Device(0)  # warm-up of the code objects on a few rows
    small.synth_bed(64, 64, seed=5, missing_rate=0.1)
    lists = small.sparse_get()
    small.close()
    for miss in [float(x) for x in args.missing.split(",")]:
        dev = capi.Device(0)
        dev.synth_bed(N, M, seed=5, missing_rate=miss)
        ceiling = dev.stream_ceiling(1 << 30, 10)
        cnt = dev.sparse_counts()
        get = []
        for _ in range(args.reps):
            lists = dev.sparse_get()
            get.append(dev.last_sparse_ms()[1])
        entries = [int(c.sum()) for c in cnt]
        # the restatement on the host, on the first columns
        hc = min(args.host_cols, M)
        bed = dev.get_bed(0, hc)
        t0 = time.perf_counter()
        host = sr.bed_to_lists(bed, N)
        host_s = time.perf_counter() - t0
        for c, n, idx in zip(sr.CLASSES, cnt, lists):
            assert np.array_equal(host["sl" + c], n[:hc]) and np.array_equal(host["si" + c], idx[:host["si" + c].size]), c
        # the lists fed back
        ls = []
        for n, idx in zip(cnt, lists):
            ss = np.zeros(M, dtype=np.uint64)
            ss[1:] = np.cumsum(n)[:-1]
            ls.append((ss, n, idx, 0))
        put = []
        for _ in range(args.reps):
            back = capi.Device(0)
            back.sparse_begin(N, M)
            back.sparse_put(0, ls)
            back.sparse_end()
            put.append(back.last_sparse_ms()[0])
            same = np.array_equal(back.get_bed(0, hc), bed) and np.array_equal(back.get_bed(M - 1, 1), dev.get_bed(M - 1, 1))
            back.close()
            assert same, "the lists fed back do not reproduce the image"
        g, p = float(np.median(get)), float(np.median(put))
        image_bytes, list_bytes = N * M / 4.0, 4.0 * sum(entries)
        moved = image_bytes + list_bytes
        rec = {"op": "sparse", "n": N, "m": M, "missing": miss, "entries": entries, "get_ms": round(g, 3), "put_ms": round(p, 3),
               "get_ms_all": [round(x, 3) for x in get], "put_ms_all": [round(x, 3) for x in put],
               "bytes_moved": int(moved), "stream_ceiling_gbps": round(ceiling, 1),
               "get_gbps": round(moved / (g * 1e-3) / 1e9, 1), "put_gbps": round(moved / (p * 1e-3) / 1e9, 1),
               "get_share_of_ceiling": round(moved / (g * 1e-3) / 1e9 / ceiling, 4), "put_share_of_ceiling": round(moved / (p * 1e-3) / 1e9 / ceiling, 4),
               "host_numpy_cols": hc, "host_numpy_s": round(host_s, 3), "host_numpy_s_for_m": round(host_s * M / hc, 1)}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        dev.close()


if __name__ == "__main__":
    main()
