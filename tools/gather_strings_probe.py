"""What the -a/--all string columns add to the device shard merge (lm_merge_sharded_device_ex, lexicmap_amd/csrc/lm_merge.hip).

Builds synthetic shard rows and their strings in the wire form (include/lexicmap_hip.h) in device memory - by default 4 shards x
250 000 rows with about 3 kb of strings per row, about 3 GB of blocks - and times the merge without and with the strings after
warm-up, beside the device-to-host rate of a pinned download of the same bytes:

    python tools/gather_strings_probe.py [--shards 4 --rows 250000 --row-bytes 3000] --json out.json

The copy kernels' time comes from a separate kernel-trace run of the same command:

    rocprofv3 --kernel-trace --stats -d DIR -o probe -- python tools/gather_strings_probe.py --reps 3
    python tools/gather_strings_probe.py --summarize DIR/.../probe_results.db --json out.json

which adds the copy kernels' time and their string bytes (read + written) over that time against the 8 TB/s HBM peak
(--summarize reads the rocpd database rocprofv3 writes by default, or the <prefix>_kernel_stats.csv of --output-format csv)."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
COPY_KERNELS = ("k_mg_copy_head", "k_mg_copy_tail")


def build(args):
    import numpy as np
    import torch
    from lexicmap_amd import merge
    rng = np.random.default_rng(5)
    n = args.shards * args.rows
    rows = np.zeros(n, dtype=merge.ROW_DTYPE)
    for r in range(args.shards):
        sl = slice(r * args.rows, (r + 1) * args.rows)
        qs = np.sort(rng.integers(0, args.queries, args.rows))
        gs = rng.integers(0, 400, args.rows) * args.shards + r     # a genome lives in ONE shard
        o = np.lexsort((gs, qs))
        rows["query"][sl], rows["batch_genome"][sl] = qs[o], gs[o]
    rows["bitscore"] = rng.integers(50, 3000, n)
    rows["pident"] = rng.integers(70, 101, n).astype(np.float64)
    # cigar ~ 1 % of the row's bytes, qseq / sseq / align a third of the rest each (lengths vary by +-50 %)
    third = np.maximum(1, (args.row_bytes * 0.33 * rng.uniform(0.5, 1.5, n)).astype(np.int64))
    lens = np.stack([np.maximum(1, third // 33), third, third, third], axis=1).astype(np.uint32)
    blk = ((lens.astype(np.int64) + 1).sum(axis=1) + 15) // 16 * 16
    nbytes = int(blk.sum())
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    d_str = torch.empty(n * 16 + nbytes, dtype=torch.uint8, device="cuda")
    d_str[:n * 16] = torch.from_numpy(lens.view(np.uint8).reshape(-1).copy()).cuda()
    d_str[n * 16:] = torch.randint(65, 91, (nbytes,), dtype=torch.uint8, device="cuda")   # (the bytes are not read as text here)
    torch.cuda.synchronize()
    return d_rows, d_str, nbytes, [args.rows] * args.shards


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def probe(args):
    import torch
    from lexicmap_amd.api import Comm
    d_rows, d_str, nbytes, counts = build(args)
    comm = Comm(Comm.unique_id(), 1, 0, device=0)
    plain = lambda: comm.merge_sharded_device(d_rows.data_ptr(), counts)
    strs = lambda: comm.merge_sharded_device(d_rows.data_ptr(), counts, strings_ptr=d_str.data_ptr(), string_bytes=nbytes)
    for _ in range(args.warmup):
        plain()
        strs()
    t_plain = timed(plain, args.reps)
    t_strs = timed(strs, args.reps)
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    src = d_str[d_str.numel() - nbytes:]

    def d2h():
        host.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
    d2h()
    t_d2h = timed(d2h, args.reps)
    comm.close()
    extra = t_strs - t_plain
    return dict(shards=args.shards, rows=sum(counts), string_bytes=nbytes, bytes_per_row=nbytes / sum(counts),
                merge_s_without_strings=t_plain, merge_s_with_strings=t_strs, extra_s=extra,
                d2h_GBps=nbytes / t_d2h / 1e9, blob_download_s=t_d2h, extra_over_download=extra / t_d2h, reps=args.reps)


def kernel_totals(path):
    """(name, calls, total ns) per kernel of a rocprofv3 run: its rocpd database (.db) or its kernel stats CSV"""
    if path.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(path)
        rows = db.execute("select name, count(*), sum(duration) from kernels group by name").fetchall()
        db.close()
        return [(n, int(c), float(t)) for n, c, t in rows]
    with open(path) as f:
        return [(r.get("Name", ""), int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)]


def summarize(path, out):
    """the copy kernels' time per merge (rocprofv3 kernel trace) and their rate: every string byte is read once and written once"""
    tot_ns, calls = {}, {}
    for name, n, ns in kernel_totals(path):
        for k in COPY_KERNELS:
            if name.split("(")[0].split("<")[0].endswith(k):
                tot_ns[k] = tot_ns.get(k, 0.0) + ns
                calls[k] = calls.get(k, 0) + n
    if not calls:
        raise SystemExit("no copy kernel in %s" % path)
    merges = calls[COPY_KERNELS[0]]
    per_merge = sum(tot_ns.values()) / merges * 1e-9
    out["copy_kernel_s_per_merge"] = per_merge
    out["copy_kernel_calls"] = calls
    out["copy_kernel_TBps"] = 2 * out["string_bytes"] / per_merge / 1e12
    out["copy_kernel_fraction_of_8TBps"] = 2 * out["string_bytes"] / per_merge / HBM_PEAK
    out["copy_kernel_over_download"] = per_merge / out["blob_download_s"]
    out["trace"] = os.path.basename(path)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shards", type=int, default=4)
    p.add_argument("--rows", type=int, default=250_000, help="rows per shard")
    p.add_argument("--row-bytes", type=int, default=3000, help="mean string bytes per row")
    p.add_argument("--queries", type=int, default=20_000)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--json", default="", help="write the result here (read back and extended by --summarize)")
    p.add_argument("--summarize", default=None, metavar="TRACE", help="a rocprofv3 results .db or kernel stats .csv of this tool")
    args = p.parse_args()
    if args.summarize is not None:
        if not args.summarize or not args.json:
            raise SystemExit("--summarize needs the trace file and --json (the untraced run's result)")
        out = summarize(args.summarize, json.load(open(args.json)))
    else:
        out = probe(args)
    line = json.dumps(out, sort_keys=True)
    print(line)
    if args.json:
        open(args.json, "w").write(line + "\n")


if __name__ == "__main__":
    main()
