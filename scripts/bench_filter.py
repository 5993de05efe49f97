#!/usr/bin/env python3
"""Row-level filter measurements: one stripe of the
C4-style file scripts/bench_file.py writes (tests/workload_files.py make_c4:
TPC-H lineitem-like, 16 columns), filtered by

  int64 ~1 % / ~50 % / 100 %   l_partkey < 200,001 / 10,000,001 / 20,000,001
  dictionary string            l_shipmode = "RAIL"  (1 of 7 entries)
  three leaves                 (l_partkey < 10,000,001 AND l_shipmode = "AIR") OR l_quantity < 2.00

Per case:
  * each kernel's time (HIP events around its launches, orcg_filter_set_timing)
    and the bytes/s it achieves against the bytes it must read and write, twice:
    "warm" (run after run over the same columns, which then sit in the
    last-level cache) and "flushed" (a 1 GiB buffer written between runs, so
    the columns come from HBM); the gathers of all columns as one figure (a
    host clock around the 16 launches, each with its synchronisation);
  * read_stripe(filter=...) end to end, and its parts by a host clock: decode,
    filter run, gathers, then the D2H and host handling of the filtered batch;
  * the comparison leg, the only thing a reader without filters can do: the
    unfiltered read_stripe with its full D2H, then the same predicate and the
    row gather with numpy on the host. The two reads alternate, run by run.
Every figure is the median of --repeats runs after --warmup, with min and max.
One JSON line per case on stdout (and in --out, which a run replaces).

    python scripts/bench_filter.py [--rows 2000000] [--repeats 9] [--out profiles/filter/bench_filter.jsonl]
"""
import argparse
import ctypes
import decimal
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from workload_files import make_c4  # noqa: E402

T = 1024  # rows of a combine / select tile


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def timed_pair(fa, fb, warmup, repeats):
    """fa and fb alternating, run by run: neither leg has the process's first
    runs, or a quieter moment of the machine, to itself"""
    a, b = [], []
    for k in range(warmup + repeats):
        for fn, out in ((fa, a), (fb, b)):
            t = time.perf_counter()
            fn()
            if k >= warmup:
                out.append((time.perf_counter() - t) * 1e3)
    return a, b


def host_filter(batch, mask):
    """the rows of every column a host consumer would keep (numpy indexing)"""
    idx = np.flatnonzero(mask)
    kept = 0
    for c in batch.columns.values():
        for name in ("not_null", "data", "length", "index", "secondary"):
            a = getattr(c, name)
            if a is not None and len(a) == c.num_elements:
                kept += a[idx].nbytes
    return idx, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded in each line (default: git rev-parse HEAD)")
    ap.add_argument("--parent-commit", default=None, help="recorded in each line (default: git rev-parse HEAD~1)")
    args = ap.parse_args()

    import orc_amd
    from orc_amd import SearchArgumentBuilder as B
    from orc_amd.reader import DECIMAL

    if args.out:  # a run replaces the file: its lines have one shape and one build
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()

    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                           text=True).stdout.strip() or "working tree"
    parent = args.parent_commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD~1"],
                                                  capture_output=True, text=True).stdout.strip() or None
    import torch

    flush_buf = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")

    def flush():
        flush_buf.add_(1)
        torch.cuda.synchronize()

    tmp = tempfile.mkdtemp(prefix="bench_filter_")
    path = os.path.join(tmp, "c4.orc")
    make_c4(path, args.rows, 512)  # one stripe
    r = orc_amd.open_reader(path)
    L = r._L
    n = r.stripe(0)["num_rows"]
    ids = dict(zip(r.types[0].field_names, r.types[0].subtypes))
    D = decimal.Decimal
    cases = [
        ("int64 ~1%", B().less_than("l_partkey", 200_001).build(), lambda b: col(b, "l_partkey") < 200_001, ["l_partkey"]),
        ("int64 ~50%", B().less_than("l_partkey", 10_000_001).build(), lambda b: col(b, "l_partkey") < 10_000_001,
         ["l_partkey"]),
        ("int64 100%", B().less_than("l_partkey", 20_000_001).build(), lambda b: col(b, "l_partkey") < 20_000_001,
         ["l_partkey"]),
        ("dictionary string =", B().equals("l_shipmode", "RAIL").build(), lambda b: dict_eq(b, "l_shipmode", b"RAIL"),
         ["l_shipmode"]),
        ("three-leaf and/or",
         B().start_or().start_and().less_than("l_partkey", 10_000_001).equals("l_shipmode", "AIR").end()
         .less_than("l_quantity", D("2.00")).end().build(),
         lambda b: ((col(b, "l_partkey") < 10_000_001) & dict_eq(b, "l_shipmode", b"AIR")) | (col(b, "l_quantity") < 200),
         ["l_partkey", "l_shipmode", "l_quantity"]),
    ]

    def col(b, name):
        return b.columns[ids[name]].data

    def dict_eq(b, name, lit):
        c = b.columns[ids[name]]
        blob, off = c.blob, c.dict_offsets
        hit = np.array([blob[off[e]:off[e + 1]] == lit for e in range(len(off) - 1)])
        return hit[c.index]

    def view_arrays(v):
        """(8-byte arrays, 16-byte arrays, has a mask) a gather of this view moves"""
        wide = v.kind == DECIMAL and r.read_types[v.type_id].precision > 18
        n8 = 0 if wide else sum(1 for p in (v.data, v.length, v.secondary, v.index) if p)
        return n8, int(wide), bool(v.has_nulls and v.not_null)

    for name, sarg, host_pred, leaf_cols in cases:
        h = sarg.handle(L, r._resolve_column)
        r.read_stripe_device(0)
        L.orcg_filter_set_timing(h, 1)
        per = {"warm": [[], [], [], []], "flushed": [[], [], [], []]}
        count = 0
        for mode in ("warm", "flushed"):
            for k in range(args.warmup + args.repeats):
                if mode == "flushed":
                    flush()
                _, count = r.filter_stripe_device(0, sarg)
                ms = (ctypes.c_double * 4)()
                L.orcg_filter_last_timing(h, ms)
                if k >= args.warmup:
                    for j in range(4):
                        per[mode][j].append(ms[j])
        L.orcg_filter_set_timing(h, 0)
        # bytes each kernel must move. string leaf: a dictionary's offsets and
        # bytes, a truth byte per entry. combine: the leaf columns (8 bytes a row),
        # the selected byte per row, the tile counts. select: the selected bytes,
        # the tile bases, 8 bytes per selected row. gather: per selected row the
        # index, and each array and mask byte read and written.
        tiles = (n + T - 1) // T
        string_bytes = 0
        for c in leaf_cols:
            v = r.stripe_column_view(0, ids[c])
            if v.dict_offsets:
                string_bytes += 8 * (v.dict_size + 1) + v.blob_len + v.dict_size
        combine_bytes = 8 * n * len(leaf_cols) + n + 8 * tiles
        select_bytes = n + 8 * tiles + 8 * count
        kernels = {}
        for mode in ("warm", "flushed"):
            kernels[mode] = {}
            for j, (kn, nbytes) in enumerate([("string_leaf", string_bytes), ("combine", combine_bytes),
                                              ("scan", 16 * tiles), ("select", select_bytes)]):
                st = stats(per[mode][j])
                if nbytes and st["median"] > 0:
                    st["bytes"] = nbytes
                    st["GBps"] = round(nbytes / (st["median"] * 1e-3) / 1e9, 1)
                kernels[mode][kn] = st
        # the parts of a filtered read, by a host clock (each ends in a synchronisation)
        parts = {"decode": [], "filter_run": [], "gathers": [], "d2h_and_host": []}
        gather_bytes = 0
        tids = [t.id for t in r.read_types]
        for k in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            r.read_stripe_device(0)
            t1 = time.perf_counter()
            r.filter_stripe_device(0, sarg)
            t2 = time.perf_counter()
            views = [r.filtered_column_view(0, tid) for tid in tids]
            t3 = time.perf_counter()
            for tid, v in zip(tids, views):
                r._column(v, r.read_types[tid])
            t4 = time.perf_counter()
            if k >= args.warmup:
                for key, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    parts[key].append(dt * 1e3)
            gather_bytes = 0
            for tid in tids:
                n8, n16, mask = view_arrays(r.stripe_column_view(0, tid))
                gather_bytes += count * (8 + 16 * n8 + 32 * n16 + 2 * mask)
        parts = {key: stats(v) for key, v in parts.items()}
        parts["gathers"]["launches"] = len(tids)
        parts["gathers"]["bytes"] = gather_bytes
        if parts["gathers"]["median"] > 0:
            parts["gathers"]["GBps"] = round(gather_bytes / (parts["gathers"]["median"] * 1e-3) / 1e9, 2)
        full, filtered = timed_pair(lambda: r.read_stripe(0), lambda: r.read_stripe(0, filter=sarg), args.warmup,
                                    args.repeats)
        batch = r.read_stripe(0)
        host = timed(lambda: host_filter(batch, host_pred(batch)), 1, args.repeats)
        idx, _ = host_filter(batch, host_pred(batch))
        assert np.array_equal(idx, r.filter_stripe(0, sarg)), name
        line = {"bench": "filter", "case": name, "commit": commit, "parent_commit": parent, "rows": int(n),
                "selected": int(count), "selectivity": round(count / n, 4), "kernel_ms": kernels,
                "filtered_read_parts_ms": parts,
                "read_stripe_filtered_ms": stats(filtered),
                "unfiltered_read_stripe_ms": stats(full), "host_numpy_filter_ms": stats(host),
                "unfiltered_plus_host_ms": round(stats(full)["median"] + stats(host)["median"], 3),
                "speedup_vs_unfiltered_plus_host": round((stats(full)["median"] + stats(host)["median"]) /
                                                         stats(filtered)["median"], 3)}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
    os.unlink(path)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
