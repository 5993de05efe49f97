#!/usr/bin/env python3
"""End-to-end cost of the Arrow export against the reader's host batches, one
process, legs interleaved round by round on one stripe of two files written
here with pyarrow (10 % nulls in every column):

  narrow   tinyint + int + a low-cardinality (dictionary-encoded) string
  bigint   four bigint columns: nothing to narrow but the validity

Legs: Reader.read_stripe (decode, wide D2H, numpy re-layout: the only host
path before the export), Reader.read_stripe_arrow (decode, re-layout in HBM,
narrow D2H, pyarrow import), Reader.read_stripe_device (the decode alone).
Host clock around calls that end in a stream synchronisation; medians.

    python scripts/bench_arrow_export.py --rows 2000000 --out profiles/arrow/e2e_<commit>.jsonl
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def files(rows, rng):
    import pyarrow as pa
    import pyarrow.orc as po

    def nulls(a):
        return pa.array(a, mask=rng.random(rows) < 0.1)

    words = np.array(["alpha", "", "beta-gamma", "x" * 40, "delta", "epsilon", "zeta"], dtype=object)
    narrow = pa.table({"t": nulls(rng.integers(-128, 128, rows).astype(np.int8)),
                       "i": nulls(rng.integers(-2 ** 31, 2 ** 31, rows).astype(np.int32)),
                       "s": nulls(words[rng.integers(0, len(words), rows)])})
    wide = pa.table({"c%d" % k: nulls(rng.integers(-2 ** 62, 2 ** 62, rows)) for k in range(4)})
    out = {}
    for name, t in (("narrow", narrow), ("bigint", wide)):
        buf = io.BytesIO()
        po.write_table(t, buf, compression="zstd", stripe_size=1 << 30, batch_size=rows,
                       dictionary_key_size_threshold=0.5)
        out[name] = (buf.getvalue(), t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()

    import pyarrow.orc as po

    import orc_amd

    ctx = orc_amd.Context(0)
    lines = []
    for name, (data, table) in files(args.rows, np.random.default_rng(3)).items():
        assert po.ORCFile(io.BytesIO(data)).nstripes == 1
        r = orc_amd.Reader(data, ctx)
        assert r.read_arrow().equals(table)
        legs = {"read_stripe": lambda: r.read_stripe(0), "read_stripe_arrow": lambda: r.read_stripe_arrow(0),
                "read_stripe_device": lambda: r.read_stripe_device(0)}
        times = {k: [] for k in legs}
        for k, f in legs.items():
            for _ in range(args.warmup):
                f()
        for _ in range(args.rounds):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                times[k].append(time.perf_counter() - t0)
        for k in legs:
            t = np.array(times[k]) * 1e3
            lines.append({"file": name, "rows": args.rows, "file_bytes": len(data), "leg": k,
                          "median_ms": round(float(np.median(t)), 3), "p10_ms": round(float(np.percentile(t, 10)), 3),
                          "p90_ms": round(float(np.percentile(t, 90)), 3), "rounds": int(t.size)})
    out = open(args.out, "w") if args.out else None
    for x in lines:
        s = json.dumps(x)
        print(s)
        if out:
            out.write(s + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
