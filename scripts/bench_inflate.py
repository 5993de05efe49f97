#!/usr/bin/env python3
"""Device decompression (orcg_reader_set_device_decompression) against the host
inflate, on DESIGN.md §6 item 9's workload: a pyarrow-written file of about
2 M rows of compressible, DIRECT-encoded strings and doubles, 256 KB
compression blocks, once with Snappy and once with LZ4 (written into a
temporary directory; compression_strategy="compression", without which this
writer's LZ4 stores every chunk).

Every stripe is read with the setting off and with it on. The two legs
alternate in one process, each after a warm-up read of its own. Per leg and
repetition, summed over the file's stripes:

  wall_s      host clock around orcg_reader_read_stripe (synchronous)
  t_decomp_s  the host's decompression phase of prepare() (with the setting
              on: the size walk / preamble read of the planned chunks and the
              inflate of every other stream)
  stage_bytes bytes of the stripe's one upload
  device_s    orcg_reader_bench_stripe_decode's device time (the inflate launch
              and the decodes; the stripe prepared once, decoded --steady times)

One JSON line per codec and leg with the median, min and max over the
repetitions, and the chunks / bytes inflated on the device. No threshold: the
setting stays off whatever comes out. The inflate kernels' own time comes from
a separate run under `rocprofv3 --kernel-trace --stats` (--reps 2 --steady 0
is enough there), never from this one.

    python scripts/bench_inflate.py [--rows 2000000] [--reps 10] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_table(rows, seed=7):
    """Unique sentences over a 40-word vocabulary (direct encoding, compressible)
    and doubles on a grid of 1,000 values."""
    import pyarrow as pa

    rng = np.random.default_rng(seed)
    words = np.array(["w%03d" % i for i in range(40)])
    base = words[rng.integers(0, 40, 4096 * 12)].reshape(4096, 12)
    sentences = np.array([" ".join(r) for r in base])
    text = np.char.add(np.char.add(sentences[rng.integers(0, 4096, rows)], " #"), np.arange(rows).astype(str))
    return pa.table({"text": pa.array(text), "d": pa.array(rng.integers(0, 1000, rows) * 0.125),
                     "e": pa.array(rng.integers(0, 50, rows).astype(np.float64))})


def write_file(table, path, codec, block, stripe_bytes):
    import pyarrow.orc as po

    po.write_table(table, path, compression=codec, compression_block_size=block, stripe_size=stripe_bytes,
                   dictionary_key_size_threshold=0.0, compression_strategy="compression")


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def one_pass(r, steady):
    """Every stripe read once: the sums of the docstring's figures."""
    import orc_amd

    wall = decomp = device = 0.0
    staged = chunks = nbytes = 0
    for s in range(r.num_stripes):
        t0 = time.perf_counter()
        r.read_stripe_device(s)
        wall += time.perf_counter() - t0
        decomp += r.last_timings()["host_decompress_s"]
        staged += r.last_stream_stats()["stage_bytes"]
        c, b = r.last_device_inflate()
        chunks += c
        nbytes += b
        if steady:
            dec, h2d = ctypes.c_double(), ctypes.c_double()
            orc_amd._lib.check(r._L.orcg_reader_bench_stripe_decode(r._h, s, steady, ctypes.byref(dec),
                                                                    ctypes.byref(h2d)), r._err)
            device += dec.value
    return {"wall_s": wall, "t_decomp_s": decomp, "stage_bytes": staged, "device_s": device,
            "device_chunks": chunks, "device_bytes": nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=10, help="timed reads per leg")
    ap.add_argument("--steady", type=int, default=5, help="decodes per stripe for the device time (0: skip)")
    ap.add_argument("--block", type=int, default=262144)
    ap.add_argument("--stripe-mb", type=int, default=16)
    ap.add_argument("--codecs", default="snappy,lz4")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_inflate.py needs a GPU: a host run measures nothing")
    import orc_amd

    ctx = orc_amd.Context(0)
    table = make_table(args.rows)
    lines = []
    with tempfile.TemporaryDirectory() as d:
        for codec in args.codecs.split(","):
            path = os.path.join(d, codec + ".orc")
            write_file(table, path, codec, args.block, args.stripe_mb << 20)
            data = open(path, "rb").read()
            readers = {}
            for leg in ("off", "on"):
                readers[leg] = orc_amd.Reader(data, ctx)
                readers[leg].set_device_decompression(leg == "on")
                one_pass(readers[leg], args.steady)  # warm-up: code objects, pinned staging, device buffers
            runs = {"off": [], "on": []}
            for _ in range(args.reps):
                for leg in ("off", "on"):
                    runs[leg].append(one_pass(readers[leg], args.steady))
            for leg in ("off", "on"):
                r = readers[leg]
                line = {"bench": "inflate", "codec": codec, "device_decompression": leg, "rows": args.rows,
                        "file_bytes": len(data), "stripes": r.num_stripes, "block": args.block, "reps": args.reps,
                        "steady": args.steady, "device_chunks": runs[leg][0]["device_chunks"],
                        "device_bytes": runs[leg][0]["device_bytes"], "stage_bytes": runs[leg][0]["stage_bytes"]}
                for k in ("wall_s", "t_decomp_s", "device_s"):
                    line[k] = {a: round(b, 6) for a, b in stats([x[k] for x in runs[leg]]).items()}
                line["wall_per_stripe_ms"] = round(1e3 * line["wall_s"]["median"] / r.num_stripes, 4)
                lines.append(line)
                print(json.dumps(line), flush=True)
            del readers
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
