#!/usr/bin/env python3
"""Timing of the Arrow export kernels (arrow_kernels.hip) against
`timestamp_kernel` at equal byte traffic, in one process (as ab_convert.py
times the conversion kernel).

Legs over n values, each launch timed singly with HIP events
(orcg_arrow_bench), bytes a value = what the algorithm reads and writes:

  validity                 1 read, 1/8 written
  int64 -> int32           8 read, 4 written
  int64 -> int8            8 read, 1 written
  double -> float32        8 read, 4 written
  decimal64 -> decimal128  8 read, 16 written
  decimal128 swap          16 read, 16 written
  timestamp -> ns          16 read, 8 written
  dictionary gather        8 (index) + 4 (offsets) read, the row's bytes written
                           (the dictionary itself stays in cache)

and, as the yardstick of each, `timestamp_kernel` (orcg_timestamp_tz_bench
mode 0: 32 B a value) over as many values as move the same bytes. Legs are
interleaved round by round; the median over all launches of a leg is reported.

    python scripts/ab_arrow.py --n 10000000 --out profiles/arrow/ab_<commit>.jsonl
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20, help="timed launches per leg per round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tzdir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                                                    "golden", "tz"))
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import orc_amd
    from orc_amd import _lib
    from orc_amd import arrow as A

    L = _lib.load()
    ctx = orc_amd.Context(0)
    with open(os.path.join(args.tzdir, "GMT"), "rb") as f:
        gmt = orc_amd.Timezone.parse("GMT", f.read())
    rng = np.random.default_rng(11)
    n = args.n

    def cuda(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    mask = cuda((rng.random(n) >= 0.1).astype(np.uint8))
    i64 = cuda(rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64))
    i64b = cuda(rng.integers(0, 10 ** 9, size=n, dtype=np.int64))
    f64 = cuda(rng.standard_normal(n).astype(np.float32).astype(np.float64))
    pairs = cuda(rng.integers(-(1 << 62), 1 << 62, size=(n, 2), dtype=np.int64))
    # a dictionary of 1,000 entries of 1 to 33 bytes: about 17 bytes a row
    entries = [bytes([97 + k % 26]) * (1 + k % 33) for k in range(1000)]
    doff = cuda(np.concatenate([[0], np.cumsum([len(e) for e in entries])]).astype(np.int64))
    blob = cuda(np.frombuffer(b"".join(entries), np.uint8))
    index = cuda(rng.integers(0, len(entries), size=n, dtype=np.int64))
    offs, gathered, total = A.dict_strings_device(ctx, index, None, doff, blob)
    out = torch.empty(A.padded(16 * n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def leg(kind, form, p, per, out_t=out, out_bytes=None, **kw):
        return dict(kind=kind, form=form, p=p, bytes=per, out=out_t, out_bytes=out_bytes, **kw)

    fx = lambda form, src, src2, per: leg(1, form, [src, src2, None, None], per,  # noqa: E731
                                          out_bytes=A.padded(A.fixed_bytes(form, n)))
    legs = {
        "validity": leg(0, 0, [mask, None, None, None], 1.125, out_bytes=A.padded((n + 7) // 8)),
        "int64->int32": fx(A.INT32, i64, None, 12),
        "int64->int8": fx(A.INT8, i64, None, 9),
        "double->float32": fx(A.FLOAT32, f64, None, 12),
        "decimal64->decimal128": fx(A.DEC64, i64, None, 24),
        "decimal128 swap": fx(A.DEC128, pairs, None, 32),
        "timestamp->ns": fx(A.TIMESTAMP_NS, i64, i64b, 24),
        "dictionary gather": leg(2, 0, [offs, index, doff, blob], 12 + total / n, out_t=gathered,
                                 out_bytes=gathered.numel(), dict_size=len(entries), blob_len=blob.numel(),
                                 total=total),
    }
    n_ts = {name: max(1, int(x["bytes"] * n) // 32) for name, x in legs.items()}
    cap = max(n_ts.values())
    secs = cuda(rng.integers(0, 1 << 31, size=cap, dtype=np.int64))
    nanos = cuda(rng.integers(0, 1_000_000, size=cap, dtype=np.int64) << 3)
    d_s, d_n = torch.empty_like(secs), torch.empty_like(nanos)
    torch.cuda.synchronize()

    def ptr(t):
        return None if t is None else t.data_ptr()

    def run_leg(x, iters):
        ms = (ctypes.c_double * iters)()
        p = x["p"]
        _lib.check(L.orcg_arrow_bench(ctx.handle, x["kind"], x["form"], ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(p[3]), n,
                                      x.get("dict_size", 0), x.get("blob_len", 0), x["out"].data_ptr(),
                                      x["out_bytes"], x.get("total", 0), iters, ms), ctx.last_error)
        return list(ms)

    def run_timestamp(count, iters):
        ms = (ctypes.c_double * iters)()
        _lib.check(L.orcg_timestamp_tz_bench(ctx.handle, secs.data_ptr(), nanos.data_ptr(), d_s.data_ptr(),
                                             d_n.data_ptr(), count, gmt.handle, gmt.handle, 0, iters, ms),
                   ctx.last_error)
        return list(ms)

    times = {}
    for name, x in legs.items():
        times[name], times["timestamp_kernel for " + name] = [], []
        run_leg(x, args.warmup)
        run_timestamp(n_ts[name], args.warmup)
    for _ in range(args.rounds):
        for name, x in legs.items():
            times[name].extend(run_leg(x, args.iters))
            times["timestamp_kernel for " + name].extend(run_timestamp(n_ts[name], args.iters))
    lines = []
    for name, x in legs.items():
        for key, count, per in ((name, n, x["bytes"]), ("timestamp_kernel for " + name, n_ts[name], 32)):
            t = np.array(times[key])
            med = float(np.median(t))
            lines.append({"leg": key, "values": count, "bytes_per_value": round(per, 3),
                          "median_us": round(med * 1e3, 2), "p10_us": round(float(np.percentile(t, 10)) * 1e3, 2),
                          "p90_us": round(float(np.percentile(t, 90)) * 1e3, 2), "launches": int(t.size),
                          "algorithmic_GBps": round(per * count / (med * 1e-3) / 1e9, 1)})
        lines[-2]["vs_timestamp_kernel"] = round(lines[-2]["median_us"] / lines[-1]["median_us"], 3)
    out_f = open(args.out, "w") if args.out else None
    for x in lines:
        s = json.dumps(x)
        print(s)
        if out_f:
            out_f.write(s + "\n")
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
