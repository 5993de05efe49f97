#!/usr/bin/env python3
"""Timing of the schema-evolution conversion kernel (convert_kernels.hip)
against `timestamp_kernel` at equal byte traffic, in one process.

Two conversions over n values with a 10 % null mask, each launch timed singly
with HIP events (orcg_convert_bench):

  bigint -> int                          8 + 1 B read, 8 + 1 B written: 18 B a value
  decimal(30,3) -> decimal(38,6)         16 + 1 B read, 16 + 1 B written: 34 B a value

and, as the yardstick of each, `timestamp_kernel` (orcg_timestamp_tz_bench
mode 0: two int64 read and written in place, 32 B a value) over as many
values as move the same bytes. The legs are interleaved round by round; the
median over all launches of a leg is reported. One JSON line per leg goes to
stdout and, with --out, to a file.

    python scripts/ab_convert.py --n 10000000 --out profiles/convert/ab_<commit>.jsonl
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="timed launches per leg per round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tzdir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                                                    "golden", "tz"))
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import orc_amd
    from orc_amd import _lib, rle

    L = _lib.load()
    ctx = orc_amd.Context(0)
    with open(os.path.join(args.tzdir, "GMT"), "rb") as f:
        gmt = orc_amd.Timezone.parse("GMT", f.read())
    rng = np.random.default_rng(11)
    n = args.n
    mask = torch.from_numpy((rng.random(n) >= 0.1).astype(np.uint8)).cuda()
    # bigint values of which about 1 in 16 does not fit int; decimal(30,3)
    # unscaled values of up to 29 digits as [hi, lo] pairs (all fit decimal(38,6))
    ints = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64)
    ints[rng.random(n) < 1 / 16] <<= 8
    hi = rng.integers(-(1 << 32), 1 << 32, size=n, dtype=np.int64)
    lo = rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64)
    legs = {
        "bigint->int": dict(src=torch.from_numpy(ints).cuda(), cls=rle.CONVERT_INT64, src_scale=0, kind=3, p=0, s=0,
                            out=torch.empty(n, dtype=torch.int64, device="cuda"), bytes=18),
        "decimal(30,3)->decimal(38,6)": dict(src=torch.from_numpy(np.stack([hi, lo], axis=1).copy()).cuda(),
                                             cls=rle.CONVERT_DECIMAL128, src_scale=3, kind=14, p=38, s=6,
                                             out=torch.empty((n, 2), dtype=torch.int64, device="cuda"), bytes=34),
    }
    out_nn = torch.empty(n, dtype=torch.uint8, device="cuda")
    # the yardstick's arrays: the larger of the two sizes, a prefix for the smaller
    n_ts = {name: leg["bytes"] * n // 32 for name, leg in legs.items()}
    cap = max(n_ts.values())
    secs = torch.from_numpy(rng.integers(0, 1 << 31, size=cap, dtype=np.int64)).cuda()
    nanos = torch.from_numpy(rng.integers(0, 1_000_000, size=cap, dtype=np.int64) << 3).cuda()
    d_s, d_n = torch.empty_like(secs), torch.empty_like(nanos)
    torch.cuda.synchronize()

    def run_convert(leg, iters):
        ms = (ctypes.c_double * iters)()
        _lib.check(L.orcg_convert_bench(ctx.handle, leg["src"].data_ptr(), leg["cls"], leg["src_scale"], n,
                                        mask.data_ptr(), leg["kind"], leg["p"], leg["s"], leg["out"].data_ptr(),
                                        out_nn.data_ptr(), iters, ms), ctx.last_error)
        return list(ms)

    def run_timestamp(count, iters):
        ms = (ctypes.c_double * iters)()
        _lib.check(L.orcg_timestamp_tz_bench(ctx.handle, secs.data_ptr(), nanos.data_ptr(), d_s.data_ptr(),
                                             d_n.data_ptr(), count, gmt.handle, gmt.handle, 0, iters, ms),
                   ctx.last_error)
        return list(ms)

    times = {}
    for name, leg in legs.items():
        times[name], times["timestamp_kernel for " + name] = [], []
        run_convert(leg, args.warmup)
        run_timestamp(n_ts[name], args.warmup)
    for _ in range(args.rounds):
        for name, leg in legs.items():
            times[name].extend(run_convert(leg, args.iters))
            times["timestamp_kernel for " + name].extend(run_timestamp(n_ts[name], args.iters))
    lines = []
    for name, leg in legs.items():
        for key, count, per in ((name, n, leg["bytes"]), ("timestamp_kernel for " + name, n_ts[name], 32)):
            t = np.array(times[key])
            med = float(np.median(t))
            lines.append({"leg": key, "values": count, "bytes_per_value": per, "median_us": round(med * 1e3, 2),
                          "p10_us": round(float(np.percentile(t, 10)) * 1e3, 2),
                          "p90_us": round(float(np.percentile(t, 90)) * 1e3, 2), "launches": int(t.size),
                          "algorithmic_GBps": round(per * count / (med * 1e-3) / 1e9, 1)})
        lines[-2]["vs_timestamp_kernel"] = round(lines[-2]["median_us"] / lines[-1]["median_us"], 3)
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
