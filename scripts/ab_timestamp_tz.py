#!/usr/bin/env python3
"""A/B of the zone-adjusting timestamp kernel (decimal_kernels.hip).

Times, per launch with HIP events (orcg_timestamp_tz_bench: every launch on a
fresh device copy of the inputs, after untimed warm-up launches of the same
shape), n values through two legs on the same arrays:

  plain      timestamp_kernel with the writer zone's epoch: no adjustment.
             The kernel is byte for byte the parent commit's (the baseline).
  tz         timestamp_tz_kernel, America/Los_Angeles -> GMT

on two inputs: `clustered` (one day of timestamps) and `spread` (uniform over
1900-2100). The legs are interleaved round by round, so that clock and
temperature drift hits all of them alike. One JSON line per (input, leg) goes
to stdout and, with --out, to a file. 32 algorithmic bytes per value (two
int64 read, two written).

    python scripts/ab_timestamp_tz.py --n 10000000 --out profiles/tz/ab_<commit>.jsonl
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = [("plain", 0), ("tz", 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="timed launches per leg per round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tzdir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                                                    "golden", "tz"))
    ap.add_argument("--writer", default="America/Los_Angeles")
    ap.add_argument("--reader", default="GMT")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import orc_amd
    from orc_amd import _lib

    L = _lib.load()
    ctx = orc_amd.Context(0)

    def zone(name):
        with open(os.path.join(args.tzdir, name), "rb") as f:
            return orc_amd.Timezone.parse(name, f.read())

    w, r = zone(args.writer), zone(args.reader)
    rng = np.random.default_rng(3)
    n = args.n
    nanos = (rng.integers(0, 1_000_000, size=n, dtype=np.int64) << 3) | rng.integers(0, 8, size=n, dtype=np.int64)
    inputs = {
        # 2023-06-15, one day; raw stream values are relative to the writer's epoch
        "clustered": rng.integers(1686787200, 1686787200 + 86400, size=n, dtype=np.int64) - w.epoch(),
        "spread": rng.integers(-2208988800, 4102444800, size=n, dtype=np.int64) - w.epoch(),
    }
    lines = []
    for name, secs in inputs.items():
        d_in_s, d_in_n = torch.from_numpy(secs).cuda(), torch.from_numpy(nanos).cuda()
        d_s, d_n = torch.empty_like(d_in_s), torch.empty_like(d_in_n)
        torch.cuda.synchronize()
        times = {leg: [] for leg, _ in LEGS}

        def run(mode, iters):
            ms = (ctypes.c_double * iters)()
            _lib.check(L.orcg_timestamp_tz_bench(ctx.handle, d_in_s.data_ptr(), d_in_n.data_ptr(), d_s.data_ptr(),
                                                 d_n.data_ptr(), n, w.handle, r.handle, mode, iters, ms),
                       ctx.last_error)
            return list(ms)

        for leg, mode in LEGS:
            run(mode, args.warmup)
        for _ in range(args.rounds):
            for leg, mode in LEGS:
                times[leg].extend(run(mode, args.iters))
        for leg, _ in LEGS:
            t = np.array(times[leg])
            med = float(np.median(t))
            lines.append({"input": name, "leg": leg, "n": n, "writer": args.writer, "reader": args.reader,
                          "median_us": round(med * 1e3, 2), "p10_us": round(float(np.percentile(t, 10)) * 1e3, 2),
                          "p90_us": round(float(np.percentile(t, 90)) * 1e3, 2), "launches": int(t.size),
                          "algorithmic_GBps": round(32.0 * n / (med * 1e-3) / 1e9, 1)})
        base = next(x for x in lines if x["input"] == name and x["leg"] == "plain")["median_us"]
        for x in lines:
            if x["input"] == name:
                x["vs_plain"] = round(x["median_us"] / base, 3)
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
