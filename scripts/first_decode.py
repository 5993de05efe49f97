#!/usr/bin/env python3
"""What a process pays before its first decoded value: the time from creating
its first context (which, under ORCG_WARMUP=1, the default, loads every kernel
file's code object with a no-op launch) to the end of its first decode, one
JSON line. One figure per process: run it several times, and with
ORCG_LIB=<another build> for an A/B.

    python scripts/first_decode.py [--variant V]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", type=int, default=0)
    args = ap.parse_args()
    import torch

    import orc_amd

    n, stride = 200_000, 10_000
    v = np.random.default_rng(0).integers(-(1 << 50), 1 << 50, size=n, dtype=np.int64)
    data, pos = orc_amd.encode_direct(v, True, aligned=False, rows_per_group=stride)
    d_src = torch.from_numpy(data).cuda()
    d_pos = torch.from_numpy(pos.view(np.int64)).cuda()
    out = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx = orc_amd.Context(0)
    t1 = time.perf_counter()
    ctx.set_rlev2_variant(args.variant)
    orc_amd.decode_positions_device(ctx, d_src, d_pos, stride, n, True, out)
    ctx.synchronize()
    t2 = time.perf_counter()
    assert np.array_equal(out.cpu().numpy(), v), "decode mismatch"
    print(json.dumps({"lib": os.environ.get("ORCG_LIB", "liborcgpu.so"), "warmup": os.environ.get("ORCG_WARMUP", "1"),
                      "variant": args.variant, "context_ms": round((t1 - t0) * 1e3, 2),
                      "first_decode_ms": round((t2 - t1) * 1e3, 2), "total_ms": round((t2 - t0) * 1e3, 2)}), flush=True)


if __name__ == "__main__":
    main()
