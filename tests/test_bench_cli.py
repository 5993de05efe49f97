"""bench.py's command line: a plain run carries the headline figure only,
`--full` adds the other legs, `--dump-outputs` writes the decoded column so
that two builds can be compared value for value."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

ROWS = 300_000  # 30 row groups, several workgroups; every leg stays under a few seconds


def run_bench(*extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--rows", str(ROWS)] + list(extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    return lines[0]


def load_dump(d, tag=""):
    parts = [np.load(os.path.join(d, tag + n + ".npy")) for n in ("rows", "values_hi32", "values_lo32")]
    assert all(p.dtype == np.float64 for p in parts)
    rows, hi, lo = (p.astype(np.int64) for p in parts)
    return rows, (hi << 32) | lo


def test_dump_outputs_is_exact_and_repeatable(tmp_path, monkeypatch):
    """dump_outputs on a column larger than the sample: the halves rebuild
    every sampled int64 exactly (full-range values, which a float64 alone
    would round), the sample holds both ends of the column, and a second
    dump picks the same rows."""
    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 20_000)
    n = 100_003
    v = np.random.default_rng(7).integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64, endpoint=True)
    v[:3] = [-(1 << 63), (1 << 63) - 1, -1]
    bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(v), 1, 0)
    bench.dump_outputs(str(tmp_path / "b"), torch.from_numpy(v), 1, 0)
    rows, got = load_dump(str(tmp_path / "a"))
    assert 4096 * 2 < rows.size <= 20_000 and np.all(np.diff(rows) > 0)
    assert rows[0] == 0 and rows[4095] == 4095 and rows[-1] == n - 1 and rows[-4096] == n - 4096
    np.testing.assert_array_equal(got, v[rows])
    rows_b, got_b = load_dump(str(tmp_path / "b"))
    np.testing.assert_array_equal(rows_b, rows)
    np.testing.assert_array_equal(got_b, got)
    # two ranks: each writes its own files, half the sample each
    bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(v), 2, 1)
    rows_r, got_r = load_dump(str(tmp_path / "a"), "rank1_")
    assert rows_r.size <= 10_000
    np.testing.assert_array_equal(got_r, v[rows_r])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_decoded_column(tmp_path):
    """A plain run: the result line has the headline fields and `--steps`
    timed steps, none of the `--full` legs; the dump is the column the timed
    path decoded, equal to the seeded values the stream was encoded from."""
    import bench

    d = run_bench("--dump-outputs", str(tmp_path / "out"))
    assert d["metric"] == bench.METRIC and d["unit"] == "GB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "int64" and d["steps"] == 3 and d["warmup"] == 1
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(ROWS * 8 / (d["ms_per_step"] * 1e-3) / 1e9, rel=2e-2)
    assert "cpu_baseline" not in d and "copy_inclusive" not in d and "concat" not in d
    assert "kernel_ms_timestamped" not in d["roofline"]
    rows, got = load_dump(str(tmp_path / "out"))
    np.testing.assert_array_equal(rows, np.arange(ROWS))
    np.testing.assert_array_equal(got, bench.make_stream(ROWS, 10_000)[0])


@pytest.mark.gpu
def test_full_run_keeps_every_leg():
    d = run_bench("--full", "--cpu-budget", "0.4")
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["one_core"]["value"] > 0
    assert d["copy_inclusive"]["ms"] > 0 and d["copy_inclusive"]["serial"]["ms"] > 0
    ts = d["roofline"]["kernel_ms_timestamped"]
    assert 0 < ts["min"] <= ts["mean"] <= ts["max"]
