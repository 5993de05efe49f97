"""GPU parity tests of the multi-stream RLEv2 launches: a stripe's
host-countable streams decoded by one launch per kernel instance over a job
table (reader_collect.cpp collect -> queue_stream, rlev2_tiled.cpp
plan_rlev2_multi -> run_multi; the kMulti instantiations of
rlev2_tiled_kernel and rlev2_expand_kernel). There is no entry point to these
instances but a file, so the streams of tests/multi_stream_files.py, built
run by run, are wrapped in hand-built ORC files with a row index.

Expected values are the generated values: tests/test_multi_stream_files.py
proves on the CPU that the oracle and pyarrow's ORC reader decode the same
bytes to them, and that the files hold the runs, positions, density classes
and segment lengths these tests aim at. Every comparison is exact.

Needs a real MI355X: run with `pytest -m gpu`.
"""
import numpy as np
import pytest

import multi_stream_files as msf
import orc_amd

pytestmark = pytest.mark.gpu

MULTI = (0, 2, 3, 4, 5, 6, 7, 8, 9)  # rlev2_multi_capable
READ_ERROR = "bad read in RleDecoderV2::readByte"
FILES = {"M": msf.file_m, "F": msf.file_f}


@pytest.fixture(scope="module")
def ctx():
    c = orc_amd.Context(0)
    yield c
    c.set_rlev2_variant(0)


@pytest.fixture
def pinned(ctx):
    """Pin a variant for one test; the default comes back afterwards."""
    yield ctx.set_rlev2_variant
    ctx.set_rlev2_variant(0)


def check_columns(f, r, columns, stripe, label):
    """Every column of a decoded stripe ({type id: ColumnBatch}) against the
    generated values: integers as arrays, strings through to_pylist()."""
    n, cols = f.stripes[stripe]
    assert sorted(columns) == list(range(len(cols) + 1)), label
    strings = []
    for tid, c in enumerate(cols, start=1):
        got = columns[tid]
        assert got.num_elements == n and got.not_null is None, (label, c.name)
        if isinstance(c.values, list):
            strings.append(c.name)
        else:
            np.testing.assert_array_equal(got.data, c.values.astype(got.data.dtype), err_msg="%s column %s" % (label, c.name))
    if strings:
        rows = orc_amd.reader.Batch(r, columns).to_pylist(strings)
        for name in strings:
            want = cols[f.names.index(name)].values
            assert [row[name] for row in rows] == want, "%s column %s" % (label, name)


def read_and_check(f, ctx, label, batching=True, stripe=0):
    r = orc_amd.Reader(f.data, ctx)
    if not batching:
        r.set_stream_batching(False)
    b = r.read_stripe(stripe)
    stats = r.last_stream_stats()
    print(label, stats)
    check_columns(f, r, b.columns, stripe, label)
    return stats


@pytest.mark.parametrize("variant", MULTI)
@pytest.mark.parametrize("name", list(FILES))
def test_every_instance_batched(ctx, pinned, name, variant):
    """Every multi-capable instance over the row-index job table: all of the
    file's RLEv2 streams ride multi-stream launches."""
    f = FILES[name]()
    pinned(variant)
    stats = read_and_check(f, ctx, "%s variant %d" % (name, variant))
    assert stats["batched"] == len(f.rle_streams()) == {"M": 11, "F": 3}[name]
    assert stats["row_index"] > 0


@pytest.mark.parametrize("name", list(FILES))
def test_wave_walk_is_not_batched(ctx, pinned, name):
    """Variant 1 (the wave walk) has no multi-stream instance: the streams the
    row index cuts are decoded one launch each, to the same values. (A stream
    without row-index positions, M's 3-value dictionary LENGTH, is still
    queued with its host plan and launched alone by plan_rlev2_multi, so it
    counts as batched: 1 for M, 0 for F.)"""
    f = FILES[name]()
    pinned(1)
    stats = read_and_check(f, ctx, "%s variant 1" % name)
    assert stats["batched"] == sum(1 for _, s in f.rle_streams() if not s.indexed) == {"M": 1, "F": 0}[name]
    assert stats["row_index"] > 0


@pytest.mark.parametrize("variant", (0, 6, 8, 9))
@pytest.mark.parametrize("name", list(FILES))
def test_control_one_launch_per_stream(ctx, pinned, name, variant):
    f = FILES[name]()
    pinned(variant)
    stats = read_and_check(f, ctx, "%s variant %d per stream" % (name, variant), batching=False)
    assert stats["batched"] == 0 and stats["row_index"] > 0


@pytest.mark.parametrize("batching", [True, False], ids=["batched", "per-stream"])
@pytest.mark.parametrize("variant", (0, 6, 8, 9))
@pytest.mark.parametrize("name", list(FILES))
def test_control_host_planned_segment_tables(ctx, pinned, monkeypatch, name, variant, batching):
    """ORCG_NO_ROW_INDEX=1: the same files through host-planned segment
    tables (RleJob::segtab)."""
    monkeypatch.setenv("ORCG_NO_ROW_INDEX", "1")
    f = FILES[name]()
    pinned(variant)
    stats = read_and_check(f, ctx, "%s variant %d host plans" % (name, variant), batching=batching)
    assert stats["row_index"] == 0 and stats["host_plan"] > 0
    assert stats["batched"] == (len(f.rle_streams()) if batching else 0)


@pytest.mark.parametrize("variant", (0, 6))
def test_control_file_without_row_index(ctx, pinned, variant):
    f = msf.file_m(stride=0)
    pinned(variant)
    assert orc_amd.Reader(f.data).row_index_stride == 0
    stats = read_and_check(f, ctx, "M without index, variant %d" % variant)
    assert stats["row_index"] == 0 and stats["host_plan"] > 0 and stats["batched"] == 11


@pytest.mark.parametrize("variant", (0, 6))
def test_pipelined_stripes(ctx, pinned, variant):
    """read_stripes_device: the job tables ride each stripe's arena; every
    stripe stays resident and equals the generated values, also on a second
    read that reuses the slots and the run table."""
    f = msf.file_s()
    pinned(variant)
    r = orc_amd.Reader(f.data, ctx)
    assert r.num_stripes == 3
    for attempt in range(2):
        r.read_stripes_device()
        assert r.last_stream_stats()["batched"] == sum(len(f.rle_streams(k)) for k in range(3)) == 33
        for k, (n, cols) in enumerate(f.stripes):
            label = "S stripe %d read %d variant %d" % (k, attempt, variant)
            columns = {}
            for tid in range(len(cols) + 1):
                v = r.stripe_column_view(k, tid)
                assert v.decoded and v.num_elements == n, label
                if tid and not isinstance(cols[tid - 1].values, list):
                    got = r._host(v.data, 8 * n, np.int64)
                    np.testing.assert_array_equal(got, cols[tid - 1].values, err_msg="%s column %d" % (label, tid))
                columns[tid] = r._column(v, r.types[tid])
            check_columns(f, r, columns, k, label)
    # the one-stripe reads of the same file
    for k in range(3):
        read_and_check(f, ctx, "S stripe %d alone" % k, stripe=k)


@pytest.mark.parametrize("batching", [True, False], ids=["batched", "per-stream"])
@pytest.mark.parametrize("variant", (6, 0))
@pytest.mark.parametrize("cut", [(2,), (6,), (2, 6)], ids=["col2", "col6", "col2+col6"])
def test_cut_streams_raise_the_reference_error(ctx, pinned, cut, variant, batching):
    """Column 2's and / or column 6's stream cut inside its last run (stream
    lengths adjusted, positions unchanged): the read raises the reference's
    error (the oracle's and pyarrow's message on the same bytes, the lower
    column's first: both cuts read past the end, so both give this message).
    Pinned to variant 6 both columns share one launch; by default column 2
    is in instance 2's and column 6 in the union instance's. The context
    decodes the whole file afterwards."""
    f = msf.file_m(cut=cut)
    pinned(variant)
    r = orc_amd.Reader(f.data, ctx)
    if not batching:
        r.set_stream_batching(False)
    with pytest.raises(orc_amd.OrcError) as e:
        r.read_stripe(0)
    print(cut, variant, batching, repr(e.value))
    assert READ_ERROR in str(e.value)
    read_and_check(msf.file_m(), ctx, "M after a failed read", batching=batching)
