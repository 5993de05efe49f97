"""GPU parity tests of the reader's RLEv1 paths over the crafted files of
tests/rlev1_files.py: the kMulti instances of rlev1_kernel at both chunk
widths over queue_stream's host-built V1SegDesc tables (the 1 KB host plans
of small streams in V; in W and R row-index positions that skip into runs and
literals, several row groups starting in one run), plan_rlev1_multi's two
launches, and RLEv1 under a PRESENT stream (R: with a row index, segments()
-> rg_segtab with the non-null prefix).

Expected values are the generated values: tests/test_rlev1_model_cpu.py proves
on the CPU that the oracle and pyarrow's ORC reader decode the same bytes to
them and that the positions skip as they mean to. Every comparison is exact.

Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import orc_amd
import rlev1_files as vf

pytestmark = pytest.mark.gpu

READ_ERROR = "bad read in readByte"
FILES = {"V": vf.file_v, "W": vf.file_w, "R": vf.file_r}
NON_NULL = {"V": 8, "W": 3, "R": 2}  # RLEv1 streams of columns without a PRESENT stream
# streams the row index cuts, at least: V's RLEv1 streams are small streams
# (1 KB host plans; its PRESENT stream keeps the index), W's and R's RLEv1
# streams are past 64 KB
ROW_INDEX = {"V": 1, "W": 3, "R": 3}


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def check_columns(f, r, columns, stripe, label):
    """A decoded stripe ({type id: ColumnBatch}) against the generated values:
    integer columns as arrays (under PRESENT: the mask, then the non-null
    rows), every column through to_pylist()."""
    n, cols = f.stripes[stripe]
    assert sorted(columns) == list(range(len(cols) + 1)), label
    for tid, c in enumerate(cols, start=1):
        got = columns[tid]
        assert got.num_elements == n, (label, c.name)
        if c.present is not None:
            np.testing.assert_array_equal(got.not_null, c.present, err_msg="%s column %s mask" % (label, c.name))
            np.testing.assert_array_equal(got.data[c.present.astype(bool)], c.rle[0].values,
                                          err_msg="%s column %s" % (label, c.name))
        else:
            assert got.not_null is None, (label, c.name)
            if not isinstance(c.values, list):
                np.testing.assert_array_equal(got.data, c.values.astype(got.data.dtype),
                                              err_msg="%s column %s" % (label, c.name))
    if n > 5000:  # (the arrays above are the whole of W and R)
        return
    rows, want = orc_amd.reader.Batch(r, columns).to_pylist(), f.rows(stripe)
    assert len(rows) == n
    for i, (g, w) in enumerate(zip(rows, want)):
        assert g == w, "%s row %d" % (label, i)


def read_and_check(f, ctx, label, batching=True, stripe=0):
    r = orc_amd.Reader(f.data, ctx)
    if not batching:
        r.set_stream_batching(False)
    b = r.read_stripe(stripe)
    stats = r.last_stream_stats()
    print(label, stats)
    check_columns(f, r, b.columns, stripe, label)
    return stats


@pytest.mark.parametrize("batching", [True, False], ids=["batched", "per-stream"])
@pytest.mark.parametrize("name", list(FILES))
def test_row_index_segments(ctx, name, batching):
    """The row index is the segment table. Batched, every RLEv1 stream of a
    column without PRESENT rides the multi-stream launches (the dictionary's
    3-value LENGTH with its host plan); the nullable column's DATA does not."""
    f = FILES[name]()
    stats = read_and_check(f, ctx, "%s batching=%s" % (name, batching), batching=batching)
    assert stats["row_index"] >= ROW_INDEX[name] > 0
    assert stats["batched"] == (NON_NULL[name] if batching else 0)
    assert len(f.rle_streams()) == NON_NULL[name] + (name != "W")


@pytest.mark.parametrize("batching", [True, False], ids=["batched", "per-stream"])
@pytest.mark.parametrize("name", list(FILES))
def test_host_planned_segment_tables(ctx, monkeypatch, name, batching):
    monkeypatch.setenv("ORCG_NO_ROW_INDEX", "1")
    f = FILES[name]()
    stats = read_and_check(f, ctx, "%s host plans batching=%s" % (name, batching), batching=batching)
    assert stats["row_index"] == 0 and stats["host_plan"] > 0
    assert stats["batched"] == (NON_NULL[name] if batching else 0)


def test_file_without_row_index(ctx):
    f = vf.file_v(stride=0)
    assert orc_amd.Reader(f.data).row_index_stride == 0
    stats = read_and_check(f, ctx, "V0")
    assert stats["row_index"] == 0 and stats["host_plan"] > 0 and stats["batched"] == NON_NULL["V"]


@pytest.mark.parametrize("capacity", [1024, 700])
def test_row_reader(ctx, capacity):
    f = vf.file_vs()
    r = orc_amd.Reader(f.data, ctx)
    want = [row for k in range(len(f.stripes)) for row in f.rows(k)]
    rr = r.create_row_reader()
    b = rr.create_row_batch(capacity)
    rows = 0
    while rr.next(b):
        assert rr.get_row_number() == rows and 0 < b.num_elements <= capacity
        got = b.to_pylist()
        assert got == want[rows:rows + b.num_elements], "rows from %d" % rows
        rows += b.num_elements
    assert rows == len(want) == r.num_rows


def test_pipelined_stripes(ctx):
    """read_stripes_device: every stripe stays resident and equals the
    generated values, also on a second read that reuses the slots."""
    f = vf.file_vs()
    r = orc_amd.Reader(f.data, ctx)
    assert r.num_stripes == 3
    for attempt in range(2):
        r.read_stripes_device()
        assert r.last_stream_stats()["batched"] == 3 * NON_NULL["V"]
        for k, (n, cols) in enumerate(f.stripes):
            columns = {}
            for tid in range(len(cols) + 1):
                v = r.stripe_column_view(k, tid)
                assert v.decoded and v.num_elements == n
                columns[tid] = r._column(v, r.types[tid])
            check_columns(f, r, columns, k, "VS stripe %d read %d" % (k, attempt))
    for k in range(3):
        read_and_check(f, ctx, "VS stripe %d alone" % k, stripe=k)


@pytest.mark.parametrize("batching", [True, False], ids=["batched", "per-stream"])
@pytest.mark.parametrize("cut", [(2,), (5,), (2, 5)], ids=["col2", "col5", "col2+col5"])
def test_cut_streams_raise_the_reference_error(ctx, cut, batching):
    """Column 2's (kCB = 4 segments) and / or column 5's (runs) stream cut
    inside its last group, stream lengths adjusted, positions unchanged: the
    read raises the reference's error (the oracle's and pyarrow's message on
    the same bytes; the lower column's first: both cuts give this message),
    and the same context reads V afterwards."""
    f = vf.file_v(cut=cut)
    r = orc_amd.Reader(f.data, ctx)
    if not batching:
        r.set_stream_batching(False)
    with pytest.raises(orc_amd.OrcError) as e:
        r.read_stripe(0)
    print(cut, batching, repr(e.value))
    assert READ_ERROR in str(e.value)
    read_and_check(vf.file_v(), ctx, "V after a failed read", batching=batching)
