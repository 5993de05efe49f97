"""GPU parity tests of the reader's byte / boolean RLE paths over the crafted
files of tests/byterle_files.py: BOOLEAN and TINYINT columns and a nullable
BIGINT whose PRESENT stream mixes runs and literals, with row-index positions
as the segment table (A; B: positions that carry bits and skip into runs,
several row groups starting in one group), 4 KB host plans (C's TINYINT; every
stream under ORCG_NO_ROW_INDEX and in a file without an index), the set-row
count that sizes the DATA decode, and a pyarrow-written nullable struct with
nullable children (the device-side row count; child positions counted in the
parent's non-null rows). A PRESENT stream cut inside its last literal reads
like the reference: all rows while their bytes are there, its error one byte
shorter.

Expected values are the generated values: tests/test_byterle_model_cpu.py
proves on the CPU that the oracle and pyarrow's ORC reader decode the same
bytes to them. Every comparison is exact.

Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import byterle_files as bf
import orc_amd

pytestmark = pytest.mark.gpu

READ_ERROR = "bad read in nextBuffer"
FILES = {"A": bf.file_a, "B": bf.file_b, "C": bf.file_c}


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def check_columns(f, r, columns, stripe, label):
    """A decoded stripe ({type id: ColumnBatch}) against the generated values:
    the columns as arrays (under PRESENT: the mask, then the non-null rows),
    then every row through to_pylist()."""
    n, cols = f.stripes[stripe]
    assert sorted(columns) == list(range(len(cols) + 1)), label
    for tid, c in enumerate(cols, start=1):
        got = columns[tid]
        assert got.num_elements == n, (label, c.name)
        if c.present is not None:
            np.testing.assert_array_equal(got.not_null, c.bits, err_msg="%s column %s mask" % (label, c.name))
            np.testing.assert_array_equal(got.data[c.bits.astype(bool)], c.data.values, err_msg="%s column %s" % (label, c.name))
        else:
            assert got.not_null is None, (label, c.name)
            np.testing.assert_array_equal(got.data, np.array(c.values, dtype=np.int64), err_msg="%s column %s" % (label, c.name))
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
    """The row index is the segment table of the byte-RLE streams that stay
    under 2 KB a row group (all three of A and B; C's TINYINT stream passes
    it and is cut by a host plan)."""
    stats = read_and_check(FILES[name](), ctx, "%s batching=%s" % (name, batching), batching=batching)
    assert stats["row_index"] >= (2 if name == "C" else 3)
    assert stats["host_plan"] >= (1 if name == "C" else 0)


@pytest.mark.parametrize("batching", [True, False], ids=["batched", "per-stream"])
@pytest.mark.parametrize("name", list(FILES))
def test_host_planned_segment_tables(ctx, monkeypatch, name, batching):
    monkeypatch.setenv("ORCG_NO_ROW_INDEX", "1")
    stats = read_and_check(FILES[name](), ctx, "%s host plans batching=%s" % (name, batching), batching=batching)
    assert stats["row_index"] == 0 and stats["host_plan"] > 0


def test_file_without_row_index(ctx):
    f = bf.file_a(stride=0)
    assert orc_amd.Reader(f.data).row_index_stride == 0
    stats = read_and_check(f, ctx, "A0")
    assert stats["row_index"] == 0 and stats["host_plan"] > 0


@pytest.mark.parametrize("capacity", [1024, 700])
def test_row_reader(ctx, capacity):
    f = bf.file_as()
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
    for k in range(len(f.stripes)):
        read_and_check(f, ctx, "AS stripe %d alone" % k, stripe=k)


# ---- the pyarrow-written nullable struct ------------------------------------------
@pytest.mark.parametrize("how", ["batched", "per-stream", "no row index"])
def test_nullable_struct_with_nullable_children(ctx, monkeypatch, how):
    """The children's PRESENT and DATA streams hold one entry per non-null
    parent row: their row counts are the parent's set-row count, read on the
    device."""
    if how == "no row index":
        monkeypatch.setenv("ORCG_NO_ROW_INDEX", "1")
    r = orc_amd.Reader(bf.file_p(), ctx)
    if how == "per-stream":
        r.set_stream_batching(False)
    assert r.num_rows == bf.P_ROWS and r.num_stripes == 1 and r.row_index_stride == bf.P_STRIDE
    b = r.read_stripe(0)
    print(how, r.last_stream_stats())
    want = bf.pyarrow_rows()
    got = b.to_pylist()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "row %d" % i
    s = np.array([w["s"] is not None for w in want], dtype=np.uint8)
    np.testing.assert_array_equal(b.columns[1].not_null, s)


@pytest.mark.parametrize("capacity", [1024, 700])
def test_nullable_struct_through_the_row_reader(ctx, capacity):
    r = orc_amd.Reader(bf.file_p(), ctx)
    want = bf.pyarrow_rows()
    rr = r.create_row_reader()
    b = rr.create_row_batch(capacity)
    rows = 0
    while rr.next(b):
        assert rr.get_row_number() == rows and 0 < b.num_elements <= capacity
        assert b.to_pylist() == want[rows:rows + b.num_elements], "rows from %d" % rows
        rows += b.num_elements
    assert rows == len(want)


# ---- a PRESENT stream cut inside its last literal ------------------------------------
@pytest.mark.parametrize("how", ["batched", "per-stream", "no row index"])
def test_present_cut_after_the_last_rows_byte_reads_like_the_whole_file(ctx, monkeypatch, how):
    """The reference reads a literal's bytes as it copies them: a literal
    whose missing bytes no row needs decodes every row."""
    if how == "no row index":
        monkeypatch.setenv("ORCG_NO_ROW_INDEX", "1")
    f = bf.file_a(cut="padding")
    assert f.rows() == bf.file_a().rows() and len(f.data) == len(bf.file_a().data) - bf.PAD
    read_and_check(f, ctx, "A without PRESENT's padding, " + how, batching=how != "per-stream")
    f0 = bf.file_a(stride=0, cut="padding")
    read_and_check(f0, ctx, "A0 without PRESENT's padding, " + how, batching=how != "per-stream")


@pytest.mark.parametrize("how", ["batched", "per-stream", "no row index"])
def test_present_cut_one_byte_shorter_raises_the_reference_error(ctx, monkeypatch, how):
    """The last row's byte is missing: the oracle's and pyarrow's "bad read in
    nextBuffer" on the same bytes; the same context reads A afterwards."""
    if how == "no row index":
        monkeypatch.setenv("ORCG_NO_ROW_INDEX", "1")
    r = orc_amd.Reader(bf.file_a(cut="short").data, ctx)
    if how == "per-stream":
        r.set_stream_batching(False)
    with pytest.raises(orc_amd.OrcError) as e:
        r.read_stripe(0)
    print(how, repr(e.value))
    assert READ_ERROR in str(e.value)
    read_and_check(bf.file_a(), ctx, "A after a failed read", batching=how != "per-stream")
