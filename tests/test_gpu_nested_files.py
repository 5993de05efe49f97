"""GPU parity tests of the reader over the crafted nested files of
tests/nested_files.py: LIST, MAP, UNION and nullable STRUCT columns with
PRESENT streams below the root, under a row index of many small row groups
(the look-back over row groups, the child row-group starts, the parent-mask ->
child-count chain), dictionaries on either side of the batched launch's 4,096
entries and of the one-workgroup scan's 65,536, and direct strings past the
one-workgroup scan, and (N9) a struct of seven fields forked over the side
lanes. Every column is compared array by array with
column_model.flatten()'s ground truth (null rows are unspecified: compared on
the rows that are not null); tests/test_column_model_cpu.py proves on the CPU
that pyarrow and the oracle read the same bytes to the same values. The bad
files raise the reference's errors. Every comparison is exact.

Needs a real MI355X: run with `pytest -m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nested_files as nf
import orc_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def check_columns(f, batch, label, lazy=False):
    """A decoded stripe against flatten()'s columns."""
    assert sorted(batch.columns) == [c.id for c in f.cols], label
    for c in f.cols:
        got, kind, msg = batch.columns[c.id], c.node.kind, "%s column %d (%s)" % (label, c.id, c.node.kind)
        assert got.num_elements == c.n, msg
        if got.not_null is None:
            assert c.not_null.all(), msg
        else:
            np.testing.assert_array_equal(got.not_null != 0, c.not_null != 0, err_msg=msg + " mask")
        m = c.not_null != 0
        if kind in ("long", "byte", "boolean"):
            np.testing.assert_array_equal(got.data[m], c.dense, err_msg=msg)
        elif kind in ("list", "map"):
            np.testing.assert_array_equal(got.offsets, c.offsets, err_msg=msg)
        elif kind == "union":
            np.testing.assert_array_equal(got.tags[m], c.tags, err_msg=msg + " tags")
            np.testing.assert_array_equal(got.offsets[m], c.offsets, err_msg=msg + " offsets")
        elif kind == "string" and c.node.dictionary:
            lens = np.array([len(e) for e in c.entries], dtype=np.int64)
            starts = np.concatenate([[0], np.cumsum(lens)])
            np.testing.assert_array_equal(got.index[m], c.dense, err_msg=msg + " index")
            np.testing.assert_array_equal(got.dict_offsets, starts, err_msg=msg + " dictionary offsets")
            assert got.blob == b"".join(c.entries), msg
            if lazy:
                assert got.data is None and got.length is None, msg
            else:
                np.testing.assert_array_equal(got.data[m], starts[c.dense], err_msg=msg + " starts")
                np.testing.assert_array_equal(got.length[m], lens[c.dense], err_msg=msg + " lengths")
        elif kind == "string":
            lens = np.array([len(b) for b in c.dense], dtype=np.int64)
            np.testing.assert_array_equal(got.length[m], lens, err_msg=msg + " lengths")
            starts = got.data[m]
            live = lens > 0  # (the host copy rebases the starts of the rows that hold bytes)
            np.testing.assert_array_equal(starts[live] - starts[live][:1], np.cumsum(lens)[live] - lens[live] -
                                          (np.cumsum(lens)[live] - lens[live])[:1], err_msg=msg + " starts")
            for s, ln, b in zip(starts[live][:200].tolist(), lens[live][:200].tolist(),
                                [x for x in c.dense if x][:200]):
                assert got.blob[s:s + ln] == b, msg
    want = f.pylist()
    rows = list(range(min(50, len(want)))) + list(range(max(len(want) - 50, 0), len(want)))
    for i in rows:
        got_row = {n: batch.value(t, i) for n, t in zip(batch.types[0].field_names, batch.types[0].subtypes)}
        assert got_row == want[i], "%s row %d" % (label, i)


def read(f, ctx, batching=True, lazy=False):
    r = orc_amd.Reader(f.data, ctx)
    if not batching:
        r.set_stream_batching(False)
    if lazy:
        r.set_lazy_dictionary(True)
    return r, r.read_stripe(0)


@pytest.mark.parametrize("name", list(nf.GOOD))
def test_stripe_columns_equal_the_ground_truth(ctx, name):
    """The default read; its stream statistics say which path it took: the
    row index for every file that has one, the batched dictionary launch for
    dictionaries of up to 4,096 entries without nulls."""
    f = nf.GOOD[name]()
    r, b = read(f, ctx)
    stats = r.last_stream_stats()
    print(name, stats)
    assert r.num_rows == len(f.rows) and r.num_stripes == 1 and r.row_index_stride == f.stride
    check_columns(f, b, name)
    if name == "N6":
        assert stats["row_index"] == 0 and stats["host_plan"] > 0
    elif name[:2] in ("N1", "N2", "N3", "N4", "N5", "N9"):
        assert stats["row_index"] > 0, stats
    if name in ("N5", "N2-16", "N2-4096", "N9"):
        assert stats["batched"] > 0, stats


@pytest.mark.parametrize("name", list(nf.GOOD))
def test_host_planned_and_per_stream_reads(ctx, monkeypatch, name):
    f = nf.GOOD[name]()
    r, b = read(f, ctx, batching=False)
    check_columns(f, b, name + " per stream")
    monkeypatch.setenv("ORCG_NO_ROW_INDEX", "1")
    r, b = read(f, ctx)
    assert r.last_stream_stats()["row_index"] == 0
    check_columns(f, b, name + " without the row index")


@pytest.mark.parametrize("D", [16, 4096, 4097])
def test_lazy_dictionary_map_keys(ctx, D):
    f = nf.n2(D)
    r, b = read(f, ctx, lazy=True)
    check_columns(f, b, "N2-%d lazy" % D, lazy=True)


@pytest.mark.parametrize("capacity", [1000, 1024])
@pytest.mark.parametrize("name", list(nf.GOOD))
def test_row_reader_batches(ctx, name, capacity):
    f = nf.GOOD[name]()
    want = f.pylist()
    r = orc_amd.Reader(f.data, ctx)
    rr = r.create_row_reader()
    b = rr.create_row_batch(capacity)
    rows = 0
    while rr.next(b):
        assert rr.get_row_number() == rows and 0 < b.num_elements <= capacity
        # the long flat files: the batch's ends; the nested ones: every row
        pick = range(b.num_elements) if len(want) < 10_000 else \
            sorted(set(range(min(20, b.num_elements))) | set(range(max(b.num_elements - 20, 0), b.num_elements)))
        ids = dict(zip(b.types[0].field_names, b.types[0].subtypes))
        for i in pick:
            assert {n: b.value(t, i) for n, t in ids.items()} == want[rows + i], "%s row %d" % (name, rows + i)
        rows += b.num_elements
    assert rows == len(want)


def _mid_run_group(f):
    """A row group at whose first row a child column's stream stands inside a
    run (values to skip > 0)."""
    for c in f.cols[2:]:
        for s, at in c.seeks:
            for g, v in enumerate(at):
                if g > 2 and s.at(v)[1] > 0:
                    return g
    raise AssertionError("no row group starts inside a child's run")


@pytest.mark.parametrize("capacity", [1000, 1024])
@pytest.mark.parametrize("name", ["N1", "N3"])
def test_row_reader_seeks_to_row_group_edges(ctx, name, capacity):
    f = nf.GOOD[name]()
    want = f.pylist()
    groups = (len(want) + f.stride - 1) // f.stride
    r = orc_amd.Reader(f.data, ctx)
    rr = r.create_row_reader()
    b = rr.create_row_batch(capacity)
    for g in (_mid_run_group(f), 1, groups - 1):
        for row in (g * f.stride, min((g + 1) * f.stride, len(want)) - 1):
            rr.seek_to_row(row)
            assert rr.next(b) and rr.get_row_number() == row
            assert b.num_elements == min(capacity, len(want) - row)
            assert b.to_pylist() == want[row:row + b.num_elements], "%s from row %d" % (name, row)


@pytest.mark.parametrize("name", list(nf.BAD))
def test_bad_files_raise_the_reference_errors(ctx, name):
    """read_stripe and the row reader's next both raise the reference's
    ParseError; of bad N3's tags 3 (two rows) and 255 (the last row) the
    lowest row's is named. The context reads a good file afterwards."""
    make, text = nf.BAD[name]
    f = make()
    for batching in (True, False):
        r = orc_amd.Reader(f.data, ctx)
        r.set_stream_batching(batching)
        with pytest.raises(orc_amd.ParseError) as e:
            r.read_stripe(0)
        assert text in str(e.value), (name, batching)
    with pytest.raises(orc_amd.ParseError) as e:
        rr = orc_amd.Reader(f.data, ctx).create_row_reader()
        rr.next(rr.create_row_batch(1000))
    assert text in str(e.value), name
    good = nf.n8()
    check_columns(good, read(good, ctx)[1], "N8 after " + name)


N9_BAD = ["N9-index", "N9-tag", "N9-tag-short"]


def lanes_child():
    """What a child process of the test below runs: N9 and its three bad
    files through the checks of the tests above, on a context of its own."""
    ctx = orc_amd.Context(0)
    good = nf.GOOD["N9"]()
    for batching in (True, False):
        check_columns(good, read(good, ctx, batching=batching)[1], "N9 batching %s" % batching)
    for name in N9_BAD:
        make, text = nf.BAD[name]
        f = make()
        for batching in (True, False):
            r = orc_amd.Reader(f.data, ctx)
            r.set_stream_batching(batching)
            with pytest.raises(orc_amd.ParseError) as e:
                r.read_stripe(0)
            assert text in str(e.value), (name, batching, str(e.value))
    check_columns(good, read(good, ctx)[1], "N9 after the bad files")


def test_one_and_two_side_lanes_read_n9_alike():
    """ORCG_LANES is read once per process: a fresh child python with one
    lane (no fork at all), then one with two (seven subtrees on two lanes, a
    map's values on the other lane of its keys), one after the other; each
    reads N9 and raises the bad files' errors as the default four lanes do.
    A first child that does not end by itself (a signal, the time limit)
    keeps the second from starting."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_nested_files as t; t.lanes_child()" % (
        here, os.path.dirname(here))
    for lanes in ("1", "2"):
        env = dict(os.environ, ORCG_LANES=lanes)
        out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], capture_output=True, text=True,
                             env=env)
        assert out.returncode in (0, 1), "ORCG_LANES=%s: exit status %d\n%s" % (lanes, out.returncode, out.stderr[-3000:])
        if lanes == "1":
            first = out
    for lanes, out in (("1", first), ("2", out)):
        assert out.returncode == 0, "ORCG_LANES=%s\n%s" % (lanes, out.stderr[-3000:])
