"""File-level GPU parity: every example file the reference's tests read
(tests/golden/files, copied from examples/) decoded end to end by the HIP
path — host tail parse + decompression, GPU RLEv1/RLEv2/byte/boolean RLE,
null scatter, dictionary gather, list/map offsets — and compared row by row
with pyarrow's ORC reader (the reference C++ library) and, where the
reference ships it, with its expected ColumnPrinter output."""
import decimal

import numpy as np
import pytest

import orc_amd
from file_parity import (CORRUPT_FILES, PARITY_FILES, expected_json, first_difference, path, printer_equal,
                         pyarrow_rows, supported_fields, to_printer_form)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def _read_all(ctx, name, fields=None):
    r = orc_amd.Reader(path(name), ctx)
    batches = [r.read_stripe(s) for s in range(r.num_stripes)]
    decoded = None
    for b in batches:
        decoded = set(b.columns) if decoded is None else decoded & set(b.columns)
    fields = supported_fields(r, decoded) if fields is None else fields
    rows = []
    for b in batches:
        rows.extend(b.to_pylist(fields))
    return r, fields, rows


@pytest.mark.parametrize("name", PARITY_FILES)
def test_file_matches_pyarrow(ctx, name):
    pytest.importorskip("pyarrow.orc")
    r, fields, got = _read_all(ctx, name)
    root = r.types[0]
    # every file with top-level fields must have decodable ones
    assert fields or root.kind != 12 or not root.subtypes, "%s: no decodable column" % name
    want = pyarrow_rows(name, fields)
    diff = first_difference(want, got)
    assert diff is None, "%s: %s" % (name, diff)


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("name", ["nulls-at-end-snappy.orc", "TestOrcFile.test1.orc", "orc_index_int_string.orc",
                                  "TestStringDictionary.testRowIndex.orc"])
def test_row_indexed_file_under_pinned_variant(name, variant):
    """Row-indexed files (row-group segment tables for their RLEv2 streams)
    under every variant the shipped library pins (orc_amd.rlev2_variants()),
    including the wave walk (1): the same rows as pyarrow (VERDICT r03 #4,
    ADVICE r02)."""
    pytest.importorskip("pyarrow.orc")
    assert variant in orc_amd.rlev2_variants()
    c = orc_amd.Context(0)
    c.set_rlev2_variant(variant)
    r, fields, got = _read_all(c, name)
    diff = first_difference(pyarrow_rows(name, fields), got)
    assert diff is None, "%s variant %d: %s" % (name, variant, diff)


@pytest.mark.parametrize("name", ["TestOrcFile.test1.orc", "nulls-at-end-snappy.orc", "orc_index_int_string.orc",
                                  "TestStringDictionary.testRowIndex.orc", "orc-file-11-format.orc"])
def test_file_matches_reference_expected_output(ctx, name):
    want = expected_json(name)
    r, fields, got = _read_all(ctx, name)
    assert len(got) == len(want)
    for i, (w, g) in enumerate(zip(want, got)):
        w = {k: w[k] for k in fields}
        assert printer_equal(w, to_printer_form(g)), "%s row %d: %r vs %r" % (name, i, w, g)


@pytest.mark.parametrize("name,messages", CORRUPT_FILES)
def test_corrupt_files_raise_reference_errors(ctx, name, messages):
    r = orc_amd.Reader(path(name), ctx)
    with pytest.raises(orc_amd.ParseError) as ei:
        for s in range(r.num_stripes):
            r.read_stripe(s)
    assert any(m in str(ei.value) for m in messages), str(ei.value)


def test_column_selection_reads_only_the_subtree(ctx):
    r = orc_amd.Reader(path("TestOrcFile.test1.orc"), ctx)
    ids = {n: s for n, s in zip(r.types[0].field_names, r.types[0].subtypes)}
    r.select([ids["string1"]])
    b = r.read_stripe(0)
    assert set(b.columns) == {0, ids["string1"]}
    assert [b.value(ids["string1"], i) for i in range(b.num_rows)] == ["hi", "bye"]
    r.select(None)
    b = r.read_stripe(0)
    assert ids["map"] in b.columns


def test_device_views_and_timings(ctx):
    r = orc_amd.Reader(path("demo-12-zlib.orc"), ctx)
    r.read_stripe_device(0)
    v = r.column_view(r.types[0].subtypes[0])
    assert v.decoded == 1 and v.num_elements == 1920800 and v.data
    t = r.last_timings()
    assert set(t) == {"host_parse_s", "host_decompress_s", "host_plan_s", "h2d_s", "device_decode_s"}


def test_reader_metrics(ctx):
    """ReaderMetrics (Reader.hh:59-76) through orcg_reader_get_metrics: one
    reader call per caller-facing call (RowReaderImpl::next's stopwatch,
    Reader.cc:1393), chunks inflated, RLE streams decoded, one I/O per stream
    read and its page-in time, no row-group counts without search arguments,
    no read-range cache; cumulative until reset."""
    r = orc_amd.Reader(path("demo-11-zlib.orc"), ctx)
    assert set(r.metrics().values()) == {0}
    r.read_stripes_device(0, 3)
    m = r.metrics()
    assert m["ReaderCall"] == 1 and m["ReaderInclusiveLatencyUs"] > 0
    assert m["DecompressionCall"] > 0 and m["DecompressionLatencyUs"] >= 0
    assert m["DecodingCall"] == 3 * 13  # demo-11: 13 RLEv1 streams per stripe
    assert m["IOCount"] == 3 * (13 + 4 + 1)  # its RLE streams, 4 dictionary blobs, the stripe footer
    assert m["SelectedRowGroupCount"] == 0 and m["EvaluatedRowGroupCount"] == 0
    assert m["ReadRangeCacheHits"] == 0 and m["ReadRangeCacheMisses"] == 0
    assert m["ReaderInclusiveLatencyUs"] >= m["DecodingLatencyUs"]
    r.read_stripe(3)
    m2 = r.metrics(reset=True)
    assert m2["ReaderCall"] == 2 and m2["DecodingCall"] == 4 * 13
    assert set(r.metrics().values()) == {0}
    # row reader: one call per next(); with event timing, device latencies of
    # both decoder kinds (a file with PRESENT streams for the byte decoder)
    r = orc_amd.Reader(path("nulls-at-end-snappy.orc"), ctx)
    r.set_metrics_timing(True)
    rr = r.create_row_reader()
    b = rr.create_row_batch(1000)
    calls = 0
    while rr.next(b):
        calls += 1
    calls += 1  # the last call returns no rows
    m = r.metrics()
    assert m["ReaderCall"] == calls
    assert m["ByteDecodingCall"] > 0 and m["ByteDecodingLatencyUs"] > 0
    assert m["DecodingCall"] > 0 and m["DecodingLatencyUs"] > 0
    assert m["IOCount"] > 0


def test_in_memory_source_matches_file(ctx):
    data = open(path("TestOrcFile.testSnappy.orc"), "rb").read()
    r1 = orc_amd.Reader(data, ctx)
    r2 = orc_amd.Reader(path("TestOrcFile.testSnappy.orc"), ctx)
    for s in range(r1.num_stripes):
        a = r1.read_stripe(s)
        b = r2.read_stripe(s)
        for tid in a.columns:
            ca, cb = a.columns[tid], b.columns[tid]
            if ca.data is not None:
                np.testing.assert_array_equal(ca.data, cb.data)


@pytest.mark.parametrize("name", ["demo-11-zlib.orc", "TestOrcFile.testWithoutIndex.orc", "nulls-at-end-snappy.orc"])
def test_pipelined_multi_stripe_read_matches_pyarrow(ctx, name):
    """read_stripes (host prepares stripe i+1 while the GPU decodes stripe i;
    every stripe stays resident) gives the same columns as pyarrow."""
    pa = pytest.importorskip("pyarrow.orc")
    r = orc_amd.Reader(path(name), ctx)
    r.read_stripes_device()
    f = pa.ORCFile(path(name))
    root = r.types[0]
    for fname, tid in zip(root.field_names, root.subtypes):
        if r.types[tid].kind not in (1, 2, 3, 4, 15):
            continue
        parts = []
        for k in range(r.num_stripes):
            v = r.stripe_column_view(k, tid)
            host = r._host(v.data, 8 * v.num_elements, np.int64)
            if v.has_nulls:
                nn = r._host(v.not_null, v.num_elements, np.uint8).astype(bool)
                host = np.where(nn, host, 0)
            parts.append(host)
        got = np.concatenate(parts)
        want = f.read(columns=[fname]).column(0).to_pylist()
        if r.types[tid].kind == 15:  # date -> days since the epoch
            want = [None if x is None else (x - __import__("datetime").date(1970, 1, 1)).days for x in want]
        want = np.array([0 if x is None else x for x in want], dtype=np.int64)
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", ["demo-11-zlib.orc", "nulls-at-end-snappy.orc"])
def test_concurrent_readers_on_stripe_ranges(ctx, name):
    """Four Readers, each with its own Context, read contiguous stripe ranges
    (RowReaderOptions::range, Reader.cc:337-345) from four threads at once
    (bench_file.py --readers): every resident batch equals the single
    reader's pipelined read of the same stripes."""
    import threading

    r = orc_amd.Reader(path(name), ctx)
    r.read_stripes_device()
    n = r.num_stripes
    bounds = np.linspace(0, n, 5).round().astype(int)
    parts = [(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
    readers = [orc_amd.Reader(path(name), orc_amd.Context(0)) for _ in parts]
    errs = []

    def one(rd, a, b):
        try:
            for _ in range(3):  # repeated scans: each one overlaps the others' launches
                rd.read_stripes_device(a, b - a)
        except Exception as e:
            errs.append(e)

    ts = [threading.Thread(target=one, args=(rd, a, b)) for rd, (a, b) in zip(readers, parts)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for rd, (a, b) in zip(readers, parts):
        for s in range(a, b):
            for t in r.types:
                v1, v0 = rd.stripe_column_view(s - a, t.id), r.stripe_column_view(s, t.id)
                assert v1.decoded == v0.decoded
                if not v0.decoded:
                    continue
                c1, c0 = vars(rd._column(v1, t)), vars(r._column(v0, t))
                for key in c0:
                    x, y = c1[key], c0[key]
                    if isinstance(y, np.ndarray) or isinstance(x, np.ndarray):
                        np.testing.assert_array_equal(x, y, err_msg="stripe %d column %d %s" % (s, t.id, key))
                    else:
                        assert x == y, (s, t.id, key)


@pytest.mark.parametrize("name", ["demo-12-zlib.orc", "TestOrcFile.test1.orc", "nulls-at-end-snappy.orc",
                                  "complextypes_iceberg.orc", "TestVectorOrcFile.testLz4.orc",
                                  "orc-file-11-format.orc", "decimal.orc"])
def test_row_index_segments_match_host_plans(ctx, name, monkeypatch):
    """Streams cut at row groups by the ROW_INDEX positions (no host header
    walk) decode exactly like the host-planned segmentation, and both equal
    pyarrow's ORC C++ reader (the reference) on every decodable field."""
    r = orc_amd.Reader(path(name), ctx)
    got = [r.read_stripe(s) for s in range(r.num_stripes)]
    stats = r.last_stream_stats()
    decoded = None
    for b in got:
        decoded = set(b.columns) if decoded is None else decoded & set(b.columns)
    fields = supported_fields(r, decoded)
    rows = [row for b in got for row in b.to_pylist(fields)]
    diff = first_difference(pyarrow_rows(name, fields), rows)
    assert diff is None, "%s: %s" % (name, diff)
    monkeypatch.setenv("ORCG_NO_ROW_INDEX", "1")
    r2 = orc_amd.Reader(path(name), ctx)
    want = [r2.read_stripe(s) for s in range(r2.num_stripes)]
    assert r2.last_stream_stats()["row_index"] == 0
    for a, b in zip(got, want):
        assert set(a.columns) == set(b.columns)
        for tid in a.columns:
            ca, cb = a.columns[tid], b.columns[tid]
            for f in ("not_null", "data", "length", "offsets", "secondary"):
                x, y = getattr(ca, f), getattr(cb, f)
                assert (x is None) == (y is None), (tid, f)
                if x is not None:
                    assert np.array_equal(x, y), (name, tid, f)
    if r.row_index_stride and r.num_rows:
        assert stats["row_index"] > 0, stats


def test_file_without_row_index_uses_host_plans(ctx):
    r = orc_amd.Reader(path("TestOrcFile.testWithoutIndex.orc"), ctx)
    r.read_stripe(0)
    st = r.last_stream_stats()
    assert st["row_index"] == 0 and st["host_plan"] > 0


def test_crafted_offsets_that_wrap_are_rejected(ctx):
    """Stripe offsets / lengths near 2^64 must fail the bounds checks instead
    of wrapping past them (the reference's InputStream reads are bounds
    checked; here every sum over file-supplied sizes is checked)."""
    from orc_craft import field_bytes, field_varint, orc_file, stripe_info, type_msg

    types = [type_msg(12, [1], ["x"]), type_msg(4)]
    # stripe footer at offset + index + data that wraps around 2^64
    wrap = orc_file(b"", [stripe_info((1 << 64) - 16, 8, 8, 4, 1)], types, 1)
    r = orc_amd.Reader(wrap, ctx)
    with pytest.raises(orc_amd.ParseError, match="Malformed StripeInformation at stripe index 0"):
        r.read_stripe(0)
    # a stream whose length wraps the running stream offset
    sfoot = (field_bytes(1, field_varint(1, 1) + field_varint(2, 1) + field_varint(3, (1 << 64) - 2)) +
             field_bytes(1, field_varint(1, 1) + field_varint(2, 1) + field_varint(3, 16)) +
             field_bytes(2, field_varint(1, 0)) + field_bytes(2, field_varint(1, 0)))
    body = bytes(8) + sfoot
    bad = orc_file(body, [stripe_info(3, 0, 8, len(sfoot), 1)], types, 1)
    r = orc_amd.Reader(bad, ctx)
    with pytest.raises(orc_amd.ParseError):
        r.read_stripe(0)


def _two_column_file(bad_index_row, bad_scale_row, n=1000):
    """struct<a:string (DICTIONARY_V2), b:decimal(10,2)>, one stripe, no row
    index: column a's DATA holds an out-of-range dictionary index at
    `bad_index_row`, column b's SECONDARY an out-of-range scale (30 for a
    column of scale 2) at `bad_scale_row` (None: no corruption)."""
    from orc_craft import field_bytes, field_varint, orc_file, stripe_info, type_msg, varint

    def rle2(vals, signed):
        v = np.asarray(vals, dtype=np.int64)
        lens = [min(512, v.size - i) for i in range(0, v.size, 512)]
        data, _ = orc_amd.encode_runs(v, signed, np.ones(len(lens), np.uint8), np.array(lens, np.uint32))
        return bytes(data)

    idx = np.zeros(n, np.int64)
    if bad_index_row is not None:
        idx[bad_index_row] = 7
    scales = np.full(n, 2, np.int64)
    if bad_scale_row is not None:
        scales[bad_scale_row] = 30
    a_data, a_len, a_dict = rle2(idx, False), rle2([3, 3, 3], False), b"xyzabcdef"
    b_data = b"".join(varint(2 * (i % 500)) for i in range(n))  # zigzag varints
    b_sec = rle2(scales, True)
    streams = [(1, 1, a_data), (2, 1, a_len), (3, 1, a_dict), (1, 2, b_data), (5, 2, b_sec)]
    body = b"".join(s[2] for s in streams)
    sfoot = b"".join(field_bytes(1, field_varint(1, k) + field_varint(2, c) + field_varint(3, len(b)))
                     for k, c, b in streams)
    sfoot += field_bytes(2, field_varint(1, 0))                            # root struct: DIRECT
    sfoot += field_bytes(2, field_varint(1, 3) + field_varint(2, 3))       # a: DICTIONARY_V2, 3 entries
    sfoot += field_bytes(2, field_varint(1, 2))                            # b: DIRECT_V2
    types = [type_msg(12, [1, 2], ["a", "b"]), type_msg(7), type_msg(14) + field_varint(5, 10) + field_varint(6, 2)]
    return orc_file(body + sfoot, [stripe_info(3, 0, len(body), len(sfoot), n)], types, n)


def test_first_error_in_column_order(ctx):
    """Two corrupt columns in one stripe: the error reported is the first
    column's (the reference decodes a batch column by column, StructColumnReader
    ::next), although the second column's bad value comes earlier in row
    order: every column has its own device error record (reader_stripes.cpp
    first_error). pyarrow's ORC C++ reader raises the same error on the
    same file."""
    ok = orc_amd.Reader(_two_column_file(None, None), ctx).read_stripe(0).to_pylist()
    assert len(ok) == 1000 and ok[0] == {"a": "xyz", "b": decimal.Decimal("0.00")}
    with pytest.raises(orc_amd.OrcError, match="Entry index out of range"):
        orc_amd.Reader(_two_column_file(900, None), ctx).read_stripe(0)
    with pytest.raises(orc_amd.OrcError, match="Decimal scale out of range"):
        orc_amd.Reader(_two_column_file(None, 10), ctx).read_stripe(0)
    with pytest.raises(orc_amd.OrcError, match="Entry index out of range"):
        orc_amd.Reader(_two_column_file(900, 10), ctx).read_stripe(0)
