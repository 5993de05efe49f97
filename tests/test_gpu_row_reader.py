"""RowReader on the GPU decode, against the reference's own expected output.

Mirrors tools/test/TestMatch.cc:123-150 (Contents): createRowBatch(1024),
next(batch) until it returns false, getRowNumber() == rows read before the
batch, every row equal to examples/expected/<file>.jsn.gz (ColumnPrinter
output), getRowNumber() == rowCount at the end. Plus the batch contract at
other capacities (batches never exceed the capacity nor span a stripe:
RowReaderImpl::next, c++/src/Reader.cc:1392-1442), seekToRow at row-group
and stripe edges (:428-499), range(offset, length) stripe selection
(:337-345) and lazy dictionary decoding (nextEncoded, ColumnReader.cc:596-607).
Last, the rule that a row reader keeps every option of its creation, on a
Snappy file written at test time whose TIMESTAMP column has a writer zone
other than UTC.
"""
import os

import numpy as np
import pytest

import orc_amd
import snappy_model
import tz_model
from conftest import GOLDEN, load_golden
from file_parity import expected_json, first_difference, path, printer_equal, to_printer_form
from orc_craft import field_bytes, field_varint

pytestmark = pytest.mark.gpu

TESTMATCH = [d for d in load_golden("testmatch.json")
             if os.path.exists(path(d["file"])) and expected_json(d["file"].replace(
                 "demo-11-zlib", "demo-12-zlib")) is not None]


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def _decodable(reader, batch):
    """Top-level fields the GPU path decodes in this batch (TIMESTAMP columns
    of writers in a zone other than UTC and Hive 0.11 decimals are not)."""
    root = reader.types[0]
    if root.kind != 12:
        return None

    def ok(tid):
        return tid in batch.columns and all(ok(s) for s in reader.types[tid].subtypes)
    return [n for n, s in zip(root.field_names, root.subtypes) if ok(s)]


def _has_timestamp(reader, tid):
    t = reader.types[tid]
    return t.kind in (9, 18) or any(_has_timestamp(reader, s) for s in t.subtypes)


def _check_rows(reader, batch, want_rows, first, where):
    fields = _decodable(reader, batch)
    if fields is not None:
        # the only fields left out are those holding timestamps (of a writer
        # zone other than UTC: the GPU path decodes UTC writers only)
        root = reader.types[0]
        for n, s in zip(root.field_names, root.subtypes):
            assert n in fields or _has_timestamp(reader, s), "%s: field %s was not decoded" % (where, n)
    if fields is None and 0 not in batch.columns:
        return None  # a non-struct root the GPU path does not decode (a non-UTC timestamp)
    got = batch.to_pylist(fields)
    for i, g in enumerate(got):
        w = want_rows[first + i]
        if fields is not None:
            w = {k: w[k] for k in fields}
        assert printer_equal(w, to_printer_form(g)), "%s row %d: %r vs %r" % (where, first + i, w, g)
    return fields


@pytest.mark.parametrize("d", TESTMATCH, ids=lambda d: d["file"])
def test_contents_match_reference_expected_output(ctx, d):
    name = d["file"]
    want = expected_json(name.replace("demo-11-zlib", "demo-12-zlib"))
    r = orc_amd.Reader(path(name), ctx)
    rr = r.create_row_reader()
    assert rr.get_row_number() == (1 << 64) - 1 or d["rows"] == 0 or r.num_stripes == 0
    batch = rr.create_row_batch(1024)
    rows = 0
    decodable = None
    while rr.next(batch):
        assert rr.get_row_number() == rows
        assert 0 < batch.num_elements <= 1024
        decodable = _check_rows(r, batch, want, rows, name)
        rows += batch.num_elements
    assert rows == d["rows"] == len(want)
    assert rr.get_row_number() == d["rows"]
    if r.types[0].kind == 12 and d["rows"]:
        assert decodable, "%s: no decodable column" % name


@pytest.mark.parametrize("capacity", [1, 1000, 1024, 5000])
@pytest.mark.parametrize("name", ["TestOrcFile.testSeek.orc", "TestOrcFile.testMemoryManagementV11.orc",
                                  "nulls-at-end-snappy.orc"])
def test_batches_respect_capacity_and_stripes(ctx, name, capacity):
    r = orc_amd.Reader(path(name), ctx)
    want = expected_json(name)
    bounds = np.cumsum([0] + [r.stripe(s)["num_rows"] for s in range(r.num_stripes)])
    rr = r.create_row_reader()
    b = rr.create_row_batch(capacity)
    rows = 0
    # capacity 1 over a whole file is slow: check the first 3,000 rows there
    limit = 3000 if capacity == 1 else None
    while (limit is None or rows < limit) and rr.next(b):
        n = b.num_elements
        assert 0 < n <= capacity
        s = int(np.searchsorted(bounds, rows, side="right") - 1)
        assert rows + n <= bounds[s + 1], "batch spans a stripe"
        assert rr.get_row_number() == rows
        _check_rows(r, b, want, rows, name)
        rows += n
    if limit is None:
        assert rows == r.num_rows and not rr.next(b) and rr.get_row_number() == r.num_rows


def test_seek_to_row_at_row_group_and_stripe_edges(ctx):
    """TestOrcFile.testSeek.orc: 32,768 rows, 7 stripes, row index stride 1,000."""
    name = "TestOrcFile.testSeek.orc"
    r = orc_amd.Reader(path(name), ctx)
    want = expected_json(name)
    firsts = np.cumsum([0] + [r.stripe(s)["num_rows"] for s in range(r.num_stripes)])
    targets = [0, 1, 999, 1000, 1001, 4999, 5000, 12345, r.num_rows - 1]
    targets += [int(x) for x in firsts[1:-1]] + [int(x) - 1 for x in firsts[1:-1]]
    rr = r.create_row_reader()
    b = rr.create_row_batch(37)
    for t in targets + targets[::-1]:
        rr.seek_to_row(t)
        assert rr.get_row_number() == t
        assert rr.next(b)
        assert rr.get_row_number() == t
        s = int(np.searchsorted(firsts, t, side="right") - 1)
        assert b.num_elements == min(37, int(firsts[s + 1]) - t)
        _check_rows(r, b, want, t, "seek %d" % t)
    # past the end: no rows, row number = number of rows
    rr.seek_to_row(r.num_rows)
    assert not rr.next(b) and b.num_elements == 0
    assert rr.get_row_number() == r.num_rows


def test_range_selects_stripes_by_offset(ctx):
    """RowReaderOptions::range(offset, length): the stripes whose first byte
    lies in [offset, offset + length) (Reader.cc:337-345)."""
    name = "TestOrcFile.testSeek.orc"
    r = orc_amd.Reader(path(name), ctx)
    want = expected_json(name)
    st = [r.stripe(s) for s in range(r.num_stripes)]
    firsts = np.cumsum([0] + [x["num_rows"] for x in st])
    for lo, hi in [(0, 1), (2, 5), (6, 7), (1, 7)]:
        off = st[lo]["offset"]
        length = st[hi - 1]["offset"] - off + 1
        rr = r.create_row_reader(offset=off, length=length)
        b = rr.create_row_batch(4096)
        rows = int(firsts[lo])
        assert rr.get_row_number() == ((1 << 64) - 1 if lo == 0 else rows - 1)
        while rr.next(b):
            assert rr.get_row_number() == rows
            _check_rows(r, b, want, rows, "range %d-%d" % (lo, hi))
            rows += b.num_elements
        assert rows == firsts[hi]
        assert rr.get_row_number() == firsts[hi]
    # an empty range reads nothing
    rr = r.create_row_reader(offset=r.stripe(0)["offset"] + 1, length=1)
    assert not rr.next(rr.create_row_batch(10))


@pytest.mark.parametrize("name", ["demo-12-zlib.orc", "TestStringDictionary.testRowIndex.orc",
                                  "TestOrcFile.testSeek.orc"])
def test_lazy_dictionary_batches_match_eager(ctx, name):
    """setEnableLazyDecoding: dictionary columns arrive as index + dictionary
    (EncodedStringVectorBatch) and resolve to the same strings."""
    r1 = orc_amd.Reader(path(name), ctx)
    r2 = orc_amd.Reader(path(name), ctx)
    a = r1.create_row_reader()
    e = r2.create_row_reader(lazy_dictionary=True)
    ba, be = a.create_row_batch(5000), e.create_row_batch(5000)
    saw_encoded = False
    while a.next(ba):
        assert e.next(be) and be.num_elements == ba.num_elements
        for tid, c in be.columns.items():
            if c.index is not None and c.data is None:
                saw_encoded = True
        assert ba.to_pylist() == be.to_pylist()
    assert not e.next(be)
    # files with a dictionary-encoded string column hand out encoded batches
    r3 = orc_amd.Reader(path(name), ctx)
    b3 = r3.read_stripe(0)
    has_dict = any(r3.types[t].kind in (7, 16, 17) and c.encoding in (1, 3) for t, c in b3.columns.items())
    assert saw_encoded == has_dict


def test_column_selection_in_row_reader(ctx):
    r = orc_amd.Reader(path("TestOrcFile.test1.orc"), ctx)
    rr = r.create_row_reader(include=["string1", "map"])
    b = rr.create_row_batch(10)
    assert rr.next(b)
    ids = dict(zip(r.types[0].field_names, r.types[0].subtypes))
    assert ids["string1"] in b.columns and ids["map"] in b.columns and ids["int1"] not in b.columns
    assert [b.value(ids["string1"], i) for i in range(b.num_rows)] == ["hi", "bye"]


def _stripe_rows(r, want, s):
    first = sum(r.stripe(k)["num_rows"] for k in range(s))
    return want[first:first + r.stripe(s)["num_rows"]]


def test_abandoned_row_reader_then_reuse_context(ctx):
    """a row reader dropped right after next() has posted
    stripe 1 to its prefetch worker, then an immediate decode on the same
    context. The worker decodes on its own context, so the reader's decode
    must see neither its stream work nor its error record."""
    name = "TestOrcFile.testSeek.orc"  # 7 stripes
    want = expected_json(name)
    r = orc_amd.Reader(path(name), ctx)
    for k in range(4):
        rr = r.create_row_reader()
        b = rr.create_row_batch(1024)
        assert rr.next(b)  # stripe 0 is current, stripe 1 is posted
        rr.close()  # the worker is joined (it may still be decoding stripe 1)
        s = 1 + k % (r.num_stripes - 1)
        got = r.read_stripe(s).to_pylist()
        exp = _stripe_rows(r, want, s)
        assert len(got) == len(exp)
        for i, (g, w) in enumerate(zip(got, exp)):
            assert printer_equal(w, to_printer_form(g)), "stripe %d row %d" % (s, i)


def test_reader_reads_while_row_reader_prefetches(ctx):
    """stripe reads and copies on the reader (its own context and
    selection) while a row reader's worker is prefetching with a different
    selection; neither sees the other's options."""
    name = "TestOrcFile.testSeek.orc"
    want = expected_json(name)
    r = orc_amd.Reader(path(name), ctx)
    ids = dict(zip(r.types[0].field_names, r.types[0].subtypes))
    rr = r.create_row_reader(include=["int1", "string1"])
    b = rr.create_row_batch(1000)
    rows = 0
    s = 0
    while rr.next(b):
        # the worker may be decoding the next stripe right now (include subset)
        if rows % 5000 == 0:
            got = r.read_stripe(s % r.num_stripes).to_pylist()  # every column
            exp = _stripe_rows(r, want, s % r.num_stripes)
            assert len(got) == len(exp) and set(got[0]) == set(exp[0])
            assert all(printer_equal(w, to_printer_form(g)) for g, w in zip(got, exp))
            s += 1
        assert set(b.columns) >= {ids["int1"], ids["string1"]} and ids["boolean1"] not in b.columns
        for i in range(b.num_rows):
            w = want[rows + i]
            assert b.value(ids["int1"], i) == w["int1"]
        rows += b.num_elements
    assert rows == r.num_rows


def test_two_row_readers_on_one_reader(ctx):
    """Two row readers with different options on one reader, interleaved:
    their prefetch workers take turns on the reader's decode state."""
    name = "TestOrcFile.testSeek.orc"
    want = expected_json(name)
    r = orc_amd.Reader(path(name), ctx)
    ids = dict(zip(r.types[0].field_names, r.types[0].subtypes))
    a = r.create_row_reader(include=["int1"])
    c = r.create_row_reader(lazy_dictionary=True)
    ba, bc = a.create_row_batch(777), c.create_row_batch(1500)
    ra = rc = 0
    more_a = more_c = True
    while more_a or more_c:
        if more_a:
            more_a = a.next(ba)
            if more_a:
                assert ids["string1"] not in ba.columns
                for i in range(ba.num_rows):
                    assert ba.value(ids["int1"], i) == want[ra + i]["int1"]
                ra += ba.num_elements
        if more_c:
            more_c = c.next(bc)
            if more_c:
                _check_rows(r, bc, want, rc, "lazy row reader")
                rc += bc.num_elements
    assert ra == rc == r.num_rows


@pytest.mark.parametrize("name", ["TestOrcFile.testSeek.orc", "demo-12-zlib.orc",
                                  "TestStringDictionary.testRowIndex.orc"])
def test_row_indexed_file_under_every_variant(ctx, name):
    """ADVICE r02 / VERDICT r03 #4: a file whose streams are cut by the ROW_INDEX
    positions, read with every pinned RLEv2 instance (1 = the wave-walk
    decoder, which takes the row-index segment path without the multi-stream
    launch) against the reference's expected output."""
    want = expected_json(name) if expected_json(name) is not None else None
    r = orc_amd.Reader(path(name), ctx)
    assert r.row_index_stride > 0
    base = [r.read_stripe(s).to_pylist() for s in range(r.num_stripes)]
    if want is not None:
        flat = [x for st in base for x in st]
        assert all(printer_equal(w, to_printer_form(g)) for g, w in zip(flat, want))
    try:
        for v in sorted(set(orc_amd.rlev2_variants()) | {1}):
            ctx.set_rlev2_variant(v)
            for s in range(r.num_stripes):
                assert r.read_stripe(s).to_pylist() == base[s], "variant %d stripe %d" % (v, s)
    finally:
        ctx.set_rlev2_variant(0)


# ---- a row reader keeps every option of its creation ------------------------

TZ = os.path.join(GOLDEN, "tz")
WRITER_ZONE, OTHER_ZONE = "America/Los_Angeles", "Asia/Shanghai"
OPT_ROWS, OPT_STRIPE = 4000, 2000


def _fields(buf):
    """[(field, wire type, value)] of a message of varint and bytes fields."""
    out, p = [], 0

    def vint():
        nonlocal p
        v = sh = 0
        while True:
            b = buf[p]
            p += 1
            v |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                return v
    while p < len(buf):
        key = vint()
        assert key & 7 in (0, 2), "wire type %d" % (key & 7)
        if key & 7 == 0:
            out.append((key >> 3, 0, vint()))
        else:
            n = vint()
            out.append((key >> 3, 2, bytes(buf[p:p + n])))
            p += n
    return out


def _message(fields):
    return b"".join(field_varint(f, v) if w == 0 else field_bytes(f, v) for f, w, v in fields)


def _stored(body):
    """One stored ("original") compression chunk."""
    return (len(body) << 1 | 1).to_bytes(3, "little") + body


def with_writer_zone(data, zone):
    """The Snappy file `data` with every StripeFooter.writerTimezone replaced
    (pyarrow's writer knows GMT only): the stripe footers and the file footer
    are rewritten as stored chunks, the stripes' offsets and footer lengths,
    the content length and the PostScript's footer length follow."""
    def get(m, f):
        return [v for g, _, v in m if g == f]
    ps_len = data[-1]
    ps = _fields(data[-1 - ps_len:-1])
    foot_len, block, meta_len = get(ps, 1)[0], get(ps, 3)[0], (get(ps, 5) or [0])[0]
    foot_at = len(data) - 1 - ps_len - foot_len
    foot, err = snappy_model.decode_framed(data[foot_at:foot_at + foot_len], block)
    assert err is None
    foot = _fields(foot)
    body, src, stripes = bytearray(data[:3]), 3, []
    for s in get(foot, 3):
        s = _fields(s)
        off, ilen, dlen, flen = (get(s, f)[0] for f in (1, 2, 3, 4))
        assert off == src, "the stripes are contiguous"
        sf, err = snappy_model.decode_framed(data[off + ilen + dlen:off + ilen + dlen + flen], block)
        assert err is None
        sf = _stored(_message([(f, w, zone.encode() if f == 3 else v) for f, w, v in _fields(sf)]))
        stripes.append(_message([(f, w, {1: len(body), 4: len(sf)}.get(f, v)) for f, w, v in s]))
        body += data[off:off + ilen + dlen] + sf
        src = off + ilen + dlen + flen
    assert src == foot_at - meta_len
    body += data[src:foot_at]  # the metadata section
    it = iter(stripes)
    foot = _stored(_message([(f, w, len(body) - meta_len if f == 2 else next(it) if f == 3 else v)
                             for f, w, v in foot]))
    ps = _message([(f, w, len(foot) if f == 1 else v) for f, w, v in ps])
    return bytes(body) + foot + ps + bytes([len(ps)])


def _zone(name):
    with open(os.path.join(TZ, name), "rb") as f:
        return f.read()


def _open_with_zones(p, ctx):
    r = orc_amd.Reader(p, ctx)
    for name in (WRITER_ZONE, OTHER_ZONE, "GMT"):
        r.set_zone_rules(name, _zone(name))  # never the machine's tzdata
    return r


@pytest.fixture(scope="module")
def options_file(tmp_path_factory):
    """struct<id:bigint,s:string,ts:timestamp>, Snappy, two stripes of 2,000
    rows: ids that fit an int, 16 distinct strings (dictionary encoded), wall
    clocks across both 2023 US transitions written in America/Los_Angeles.
    Returns (path, rows as read in GMT, rows as read in Asia/Shanghai), the
    timestamps by tests/tz_model.py."""
    import pyarrow as pa
    import pyarrow.orc as po
    os.environ.setdefault("TZDIR", TZ)  # the ORC writer looks its zone (GMT) up
    rng = np.random.default_rng(5)
    ids = rng.integers(-(1 << 31), 1 << 31, OPT_ROWS, dtype=np.int64)
    words = ["word-%02d" % i for i in range(16)]
    strs = [words[int(k)] for k in rng.integers(0, 16, OPT_ROWS)]
    secs = np.concatenate([np.arange(e - 1000, e + 1000) for e in (1678586400, 1699146000)])
    nanos = rng.integers(0, 1_000_000_000, OPT_ROWS)
    t = pa.table({"id": pa.array(ids), "s": pa.array(strs),
                  "ts": pa.array(secs * 1_000_000_000 + nanos, pa.timestamp("ns"))})
    d = tmp_path_factory.mktemp("options")
    po.write_table(t, str(d / "gmt.orc"), compression="snappy", compression_block_size=65536, stripe_size=1,
                   batch_size=OPT_STRIPE, dictionary_key_size_threshold=0.5)
    p = str(d / "los_angeles.orc")
    with open(str(d / "gmt.orc"), "rb") as f:
        data = with_writer_zone(f.read(), WRITER_ZONE)
    with open(p, "wb") as f:
        f.write(data)
    # pyarrow reads the rewritten file; not its ts column, for which it would
    # look the writer zone up under whatever $TZDIR is by now
    f = po.ORCFile(p)
    assert [f.read_stripe(s, columns=["id"]).num_rows for s in range(f.nstripes)] == [OPT_STRIPE] * 2
    assert f.compression == "SNAPPY"
    assert f.read(columns=["id", "s"]).equals(t.select(["id", "s"]))
    # the stream values are the GMT writer's: read as the writer zone's, then in the reader zone
    la = tz_model.Zone(WRITER_ZONE, _zone(WRITER_ZONE))
    rows = {}
    for name in ("GMT", OTHER_ZONE):
        z = tz_model.Zone(name, _zone(name))
        ts = [tz_model.convert(la, z, int(v) - tz_model.ORC_EPOCH_UTC + la.epoch) for v in secs]
        rows[name] = [{"id": int(i), "s": w, "ts": np.datetime64(int(x) * 1_000_000_000 + int(n), "ns")}
                      for i, w, x, n in zip(ids, strs, ts, nanos)]
    return p, rows["GMT"], rows[OTHER_ZONE]


def _drain(rr, capacity=512):
    b = rr.create_row_batch(capacity)
    rows = []
    while rr.next(b):
        rows += b.to_pylist()
    return rows


def test_a_row_reader_keeps_every_option_of_its_creation(ctx, options_file):
    """Row reader A is created, then every option of the reader changes (the
    selection, lazy dictionaries, the reader zone, the read type with throwing
    overflow, device decompression), row reader B is created and the options
    are put back. A and B read interleaved, a batch each in turn, across a
    stripe edge and batch edges: A gives the reader's rows of before the
    change, B those of a reader that had B's options from the start, and the
    reader's own read afterwards equals its first. The Snappy chunks inflated
    on the device are exactly B's."""
    import test_gpu_snappy_files as snappy_files
    p, want_gmt, want_other = options_file
    with open(p, "rb") as f:
        b_chunks, b_bytes = snappy_files.expected_inflate(f.read())
    assert b_chunks > 0
    read_type = "struct<id:int,s:string,ts:timestamp>"
    r = _open_with_zones(p, ctx)
    first = r.read()
    assert first_difference(want_gmt, first) is None
    a = r.create_row_reader()
    r.select([1])
    r.set_lazy_dictionary(True)
    r.set_timezone(OTHER_ZONE)
    r.set_read_type(read_type, throw_on_overflow=True)
    r.set_device_decompression(True)
    assert r.last_device_inflate() == (0, 0)  # whatever A's worker has decoded by now
    b = r.create_row_reader()
    r.select(None)
    r.set_lazy_dictionary(False)
    r.set_timezone("GMT")
    r.set_read_type(None, throw_on_overflow=False)
    r.set_device_decompression(False)
    ba, bb = a.create_row_batch(512), b.create_row_batch(512)
    rows_a, rows_b = [], []
    more_a = more_b = True
    while more_a or more_b:
        if more_a:
            more_a = a.next(ba)
            if more_a:
                assert ba.types[1].kind == 4 and ba.columns[2].data is not None  # bigint, strings resolved
                rows_a += ba.to_pylist()
        if more_b:
            more_b = b.next(bb)
            if more_b:
                assert bb.types[1].kind == 3 and set(bb.columns) == {0, 1, 2, 3}  # int; its own selection
                rows_b += bb.to_pylist()
    # every stripe of both is decoded: the reader's counter holds B's chunks and none of A's
    assert r.last_device_inflate() == (b_chunks, b_bytes)
    assert first_difference(first, rows_a) is None
    assert first_difference(want_other, rows_b) is None
    once = _open_with_zones(p, ctx)
    once.set_timezone(OTHER_ZONE)
    once.set_read_type(read_type, throw_on_overflow=True)
    once.set_device_decompression(True)
    assert first_difference(_drain(once.create_row_reader()), rows_b) is None
    last = r.read()
    assert r.last_device_inflate() == (0, 0)
    assert first_difference(first, last) is None
