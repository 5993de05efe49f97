"""Reader.set_device_decompression on Snappy files: a pyarrow-written file
(65,536-byte compression blocks, the smallest its ORC writer accepts: a block
must be a multiple of the writer's 64 KB memory block, so a 1,024-byte file
cannot be written; row_index_stride 1,000, three stripes and more, streams of
several chunks, direct and dictionary strings, binary, float, double,
decimal(30,5), a nullable struct of those and a list of strings) and the two
golden Snappy files (256 KB blocks) read with the
setting on equal the setting off and pyarrow, stripe by stripe, through
read_stripe, read_stripes_device, read_stripe_arrow and a row reader; the
counters say what was inflated where; corrupt chunks fail with the same status
and text on and off (the corruptions are chosen with tests/snappy_model.py)."""
import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import orc_amd
import snappy_model as M
from file_parity import first_difference, path

pytestmark = pytest.mark.gpu

ROWS = 9000
BLOCKS = [65536]
GOLDEN = ["TestOrcFile.testSnappy.orc", "nulls-at-end-snappy.orc"]


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def _table():
    rng = np.random.default_rng(11)
    words = ["w%03d" % i for i in range(40)]

    def sentence(i):  # unique (direct encoding) and compressible
        return " ".join(words[int(k)] for k in rng.integers(0, 40, 24)) + " #%d" % i

    direct = [sentence(i) for i in range(ROWS)]
    dic = [words[int(k)] for k in rng.integers(0, 40, ROWS)]
    binary = [bytes(rng.integers(0, 4, int(n), dtype=np.uint8)) for n in rng.integers(0, 30, ROWS)]
    f32 = (rng.integers(0, 50, ROWS) / 4).astype(np.float32)
    f64 = rng.integers(0, 1000, ROWS).astype(np.float64) * 0.125
    dec = [decimal.Decimal(int(v)).scaleb(-5) for v in rng.integers(-10 ** 15, 10 ** 15, ROWS)]
    noise = rng.integers(-(1 << 62), 1 << 62, ROWS, dtype=np.int64)  # incompressible: stored chunks
    struct = [None if i % 7 == 0 else {"s": direct[i][:9], "d": float(f64[i]), "b": binary[i], "m": dec[i]}
              for i in range(ROWS)]
    lists = [[dic[(i + k) % ROWS] + direct[i][:4] for k in range(i % 4)] for i in range(ROWS)]
    dec_t = pa.decimal128(30, 5)
    return pa.table({
        "noise": pa.array(noise),
        "direct": pa.array(direct), "dict": pa.array(dic), "bin": pa.array(binary, pa.binary()),
        "f": pa.array(f32), "d": pa.array(f64), "dec": pa.array(dec, dec_t),
        "st": pa.array(struct, pa.struct([("s", pa.string()), ("d", pa.float64()), ("b", pa.binary()),
                                          ("m", dec_t)])),
        "ls": pa.array(lists, pa.list_(pa.string())),
    })


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("snappy")
    t = _table()
    out = {}
    for block in BLOCKS:
        p = str(d / ("block%d.orc" % block))
        po.write_table(t, p, compression="snappy", compression_block_size=block, row_index_stride=1000,
                       stripe_size=128 << 10, dictionary_key_size_threshold=0.5)
        out[block] = p
    pz = str(d / "zlib.orc")
    po.write_table(t.slice(0, 2000), pz, compression="zlib", dictionary_key_size_threshold=0.5)
    out["zlib"] = pz
    return out


# ---- the file's layout, read with a small protobuf walk --------------------

def _pb(buf):
    p, n = 0, len(buf)
    while p < n:
        key, sh = 0, 0
        while True:
            b = buf[p]
            p += 1
            key |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        f, w = key >> 3, key & 7
        if w == 0:
            v, sh = 0, 0
            while True:
                b = buf[p]
                p += 1
                v |= (b & 0x7F) << sh
                sh += 7
                if not b & 0x80:
                    break
            yield f, v
        elif w == 2:
            ln, sh = 0, 0
            while True:
                b = buf[p]
                p += 1
                ln |= (b & 0x7F) << sh
                sh += 7
                if not b & 0x80:
                    break
            yield f, bytes(buf[p:p + ln])
            p += ln
        elif w == 1:
            p += 8
        elif w == 5:
            p += 4
        else:
            raise AssertionError("wire type %d" % w)


def _msg(buf):
    d = {}
    for f, v in _pb(buf):
        d.setdefault(f, []).append(v)
    return d


def layout(data):
    """(block size, [stripe: [(column, stream kind, file offset, length)]],
    type kinds, [stripe: column encodings]) of a Snappy ORC file."""
    ps_len = data[-1]
    ps = _msg(data[-1 - ps_len:-1])
    assert ps[2] == [2], "not a Snappy file"
    block = ps[3][0]
    foot_len = ps[1][0]
    foot, err = M.decode_framed(data[-1 - ps_len - foot_len:-1 - ps_len], block)
    assert err is None
    foot = _msg(foot)
    kinds = [_msg(t).get(1, [0])[0] for t in foot[4]]
    stripes, encodings = [], []
    for s in foot[3]:
        s = _msg(s)
        off, ilen, dlen, flen = s[1][0], s[2][0], s[3][0], s[4][0]
        sf, err = M.decode_framed(data[off + ilen + dlen:off + ilen + dlen + flen], block)
        assert err is None
        sf = _msg(sf)
        at, streams = off, []
        for st in sf[1]:
            st = _msg(st)
            kind, col, ln = st.get(1, [0])[0], st.get(2, [0])[0], st.get(3, [0])[0]
            streams.append((col, kind, at, ln))
            at += ln
        stripes.append(streams)
        encodings.append([_msg(e).get(1, [0])[0] for e in sf[2]])
    return block, stripes, kinds, encodings


def chunks_of(data, off, ln):
    """[(body offset, body length, stored)] of a stream."""
    out, p = [], off
    while p < off + ln:
        h = int.from_bytes(data[p:p + 3], "little")
        out.append((p + 3, h >> 1, bool(h & 1)))
        p += 3 + (h >> 1)
    assert p == off + ln
    return out


def device_streams(kinds, enc, streams):
    """The streams the host never walks: raw bytes and varints."""
    for col, kind, off, ln in streams:
        k = kinds[col]
        if kind == 3 or (kind == 1 and (k in (5, 6, 8, 14) or (k in (7, 16, 17) and enc[col] in (0, 2)))):
            yield col, kind, off, ln


def expected_inflate(data):
    block, stripes, kinds, encodings = layout(data)
    n = total = 0
    for streams, enc in zip(stripes, encodings):
        for col, kind, off, ln in device_streams(kinds, enc, streams):
            for boff, bln, stored in chunks_of(data, off, ln):
                n += 1
                total += bln if stored else M.preamble(data[boff:boff + bln])[0]
    return n, total


# ---- equality ----------------------------------------------------------------

def same_batch(got, want, what):
    assert got.schema.equals(want.schema, check_metadata=False), what
    got.validate(full=True)
    for name, g, w in zip(got.schema.names, got.columns, want.columns):
        assert g.equals(w), "%s column %s" % (what, name)


def raw_columns(r, s):
    """Every decoded buffer of resident stripe s, as bytes."""
    out = {}
    for t in r.read_types:
        v = r.stripe_column_view(s, t.id)
        if not v.decoded:
            continue
        n = v.num_elements
        out[t.id, "n"] = n
        if v.not_null:
            out[t.id, "nn"] = r._host(v.not_null, n, np.uint8).tobytes()
        if v.blob and v.blob_len:
            out[t.id, "blob"] = r._host(v.blob, v.blob_len, np.uint8).tobytes()
        if v.length:
            out[t.id, "length"] = r._host(v.length, 8 * n, np.uint8).tobytes()
    return out


def check_file(ctx, p, block=None):
    f = po.ORCFile(p)
    on, off = orc_amd.Reader(p, ctx), orc_amd.Reader(p, ctx)
    on.set_device_decompression(True)
    data = open(p, "rb").read()
    want_chunks, want_bytes = expected_inflate(data)
    assert want_chunks > 0
    if block is not None:
        assert on.num_stripes >= 3 and on.compression_block_size == block
    per_stripe = 0
    for s in range(on.num_stripes):
        want = f.read_stripe(s)
        rows = want.to_pylist()
        # read_stripe
        b_on, b_off = on.read_stripe(s), off.read_stripe(s)
        per_stripe += on.last_device_inflate()[0]
        assert off.last_device_inflate() == (0, 0)
        assert first_difference(rows, b_off.to_pylist()) is None, "stripe %d off" % s
        assert first_difference(rows, b_on.to_pylist()) is None, "stripe %d on" % s
        # read_stripe_arrow
        same_batch(off.read_stripe_arrow(s), want, "stripe %d off" % s)
        same_batch(on.read_stripe_arrow(s), want, "stripe %d on" % s)
    assert per_stripe == want_chunks
    # read_stripes_device: every stripe resident, the same buffers on and off
    on.read_stripes_device()
    assert on.last_device_inflate() == (want_chunks, want_bytes)
    off.read_stripes_device()
    assert off.last_device_inflate() == (0, 0)
    assert on.last_stream_stats()["stage_bytes"] < off.last_stream_stats()["stage_bytes"]
    for s in range(on.num_stripes):
        a, b = raw_columns(on, s), raw_columns(off, s)
        assert a.keys() == b.keys() and len(a) > 0
        for k in a:
            assert a[k] == b[k], "stripe %d column %s" % (s, k)
    # a row reader created after the setting takes it with it
    want_rows = f.read().to_pylist()
    for r in (on, off):
        rr = r.create_row_reader()
        batch = rr.create_row_batch(777)
        got = []
        while rr.next(batch):
            assert 0 < batch.num_elements <= 777
            got += batch.to_pylist()
        assert first_difference(want_rows, got) is None
    return on, off


@pytest.mark.parametrize("block", BLOCKS)
def test_written_files_equal_on_off_and_pyarrow(ctx, files, block):
    p = files[block]
    _, stripes, kinds, encodings = layout(open(p, "rb").read())
    # the file holds what the test is about: direct and dictionary strings
    assert encodings[0][2] in (0, 2) and encodings[0][3] in (1, 3), encodings[0]
    assert any(kind == 3 for _, kind, _, _ in stripes[0])
    check_file(ctx, p, block)


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_snappy_files_equal_on_and_off(ctx, name):
    p = path(name)
    f = po.ORCFile(p)
    on, off = orc_amd.Reader(p, ctx), orc_amd.Reader(p, ctx)
    on.set_device_decompression(True)
    want_chunks, want_bytes = expected_inflate(open(p, "rb").read())
    assert want_chunks > 0
    for s in range(on.num_stripes):
        a, b = on.read_stripe_arrow(s), off.read_stripe_arrow(s)
        assert a.equals(b)
        same_batch(a, f.read_stripe(s), "%s stripe %d" % (name, s))
        assert first_difference(off.read_stripe(s).to_pylist(), on.read_stripe(s).to_pylist()) is None
    on.read_stripes_device()
    off.read_stripes_device()
    assert on.last_device_inflate() == (want_chunks, want_bytes) and off.last_device_inflate() == (0, 0)
    for s in range(on.num_stripes):
        assert raw_columns(on, s) == raw_columns(off, s)
    rows = []
    for r in (on, off):
        rr = r.create_row_reader()
        batch = rr.create_row_batch(777)
        got = []
        while rr.next(batch):
            got += batch.to_pylist()
        rows.append(got)
    assert len(rows[0]) == f.nrows and first_difference(rows[1], rows[0]) is None


def test_other_codecs_ignore_the_setting(ctx, files):
    r = orc_amd.Reader(files["zlib"], ctx)
    r.set_device_decompression(True)
    f = po.ORCFile(files["zlib"])
    for s in range(r.num_stripes):
        same_batch(r.read_stripe_arrow(s), f.read_stripe(s), "zlib stripe %d" % s)
        assert r.last_device_inflate() == (0, 0)


# ---- corruption --------------------------------------------------------------

def _direct_data_chunk(data):
    """A compressed chunk of the first stripe's direct string DATA stream
    (column 2): (body offset, body, block size)."""
    block, stripes, kinds, encodings = layout(data)
    assert kinds[2] == 7 and encodings[0][2] in (0, 2)
    (off, ln), = [(o, n) for col, kind, o, n in stripes[0] if col == 2 and kind == 1]
    for boff, bln, stored in chunks_of(data, off, ln):
        if not stored and bln > 40:
            return boff, data[boff:boff + bln], block
    raise AssertionError("no compressed chunk in the string DATA stream")


def _corrupt_body(data):
    """One body byte changed so that the model fails: (file bytes, text)."""
    boff, body, block = _direct_data_chunk(data)
    _, p0 = M.preamble(body)
    for at in range(p0, len(body)):
        for v in (0xFF, 0x00, body[at] ^ 0x40):
            if v == body[at]:
                continue
            bad = body[:at] + bytes([v]) + body[at + 1:]
            r = M.decode(bad, block)
            if isinstance(r, str):
                return data[:boff + at] + bytes([v]) + data[boff + at + 1:], r
    raise AssertionError("no failing corruption found")


def _corrupt_preamble(data):
    boff, body, block = _direct_data_chunk(data)
    _, p0 = M.preamble(body)
    for at in range(p0):
        for v in range(256):
            bad = body[:at] + bytes([v]) + body[at + 1:]
            r = M.preamble(bad, block)
            if isinstance(r, str):
                return data[:boff + at] + bytes([v]) + data[boff + at + 1:], r
    raise AssertionError("no failing preamble found")


def _read_error(ctx, data, on):
    r = orc_amd.Reader(data, ctx)
    r.set_device_decompression(on)
    with pytest.raises(orc_amd.OrcError) as e:
        r.read_stripe(0)
    return type(e.value), str(e.value)


@pytest.mark.parametrize("which", ["body", "preamble"])
def test_corrupt_chunk_fails_alike_on_and_off(ctx, files, which):
    data = open(files[65536], "rb").read()
    bad, text = (_corrupt_body if which == "body" else _corrupt_preamble)(data)
    assert text in ((M.LITERAL_TRUNCATED, M.LITERAL_RANGE, M.COPY_TRUNCATED, M.COPY_RANGE, M.LENGTH_MISMATCH)
                    if which == "body" else (M.BAD_LENGTH, M.TOO_LARGE))
    assert _read_error(ctx, bad, False) == (orc_amd.ParseError, text)
    assert _read_error(ctx, bad, True) == (orc_amd.ParseError, text)
    # the other stripes still read
    r = orc_amd.Reader(bad, ctx)
    r.set_device_decompression(True)
    same_batch(r.read_stripe_arrow(1), po.ORCFile(files[65536]).read_stripe(1), "stripe 1")


def test_inflate_error_comes_ahead_of_an_earlier_columns_rle_error(ctx, files):
    data = open(files[65536], "rb").read()
    block, stripes, kinds, encodings = layout(data)
    # column 1 (int64 noise): its DATA stream's chunks are stored, so its RLE bytes can be rewritten in place
    (off, ln), = [(o, n) for col, kind, o, n in stripes[0] if col == 1 and kind == 1]
    boff, bln, stored = chunks_of(data, off, ln)[0]
    assert stored and bln > 8
    rle_bad = data[:boff] + bytes([0x8E, 0x09, 0x2B, 0x20]) + data[boff + 4:]  # PATCHED_BASE with pl == 0
    for on in (False, True):
        kind, text = _read_error(ctx, rle_bad, on)
        assert kind is orc_amd.ParseError and "PATCHED_BASE" in text, text
    both, text = _corrupt_body(rle_bad)
    assert _read_error(ctx, both, False) == (orc_amd.ParseError, text)
    assert _read_error(ctx, both, True) == (orc_amd.ParseError, text)
