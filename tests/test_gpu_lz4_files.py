"""Reader.set_device_decompression on LZ4 files: the pyarrow-written table of
tests/test_gpu_snappy_files.py (65,536-byte compression blocks, row_index_stride
1,000, three stripes and more, streams of several chunks, direct and
dictionary strings, binary, float, double, decimal(30,5), a nullable struct of
those and a list of strings) written with compression="lz4", read with the
setting on, equals the setting off and pyarrow, stripe by stripe, through
read_stripe, read_stripes_device, read_stripe_arrow and a row reader; the
counters say what was inflated where; the golden LZ4 file (int columns only)
has nothing eligible; a corrupt chunk fails with the same status and text on
and off (the corruption is chosen with tests/lz4_model.py). The protobuf walk,
the table and the comparisons are the Snappy file test's."""
import pyarrow.orc as po
import pytest

import orc_amd
import lz4_model as M
import test_gpu_snappy_files as S
from file_parity import first_difference, path

pytestmark = pytest.mark.gpu

BLOCK = 65536
GOLDEN = "TestVectorOrcFile.testLz4.orc"


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lz4")
    t = S._table()
    out = {}
    p = str(d / ("block%d.orc" % BLOCK))
    # (compression_strategy: under the default, "speed", this writer's LZ4 stores every chunk)
    po.write_table(t, p, compression="lz4", compression_block_size=BLOCK, row_index_stride=1000,
                   stripe_size=128 << 10, dictionary_key_size_threshold=0.5, compression_strategy="compression")
    out[BLOCK] = p
    pz = str(d / "zlib.orc")
    po.write_table(t.slice(0, 2000), pz, compression="zlib", dictionary_key_size_threshold=0.5)
    out["zlib"] = pz
    return out


def layout(data):
    """(block size, [stripe: [(column, stream kind, file offset, length)]],
    type kinds, [stripe: column encodings]) of an LZ4 ORC file; the footers are
    inflated with the model."""
    ps_len = data[-1]
    ps = S._msg(data[-1 - ps_len:-1])
    assert ps[2] == [4], "not an LZ4 file"
    block = ps[3][0]
    foot_len = ps[1][0]
    foot, err = M.decode_framed(data[-1 - ps_len - foot_len:-1 - ps_len], block)
    assert err is None
    foot = S._msg(foot)
    kinds = [S._msg(t).get(1, [0])[0] for t in foot[4]]
    stripes, encodings = [], []
    for s in foot[3]:
        s = S._msg(s)
        off, ilen, dlen, flen = s[1][0], s[2][0], s[3][0], s[4][0]
        sf, err = M.decode_framed(data[off + ilen + dlen:off + ilen + dlen + flen], block)
        assert err is None
        sf = S._msg(sf)
        at, streams = off, []
        for st in sf[1]:
            st = S._msg(st)
            kind, col, ln = st.get(1, [0])[0], st.get(2, [0])[0], st.get(3, [0])[0]
            streams.append((col, kind, at, ln))
            at += ln
        stripes.append(streams)
        encodings.append([S._msg(e).get(1, [0])[0] for e in sf[2]])
    return block, stripes, kinds, encodings


def expected_inflate(data):
    """(chunks, decompressed bytes) of the streams the host never walks."""
    block, stripes, kinds, encodings = layout(data)
    n = total = 0
    for streams, enc in zip(stripes, encodings):
        for col, kind, off, ln in S.device_streams(kinds, enc, streams):
            for boff, bln, stored in S.chunks_of(data, off, ln):
                n += 1
                total += bln if stored else M.size(data[boff:boff + bln], block)
    return n, total


def test_written_file_equals_on_off_and_pyarrow(ctx, files):
    p = files[BLOCK]
    f = po.ORCFile(p)
    data = open(p, "rb").read()
    _, stripes, kinds, encodings = layout(data)
    # the file holds what the test is about: direct and dictionary strings, compressed chunks
    assert encodings[0][2] in (0, 2) and encodings[0][3] in (1, 3), encodings[0]
    assert any(kind == 3 for _, kind, _, _ in stripes[0])
    assert any(not stored for col, kind, o, n in S.device_streams(kinds, encodings[0], stripes[0])
               for _, _, stored in S.chunks_of(data, o, n))
    want_chunks, want_bytes = expected_inflate(data)
    assert want_chunks > 0
    on, off = orc_amd.Reader(p, ctx), orc_amd.Reader(p, ctx)
    on.set_device_decompression(True)
    assert on.num_stripes >= 3 and on.compression_block_size == BLOCK
    per_stripe = 0
    for s in range(on.num_stripes):
        want = f.read_stripe(s)
        rows = want.to_pylist()
        b_on, b_off = on.read_stripe(s), off.read_stripe(s)
        per_stripe += on.last_device_inflate()[0]
        assert off.last_device_inflate() == (0, 0)
        assert first_difference(rows, b_off.to_pylist()) is None, "stripe %d off" % s
        assert first_difference(rows, b_on.to_pylist()) is None, "stripe %d on" % s
        S.same_batch(off.read_stripe_arrow(s), want, "stripe %d off" % s)
        S.same_batch(on.read_stripe_arrow(s), want, "stripe %d on" % s)
    assert per_stripe == want_chunks
    # read_stripes_device: every stripe resident, the same buffers on and off
    on.read_stripes_device()
    assert on.last_device_inflate() == (want_chunks, want_bytes)
    off.read_stripes_device()
    assert off.last_device_inflate() == (0, 0)
    assert on.last_stream_stats()["stage_bytes"] < off.last_stream_stats()["stage_bytes"]
    for s in range(on.num_stripes):
        a, b = S.raw_columns(on, s), S.raw_columns(off, s)
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


def test_golden_lz4_file_has_nothing_eligible(ctx):
    p = path(GOLDEN)
    f = po.ORCFile(p)
    assert expected_inflate(open(p, "rb").read()) == (0, 0)  # int columns only
    on, off = orc_amd.Reader(p, ctx), orc_amd.Reader(p, ctx)
    on.set_device_decompression(True)
    for s in range(on.num_stripes):
        a, b = on.read_stripe_arrow(s), off.read_stripe_arrow(s)
        assert a.equals(b)
        S.same_batch(a, f.read_stripe(s), "stripe %d" % s)
        assert on.last_device_inflate() == (0, 0) and off.last_device_inflate() == (0, 0)


def test_zlib_still_ignores_the_setting(ctx, files):
    r = orc_amd.Reader(files["zlib"], ctx)
    r.set_device_decompression(True)
    f = po.ORCFile(files["zlib"])
    for s in range(r.num_stripes):
        S.same_batch(r.read_stripe_arrow(s), f.read_stripe(s), "zlib stripe %d" % s)
        assert r.last_device_inflate() == (0, 0)


# ---- corruption --------------------------------------------------------------

def _corrupt_body(data):
    """One body byte of a compressed chunk of the first stripe's direct string
    DATA stream (column 2) changed so that the model fails."""
    block, stripes, kinds, encodings = layout(data)
    assert kinds[2] == 7 and encodings[0][2] in (0, 2)
    (off, ln), = [(o, n) for col, kind, o, n in stripes[0] if col == 2 and kind == 1]
    for boff, bln, stored in S.chunks_of(data, off, ln):
        if stored or bln <= 40:
            continue
        body = data[boff:boff + bln]
        for at in range(len(body)):
            for v in (0xFF, 0x00, body[at] ^ 0x40):
                if v == body[at]:
                    continue
                why = M.decode(body[:at] + bytes([v]) + body[at + 1:], block, why=True)
                # (a zero offset is the one failure liblz4, the host path, may not share)
                if isinstance(why, str) and why != M.ZERO_OFFSET:
                    return data[:boff + at] + bytes([v]) + data[boff + at + 1:]
    raise AssertionError("no failing corruption found")


def _read_error(ctx, data, on):
    r = orc_amd.Reader(data, ctx)
    r.set_device_decompression(on)
    with pytest.raises(orc_amd.OrcError) as e:
        r.read_stripe(0)
    return type(e.value), str(e.value)


def test_corrupt_chunk_fails_alike_on_and_off(ctx, files):
    data = open(files[BLOCK], "rb").read()
    bad = _corrupt_body(data)
    assert M.CORRUPT == "Corrupt lz4 compressed block"
    assert _read_error(ctx, bad, False) == (orc_amd.ParseError, M.CORRUPT)
    assert _read_error(ctx, bad, True) == (orc_amd.ParseError, M.CORRUPT)
    # the other stripes still read
    r = orc_amd.Reader(bad, ctx)
    r.set_device_decompression(True)
    S.same_batch(r.read_stripe_arrow(1), po.ORCFile(files[BLOCK]).read_stripe(1), "stripe 1")


def test_lz4_error_comes_ahead_of_an_earlier_columns_rle_error(ctx, files):
    data = open(files[BLOCK], "rb").read()
    block, stripes, kinds, encodings = layout(data)
    # column 1 (int64 noise): its DATA stream's chunks are stored, so its RLE bytes can be rewritten in place
    (off, ln), = [(o, n) for col, kind, o, n in stripes[0] if col == 1 and kind == 1]
    boff, bln, stored = S.chunks_of(data, off, ln)[0]
    assert stored and bln > 8
    rle_bad = data[:boff] + bytes([0x8E, 0x09, 0x2B, 0x20]) + data[boff + 4:]  # PATCHED_BASE with pl == 0
    for on in (False, True):
        kind, text = _read_error(ctx, rle_bad, on)
        assert kind is orc_amd.ParseError and "PATCHED_BASE" in text, text
    both = _corrupt_body(rle_bad)
    assert _read_error(ctx, both, False) == (orc_amd.ParseError, M.CORRUPT)
    assert _read_error(ctx, both, True) == (orc_amd.ParseError, M.CORRUPT)
