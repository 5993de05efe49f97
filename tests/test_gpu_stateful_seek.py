"""The stateful host decoders (RleDecoderV2, ByteRleDecoder) and the one-shot
host decodes against the CPU oracle driven through the same calls: seeks that
reuse the current decoding (a group start found from a segment cut of its
plan) and seeks that decode again, reads and skips at the stream's end, and
not-null masks that ask for exactly the values left and for one more.

The decoders plan with 16 KB / 8192-value segments (16384 for byte RLE): the
streams hold about 20,000 values (40,000 decoded bytes), the smallest that
give the lookup three segments to choose from.

Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import byterle_model as bm
from oracle import oracle
from rlev1_writer import encode as v1_encode, random_groups

pytestmark = pytest.mark.gpu

V2_EOF = "bad read in RleDecoderV2::readByte"
PAST_END = "Seek past end of stream"


@pytest.fixture(scope="module", params=[0, 1], ids=["tiled", "wavewalk"])
def orc(request):
    import orc_amd

    ctx = orc_amd.default_context(0)
    ctx.set_rlev2_variant(request.param)
    yield orc_amd
    ctx.set_rlev2_variant(0)


class Pair:
    """A decoder and the oracle's, driven through the same calls: what a call
    returns, or the text of the error it raises, must be the same."""

    def __init__(self, orc, ours, ref, dtype):
        self.orc, self.ours, self.ref, self.dtype = orc, ours, ref, dtype

    def _call(self, d, op, args):
        try:
            getattr(d, op)(*args)
            return None
        except (self.orc.OrcError, oracle.OracleError) as e:
            return str(e)

    def seek(self, *pos, error=None):
        got, want = self._call(self.ours, "seek", pos), self._call(self.ref, "seek", pos)
        assert got == want == error, (pos, got, want)

    def skip(self, n, error=None):
        got, want = self._call(self.ours, "skip", (n,)), self._call(self.ref, "skip", (n,))
        assert got == want == error, (n, got, want)

    def next(self, n, nn=None, error=None, delivered=None, text=True):
        """delivered: with an error, the values both hand out before it.
        text=False: only that both fail (Java's texts differ from the oracle's)."""
        a, b = np.zeros(n, dtype=self.dtype), np.zeros(n, dtype=self.dtype)
        got = self._call(self.ours, "next", (n, nn, a) if self.dtype == np.uint8 else (n, nn, self.dtype, a))
        want = self._call(self.ref, "next", (n, nn, b) if self.dtype == np.uint8 else (n, nn, self.dtype, b))
        if text:
            assert got == want == error, (n, got, want)
        else:
            assert got is not None and want is not None
        if error is None:
            np.testing.assert_array_equal(a, b)
        else:
            rows = np.arange(n) if nn is None else np.flatnonzero(nn)
            np.testing.assert_array_equal(a[rows[:delivered]], b[rows[:delivered]])
            if nn is not None:
                assert not a[np.asarray(nn) == 0].any()  # null slots untouched (or 0)
        return a


def half_mask(count):
    """2 * count rows of which `count` are set, at random."""
    nn = np.zeros(2 * count, dtype=np.uint8)
    nn[np.random.default_rng(count).choice(2 * count, size=count, replace=False)] = 1
    return nn


# ---- RLEv2 ------------------------------------------------------------------
# a PATCHED_BASE run whose patch entries would be 64 + 1 bits wide: corrupt by
# the C++ and by Java's rules (without skipCorrupt)
BAD_RUN = bytes([0x80, 0x00, 0x1F, 0x01, 0x00, 0x00])
BAD_TEXT = "Corrupt PATCHED_BASE encoded data (patchBitSize + pgw > 64)!"


def v2_part(orc, seed, nruns, signed):
    rng = np.random.default_rng(seed)
    kinds = [int(k) for k in rng.integers(0, 4, size=nruns)]
    lens = [int(rng.integers(3, 11)) if k == 0 else int(rng.integers(60, 140)) for k in kinds]
    vals = []
    for k, n in zip(kinds, lens):
        lo = -(1 << 29) if signed else 0
        if k == 0:
            vals.append(np.full(n, int(rng.integers(0, 1000)), dtype=np.int64))
        elif k == 1:
            vals.append(rng.integers(lo, 1 << 30, size=n).astype(np.int64))
        elif k == 2:
            x = 1000 + rng.integers(0, 200, size=n).astype(np.int64)
            x[int(rng.integers(0, n))] += 1 << 25
            vals.append(x)
        else:
            vals.append((int(rng.integers(0, 10 ** 6)) + 37 * np.arange(n)).astype(np.int64))
    data, offs = orc.encode_runs(np.concatenate(vals), signed, kinds, lens)
    return data.tobytes(), [int(o) for o in offs], lens


@pytest.mark.parametrize("mode", ["signed", "unsigned", "java"])
def test_rlev2_seek_sequence(orc, mode):
    signed = mode != "unsigned"
    a, offs_a, lens_a = v2_part(orc, 1, 260, signed)
    b, offs_b, lens_b = v2_part(orc, 2, 30, signed)
    data = a + BAD_RUN + b
    offs_b = [o + len(a) + len(BAD_RUN) for o in offs_b]
    cuts = [int(s[0]) for s in orc.Plan(a).segments()]
    assert len(cuts) >= 3 and 15_000 < sum(lens_a) < 25_000
    ours = (orc.create_java_rle_decoder(data, signed, skip_corrupt=False) if mode == "java"
            else orc.create_rle_decoder(data, signed))
    p = Pair(orc, ours, oracle.RleDecoderV2(data, signed), np.int64)

    # 1. a run start inside the third segment (found by the walk from its cut)
    k = next(i for i, o in enumerate(offs_a) if o > cuts[2] and lens_a[i] > 10)
    assert offs_a[k] not in cuts and (len(cuts) == 3 or offs_a[k] < cuts[3])
    for skip in (0, lens_a[k] - 1, lens_a[k]):
        p.seek(offs_a[k], skip)
        p.next(5)
    # 2. back to a run start in the first segment
    assert 0 < offs_a[3] < cuts[1]
    p.seek(offs_a[3], 0)
    first = p.next(50)
    # 3. a run past the corrupt one is no run of the current decoding: decoded
    # again from there; then a run start before that origin
    p.seek(offs_b[5], 2)
    p.next(20)
    p.seek(offs_a[3], 0)
    np.testing.assert_array_equal(p.next(50), first)
    # reading into the corrupt run: the values before it, then its error
    p.seek(offs_a[-2], 1)
    left = lens_a[-2] - 1 + lens_a[-1]
    p.next(left + 10, error=BAD_TEXT, delivered=left, text=mode != "java")
    # 4. the stream's end is an empty suffix
    p.seek(len(data), 0)
    p.next(0)
    p.next(1, error=V2_EOF, delivered=0)
    # 5., 6.
    p.seek(len(data) + 1, 0, error=PAST_END)
    with pytest.raises(orc.InvalidArgument, match="uncompressed RLE position needs 2 values"):
        ours.seek(offs_a[3])
    # 7. a mask that asks for exactly the values left, then for one more
    left = sum(lens_b[-3:])
    p.seek(offs_b[-3], 0)
    p.next(2 * left, half_mask(left))
    p.seek(offs_b[-3], 0)
    p.next(2 * left + 2, half_mask(left + 1), error=V2_EOF, delivered=left)


# ---- byte / boolean RLE -----------------------------------------------------
BYTE_EOF = "bad read in nextBuffer"
# a literal of two bytes that are themselves a group (a run of 3 x 7): its
# second byte is a place to seek to that no walk from a group start reaches
INNER = bm.lit(b"\x00\x07")


def build_byte_stream():
    """(stream, the offset of INNER in its third segment, its group table)."""
    rng = np.random.default_rng(5)
    groups = [bm.rand_run(rng) if rng.random() < 0.5 else bm.rand_lit(rng, int(rng.integers(1, 129)))
              for _ in range(660)]
    inner = len(b"".join(groups[:600]))
    data = b"".join(groups[:600]) + INNER + b"".join(groups[600:])
    return data, inner, bm.group_table(data)


@pytest.fixture(scope="module")
def byte_stream():
    return build_byte_stream()


@pytest.mark.parametrize("boolean", [False, True], ids=["byte", "boolean"])
def test_byterle_seek_sequence(orc, byte_stream, boolean):
    data, inner, table = byte_stream
    total = bm.decode(data)[1]
    cuts = [int(s[0]) for s in orc.BytePlan(data).segments()]
    assert len(cuts) >= 3 and 36_000 < total < 45_000 and inner > cuts[2]
    ours = orc.ByteRleDecoder(data, boolean=boolean)
    p = Pair(orc, ours, oracle.ByteRleDecoder(data, boolean=boolean), np.uint8)
    sizes = [b[1] - a[1] for a, b in zip(table, table[1:] + [(len(data), total)])]
    unit = 8 if boolean else 1

    def pos(off, skip, bits=0):
        return (off, skip, bits) if boolean else (off, skip)

    # 1. a group start inside the third segment
    k = next(i for i, (o, _) in enumerate(table) if o > cuts[2] and sizes[i] > 10)
    off = table[k][0]
    assert off not in cuts and off < inner
    for skip in (0, sizes[k] - 1, sizes[k]):
        p.seek(*pos(off, skip))
        p.next(13)
    if boolean:
        for bits in (0, 1, 7, 8):
            p.seek(off, 2, bits)
            p.next(13)
        p.seek(off, 2, 9, error="bad position")
    # 2. back to a group start in the first segment
    assert 0 < table[3][0] < cuts[1]
    p.seek(*pos(table[3][0], 0))
    first = p.next(50)
    # 3. a byte inside a literal: decoded again from there; then a group start
    # before that origin
    p.seek(*pos(inner + 1, 1))
    p.next(20)
    p.seek(*pos(table[3][0], 0))
    np.testing.assert_array_equal(p.next(50), first)
    # 4. the stream's end is an empty suffix
    p.seek(*pos(len(data), 0))
    p.next(0)
    p.next(1, error=BYTE_EOF, delivered=0)
    # 5., 6.
    p.seek(*pos(len(data) + 1, 0), error=PAST_END)
    with pytest.raises(orc.InvalidArgument, match="bad position"):
        ours.seek(table[3][0])
    # 7. a mask that asks for exactly what is left, then for one more
    left = unit * (total - table[-3][1])
    p.seek(*pos(table[-3][0], 0))
    p.next(2 * left, half_mask(left))
    p.seek(*pos(table[-3][0], 0))
    # (the reference's boolean decoder fails while it still holds bytes, not rows, in the caller's buffer)
    p.next(2 * left + 2, half_mask(left + 1), error=BYTE_EOF, delivered=0 if boolean else left)
    if boolean:
        # a skip that ends inside the stream's last byte
        p.seek(table[-3][0], 0, 0)
        p.skip(left - 3)
        p.next(3)
        p.next(1, error=BYTE_EOF, delivered=0)


# ---- one-shot host decodes --------------------------------------------------
ONE_SHOT = [("rlev2", np.int16), ("rlev2", np.int32), ("rlev2", np.int64), ("rlev1", np.int32), ("rlev1", np.int64)]


@pytest.mark.parametrize("fmt,dtype", ONE_SHOT, ids=["%s-%s" % (f, np.dtype(d).name) for f, d in ONE_SHOT])
def test_one_shot_masks(orc, fmt, dtype):
    if fmt == "rlev2":
        data, _, lens = v2_part(orc, 9, 6, True)
        total, eof = sum(lens), V2_EOF
        decode = orc.rlev2_decode

        def want(n, nn):
            return oracle.RleDecoderV2(data, True).next(n, nn, dtype=dtype)
    else:
        data, vals = v1_encode(random_groups(np.random.default_rng(9), 400, True, 30), True)
        data, total, eof = bytes(data), vals.size, "bad read in readByte"
        decode = orc.rlev1_decode

        def want(n, nn):
            return oracle.RleDecoderV1(data, True).next(n, nn).astype(dtype)

    assert decode(data, 0, True, dtype=dtype).size == 0
    # no row set: nothing is decoded and no slot written
    out = np.full(50, 77, dtype=dtype)
    decode(data, 50, True, not_null=np.zeros(50, dtype=np.uint8), out=out)
    assert (out == 77).all()
    # exactly the values the stream holds, then one more
    nn = half_mask(total)
    np.testing.assert_array_equal(decode(data, nn.size, True, not_null=nn, dtype=dtype), want(nn.size, nn))
    np.testing.assert_array_equal(decode(data, total, True, dtype=dtype), want(total, None))
    nn = half_mask(total + 1)
    with pytest.raises(oracle.OracleError) as ref:
        want(nn.size, nn)
    with pytest.raises(orc.ParseError) as got:
        decode(data, nn.size, True, not_null=nn, dtype=dtype)
    assert str(got.value) == str(ref.value) == eof
