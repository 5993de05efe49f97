"""The Arrow export kernels (orc_amd/csrc/arrow_kernels.hip) through their
column-level entries (include/orcg_arrow.h, orc_amd/arrow.py), against numpy
and pyarrow built from the same host arrays. Every comparison is exact and
covers the whole buffer: the payload and the zero padding up to 64 bytes (the
outputs are pre-filled with 0xAA).

Counts are the smallest that cross every edge: around a byte of bitmap (7, 8,
9), a 64-byte padding unit and a wave (63, 64, 65), a workgroup's trip (255,
256, 257), four of them (1023, 1025), sixteen (4097), and 70,001: more items
than one pass of the capped grid takes for the bitmap kernels' callers and a
ragged tail for every item width."""
import decimal

import numpy as np
import pytest
import torch

import orc_amd
from orc_amd import arrow as A

pa = pytest.importorskip("pyarrow")

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 70001]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def pad(raw):
    """The bytes of a host array with the export's zero padding."""
    b = np.frombuffer(np.ascontiguousarray(raw).tobytes(), np.uint8)
    return np.concatenate([b, np.zeros(A.padded(b.size) - b.size, np.uint8)])


def bitmap(mask):
    return pad(np.packbits(np.asarray(mask, bool), bitorder="little"))


def masks(n, rng):
    """(label, not_null bytes) patterns of n rows."""
    out = [("all", np.ones(n, np.uint8)), ("none", np.zeros(n, np.uint8)),
           ("random", (rng.random(n) >= 0.1).astype(np.uint8))]
    for at in sorted({0, n - 1, 7, 8, 63, 64}):
        if 0 <= at < n:
            m = np.ones(n, np.uint8)
            m[at] = 0
            out.append(("null@%d" % at, m))
    # any non-zero byte is a set row
    odd = (rng.integers(0, 4, n) * 85).astype(np.uint8)
    out.append(("bytes", odd))
    return out


# ---- validity ----

@pytest.mark.parametrize("n", SIZES)
def test_validity_bitmap(ctx, n):
    rng = np.random.default_rng(n)
    data = np.arange(n, dtype=np.int8)
    for label, m in masks(n, rng):
        got, nulls = A.validity_device(ctx, dev(m))
        want = bitmap(m != 0)
        assert got.numel() == want.size == A.padded((n + 7) // 8)
        assert np.array_equal(host(got), want), (n, label)
        assert nulls == int((m == 0).sum()), (n, label)
        arr = pa.Array.from_buffers(pa.int8(), n, [pa.py_buffer(host(got).tobytes()), pa.py_buffer(data.tobytes())],
                                    null_count=nulls)
        arr.validate(full=True)
        assert arr.equals(pa.array(data, mask=(m == 0)))


def test_validity_of_an_unaligned_mask(ctx):
    """A mask that does not start on 16 bytes takes the byte path."""
    rng = np.random.default_rng(5)
    m = (rng.random(1000 + 3) >= 0.3).astype(np.uint8)
    got, nulls = A.validity_device(ctx, dev(m)[3:])
    assert np.array_equal(host(got), bitmap(m[3:] != 0)) and nulls == int((m[3:] == 0).sum())


def test_no_mask_gives_no_buffer(ctx):
    assert A.validity_device(ctx, None) == (None, 0)


# ---- fixed width ----

def int_values(n, bits, rng):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    edge = np.array([lo, hi, -1, 0, 1, lo + 1, hi - 1], np.int64)
    v = rng.integers(lo, hi + 1, size=n, dtype=np.int64)
    v[:min(n, edge.size)] = edge[:n]
    if n > 16:
        v[-7:] = edge  # the ragged tail holds the extremes too
    return v


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form,bits,dtype,typ", [(A.INT8, 8, np.int8, "int8"), (A.INT16, 16, np.int16, "int16"),
                                                 (A.INT32, 32, np.int32, "int32")])
def test_fixed_integers(ctx, n, form, bits, dtype, typ):
    v = int_values(n, bits, np.random.default_rng(n + bits))
    got = host(A.fixed_device(ctx, form, dev(v)))
    assert np.array_equal(got, pad(v.astype(dtype))), (n, typ)
    arr = pa.Array.from_buffers(getattr(pa, typ)(), n, [None, pa.py_buffer(got.tobytes())])
    arr.validate(full=True)
    assert arr.equals(pa.array(v.astype(dtype)))
    if form == A.INT32:
        d = pa.Array.from_buffers(pa.date32(), n, [None, pa.py_buffer(got.tobytes())])
        d.validate(full=True)
        assert d.equals(pa.array(v.astype(np.int32)).cast(pa.date32()))


@pytest.mark.parametrize("n", SIZES)
def test_fixed_boolean_bitmap(ctx, n):
    rng = np.random.default_rng(n)
    v = rng.integers(0, 2, size=n, dtype=np.int64)
    v[rng.random(n) < 0.05] = -1       # any non-zero value is true
    v[rng.random(n) < 0.05] = 1 << 40  # (the low word alone is zero)
    got = host(A.fixed_device(ctx, A.BOOL, dev(v)))
    assert np.array_equal(got, bitmap(v != 0)), n
    arr = pa.Array.from_buffers(pa.bool_(), n, [None, pa.py_buffer(got.tobytes())])
    arr.validate(full=True)
    assert arr.equals(pa.array(v != 0))


@pytest.mark.parametrize("n", SIZES)
def test_fixed_float32(ctx, n):
    rng = np.random.default_rng(n)
    f = (rng.standard_normal(n) * 1e3).astype(np.float32)
    edge = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, np.finfo(np.float32).max, np.finfo(np.float32).tiny,
                     -np.finfo(np.float32).max, 1e-45], np.float32)
    f[:min(n, edge.size)] = edge[:n]
    got = host(A.fixed_device(ctx, A.FLOAT32, dev(f.astype(np.float64))))
    assert np.array_equal(got, pad(f)), n  # bit patterns
    arr = pa.Array.from_buffers(pa.float32(), n, [None, pa.py_buffer(got.tobytes())])
    arr.validate(full=True)


def _decimals(ints, typ):
    return pa.array([decimal.Decimal(int(x)) for x in ints], type=typ)


@pytest.mark.parametrize("n", SIZES)
def test_fixed_decimal64_sign_extends(ctx, n):
    rng = np.random.default_rng(n)
    v = rng.integers(-10 ** 18 + 1, 10 ** 18, size=n, dtype=np.int64)
    edge = np.array([-1, 0, 1, -10 ** 18 + 1, 10 ** 18 - 1, -(1 << 32), (1 << 32) - 1, -5], np.int64)
    v[:min(n, edge.size)] = edge[:n]
    got = host(A.fixed_device(ctx, A.DEC64, dev(v)))
    want = np.stack([v, v >> 63], axis=1)  # little-endian words [lo, hi]
    assert np.array_equal(got, pad(want)), n
    if n <= 4097:
        arr = pa.Array.from_buffers(pa.decimal128(18, 0), n, [None, pa.py_buffer(got.tobytes())])
        arr.validate(full=True)
        assert arr.equals(_decimals(v, pa.decimal128(18, 0)))


@pytest.mark.parametrize("n", SIZES)
def test_fixed_decimal128_swaps_words(ctx, n):
    rng = np.random.default_rng(n)
    big = [int(x) * int(y) for x, y in zip(rng.integers(-10 ** 18, 10 ** 18, n), rng.integers(0, 10 ** 18, n))]
    edge = [-1, 0, 1, -(1 << 63), (1 << 63), -(1 << 64), (1 << 64) - 1, -(1 << 63) - 1, 10 ** 38 - 1, -10 ** 38 + 1,
            -(1 << 64) - 5, -3]  # hi = -1 with lo of either sign; lo = 0; hi = -2
    big[:min(n, len(edge))] = edge[:n]
    hi = np.array([x >> 64 for x in big], dtype=np.int64).reshape(n)
    lo = np.array([x & ((1 << 64) - 1) for x in big], dtype=np.uint64).view(np.int64).reshape(n)
    got = host(A.fixed_device(ctx, A.DEC128, dev(np.stack([hi, lo], axis=1))))
    assert np.array_equal(got, pad(np.stack([lo, hi], axis=1))), n
    if n <= 4097:
        arr = pa.Array.from_buffers(pa.decimal128(38, 0), n, [None, pa.py_buffer(got.tobytes())])
        arr.validate(full=True)
        assert arr.equals(_decimals(big, pa.decimal128(38, 0)))


@pytest.mark.parametrize("n", SIZES)
def test_fixed_timestamp_nanoseconds(ctx, n):
    rng = np.random.default_rng(n)
    secs = rng.integers(-(1 << 33), 1 << 33, size=n, dtype=np.int64)
    nanos = rng.integers(0, 10 ** 9, size=n, dtype=np.int64)
    edge_s = np.array([-1, 0, -1, 9223372036, -9223372036, 1 << 40, -(1 << 62)], np.int64)
    edge_n = np.array([999999999, 0, 1, 854775807, 145224193, 5, 7], np.int64)
    k = min(n, edge_s.size)
    secs[:k], nanos[:k] = edge_s[:k], edge_n[:k]
    got = host(A.fixed_device(ctx, A.TIMESTAMP_NS, dev(secs), dev(nanos)))
    # wrapping arithmetic modulo 2^64 (rows 5 and 6 wrap)
    want = (secs.view(np.uint64) * np.uint64(10 ** 9) + nanos.view(np.uint64)).view(np.int64)
    assert np.array_equal(got, pad(want)), n
    if n > 3:
        assert want[0] == -1 and want[2] == -999999999 and want[3] == 9223372036854775807
    arr = pa.Array.from_buffers(pa.timestamp("ns"), n, [None, pa.py_buffer(got.tobytes())])
    arr.validate(full=True)
    assert arr.equals(pa.array(want, type=pa.timestamp("ns")))


# ---- offsets ----

def string_array(n, validity, offsets, data, nulls, typ=None):
    arr = pa.Array.from_buffers(typ or pa.string(), n,
                                [None if validity is None else pa.py_buffer(validity.tobytes()),
                                 pa.py_buffer(offsets.tobytes()), pa.py_buffer(data.tobytes())], null_count=nulls)
    arr.validate(full=True)
    return arr


@pytest.mark.parametrize("n", SIZES)
def test_offsets_from_masked_lengths(ctx, n):
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 12, size=n, dtype=np.int64)
    lens[rng.random(n) < 0.2] = 0  # empty strings
    for label, m in masks(n, rng) + [("runs", (np.arange(n) % 7 > 2).astype(np.uint8)), ("no mask", None)]:
        live = lens if m is None else np.where(m != 0, lens, 0)
        # the length slot of a null row is not trusted to hold 0
        shown = lens if m is None else np.where(m != 0, lens, 5)
        got = host(A.offsets_device(ctx, n, lengths=dev(shown), not_null=None if m is None else dev(m)))
        want = np.concatenate([[0], np.cumsum(live)]).astype(np.int32)
        assert np.array_equal(got, pad(want)), (n, label)
        total = int(want[-1])
        data = np.frombuffer((b"abcdefghij" * (total // 10 + 1))[:total], np.uint8)
        valid = None if m is None else bitmap(m != 0)
        arr = string_array(n, valid, got, data, 0 if m is None else int((m == 0).sum()))
        raw = data.tobytes()
        rows = [None if (m is not None and not m[i]) else raw[want[i]:want[i + 1]].decode() for i in range(n)]
        assert arr.equals(pa.array(rows, type=pa.string())), (n, label)


@pytest.mark.parametrize("n", SIZES)
def test_offsets_from_int64_offsets(ctx, n):
    rng = np.random.default_rng(n)
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 5, size=n))]).astype(np.int64)
    got = host(A.offsets_device(ctx, n, offsets64=dev(off)))
    assert np.array_equal(got, pad(off.astype(np.int32))), n


@pytest.mark.parametrize("n", [1, 3, 4, 1025])
def test_offsets_range_check(ctx, n):
    """No data buffer that large is needed: the offsets are crafted."""
    off = np.zeros(n + 1, np.int64)
    off[-1] = (1 << 31) - 1
    got = host(A.offsets_device(ctx, n, offsets64=dev(off)))
    assert np.array_equal(got, pad(off.astype(np.int32)))
    off[-1] = 1 << 31
    with pytest.raises(orc_amd.InvalidArgument, match="offsets do not fit int32"):
        A.offsets_device(ctx, n, offsets64=dev(off))
    # the lengths' scan is checked the same way
    lens = np.zeros(n, np.int64)
    lens[0] = 1 << 31
    with pytest.raises(orc_amd.InvalidArgument, match="offsets do not fit int32"):
        A.offsets_device(ctx, n, lengths=dev(lens))
    lens[0] = (1 << 31) - 1
    got = host(A.offsets_device(ctx, n, lengths=dev(lens)))
    assert got.view(np.int32)[n] == (1 << 31) - 1
    # and the context is usable afterwards
    assert np.array_equal(host(A.offsets_device(ctx, 1, lengths=dev(np.array([3], np.int64)))), pad(np.array([0, 3], np.int32)))


# ---- dictionary strings ----

def dictionary(entries):
    """(dict_offsets int64 [k + 1], blob uint8, pyarrow values) of byte strings."""
    off = np.concatenate([[0], np.cumsum([len(e) for e in entries])]).astype(np.int64)
    blob = np.frombuffer(b"".join(entries), np.uint8)
    return off, blob, pa.array([e.decode() for e in entries], type=pa.string())


def check_dict_strings(ctx, entries, index, m, label):
    n = index.size
    off, blob, values = dictionary(entries)
    d_blob = dev(blob) if blob.size else torch.zeros(0, dtype=torch.uint8, device=DEV)
    nn = None if m is None else dev(m)
    nulls = 0 if m is None else int((m == 0).sum())
    take = pa.array(index, mask=None if m is None else (m == 0))
    want = values.take(take) if len(values) else pa.array([None] * n, type=pa.string())
    # materialised
    offs, data, nbytes = A.dict_strings_device(ctx, dev(index), nn, dev(off), d_blob)
    lens = (off[1:] - off[:-1])[index] if len(entries) else np.zeros(n, np.int64)
    live = lens if m is None else np.where(m != 0, lens, 0)
    want_off = np.concatenate([[0], np.cumsum(live)]).astype(np.int32)
    assert np.array_equal(host(offs), pad(want_off)), label
    assert nbytes == int(want_off[-1]) and data.numel() == A.padded(nbytes), label
    got = string_array(n, None if m is None else bitmap(m != 0), host(offs), host(data), nulls)
    assert got.equals(want), label
    assert not host(data)[nbytes:].any(), label  # the padding
    # dictionary form
    idx, doff, dbytes = A.dict_strings_device(ctx, dev(index), nn, dev(off), d_blob, dictionary=True)
    assert np.array_equal(host(idx), pad(index.astype(np.int32))), label
    assert dbytes == 4 * off.size and np.array_equal(host(doff), pad(off.astype(np.int32))), label
    dvalues = string_array(len(entries), None, host(doff), blob, 0)
    codes = pa.Array.from_buffers(pa.int32(), n, [None if m is None else pa.py_buffer(bitmap(m != 0).tobytes()),
                                                  pa.py_buffer(host(idx).tobytes())], null_count=nulls)
    darr = pa.DictionaryArray.from_arrays(codes, dvalues)
    darr.validate(full=True)
    assert darr.dictionary_decode().equals(want), label


@pytest.mark.parametrize("n", SIZES)
def test_dictionary_one_entry_repeated(ctx, n):
    rng = np.random.default_rng(n)
    check_dict_strings(ctx, [b"hello"], np.zeros(n, np.int64), None, n)
    check_dict_strings(ctx, [b"hello"], np.zeros(n, np.int64), (rng.random(n) >= 0.1).astype(np.uint8), n)


ENTRIES = [b"", b"Z" * 5000] + [bytes([97 + k % 26]) * k for k in range(1, 34)]


@pytest.mark.parametrize("n", [1, 9, 65, 257, 1025, 4097])
def test_dictionary_gather_straddles_chunks_and_tiles(ctx, n):
    """A zero-length entry, one of 5,000 bytes (longer than a tile), entries
    of 1 to 33 bytes: rows straddle 16-byte chunks and 4,096-byte tiles."""
    rng = np.random.default_rng(n)
    index = rng.integers(0, len(ENTRIES), size=n, dtype=np.int64)
    index[index == 1] = np.where(rng.random((index == 1).sum()) < 0.5, 1, 7)  # fewer of the long entry
    index[0] = 1
    check_dict_strings(ctx, ENTRIES, index, None, (n, "no mask"))
    m = (rng.random(n) >= 0.1).astype(np.uint8)
    for label, first, last in [("first null", 0, 1), ("last null", 1, 0), ("both null", 0, 0), ("random", 1, 1)]:
        mm = m.copy()
        mm[0], mm[-1] = first, last
        idx = np.where(mm != 0, index, 0)  # the slot of a null row holds 0
        check_dict_strings(ctx, ENTRIES, idx, mm, (n, label))


def test_dictionary_of_size_zero_with_all_rows_null(ctx):
    n = 257
    check_dict_strings(ctx, [], np.zeros(n, np.int64), np.zeros(n, np.uint8), "empty dictionary")


def test_dictionary_tiles_with_more_rows_than_the_stage(ctx):
    """Tiles whose rows outnumber the offsets staged in LDS: one-byte rows
    (4,096 rows a tile) and long runs of empty rows."""
    n = 70001
    rng = np.random.default_rng(1)
    check_dict_strings(ctx, [b"a", b"b"], rng.integers(0, 2, size=n, dtype=np.int64), None, "one-byte rows")
    index = (rng.random(n) < 0.001).astype(np.int64)
    index[-1] = 1
    check_dict_strings(ctx, [b"", b"x" * 40], index, None, "runs of empty rows")
    m = (rng.random(n) >= 0.5).astype(np.uint8)
    check_dict_strings(ctx, [b"", b"x" * 40, b"yz"], np.where(m != 0, index + (np.arange(n) % 2), 0), m, "mixed")


def test_dictionary_entry_out_of_range_is_an_error(ctx):
    off, blob, _ = dictionary([b"ab", b"c"])
    index = np.array([0, 1, 2, 0], np.int64)
    with pytest.raises(orc_amd.OrcError, match="Entry index out of range"):
        A.dict_strings_device(ctx, dev(index), None, dev(off), dev(blob))
    # a null row's slot is not looked up
    m = np.array([1, 1, 0, 1], np.uint8)
    offs, data, nbytes = A.dict_strings_device(ctx, dev(index), dev(m), dev(off), dev(blob))
    assert nbytes == 5 and host(data)[:5].tobytes() == b"abcab"
