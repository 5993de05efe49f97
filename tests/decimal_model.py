"""Exact-integer model of the DECIMAL value decode, and varint stream builders.

The model is written from the ORC specification ("Decimal Columns": the DATA
stream is a run of zigzag base-128 varints, SECONDARY holds each value's
scale) and from the behaviour decimal_kernels.hip documents for the three
column readers it stands in for. It uses Python ints only: no ctypes, no
fixed-width arithmetic except the explicit wraps below. Modes, as in the
kernel:

0  Decimal64: int64 values. Payload bits are or-ed in at (offset & 63); a
   value is multiplied (wrapping at 64 bits) or divided (truncating toward
   zero) by 10^d, d <= 18, else "Decimal scale out of range".
1  Decimal128: payload bits at offset >= 128 are dropped; unzigzag is a
   logical shift, then negate and subtract 1 if the raw value was odd;
   rescale in steps of at most 18 digits (wrap at 128 bits after each
   multiply, truncate toward zero on each divide, stop once the value is 0);
   scales are taken as uint32.
2  Hive 0.11: as 1, and a varint with a byte at offset > 128, or a payload
   above 3 at offset 126, is too long; too long or |v| > 10^38 - 1 raises
   "Hive 0.11 decimal was more than 38 digits."
3  as 2, but such a value becomes (0, keep 0); every other keep is 1.

Running out of bytes raises "Read past end of stream in
Decimal64ColumnReader" in every mode.
"""
import numpy as np

TILE = 4096  # bytes of DATA stream per workgroup (256 threads x 16 bytes)
PER_THREAD = 16
LOOK = 64  # look-back bytes staged in LDS before the tile

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
HIVE_MAX = 10 ** 38 - 1

PAST_END = "Read past end of stream in Decimal64ColumnReader"
BAD_SCALE = "Decimal scale out of range"
HIVE_OVERFLOW = "Hive 0.11 decimal was more than 38 digits."


class ModelError(Exception):
    """The error the decode raises; `index` is the value it was raised at."""

    def __init__(self, msg, index):
        super().__init__(msg)
        self.index = index


def _signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _trunc_div(v, d):
    q = abs(v) // d
    return -q if v < 0 else q


def _int32(s):
    return _signed(int(s), 32)


def decode_ints(data, scales, n, col_scale, mode):
    """The decode as Python ints: ([values], [keep]); keep is None below mode 3."""
    data = bytes(data)
    wide = mode >= 1
    hive = mode >= 2
    vals, keep = [], ([] if mode == 3 else None)
    pos = 0
    for i in range(n):
        raw, offset, too_long = 0, 0, False
        while True:
            if pos >= len(data):
                raise ModelError(PAST_END, i)
            b = data[pos]
            pos += 1
            x = b & 0x7F
            if offset > 128 or (offset == 126 and x > 3):
                too_long = True
            if not wide:
                raw |= (x << (offset & 63)) & M64
            elif offset < 128:
                raw |= (x << offset) & M128
            offset += 7
            if b < 0x80:
                break
        cur = _int32(scales[i])
        if not wide:
            v = _signed((raw >> 1) ^ (-(raw & 1) & M64), 64)
            if col_scale > cur and col_scale - cur <= 18:
                v = _signed(v * 10 ** (col_scale - cur), 64)
            elif col_scale < cur and cur - col_scale <= 18:
                v = _trunc_div(v, 10 ** (cur - col_scale))
            elif col_scale != cur:
                raise ModelError(BAD_SCALE, i)
            vals.append(v)
            continue
        v = raw >> 1
        if raw & 1:
            v = (-v - 1) & M128
        v = _signed(v, 128)
        s, c = col_scale & 0xFFFFFFFF, cur & 0xFFFFFFFF
        while s > c and v != 0:
            a = min(18, s - c)
            v = _signed(v * 10 ** a, 128)
            c += a
        while c > s and v != 0:
            a = min(18, c - s)
            v = _trunc_div(v, 10 ** a)
            c -= a
        if hive:
            over = too_long or abs(v) > HIVE_MAX
            if mode == 2 and over:
                raise ModelError(HIVE_OVERFLOW, i)
            if mode == 3:
                keep.append(0 if over else 1)
                if over:
                    v = 0
        vals.append(v)
    return vals, keep


def pack(vals, wide):
    """Python ints as the decoders' output: int64[n], or int64[n, 2] of [hi, lo]."""
    if not wide:
        return np.array([_signed(v, 64) for v in vals], dtype=np.int64).reshape(len(vals))
    out = np.zeros((len(vals), 2), dtype=np.int64)
    for i, v in enumerate(vals):
        u = v & M128
        out[i, 0] = _signed(u >> 64, 64)
        out[i, 1] = _signed(u & M64, 64)
    return out


def decode(data, scales, n, col_scale, mode):
    """int64[n] (mode 0), int64[n, 2] (modes 1, 2) or (int64[n, 2], uint8[n]
    keep) (mode 3); raises ModelError with the decoders' message."""
    vals, keep = decode_ints(data, scales, n, col_scale, mode)
    out = pack(vals, mode >= 1)
    return (out, np.array(keep, dtype=np.uint8).reshape(n)) if mode == 3 else out


# ---- varints ---------------------------------------------------------------

def zigzag(v):
    return v << 1 if v >= 0 else ((-v) << 1) - 1


def varint(u, length=None):
    """The base-128 varint of the unsigned u: minimal, or exactly `length`
    bytes (payload bits past 7 * length dropped, zero bytes as padding)."""
    out = bytearray()
    if length is None:
        length = max(1, (u.bit_length() + 6) // 7)
    for i in range(length):
        out.append(((u >> (7 * i)) & 0x7F) | (0x80 if i < length - 1 else 0))
    return bytes(out)


def padded_zero(k):
    """A zero of k bytes: k - 1 continuation bytes 0x80, then 0x00."""
    return b"\x80" * (k - 1) + b"\x00"


def filler(i):
    """The i-th one-byte filler varint (a non-constant small value)."""
    return bytes([(i * 37 + 11) & 0x7F])


def terminators(data):
    """Byte offsets of the varint terminators of a stream."""
    return np.flatnonzero(np.frombuffer(bytes(data), dtype=np.uint8) < 0x80)


# ---- stream builders (deterministic; all return bytes) ---------------------

def dense(n):
    """n one-byte varints."""
    return b"".join(filler(i) for i in range(n))


def mixed(n, wide, rng, max_len=None, max_pad=199):
    """n varints: ~40 % one byte, the rest uniform in byte length 1..max_len
    (default 10 for Decimal64, 19 for Decimal128) with random payload bits;
    ~1 % of the values are instead a zero of 1..max_pad continuation bytes
    0x80 and a 0x00 terminator. A Decimal64 payload never goes past 10 bytes
    (the reference's shift past 63 bits is undefined)."""
    top = max_len or (19 if wide else 10)
    out = bytearray()
    for _ in range(n):
        r = rng.random()
        if r < 0.01 and max_pad > 0:
            out += padded_zero(1 + int(rng.integers(1, max_pad + 1)))
            continue
        ln = 1 if r < 0.41 else int(rng.integers(1, top + 1))
        out += varint(int.from_bytes(rng.bytes(ln), "little"), ln)
    return bytes(out)


def with_length(body, length, last):
    """`body` cut at a varint boundary and extended with one-byte fillers to
    exactly `length` bytes, the bytes `last` (one varint) ending at `length`."""
    room = length - len(last)
    ends = terminators(body) + 1
    fit = ends[ends <= room]
    cut = int(fit[-1]) if len(fit) else 0
    return body[:cut] + b"".join(filler(i) for i in range(room - cut)) + last


def long_varint(wide, seed):
    """A full-width varint whose value every mode accepts unscaled: 10 bytes
    with the 64th bit set (Decimal64), 19 bytes with last byte 1 (Decimal128:
    |v| about 2^126 < 10^38)."""
    rng = np.random.default_rng(1000 + seed)
    ln = 19 if wide else 10
    u = int.from_bytes(rng.bytes(ln), "little") & ((1 << (7 * (ln - 1))) - 1)
    return varint(u | (1 << (7 * (ln - 1))), ln)


def straddle(split, wide):
    """One full-width varint (long_varint) with exactly `split` of its bytes
    before byte TILE; one-byte fillers before it and 40 after."""
    lv = long_varint(wide, split)
    assert 1 <= split < len(lv)
    return dense(TILE - split) + lv + b"".join(filler(i) for i in range(40))


LONG_BACK_K = (63, 64, 65, 66, 80, 4100)
LONG_BACK_RAW = 0x55  # the padded varint's payload, all in its first byte: unzigzags to -43
# (thread, byte in the thread's 16) of the terminator: the first byte of a tile
# (65 bytes end where the look-back ends, 66 reach past it, and 4100 cover the
# whole tile before), a middle thread, and the last byte of a tile
LONG_BACK_AT = {"first": (0, 0), "middle": (128, 7), "last": (255, 15)}


def long_back(k, where):
    """LONG_BACK_RAW padded with zero payload to k bytes, its terminator in the
    given thread of a tile; one-byte fillers before it and 40 after. The
    payload sits in the varint's first byte, k - 1 bytes before the
    terminator: past the LDS look-back it is found only by reading global
    memory. k = 4100 at "first" covers a whole tile without a terminator."""
    thread, byte = LONG_BACK_AT[where]
    tile = (k + TILE - 1) // TILE
    end = tile * TILE + thread * PER_THREAD + byte  # offset of the terminator
    return dense(end - (k - 1)) + varint(LONG_BACK_RAW, k) + b"".join(filler(i) for i in range(40))


def extremes():
    """Raw varints at the edges of 128 bits and of 38 digits, one bytes object each."""
    last3 = varint(int.from_bytes(b"\xa5" * 16, "little") | (3 << 126), 19)
    last4 = last3[:-1] + b"\x04"
    raws = [(1 << 128) - 1, (1 << 128) - 2, 1 << 127, (1 << 127) - 1, 0, 1, 2, zigzag(HIVE_MAX), zigzag(-HIVE_MAX),
            zigzag(HIVE_MAX + 1), zigzag(-HIVE_MAX - 1), (1 << 126) | 1]
    return [varint(u) for u in raws] + [last3, last4]


def hive_mixed(n, rng):
    """n varints for the Hive 0.11 modes at equal column and value scale:
    mixed values of at most 17 bytes (|v| < 2^118, in range), ~2 % replaced by
    +-(10^38 + r) (19 bytes, last byte 2: overflows), ~1 % by a too-long
    varint (19 bytes with a last byte above 3, or a zero of 20..40 bytes);
    both kinds every 97 / 193 values as well and an overflow as the last
    value, so that no tile goes without."""
    out = bytearray()
    for i in range(n):
        r = rng.random()
        if r < 0.02 or i % 97 == 5 or i == n - 1:
            m = HIVE_MAX + 1 + int(rng.integers(0, 1 << 40))
            out += varint(zigzag(m if rng.random() < 0.5 else -m))
        elif r < 0.03 or i % 193 == 7:
            if rng.random() < 0.5:
                out += varint(int.from_bytes(rng.bytes(19), "little") | (4 << 126), 19)
            else:
                out += padded_zero(int(rng.integers(20, 41)))
        else:
            out += mixed(1, True, rng, max_len=17, max_pad=0)
    return bytes(out)


def spread_scales(n, col_scale, mode, rng):
    """Per-value scales around the column's: +-18 (Decimal64), +-40 clipped
    at 0 (Decimal128 and Hive 0.11)."""
    if mode == 0:
        return (col_scale + rng.integers(-18, 19, size=n)).astype(np.int64)
    return np.clip(col_scale + rng.integers(-40, 41, size=n), 0, None).astype(np.int64)
