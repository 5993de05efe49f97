"""An exact model of the Snappy raw block format as the reader decodes it:
`decode` restates snappy_decompress (orc_amd/csrc/orc_file.cpp) rule by rule
and in its order, `plan` restates plan_snappy_framed (inflate_plan.cpp), and
`Stream` builds blocks element by element so that a test can put one feature
at a chosen output offset. Pure Python, no GPU."""

BAD_LENGTH = "snappy: bad length"
TOO_LARGE = "snappy: output exceeds the compression block size"
LITERAL_TRUNCATED = "snappy: truncated literal"
LITERAL_RANGE = "snappy: literal out of range"
COPY_TRUNCATED = "snappy: truncated copy"
COPY_RANGE = "snappy: copy out of range"
LENGTH_MISMATCH = "snappy: length mismatch"
PAST_EOF = "Read past EOF in DecompressionStream::readBuffer"

STORED = 1
MAX_BYTES = 1 << 31  # a chunk's offsets are 32-bit on the device: the plan caps the block size below it


def preamble(chunk, cap=None):
    """(ulen, bytes consumed) or an error text."""
    ulen, p, sh = 0, 0, 0
    while True:
        if p >= len(chunk) or sh > 35:
            return BAD_LENGTH
        b = chunk[p]
        p += 1
        ulen |= (b & 0x7F) << sh
        if not b & 0x80:
            break
        sh += 7
    if cap is not None and ulen > cap:
        return TOO_LARGE
    return ulen, p


def decode(chunk, cap=None):
    """The decompressed bytes of one raw Snappy block, or the error text of the
    first check that fails."""
    chunk = bytes(chunk)
    r = preamble(chunk, cap)
    if isinstance(r, str):
        return r
    ulen, p = r
    n = len(chunk)
    out = bytearray()
    while p < n:
        tag = chunk[p]
        p += 1
        kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1
            if ln > 60:
                nb = ln - 60
                if n - p < nb:
                    return LITERAL_TRUNCATED
                ln = int.from_bytes(chunk[p:p + nb], "little") + 1
                p += nb
            if n - p < ln or len(out) + ln > ulen:
                return LITERAL_RANGE
            out += chunk[p:p + ln]
            p += ln
            continue
        if kind == 1:
            if p >= n:
                return COPY_TRUNCATED
            ln = 4 + ((tag >> 2) & 7)
            off = ((tag >> 5) << 8) | chunk[p]
            p += 1
        elif kind == 2:
            if n - p < 2:
                return COPY_TRUNCATED
            ln = 1 + (tag >> 2)
            off = int.from_bytes(chunk[p:p + 2], "little")
            p += 2
        else:
            if n - p < 4:
                return COPY_TRUNCATED
            ln = 1 + (tag >> 2)
            off = int.from_bytes(chunk[p:p + 4], "little")
            p += 4
        if off == 0 or off > len(out) or len(out) + ln > ulen:
            return COPY_RANGE
        o = len(out)
        if off >= ln:
            out += out[o - off:o - off + ln]
        else:
            for i in range(ln):
                out.append(out[o - off + i])
    if len(out) != ulen:
        return LENGTH_MISMATCH
    return bytes(out)


def frame(body, original=False):
    """An ORC chunk: the 3-byte header (length << 1 | original) and the body."""
    h = (len(body) << 1) | int(original)
    assert h < 1 << 24
    return h.to_bytes(3, "little") + bytes(body)


def plan(framed, block_size):
    """([(src_offset, src_bytes, dst_offset, dst_bytes, flags)], total) of a
    run of framed chunks, or the error text."""
    framed = bytes(framed)
    chunks, p, n = [], 0, len(framed)
    while p < n:
        if n - p < 3:
            return PAST_EOF
        h = int.from_bytes(framed[p:p + 3], "little")
        ln, original = h >> 1, h & 1
        if ln > n - (p + 3):
            return PAST_EOF
        chunks.append((p + 3, ln, original))
        p += 3 + ln
    table, at = [], 0
    for off, ln, original in chunks:
        ulen = ln
        if not original:
            r = preamble(framed[off:off + ln], min(block_size, MAX_BYTES - 1))
            if isinstance(r, str):
                return r
            ulen = r[0]
        table.append((off, ln, at, ulen, STORED if original else 0))
        at += ulen
    return table, at


def decode_framed(framed, block_size):
    """Every chunk of a framed run decoded: (bytes, None), or (None, (index of
    the first failing chunk, text)); a plan error has index None."""
    r = plan(framed, block_size)
    if isinstance(r, str):
        return None, (None, r)
    out = bytearray()
    for i, (off, ln, _, ulen, flags) in enumerate(r[0]):
        body = framed[off:off + ln]
        d = bytes(body) if flags & STORED else decode(body, block_size)
        if isinstance(d, str):
            return None, (i, d)
        out += d
    return bytes(out), None


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def literal(data, extra=None):
    """A literal element. extra: the number of length bytes after the tag (0 =
    inline, lengths up to 60; 1-4); None = the shortest form."""
    n = len(data)
    assert n >= 1
    if extra is None:
        extra = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
    if extra == 0:
        assert n <= 60
        return bytes([(n - 1) << 2]) + bytes(data)
    assert 1 <= extra <= 4 and n - 1 < 1 << (8 * extra)
    return bytes([(59 + extra) << 2]) + (n - 1).to_bytes(extra, "little") + bytes(data)


def copy1(ln, off):
    assert 4 <= ln <= 11 and 0 <= off < 2048
    return bytes([1 | ((ln - 4) << 2) | ((off >> 8) << 5), off & 0xFF])


def copy2(ln, off):
    assert 1 <= ln <= 64 and 0 <= off < 1 << 16
    return bytes([2 | ((ln - 1) << 2)]) + off.to_bytes(2, "little")


def copy4(ln, off):
    assert 1 <= ln <= 64 and 0 <= off < 1 << 32
    return bytes([3 | ((ln - 1) << 2)]) + off.to_bytes(4, "little")


class Stream:
    """A block under construction: `elements` and the output they decode to.
    Filler bytes come from a fixed generator, so a stream is reproducible."""

    def __init__(self, seed=1):
        self.elements = bytearray()
        self.out = bytearray()
        self._x = (seed * 2654435761 + 12345) & 0xFFFFFFFF

    def _fill(self, n):
        b = bytearray(n)
        x = self._x
        for i in range(n):
            x = (x * 1103515245 + 12345) & 0x7FFFFFFF
            b[i] = (x >> 16) & 0xFF
        self._x = x
        return bytes(b)

    @property
    def o(self):
        return len(self.out)

    def literal(self, n=None, data=None, extra=None):
        data = self._fill(n) if data is None else bytes(data)
        self.elements += literal(data, extra)
        self.out += data
        return self

    def fill_to(self, o, piece=60000):
        """Literals of filler up to output offset o."""
        assert o >= self.o
        while self.o < o:
            self.literal(min(piece, o - self.o))
        return self

    def copy(self, ln, off, kind=None):
        """A copy element (kind 1, 2 or 4; None = the smallest that fits)."""
        assert 0 < off <= self.o
        if kind is None:
            kind = 1 if 4 <= ln <= 11 and off < 2048 else (2 if off < 65536 else 4)
        self.elements += {1: copy1, 2: copy2, 4: copy4}[kind](ln, off)
        o = self.o
        for i in range(ln):
            self.out.append(self.out[o - off + i])
        return self

    def raw(self, element_bytes):
        """Element bytes appended as they are (crafted errors)."""
        self.elements += bytes(element_bytes)
        return self

    def block(self, ulen=None):
        """The raw block: preamble (the output's length, or `ulen`) + elements."""
        return varint(self.o if ulen is None else ulen) + bytes(self.elements)
