"""An exact model of the LZ4 raw block format as the reader's device path
decodes it: `size` restates lz4_block_size (orc_amd/csrc/inflate_plan.cpp) rule
by rule and in its order, `decode` follows the same walk and copies, `plan`
restates plan_lz4_framed, and `Stream` builds blocks sequence by sequence so
that a test can put one feature at a chosen output offset. Pure Python, no GPU.

The rules are the format's safety rules. liblz4 differs on crafted blocks in
two ways: 1.9.3 accepts a zero offset, and it refuses blocks that break its
compressor's end-of-block margins (`decode(..., why=True)` names the zero
offset, so that a comparison can set it aside)."""
from snappy_model import PAST_EOF, frame  # noqa: F401  (the chunk framing is the codec's neighbour, not its part)

CORRUPT = "Corrupt lz4 compressed block"
ZERO_OFFSET = "zero offset"  # a reason, not a text: every failure reads CORRUPT

STORED = 1
MAX_BYTES = 1 << 31  # a chunk's offsets are 32-bit on the device: the plan caps the block size below it


def _walk(chunk, cap, out):
    """The walk of lz4_block_size over `chunk`; with `out` (a bytearray) the
    bytes are copied as well. Returns the decompressed size, or a reason."""
    n = len(chunk)
    p = o = 0

    def extend(ln, room):
        nonlocal p
        while True:
            if p >= n:
                return None
            b = chunk[p]
            p += 1
            ln += b
            if ln > room:
                return None
            if b != 255:
                return ln

    while True:
        if p >= n:
            return "no token"
        token = chunk[p]
        p += 1
        lit = token >> 4
        if lit == 15:
            lit = extend(lit, min(n - p, cap - o))
            if lit is None:
                return "literal length"
        if lit > n - p or lit > cap - o:
            return "literal range"
        if out is not None:
            out += chunk[p:p + lit]
        p += lit
        o += lit
        if p == n:
            return o
        if n - p < 2:
            return "offset cut"
        off = chunk[p] | (chunk[p + 1] << 8)
        p += 2
        ln = token & 15
        if ln == 15:
            ln = extend(ln, cap - o)
            if ln is None:
                return "match length"
        ln += 4
        if off == 0:
            return ZERO_OFFSET
        if off > o or ln > cap - o:
            return "match range"
        if out is not None:
            if off >= ln:
                out += out[o - off:o - off + ln]
            else:
                pat = bytes(out[o - off:o])
                out += (pat * (ln // off + 1))[:ln]
        o += ln


def size(chunk, cap):
    """The decompressed size of one raw block under `cap`, or CORRUPT."""
    r = _walk(bytes(chunk), cap, None)
    return r if isinstance(r, int) else CORRUPT


def decode(chunk, cap, why=False):
    """The decompressed bytes of one raw block, or CORRUPT (why: the reason of
    the first failing rule instead)."""
    out = bytearray()
    r = _walk(bytes(chunk), cap, out)
    if isinstance(r, int):
        assert r == len(out)
        return bytes(out)
    return r if why else CORRUPT


def decode_exact(chunk, dst_bytes):
    """What the kernel makes of a table entry: the block decoded under cap =
    dst_bytes, and it must end there exactly."""
    d = decode(chunk, dst_bytes)
    return d if isinstance(d, bytes) and len(d) == dst_bytes else CORRUPT


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
            ulen = size(framed[off:off + ln], min(block_size, MAX_BYTES - 1))
            if isinstance(ulen, str):
                return ulen
        table.append((off, ln, at, ulen, STORED if original else 0))
        at += ulen
    return table, at


def decode_framed(framed, block_size):
    """Every chunk of a framed run decoded: (bytes, None), or (None, (None,
    text)): a corrupt block fails the plan, before any chunk is decoded."""
    r = plan(framed, block_size)
    if isinstance(r, str):
        return None, (None, r)
    out = bytearray()
    for off, ln, _, ulen, flags in r[0]:
        body = framed[off:off + ln]
        d = bytes(body) if flags & STORED else decode(body, block_size)
        assert len(d) == ulen
        out += d
    return bytes(out), None


def _length(v):
    """The extension bytes of a length field whose token nibble is 15."""
    v -= 15
    return b"\xff" * (v // 255) + bytes([v % 255])


def sequence(literal, match_len=None, off=0):
    """One sequence: the token, the literal, and (unless match_len is None: the
    block's last sequence) the offset and the match length."""
    lit = len(literal)
    ml = 0 if match_len is None else match_len - 4
    assert ml >= 0 and 0 <= off < 1 << 16
    out = bytearray([(min(lit, 15) << 4) | min(ml, 15)])
    if lit >= 15:
        out += _length(lit)
    out += literal
    if match_len is not None:
        out += off.to_bytes(2, "little")
        if ml >= 15:
            out += _length(ml)
    return bytes(out)


class Stream:
    """A block under construction: the sequences so far, a pending literal and
    the output they decode to. Filler bytes come from a fixed generator, so a
    stream is reproducible."""

    def __init__(self, seed=1):
        self.elements = bytearray()
        self.pending = bytearray()
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

    def literal(self, n=None, data=None):
        """Literal bytes: they join the next sequence (or the block's last)."""
        data = self._fill(n) if data is None else bytes(data)
        self.pending += data
        self.out += data
        return self

    def fill_to(self, o):
        assert o >= self.o
        return self.literal(o - self.o)

    def match(self, ln, off):
        """A match: it closes the sequence of the pending literal (0 bytes
        included)."""
        assert ln >= 4 and 0 < off <= self.o
        self.elements += sequence(self.pending, ln, off)
        self.pending = bytearray()
        o = self.o
        pat = bytes(self.out[o - off:o])
        self.out += (pat * (ln // off + 1))[:ln] if off < ln else pat[:ln]
        return self

    def raw(self, element_bytes):
        """Bytes appended as they are (crafted errors), on a sequence boundary."""
        assert not self.pending
        self.elements += bytes(element_bytes)
        return self

    def block(self, last=True):
        """The raw block: the sequences and the final literal run (the pending
        literal, 0 bytes included); last=False leaves the final run out."""
        return bytes(self.elements) + (sequence(self.pending) if last else b"")
