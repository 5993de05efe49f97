"""An exact model of byte / boolean RLE decode for tests, in Python (no GPU,
no C): the decoder (ByteRleDecoderImpl readHeader / nextInternal as the
header of orc_amd/csrc/byterle_kernels.hip restates them, a cut literal read
lazily), the group walker and row-index positions, the window schedule of
byterle_kernel, and the builders that put a feature of a stream at a named
window byte or decoded offset. The CPU tests (tests/test_byterle_model_cpu.py)
prove the model against the oracle and that every shape holds what it means to
hold; the GPU tests (tests/test_gpu_byterle_shapes.py) compare the kernel with
the model exactly."""
import numpy as np

RUN, LIT = "run", "lit"
# byterle_kernel: a window owns the groups starting in its first CHUNK bytes;
# 256 threads own THREAD bytes each, the chain hops BLOCK bytes; the owner map
# covers ROUND decoded bytes a round; the group table has SLOTS entries
CHUNK, THREAD, BLOCK, ROUND, SLOTS = 4096, 16, 128, 16384, 2048
OFFS = (0, 1, 15)


def header(h):
    """(kind, decoded bytes, stream bytes) of the group a control byte opens
    (ByteRleDecoderImpl::readHeader, ByteRLE.cc:378-388)."""
    return (RUN, h + 3, 2) if h < 0x80 else (LIT, 256 - h, 257 - h)


def headers(data):
    """Every group the control bytes name: (stream offset, kind, decoded
    bytes, stream bytes); the stream may end inside the last one."""
    b, out, p = bytes(data), [], 0
    while p < len(b):
        out.append((p,) + header(b[p]))
        p += out[-1][3]
    return out


def walk(data):
    """The stream's whole groups: (stream offset, kind, decoded bytes, stream bytes)."""
    return [g for g in headers(data) if g[0] + g[3] <= len(data)]


def decode_bytes(data):
    """The decoded bytes the reference can produce: a run needs its value
    byte (readHeader reads it), a literal hands out the bytes that are there
    (nextInternal reads them one buffer at a time) and fails on the first that
    is not."""
    b, out = bytes(data), bytearray()
    for off, kind, dec, size in headers(b):
        if kind == RUN:
            if off + 2 > len(b):
                break
            out += b[off + 1:off + 2] * dec
        else:
            out += b[off + 1:off + size]
    return bytes(out)


def decode(data, boolean=False):
    """(the decoded bytes, or rows: their bits, most significant first; the
    count of them = the index of the first the reference cannot produce). A
    row r needs decoded byte r // 8 whole (BooleanRleDecoderImpl::next reads
    (rows + 7) / 8 bytes)."""
    by = np.frombuffer(decode_bytes(data), dtype=np.uint8)
    out = np.unpackbits(by) if boolean else by.copy()
    return out, int(out.size)


def firsts(walked):
    """The first decoded index of each group, and of the stream's end."""
    return np.concatenate([[0], np.cumsum([g[2] for g in walked])]).astype(np.int64).tolist()


def group_table(data):
    """One segment per whole group: [(offset, first decoded index)]."""
    w = walk(data)
    return [(g[0], v) for g, v in zip(w, firsts(w))]


def positions(groups, rows, stride, boolean=False):
    """Row-index positions of the row groups of `rows` rows (decoded bytes in
    byte mode), `stride` rows each: (group start, decoded bytes to skip in it)
    and, for a boolean stream, the bits consumed of the next byte
    (ByteRleDecoderImpl::seek, BooleanRleDecoderImpl::seek)."""
    first = np.array(firsts(groups), dtype=np.int64)
    offs = [g[0] for g in groups]
    out = []
    for r in range(0, rows, stride):
        byte = r // 8 if boolean else r
        k = int(np.searchsorted(first, byte, side="right")) - 1
        assert 0 <= k < len(groups), (r, byte)
        out.append((offs[k], byte - int(first[k])) + ((r % 8,) if boolean else ()))
    return out


class Window:
    """One pass of byterle_kernel's window loop over a segment: seg (its
    index), wpos (the stream offset of window byte 0; negative where the
    source pointer's low bits put the descriptor's start before the stream),
    p0 (the window byte of the first group), lim, the groups it owns (stream
    offsets), vi (the decoded index of its first byte), dec (the decoded bytes
    of its groups), rounds (owner-map rounds) and nxt (the stream offset the
    next window starts at)."""

    def __init__(self, seg, wpos, p0, lim, vi):
        self.seg, self.wpos, self.p0, self.lim, self.vi = seg, wpos, p0, lim, vi
        self.groups, self.dec, self.rounds, self.nxt = [], 0, 0, None

    def byte(self, off):
        return off - self.wpos


def windows(data, segs, off=0, begin=0, count=None, boolean=False):
    """The windows the workgroups walk for the range [begin, begin + count)
    (decoded bytes, or rows) of a stream whose byte 0 lies at an address = off
    mod 16; count None: all the stream holds. A segment whose values lie
    wholly outside the range returns before its first window."""
    b = bytes(data)
    scale = 8 if boolean else 1
    if count is None:
        count = sum(h[2] for h in headers(b)) * scale - begin
    end = begin + count
    vend = (end + scale - 1) // scale
    out = []
    for g, (seg_start, vi) in enumerate(segs):
        last = g + 1 == len(segs)
        seg_end = len(b) if last else min(segs[g + 1][0], len(b))
        if vi * scale >= end or (not last and segs[g + 1][1] * scale <= begin):
            continue
        bias = seg_start - (off + seg_start) % 16  # descriptor byte 0
        pos = seg_start
        while pos < seg_end and vi < vend:
            wpos = bias + (pos - bias) // 16 * 16
            w = Window(g, wpos, pos - wpos, min(seg_end - wpos, CHUNK), vi)
            out.append(w)
            p, stop = pos, False
            while p - wpos < w.lim:
                _, dec, size = header(b[p])
                if vi + w.dec < vend and (p + size > len(b) or p + size > seg_end):
                    stop = True  # reported: the workgroup ends after this window
                w.groups.append(p)
                w.dec += dec
                p += size
            assert len(w.groups) <= SLOTS
            w.rounds = (w.dec + ROUND - 1) // ROUND
            w.nxt = p
            if stop:
                break
            pos = p
            vi += w.dec
    return out


def window_of(wins, off):
    """(segment, index of the window among the segment's, window byte) of the
    group at stream offset off."""
    for w in wins:
        if off in w.groups:
            return w.seg, [x for x in wins if x.seg == w.seg].index(w), w.byte(off)
    raise KeyError(off)


# ---- builders ---------------------------------------------------------------
def run(n, value):
    assert 3 <= n <= 130
    return bytes([n - 3, value])


def lit(payload):
    assert 1 <= len(payload) <= 128
    return bytes([256 - len(payload)]) + bytes(payload)


def rand_bytes(rng, k):
    """k non-zero bytes (zeros are what a read past the stream gives)."""
    return rng.integers(1, 256, size=k, dtype=np.uint8).tobytes()


def rand_lit(rng, k):
    return lit(rand_bytes(rng, k))


def rand_run(rng, n=None):
    return run(int(rng.integers(3, 131)) if n is None else n, int(rng.integers(1, 256)))


def filler(rng, nbytes):
    """Whole groups of exactly nbytes stream bytes (0, or >= 2): runs and
    literals of up to 40 bytes."""
    assert nbytes == 0 or nbytes >= 2, nbytes
    out = bytearray()
    while len(out) < nbytes:
        left = nbytes - len(out)
        if left == 2 or (left >= 4 and rng.random() < 0.3):
            out += rand_run(rng) if rng.random() < 0.7 or left > 2 else rand_lit(rng, 1)
            continue
        k = min(left - 1, int(rng.integers(1, 41)))
        if left - (1 + k) == 1:
            k += -1 if k > 1 else 1
        out += rand_lit(rng, k)
    assert len(out) == nbytes
    return bytes(out)


def place(rng, feature, at, head=b""):
    """head + filler + feature, the feature's first byte at stream offset at."""
    return head + filler(rng, at - len(head)) + feature, at


def tail_groups(rng, n=6):
    """A few ordinary groups to follow a feature (a wrong group end shows)."""
    return b"".join(rand_run(rng) if i % 2 else rand_lit(rng, int(rng.integers(1, 60))) for i in range(n))


class Shape:
    """A stream built for one launch: its bytes, segment table, the source
    pointer's low four bits it is built for, and the marks of what it places."""

    def __init__(self, data, segs, off=0, **marks):
        self.data, self.segs, self.off, self.marks = bytes(data), list(segs), off, marks

    def windows(self, **kw):
        return windows(self.data, self.segs, self.off, **kw)


def seg_at(data):
    """A segment entry for a group that starts at the stream's present end."""
    return len(data), decode(data)[1]


EDGE_KINDS = ("run", "lit128", "lit1")
EDGE_D = tuple(range(18)) + (None,)  # header at window byte CHUNK - 1 - d; None: at CHUNK


def edge_feature(rng, kind):
    if kind == "run":  # from CHUNK - 1 its value byte lies in the tail
        return rand_run(rng)
    return rand_lit(rng, 128 if kind == "lit128" else 1)  # 129 stream bytes: from CHUNK - 1 up to CHUNK + 128


def window_edge(kind, d, off):
    """The feature with its header at window byte CHUNK - 1 - d (d None: at
    CHUNK, where it opens the next window) of segment 0's first window (p0 =
    off), and again of segment 1's first window, whose p0 is whatever the
    groups before it leave; marks a, b: the headers' stream offsets, wb."""
    rng = np.random.default_rng([EDGE_KINDS.index(kind), 99 if d is None else d, off])
    wb = CHUNK if d is None else CHUNK - 1 - d
    data, a = place(rng, edge_feature(rng, kind), wb - off)
    data += tail_groups(rng) + filler(rng, int(rng.integers(2, 40)))
    s = seg_at(data)
    wpos = s[0] - (off + s[0]) % 16
    data, b = place(rng, edge_feature(rng, kind), wpos + wb, head=data)
    data += tail_groups(rng)
    return Shape(data, [(0, 0), s], off, a=a, b=b, wb=wb)


BANDS = 16  # stream lengths 2 .. 129 in bands of 8


def length_phases(band, off):
    """Groups of the stream lengths 2 + 8 * band .. 9 + 8 * band (a run and a
    1-byte literal for 2, literals otherwise), each starting at every window
    byte mod 16: the chunk exits, the block hops and the literal extraction at
    every alignment. marks heads: (stream offset, stream bytes)."""
    rng = np.random.default_rng([3, band, off])
    data, heads = filler(rng, 4), []
    for size in range(2 + 8 * band, 10 + 8 * band):
        for ph in range(16):
            gap = (ph - off - len(data)) % 16
            data += filler(rng, gap + 16 if gap == 1 else gap)
            heads.append((len(data), size))
            data += rand_run(rng) if size == 2 and ph % 2 else rand_lit(rng, size - 1)
    data += tail_groups(rng)
    return Shape(data, [(0, 0)], off, heads=heads)


def block_hops(off):
    """129-byte literals from the last byte of every other 128-byte block with
    a 127-byte literal between them: every other block holds no group start
    (it lies inside a literal). marks heads: the 129-byte literals."""
    rng = np.random.default_rng([5, off])
    data, heads = filler(rng, BLOCK - 1 - off), []
    for _ in range(12):
        heads.append(len(data))
        data += rand_lit(rng, 128) + rand_lit(rng, 126)
    data += tail_groups(rng)
    return Shape(data, [(0, 0)], off, heads=heads)


DENSE = ("lit1", "run3", "run130")


def dense(kind, off, nwin=2):
    """nwin windows of SLOTS two-byte groups each: 1-byte literals, runs of 3
    or runs of 130 (266,240 decoded bytes a window: 17 owner-map rounds)."""
    rng = np.random.default_rng([7, DENSE.index(kind), off])
    n = nwin * SLOTS
    v = rng.integers(1, 256, size=n).astype(np.uint8)
    h = {"lit1": 0xFF, "run3": 0, "run130": 127}[kind]
    data = np.stack([np.full(n, h, np.uint8), v], axis=1).tobytes()
    return Shape(data, [(0, 0)], off)


def small_groups(off):
    """Groups of 1, 2 and 3 decoded bytes (literals, and runs of 3) among
    groups of 4 to 9, at every decoded offset mod 4, and a run of 5, a literal
    of 2 and a run at decoded bytes 0 .. 7 (dword 1 = run, literal, literal,
    run). marks mixed: the decoded offset of that dword."""
    rng = np.random.default_rng([11, off])
    data = run(5, 0x11) + lit(b"\x22\x33") + run(9, 0x44)
    for _ in range(400):
        k = int(rng.integers(0, 6))
        if k < 3:
            data += rand_lit(rng, k + 1)
        elif k == 3:
            data += rand_run(rng, 3)
        else:
            data += rand_run(rng, int(rng.integers(4, 10))) if k == 4 else rand_lit(rng, int(rng.integers(4, 10)))
    return Shape(data, [(0, 0)], off, mixed=4)


ROUND_KINDS = ("run", "lit")
ROUND_BEFORE = (0, 1, 2, 3)


def round_edges(off):
    """One segment per (kind, k, round): runs of 130 and a shorter run up to
    decoded offset round * ROUND - k of the segment's only window, then a run
    of 100 or a literal of 100 that starts exactly on the owner map's round
    edge (k = 0) or straddles it by k bytes, then ordinary groups. marks
    feats: (segment, stream offset, decoded offset in the window)."""
    rng = np.random.default_rng([13, off])
    data, segs, feats = b"", [], []
    for rnd in (1, 2):
        for kind in ROUND_KINDS:
            for k in ROUND_BEFORE:
                segs.append(seg_at(data))
                need = rnd * ROUND - k
                full, rest = divmod(need, 130)
                if rest < 3:  # no run is that short: take it from two runs
                    full, rest = full - 1, rest + 130
                for _ in range(full):
                    data += rand_run(rng, 130)
                data += rand_run(rng, rest - 65) + rand_run(rng, 65) if rest > 130 else rand_run(rng, rest)
                feats.append((len(segs) - 1, len(data), need))
                data += rand_run(rng, 100) if kind == "run" else rand_lit(rng, 100)
                data += tail_groups(rng)
    return Shape(data, segs, off, feats=feats)


def crossing(ph, off, nwin=3):
    """nwin windows in one segment; the group that crosses each window's byte
    CHUNK ends at CHUNK + ph (ph = 0: on it), so the next window's p0 = ph."""
    rng = np.random.default_rng([17, ph, off])
    data, wpos = b"", -off
    for _ in range(nwin - 1):
        size = int(rng.integers(max(ph + 1, 3), 130))  # the crossing literal's stream bytes
        start = wpos + CHUNK + ph - size
        data, _ = place(rng, rand_lit(rng, size - 1), start, head=data)
        wpos = wpos + CHUNK  # the next window: byte 0 at the 16 bytes holding stream offset len(data)
        assert (len(data) - wpos) == ph
    data += filler(rng, 700)
    return Shape(data, [(0, 0)], off)


def ranged():
    """About 2.5 KB in five segments of runs and literals, for output ranges.
    marks first: the first decoded index of every group."""
    rng = np.random.default_rng(19)
    data, segs = b"", []
    for _ in range(5):
        segs.append(seg_at(data))
        data += rand_lit(rng, 7) + rand_run(rng, 130) + rand_lit(rng, 128) + rand_run(rng, 3) + rand_lit(rng, 1)
        data += filler(rng, int(rng.integers(200, 400)))
    return Shape(data, segs, 0, first=firsts(walk(data)))


def byte_ranges(s):
    """(value_begin, count): begins at every residue mod 4, counts that end
    inside a dword, ranges inside one group, whole segments skipped at either
    end."""
    n = decode(s.data)[1]
    v = [x[1] for x in s.segs]
    out = [(0, n), (n - 1, 1), (0, 1)]
    for r in range(4):
        out += [(r, 64 + c) for c in range(4)] + [(v[2] + r, 9), (v[1] - 5 + r, 11)]
    out += [(v[2], n - v[2]), (v[3] + 3, n - v[3] - 3), (0, v[2]), (1, v[1] - 3), (v[1] + 1, v[3] - v[1]), (v[4] + 5, 1)]
    return [(a, c) for a, c in out if c > 0 and a + c <= n]


def bool_ranges(s):
    """(row_begin, nrows): begins and counts at every residue mod 8, ranges
    inside one decoded byte, whole segments skipped at either end."""
    n = 8 * decode(s.data)[1]
    v = [8 * x[1] for x in s.segs]
    out = [(0, n), (n - 1, 1), (0, 1)]
    for r in range(8):
        out += [(r, 200 + r), (8 + r, 203 - 2 * r), (v[2] + r, 61)]
    out += [(17, 5), (18, 1), (16, 8), (23, 2), (v[1] + 3, 4)]
    out += [(v[2], n - v[2]), (v[3] + 3, n - v[3] - 3), (0, v[2]), (1, v[1] - 3), (v[1] + 1, v[3] - v[1]), (v[4] + 5, 1)]
    return [(a, c) for a, c in out if c > 0 and a + c <= n]


def grouped(repeat=False):
    """(stream, one segment per group): 300 random groups. repeat: every
    third entry twice and every fifth three times (several row groups that
    start in one run: empty segments)."""
    rng = np.random.default_rng(23)
    data = b"".join(rand_run(rng) if rng.random() < 0.5 else rand_lit(rng, int(rng.integers(1, 129))) for _ in range(300))
    table = group_table(data)
    if repeat:
        table = [e for k, e in enumerate(table) for _ in range(1 + (k % 3 == 0) + (k % 5 == 0))]
    return data, table


def trunc_small():
    """About 300 bytes of runs and literals, to be cut at every byte."""
    rng = np.random.default_rng(29)
    data = b"".join(rand_run(rng) if i % 3 == 1 else rand_lit(rng, int(rng.integers(1, 40))) for i in range(18))
    data += rand_lit(rng, 1) + rand_run(rng, 3)
    assert 250 <= len(data) <= 400, len(data)
    return Shape(data, [(0, 0)])


def trunc_window():
    """A segment of two windows whose groups around window byte CHUNK are a
    run ending on CHUNK - 20, literals of 5, 128 (crossing CHUNK) and 1 bytes
    and runs, to be cut at CHUNK - 20 .. CHUNK + 140 (marks cuts)."""
    rng = np.random.default_rng(31)
    data = filler(rng, CHUNK - 22) + rand_run(rng) + rand_lit(rng, 5) + rand_run(rng) + rand_lit(rng, 1)
    data += rand_lit(rng, 128) + rand_run(rng) + rand_lit(rng, 1) + rand_lit(rng, 30) + filler(rng, 300)
    return Shape(data, [(0, 0)], cuts=list(range(CHUNK - 20, CHUNK + 141)))
