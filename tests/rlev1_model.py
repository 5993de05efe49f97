"""An exact model of RLEv1 decode for tests, in Python integers (no GPU, no
C): the decoder (RleDecoderV1 readHeader / readLong as the header of
orc_amd/csrc/rlev1_kernels.hip restates them), the group walker and
row-index positions, the window schedule of rlev1_kernel (V1Geo), and the
builders that put a feature of a stream at a named window byte. The CPU tests
(tests/test_rlev1_model_cpu.py) prove the model against the oracle and that
every shape holds what it means to hold; the GPU tests
(tests/test_gpu_rlev1_shapes.py) compare the kernel with the model exactly."""
import numpy as np

import rle_streams
from rlev1_writer import _padded, _varint, _zz, encode, random_groups

M64 = (1 << 64) - 1
RUN, LIT = "run", "lit"

# V1Geo<kCB> (rlev1_kernels.hip): 256 threads own kCB bytes each; a window is
# kChunk bytes plus a tail of kV1Tail; the chain hops blocks of 8 chunks
THREADS, TAIL, LANE_RUN = 256, 1536, 32
WIDTHS = (4, 16)


def geo(cb):
    """kChunk, kWin, kBlock of V1Geo<cb>."""
    chunk = THREADS * cb
    return chunk, chunk + TAIL, 8 * cb


def v1_chunk(src_len, nsegs):
    """launch_rlev1's chunk width: 4 up to 2 KB a segment on average."""
    return 4 if src_len // nsegs <= 2048 else 16


def signed64(u):
    u &= M64
    return u - (1 << 64) if u >> 63 else u


def unzigzag(u):
    return ((u >> 1) ^ (M64 if u & 1 else 0)) & M64


def truncate(values, nbytes):
    """The low nbytes bytes of each value as a signed integer (the int32 /
    int16 outputs: (T)(int64_t)v)."""
    bits = 8 * nbytes
    out = []
    for v in values:
        u = int(v) & ((1 << bits) - 1)
        out.append(u - (1 << bits) if u >> (bits - 1) else u)
    return np.array(out, dtype={8: np.int64, 4: np.int32, 2: np.int16}[nbytes])


def padded_varint(u, nbytes):
    """A base-128 varint of exactly nbytes bytes with the payload in the first
    bytes (rlev1_writer._padded): legal for readLong (RLEv1.cc:154-170).
    Payload bits that nbytes bytes cannot hold are left out."""
    out = bytearray()
    _padded(u, nbytes, out)
    return bytes(out)


def _read_varint(b, p):
    """(value mod 2^64, end) of the varint at p; end None: the stream ends first."""
    u, sh = 0, 0
    while p < len(b):
        y = b[p]
        p += 1
        if sh < 64:
            u |= (y & 0x7F) << sh
        sh += 7
        if y < 0x80:
            return u & M64, p
    return None, None


def groups(data, signed):
    """Every group of the stream: (offset, kind, values, bytes, whole). The
    last one may be cut by the stream's end (whole False): a cut run has no
    values, a cut literal its whole varints; bytes is then what is left."""
    b = bytes(data)
    out, p = [], 0
    fix = (lambda u: signed64(unzigzag(u))) if signed else signed64
    while p < len(b):
        h = b[p] - 256 if b[p] >= 0x80 else b[p]
        if h >= 0:
            u, e = _read_varint(b, p + 2) if p + 2 <= len(b) else (None, None)
            if e is None:
                out.append((p, RUN, [], len(b) - p, False))
                break
            delta = b[p + 1] - 256 if b[p + 1] >= 0x80 else b[p + 1]
            base = fix(u)
            out.append((p, RUN, [signed64(base + i * delta) for i in range(h + 3)], e - p, True))
            p = e
        else:
            vals, q = [], p + 1
            while len(vals) < -h:
                u, e = _read_varint(b, q)
                if e is None:
                    break
                vals.append(fix(u))
                q = e
            whole = len(vals) == -h
            out.append((p, LIT, vals, (q if whole else len(b)) - p, whole))
            if not whole:
                break
            p = q
    return out


def decode(data, signed, n=None):
    """(the first n values, or all, as int64; the count of values producible
    before the stream ends = the index of the first value that is not)."""
    vals = [v for g in groups(data, signed) for v in g[2]]
    return np.array(vals if n is None else vals[:n], dtype=np.int64), len(vals)


def walk(data):
    """The stream's whole groups: (offset, kind, values, bytes) each."""
    return [(g[0], g[1], len(g[2]), g[3]) for g in groups(data, False) if g[4]]


def positions(walked, n, stride):
    """Row-index positions every `stride` values (rle_streams.positions)."""
    return rle_streams.positions([(g[0], g[1], 0, g[2]) for g in walked], n, stride)


class Window:
    """One pass of rlev1_kernel's window loop: the stream offset of window
    byte 0 (negative in a first window: the source pointer's low bits), p0,
    the offsets of the groups it decodes, and how it ends: "next" (the next
    group opens the next window), "restart" (a group not whole in the window
    opens the next), "serial" (its first group is not whole in it: wave 0
    decodes that group through the descriptor), "cut" (the stream ends inside
    a group), "end" (the segment is done)."""

    def __init__(self, wpos, p0):
        self.wpos, self.p0, self.groups, self.how = wpos, p0, [], None

    def byte(self, off):
        """The window byte of stream offset off."""
        return off - self.wpos


def windows(data, seg_start, seg_end, addr_mod16, cb):
    """The windows a workgroup walks over segment [seg_start, seg_end) of a
    stream whose byte 0 lies at an address = addr_mod16 mod 16 (V1Geo<cb>)."""
    chunk, win, _ = geo(cb)
    gs = {g[0]: g for g in groups(data, False)}
    seg_end = min(seg_end, len(data))
    out, pos = [], seg_start
    while pos < seg_end:
        wpos = pos - ((addr_mod16 + pos) % 16)
        w = Window(wpos, pos - wpos)
        out.append(w)
        lim = min(seg_end - wpos, chunk)
        valid = min(len(data) - wpos, win)
        p = pos
        while True:
            if p - wpos >= lim:
                w.how = "next" if p < seg_end else "end"
                pos = p
                break
            g = gs[p]
            if not g[4] and len(data) - wpos <= win:  # the window holds the stream's end
                w.groups.append(p)
                w.how = "cut"
                return out
            if not g[4] or g[0] + g[3] - wpos > valid:
                if p == pos:
                    w.how = "serial"
                    if not g[4]:
                        return out
                    pos = g[0] + g[3]
                else:
                    w.how = "restart"
                    pos = p
                break
            w.groups.append(p)
            p += g[3]
    return out


def window_of(wins, off):
    """(window index, window byte) of the group at stream offset off."""
    for k, w in enumerate(wins):
        if off in w.groups or (w.how == "serial" and off == w.wpos + w.p0):
            return k, w.byte(off)
    raise KeyError(off)


# ---- builders ---------------------------------------------------------------
def run_bytes(length, delta, base_varint):
    """A run with its base given as varint bytes (padded_varint, or varint())."""
    assert 3 <= length <= 130 and -128 <= delta <= 127
    return bytes([length - 3, delta & 0xFF]) + bytes(base_varint)


def lit_bytes(varints):
    """A literal group of the given varints' bytes."""
    assert 1 <= len(varints) <= 128
    return bytes([256 - len(varints)]) + b"".join(bytes(v) for v in varints)


def varint(u):
    out = bytearray()
    _varint(u, out)
    return bytes(out)


def zigzag(v):
    return _zz(v)


def wide_varints(rng, k):
    """k random varints of 10 bytes (bit 63 set: their canonical length)."""
    return [varint(int(rng.integers(0, 1 << 63)) | (1 << 63)) for _ in range(k)]


def filler(rng, nbytes):
    """Whole groups of exactly nbytes bytes (0, or >= 2): literal groups of
    1-byte varints and 3-byte runs, nonzero values."""
    assert nbytes == 0 or nbytes >= 2
    out = bytearray()
    while len(out) < nbytes:
        left = nbytes - len(out)
        if left == 3 or (left >= 5 and rng.random() < 0.3):
            out += bytes([int(rng.integers(0, 30)), int(rng.integers(1, 256)), int(rng.integers(1, 128))])
            continue
        k = left - 1 if left <= 40 else int(rng.integers(1, 38))
        if left - (1 + k) == 1:
            k -= 1
        out += bytes([256 - k]) + bytes(int(x) for x in rng.integers(1, 128, size=k))
    assert len(out) == nbytes
    return bytes(out)


def place(rng, feature, at, head=b""):
    """head + filler + feature with the feature's first byte at stream offset
    `at`; the offset is returned with the bytes."""
    gap = at - len(head)
    return head + filler(rng, gap) + feature, at


def tail_groups(rng, n=6):
    """A few ordinary groups to follow a feature (a wrong group end shows)."""
    gs = []
    for i in range(n):
        if i % 2:
            gs.append(("run", int(rng.integers(-(1 << 40), 1 << 40)), int(rng.integers(-128, 128)), int(rng.integers(3, 131))))
        else:
            gs.append(("lit", [int(x) for x in rng.integers(-(1 << 62), 1 << 62, size=int(rng.integers(1, 60)))]))
    return encode(gs, True)[0]


def force_width(rng, data, segs, cb):
    """Append groups so that launch_rlev1 picks chunk width cb for the table
    `segs` ([(offset, value index)]) over the longer stream: 2-byte groups of
    a segment each for cb = 4, one long segment for cb = 16. Returns the
    stream and the table (offsets and value indices of the added segments
    from the model)."""
    data, segs = bytes(data), list(segs)
    n = decode(data, False)[1]
    assert not segs or segs[0] == (0, 0)
    segs = segs or [(0, 0)]
    if cb == 4:
        while v1_chunk(len(data), len(segs)) != 4:
            segs.append((len(data), n))
            data += bytes([0xFF, int(rng.integers(1, 128))])
            n += 1
    else:
        need = 2049 * (len(segs) + 1) - len(data)
        if v1_chunk(len(data), len(segs)) != 16:
            segs.append((len(data), n))
            data += filler(rng, max(need, 2))
    assert v1_chunk(len(data), len(segs)) == cb
    return data, segs


# ---- shapes -----------------------------------------------------------------
class Shape:
    """A stream built for one launch: its bytes, signedness, segment table,
    the chunk width and source-pointer offset it is built for, and the
    offsets (marks) of the features it places."""

    def __init__(self, data, segs, cb, off, signed=True, **marks):
        self.data, self.segs, self.cb, self.off, self.signed, self.marks = data, segs, cb, off, signed, marks

    def windows(self, seg=0):
        end = self.segs[seg + 1][0] if seg + 1 < len(self.segs) else len(self.data)
        return windows(self.data, self.segs[seg][0], end, self.off, self.cb)


EDGE_KINDS = ("run", "run10", "lit128")
EDGE_D = tuple(range(18)) + (None,)  # header at window byte kChunk - 1 - d; None: at kChunk


def edge_feature(rng, kind):
    if kind == "run":  # 4 bytes: from kChunk - 1 its delta and base lie in the tail
        return run_bytes(int(rng.integers(33, 131)), int(rng.integers(-128, 128)), varint(int(rng.integers(128, 1 << 14))))
    if kind == "run10":
        return run_bytes(int(rng.integers(3, 131)), int(rng.integers(-128, 128)), wide_varints(rng, 1)[0])
    return lit_bytes(wide_varints(rng, 128))  # 1281 bytes: from kChunk - 1 it reaches kChunk + 1280


def window_edge(kind, d, off, cb):
    """The feature with its header at window byte kChunk - 1 - d (d None: at
    kChunk, where it opens the next window) of the first window, and again of
    a later window; marks a, b: the two headers' stream offsets."""
    rng = np.random.default_rng([EDGE_KINDS.index(kind), 99 if d is None else d, off, cb])
    chunk = geo(cb)[0]
    wb = chunk if d is None else chunk - 1 - d
    data, a = place(rng, edge_feature(rng, kind), wb - off)
    if len(data) < chunk - off:  # whole groups up to kChunk: the next window starts there
        gap = chunk - off - len(data)
        data += filler(rng, gap + (gap == 1))
    start = a if d is None else len(data)
    while True:
        wpos = start - (off + start) % 16
        if wpos + wb - len(data) >= 2:  # room for whole groups up to the header
            break
        start = len(data)  # the group at `start` runs past this window's kChunk: the next one opens at its end
    data, b = place(rng, edge_feature(rng, kind), wpos + wb, head=data)
    data += tail_groups(rng)
    data, segs = force_width(rng, data, [], cb)
    return Shape(data, segs, cb, off, a=a, b=b, wb=wb)


def literal_phases(j, off, cb):
    """A 128-literal of 10-byte varints with its header at window byte
    kChunk - 51 - j: over j = 0..9 its varints cross kChunk, (kCB = 4) the
    tail passes' boundary kChunk + 1024 and the chunk and block edges between
    at every phase. mark a: the header."""
    rng = np.random.default_rng([7, j, off, cb])
    chunk = geo(cb)[0]
    data, a = place(rng, lit_bytes(wide_varints(rng, 128)), chunk - 51 - j - off)
    data += tail_groups(rng)
    data, segs = force_width(rng, data, [], cb)
    return Shape(data, segs, cb, off, a=a)


def crossing_phases(shape, edge_every, first_edge=0):
    """The set of (bytes of a varint before an edge) over the varints of the
    literal at mark a that cross an edge (window bytes first_edge + k *
    edge_every), nbytes = 10."""
    w = shape.windows()[0]
    s0 = w.byte(shape.marks["a"]) + 1
    out = set()
    for i in range(128):
        s = s0 + 10 * i
        for e in range(first_edge, s + 10, edge_every):
            if s < e < s + 10:
                out.add(e - s)
    return out


PADDED = (11, 16, 17, 18, 40)


def padded_literals(nbytes, off, cb):
    """16 literal groups of 20 padded varints of nbytes bytes, the headers'
    window bytes stepping through every residue mod cb; marks heads."""
    rng = np.random.default_rng([11, nbytes, off, cb])
    data, heads = filler(rng, 5), []
    for j in range(16):
        want = (j - off) % cb  # the header's stream offset mod cb
        gap = (want - len(data)) % cb
        data += filler(rng, gap + cb if gap == 1 else gap)
        assert len(data) % cb == want
        heads.append(len(data))
        data += lit_bytes([padded_varint(int(rng.integers(1 << 62, 1 << 63)) * 2 + 1, nbytes) for _ in range(20)])
        data += bytes([3, 0xFE]) + varint(int(rng.integers(1, 1 << 30)))
    data, segs = force_width(rng, data, [], cb)
    return Shape(data, segs, cb, off, signed=False, heads=heads)


def literal_ends(off, cb):
    """Literals whose last varint ends on a chunk's last byte (marks last) and
    on a chunk's first byte (marks first), in the first window."""
    rng = np.random.default_rng([13, off, cb])
    data, last, first = b"", [], []
    for c, where in ((9, last), (14, first), (40, last), (47, first), (200, first), (230, last)):
        end = c * cb - 1 - off + (where is first)  # stream offset of the terminator
        k = 3 if cb == 4 else 7
        g = lit_bytes([padded_varint(int(rng.integers(1 << 13, 1 << 14)), 2) for _ in range(k)])
        data, a = place(rng, g, end - len(g) + 1, head=data)
        where.append(a)
    data += tail_groups(rng)
    data, segs = force_width(rng, data, [], cb)
    return Shape(data, segs, cb, off, last=last, first=first)


DENSE = ("lit2", "run3", "run130")


def dense(kind, off, cb, nwin=3):
    """nwin windows of only 2-byte literal groups (kMaxGroups a window), only
    3-byte runs of 3 values (kMaxRuns), or only 3-byte runs of 130 values
    (s_rlong full)."""
    rng = np.random.default_rng([17, DENSE.index(kind), off, cb])
    chunk = geo(cb)[0]
    n = nwin * chunk // (2 if kind == "lit2" else 3)
    b = rng.integers(1, 128, size=n).astype(np.uint8)
    if kind == "lit2":
        data = np.stack([np.full(n, 0xFF, np.uint8), b], axis=1).tobytes()
    else:
        dl = rng.integers(0, 256, size=n).astype(np.uint8)
        data = np.stack([np.full(n, 0 if kind == "run3" else 127, np.uint8), dl, b], axis=1).tobytes()
    data, segs = force_width(rng, data, [], cb)
    return Shape(data, segs, cb, off)


RUN_LENGTHS = (3, 31, 32, 33, 64, 65, 66, 129, 130)
RUN_DELTAS = (-128, -1, 0, 1, 127)


def run_matrix(signed, cb):
    """Every length x delta with bases at the extremes (wrap-around mod 2^64),
    as canonical and as padded varints."""
    rng = np.random.default_rng([19, int(signed), cb])
    if signed:
        bases = [0, -1, (1 << 63) - 1, -(1 << 63), (1 << 63) - 130, -(1 << 63) + 130, int(rng.integers(-(1 << 62), 1 << 62))]
    else:
        bases = [0, 1, M64, M64 - 130, 1 << 63, (1 << 63) - 1, int(rng.integers(0, 1 << 63))]
    data, k = b"", 0
    for L in RUN_LENGTHS:
        for dl in RUN_DELTAS:
            for base in bases:
                u = zigzag(base) if signed else base
                nb = len(varint(u))
                vb = varint(u) if k % 3 else padded_varint(u, nb + 1 + k % 7)
                data += run_bytes(L, dl, vb)
                k += 1
    data, segs = force_width(rng, data, [], cb)
    return Shape(data, segs, cb, 0, signed=signed)


def runs_of_10(cb):
    """500 consecutive runs of 10 values: the lane-per-run rounds."""
    rng = np.random.default_rng([23, cb])
    gs = [("run", int(rng.integers(-(1 << 50), 1 << 50)), int(rng.integers(-128, 128)), 10) for _ in range(500)]
    data, segs = force_width(rng, encode(gs, True)[0], [], cb)
    return Shape(data, segs, cb, 0)


LONG_KINDS = ("lit45", "runwin")
LONG_WHERE = ("first", "after", "cut")


def long_group(kind, where, cb):
    """A group longer than a window: a 128-literal of 45-byte varints, or a
    run whose base is a padded varint of kWin + 100 bytes. first: it opens the
    segment (the serial path at once) and ordinary groups follow; after: it
    follows ordinary groups (the window restarts at it); cut: the stream ends
    inside it. mark a: its header; the stream is `cut` bytes long."""
    rng = np.random.default_rng([29, LONG_KINDS.index(kind), LONG_WHERE.index(where), cb])
    win = geo(cb)[1]
    if kind == "lit45":
        g = lit_bytes([padded_varint(int(rng.integers(1 << 62, 1 << 63)) * 2 + 1, 45) for _ in range(128)])
    else:
        g = run_bytes(100, -7, padded_varint(int(rng.integers(1 << 62, 1 << 63)) * 2 + 1, win + 100))
    assert len(g) > win
    head = b"" if where == "first" else filler(rng, 300) + run_bytes(50, 9, wide_varints(rng, 1)[0])
    data = head + g
    if where == "cut":
        data = data[:len(head) + win + 50]
        # (kCB = 4: a segment per group keeps the average under 2 KB)
        segs = [(0, 0)] if cb == 16 else group_table(head) + [(len(head), decode(head, False)[1])]
        assert v1_chunk(len(data), len(segs)) == cb
    else:
        data += tail_groups(rng)
        data, segs = force_width(rng, data, [], cb)
    return Shape(data, segs, cb, 0, signed=False, a=len(head))


def _firsts(walked):
    """The first value index of each group, and of the stream's end."""
    return np.concatenate([[0], np.cumsum([g[2] for g in walked])]).astype(np.int64).tolist()


def group_table(data):
    """One segment per whole group: [(offset, first value index)]."""
    w = walk(data)
    return [(g[0], v) for g, v in zip(w, _firsts(w))]


def trunc_small():
    """About 300 bytes of runs and literals of 1- to 10-byte varints, to be
    cut at every byte."""
    rng = np.random.default_rng(31)
    gs = []
    for i, bits in enumerate((6, 63, 13, 40, 20, 62, 27, 7, 55, 34, 48, 63, 10, 63, 30)):
        lim = 1 << bits
        if i % 3 == 1:
            gs.append(("run", int(rng.integers(-lim, lim)), int(rng.integers(-128, 128)), int(rng.integers(3, 131))))
        else:
            gs.append(("lit", [int(x) for x in rng.integers(-lim, lim, size=int(rng.integers(2, 9)))]))
    data = encode(gs, True)[0]
    assert 250 <= len(data) <= 350, len(data)
    return Shape(data, [(0, 0)], 4, 0)


def trunc_long(cb):
    """A segment of more than three windows, to be cut around kChunk and kWin
    of each (marks cuts). kCB = 4: eight 2-byte segments come first, so the
    average stays under 2 KB when the stream is cut."""
    rng = np.random.default_rng([37, cb])
    chunk, win, _ = geo(cb)
    front = 8 if cb == 4 else 0
    data = b"".join(bytes([0xFF, int(x)]) for x in rng.integers(1, 128, size=front))
    while len(data) <= 2 * front + 3 * chunk + win + 64:
        data += encode(random_groups(rng, 500, True, 40), True)[0]
    segs = [(2 * i, i) for i in range(front + 1)]
    s = Shape(data, segs, cb, 0)
    cuts = set()
    for w in s.windows(front)[:3]:
        for e in (chunk, win):
            cuts.update(w.wpos + e + k for k in (-2, -1, 0, 1, 2))
    s.marks["cuts"] = sorted(c for c in cuts if 2 * front + 2048 * (cb == 16) < c < len(data))
    return s


def range_stream(cb):
    """A literal, a lane run, a wave run, a full literal, runs of 32 and 33
    and a short literal, of full-width values; marks ranges: (begin, count)
    starting and ending inside each, at the segment's first and last value,
    and of one value."""
    rng = np.random.default_rng([41, cb])
    big = lambda k: [int(x) for x in rng.integers(-(1 << 63), (1 << 63) - 1, size=k, dtype=np.int64)]
    gs = [("lit", big(50)), ("run", big(1)[0], -77, 20), ("run", big(1)[0], 101, 100), ("lit", big(128)),
          ("run", big(1)[0], 3, 32), ("run", big(1)[0], -3, 33), ("lit", big(5))]
    data = encode(gs, True)[0]
    f = _firsts(walk(data))
    n = f[-1]
    data, segs = force_width(rng, data, [], cb)
    total = decode(data, True)[1]
    ranges = [(0, n), (0, 1), (n - 1, 1), (0, total), (total - 1, 1), (n - 1, 2)]
    for a, b in zip(f[:-1], f[1:]):
        ranges += [(a + 1, b - a - 2), (a + (b - a) // 2, b - a), (a - 1 if a else 0, 3), (b - 1, 1)]
    return Shape(data, segs, cb, 0, ranges=[(a, c) for a, c in ranges if c > 0 and a + c <= total], first=f)


def grouped(cb, empty=False):
    """(stream, one segment per group) at chunk width cb: 350 groups for 4,
    16 groups and a long segment for 16. empty: every third entry twice and
    every fifth three times, which gives empty segments whose offset and
    value index equal their neighbour's."""
    rng = np.random.default_rng([47, cb])
    data = encode(random_groups(rng, 100_000, True, 50)[:350 if cb == 4 else 16], True)[0]
    table = group_table(data)
    if empty:
        table = [e for k, e in enumerate(table) for _ in range(1 + (k % 3 == 0) + (k % 5 == 0))]
    return force_width(rng, data, table, cb)
