"""An exact model of RLEv2 decode for tests (no GPU, no C): a writer of run
bytes with every header field free (it writes bytes, it does not encode
values, so it can say everything the format can), the decoder (RleDecoderV2
readByte order, nextShortRepeats / nextDirect / nextPatched with
adjustGapAndPatch / nextDelta, as orc_amd/csrc/rlev2_device.hh parse_run cites
them), the kernels' geometry restated as data, the window schedule of the
serial walk (rlev2_tiled_walk.hh walk()), and the builders that put a run at a
named window byte. tests/test_rlev2_model_cpu.py proves the model against the
oracle and that every shape holds what it claims; tests/
test_gpu_rlev2_shapes.py compares every kernel instance with the model exactly.

Values are Python integers mod 2^64 wherever the arithmetic is the point
(bases, patches, delta sums); numpy only unpacks byte-multiple fields."""
import numpy as np

from rle_streams import DELTA, DIRECT, FBS, PATCHED, SR
from rlev1_model import M64, signed64, truncate, unzigzag  # noqa: F401 (truncate: the int32 / int16 outputs)
from rlev1_writer import _padded, _varint, _zz

READ_ERROR = "bad read in RleDecoderV2::readByte"
PL0_ERROR = "Corrupt PATCHED_BASE encoded data (pl==0)!"
WIDTH_ERROR = "Corrupt PATCHED_BASE encoded data (patchBitSize + pgw > 64)!"
DELTA_ERROR = "Illegal run length for delta encoding: 1"
SEGMENT_ERROR = "Stream position is not at a run boundary"

# ---- the kernels' geometry (tests/test_rlev2_model_cpu.py reads the sources
# and fails when one of these differs) ----------------------------------------
# The one rule of the model that is not the reference's: a DELTA header (two
# bytes and two varints) longer than HDR_LIM bytes is a bad read at the run's
# first value (include/orcg.h; the reference reads varints of any length)
HDR_LIM = 64
CONSTANTS = {
    "rlev2_tiled_common.hh": dict(kThreads=256, kMaxRun=4608, kSlab=2048, kStage=256, kShortL=16, kVparL=256,
                                  ORCG_VPAR_MIN=16, kToDense=24, kToSerial=64, ORCG_TAB_TO_DENSE=128,
                                  ORCG_TAB_TO_SERIAL=512),
    "rlev2_tiled_walk.hh": dict(ORCG_ITEM_MAX=64),
    "rlev2_expand.hip": dict(kRound=256),
    "rlev2_route.hh": dict(kSliceMax=1024, kMaxRlev2Variant=10),
    "host_plan.hh": dict(kRlev2HdrLim=HDR_LIM),
}
_T = dict(CONSTANTS["rlev2_tiled_common.hh"], **CONSTANTS["rlev2_tiled_walk.hh"])
MAX_RUN, SLAB, SHORT_L, ITEM_MAX = _T["kMaxRun"], _T["kSlab"], _T["kShortL"], _T["ORCG_ITEM_MAX"]
BLK = SLAB // _T["kThreads"]  # kBlk: bytes a thread owns in dense discovery
SUPER = 8 * BLK               # kSup
DENSE_RUNS = SLAB // 2        # kDenseRuns
SERIAL_RUNS = 512             # kCap of the serial instances
SLICE_MAX, ROUND = CONSTANTS["rlev2_route.hh"]["kSliceMax"], CONSTANTS["rlev2_expand.hip"]["kRound"]
LONGEST_RUN = 4356            # PATCHED W=64 L=512 bw=8, 31 entries of 64 bits
_WINS = _T["kThreads"] // 64 * _T["kStage"] * 8 + SLAB // 8  # what a union instance's serial window adds

# variant -> (kWin, what walks it, kWinS: the serial window of a union instance)
# rlev2_tiled.cpp kInstances' rows: kWin = KB * 1024, + 512 in dense-capable instances
VARIANTS = {
    0: (None, "default", None),  # picks 2, 3, 6 or 8 by the stream's bytes per value
    1: (None, "wave-walk", None),
    2: (33 << 10, "serial", None),
    3: (21 << 10, "serial", None),  # + the dense drain for short-run segments
    4: ((8 << 10) + 512, "dense", None),
    5: ((12 << 10) + 512, "dense", None),
    6: ((8 << 10) + 512, "two-pass", (8 << 10) + 512 + _WINS),
    7: (33 << 10, "serial", None),
    8: ((8 << 10) + 512, "union", (8 << 10) + 512 + _WINS),
    9: (33 << 10, "serial", None),
    10: (33 << 10, "serial", None),
}
# the distinct (first window, later windows) sizes a placement is built for
WINDOWS = sorted({(w, ws or w) for w, _, ws in VARIANTS.values() if w})


def closest_fixed_bits(n):
    for w in FBS:
        if n <= w:
            return w
    return 64


# ---- writer ---------------------------------------------------------------------
def pack(fields, W, pad_bits=0):
    """W-bit fields MSB first; the last byte's unused low bits take pad_bits."""
    acc = 0
    for f in fields:
        acc = (acc << W) | (int(f) & ((1 << W) - 1))
    bits = W * len(fields)
    nbytes = (bits + 7) // 8
    spare = 8 * nbytes - bits
    acc = (acc << spare) | (pad_bits & ((1 << spare) - 1))
    return acc.to_bytes(nbytes, "big")


def varint(u, nbytes=None):
    """u as a base-128 varint: minimal, or padded to exactly nbytes bytes."""
    out = bytearray()
    if nbytes is None:
        _varint(u, out)
    else:
        _padded(u, nbytes, out)
    return bytes(out)


def zigzag(v):
    return _zz(v)


def sr(nb, L, raw):
    """SHORT_REPEAT: raw in nb bytes (leading zero bytes if it needs fewer)."""
    assert 1 <= nb <= 8 and 3 <= L <= 10
    return bytes([(nb - 1) << 3 | (L - 3)]) + (raw & ((1 << 8 * nb) - 1)).to_bytes(nb, "big")


def _head(kind, code, L):
    assert 0 <= code < 32 and 1 <= L <= 512
    return bytes([kind << 6 | code << 1 | (L - 1) >> 8, (L - 1) & 0xFF])


def direct(code, L, fields, pad_bits=0):
    assert len(fields) == L
    return _head(DIRECT, code, L) + pack(fields, FBS[code], pad_bits)


def entry(gap, patch, pw):
    """A patch-list entry: the gap above the pw patch bits."""
    return gap << pw | patch


def patched(code, L, bw, base_raw, pw_code, pgw, entries, lits, pad_bits=0, pl=None):
    """base_raw: the bw sign-magnitude base bytes as an integer; entries: raw
    integers of closest_fixed_bits(pw + pgw) bits (entry()); pl: the header's
    count when it is not len(entries)."""
    assert 1 <= bw <= 8 and 1 <= pgw <= 8 and len(lits) == L
    pl = len(entries) if pl is None else pl
    assert 0 <= pl < 32
    cfb = closest_fixed_bits(FBS[pw_code] + pgw)
    return (_head(PATCHED, code, L) + bytes([(bw - 1) << 5 | pw_code, (pgw - 1) << 5 | pl])
            + (base_raw & ((1 << 8 * bw) - 1)).to_bytes(bw, "big") + pack(lits, FBS[code], pad_bits)
            + pack(entries, cfb, pad_bits))


def delta(code, L, base_u, delta_u, n1=None, n2=None, fields=(), pad_bits=0):
    """base_u / delta_u: the varints' payloads (zigzag() them for signed
    values); n1 / n2: their padded byte lengths (None: minimal); fields: the
    L - 2 deltas of width FBS[code] (code 0: none, a fixed delta)."""
    assert len(fields) == (max(L - 2, 0) if code else 0)
    return _head(DELTA, code, L) + varint(base_u, n1) + varint(delta_u, n2) + (pack(fields, FBS[code], pad_bits) if code else b"")


# ---- decoder --------------------------------------------------------------------
class Run:
    """A run of the stream: its offset, kind, width (0: a fixed delta), value
    count, size in bytes and values (int64), or the ParseError reading it
    throws (values None; size and W / L as far as they were read)."""

    def __init__(self, off, kind):
        self.off, self.kind, self.W, self.L, self.size, self.values, self.err = off, kind, 0, 0, None, None, None
        self.hdr = 0  # header bytes before the packed data (0: the header is cut)

    def __repr__(self):
        return "Run(%d, kind %d, W %d, L %d, %s bytes%s)" % (self.off, self.kind, self.W, self.L, self.size,
                                                             ", " + self.err if self.err else "")


def _unpack(b, p, W, count):
    """count W-bit fields from byte p as unsigned integers (a uint64 array)."""
    if count == 0:
        return np.zeros(0, dtype=np.uint64)
    nbytes = (W * count + 7) // 8
    if W % 8 == 0:
        a = np.frombuffer(b, dtype=np.uint8, count=nbytes, offset=p).reshape(count, W // 8).astype(np.uint64)
        out = np.zeros(count, dtype=np.uint64)
        for k in range(W // 8):
            out = (out << np.uint64(8)) | a[:, k]
        return out
    acc = int.from_bytes(b[p:p + nbytes], "big") >> (8 * nbytes - W * count)
    mask = (1 << W) - 1
    return np.array([(acc >> (W * (count - 1 - i))) & mask for i in range(count)], dtype=np.uint64)


def _unzigzag_array(u):
    return (u >> np.uint64(1)) ^ (np.uint64(0) - (u & np.uint64(1)))


def _read_varint(b, p, stop):
    """(payload mod 2^64, end) of the varint at p, reading no byte at or past
    `stop`; end None: the read fails. Bits at shift >= 64 are dropped."""
    u, sh = 0, 0
    while p < stop:
        y = b[p]
        p += 1
        if sh < 64:
            u = (u | (y & 0x7F) << sh) & M64
        sh += 7
        if y < 0x80:
            return u, p
    return None, None


def parse(b, p, signed, hdr_lim=HDR_LIM):
    """The run at p, its bytes read in the reference's order: the first thing
    that fails (a missing byte or one of the three ParseErrors) is the error."""
    n = len(b)
    fb = b[p]
    r = Run(p, fb >> 6)
    code = (fb >> 1) & 0x1F
    if r.kind == SR:  # nextShortRepeats (:184-203)
        nb = ((fb >> 3) & 7) + 1
        r.W, r.L, r.hdr = 8 * nb, (fb & 7) + 3, 1
        if p + 1 + nb > n:
            r.err = READ_ERROR
            return r
        v = int.from_bytes(b[p + 1:p + 1 + nb], "big")
        r.values = np.full(r.L, signed64(unzigzag(v) if signed else v), dtype=np.int64)
        r.size = 1 + nb
        return r
    if p + 2 > n:
        r.err = READ_ERROR
        return r
    r.L = ((fb & 1) << 8 | b[p + 1]) + 1
    if r.kind == DIRECT:  # nextDirect (:224-248)
        r.W, r.hdr = FBS[code], 2
        size = 2 + (r.W * r.L + 7) // 8
        if p + size > n:
            r.err = READ_ERROR
            return r
        u = _unpack(b, p + 2, r.W, r.L)
        r.values = (_unzigzag_array(u) if signed else u).view(np.int64)
        r.size = size
        return r
    if r.kind == PATCHED:  # nextPatched (:273-370)
        r.W = FBS[code]
        if p + 4 > n:
            r.err = READ_ERROR
            return r
        third, fourth = b[p + 2], b[p + 3]
        bw, pw = (third >> 5) + 1, FBS[third & 0x1F]
        pgw, pl = (fourth >> 5) + 1, fourth & 0x1F
        if pl == 0:  # (:307)
            r.err = PL0_ERROR
            return r
        if p + 4 + bw > n:
            r.err = READ_ERROR
            return r
        r.hdr = 4 + bw
        base = int.from_bytes(b[p + 4:p + 4 + bw], "big")
        sign = 1 << (8 * bw - 1)
        if base & sign:  # sign-magnitude (:311-317): 0x80 is zero, and so is every "negative zero"
            base = -(base & ~sign) & M64
        data = p + 4 + bw
        lit_bytes = (r.W * r.L + 7) // 8
        if data + lit_bytes > n:
            r.err = READ_ERROR
            return r
        if pw + pgw > 64:  # after the literals are read (:328-330)
            r.err = WIDTH_ERROR
            return r
        cfb = closest_fixed_bits(pw + pgw)
        size = 4 + bw + lit_bytes + (cfb * pl + 7) // 8
        if p + size > n:
            r.err = READ_ERROR
            return r
        lits = [int(x) for x in _unpack(b, data, r.W, r.L)]
        ents = [int(x) for x in _unpack(b, data + lit_bytes, cfb, pl)]
        pmask = (1 << pw) - 1

        # adjustGapAndPatch (:250-271): entries of gap 255 and patch 0 add 255
        # to the next entry's gap; the walk stays inside the list
        def adjust(idx):
            actual = 0
            g, q = ents[idx] >> pw, ents[idx] & pmask
            while g == 255 and q == 0 and idx + 1 < pl:
                actual += 255
                idx += 1
                g, q = ents[idx] >> pw, ents[idx] & pmask
            return idx, actual + g, q

        idx, gap, patch = adjust(0)
        out = []
        for i in range(r.L):
            if i != gap:
                out.append((lits[i] + base) & M64)
            else:  # the patch goes above the W literal bits; W = 64 shifts by 0 (mod 64)
                out.append((base + (lits[i] | (patch << (r.W & 63) & M64))) & M64)
                idx += 1
                if idx < pl:
                    idx, g, patch = adjust(idx)
                    gap = g + i  # a gap of 0 names this value again: no later value is patched
        r.values = np.array([signed64(v) for v in out], dtype=np.int64)
        r.size = size
        return r
    # nextDelta (:372-435)
    r.W = FBS[code] if code else 0
    stop = min(n, p + hdr_lim) if hdr_lim else n
    u1, q = _read_varint(b, p + 2, stop)
    u2, q = _read_varint(b, q, stop) if q is not None else (None, None)
    if q is None:
        r.err = READ_ERROR
        return r
    r.hdr = q - p
    base = unzigzag(u1) if signed else u1
    db = unzigzag(u2)
    if r.W == 0:
        r.values = (np.uint64(base) + np.arange(r.L, dtype=np.uint64) * np.uint64(db)).view(np.int64)  # mod 2^64
        r.size = q - p
        return r
    if r.L < 2:  # (:412-415), before the deltas are read
        r.err = DELTA_ERROR
        return r
    size = q - p + (r.W * (r.L - 2) + 7) // 8
    if p + size > n:
        r.err = READ_ERROR
        return r
    out, prev = [base, (base + db) & M64], (base + db) & M64
    down = db >> 63  # the delta base's sign gives the direction; a base of 0 counts up
    for d in _unpack(b, q, r.W, r.L - 2):
        prev = (prev - int(d) if down else prev + int(d)) & M64
        out.append(prev)
    r.values = np.array([signed64(v) for v in out], dtype=np.int64)
    r.size = size
    return r


def runs(data, signed=False, hdr_lim=HDR_LIM):
    """Every run of the stream; the last one carries the error that ends it,
    if one does."""
    b, out, p = bytes(data), [], 0
    while p < len(b):
        r = parse(b, p, signed, hdr_lim)
        out.append(r)
        if r.err:
            break
        p += r.size
    return out


def decode(data, signed, dst_bytes=8, hdr_lim=HDR_LIM):
    """(values, n, error text, error value index): the n values the reference
    hands out before it throws, as the output type holds them; the error of
    asking for one more (a bad read where the stream just ends), and the index
    of the value it is thrown at (= n: a bad run hands out none of its values)."""
    rs = runs(data, signed, hdr_lim)
    good = [r.values for r in rs if not r.err]
    vals = np.concatenate(good) if good else np.zeros(0, dtype=np.int64)
    err = rs[-1].err if rs and rs[-1].err else READ_ERROR
    if dst_bytes != 8:
        vals = vals.astype({4: np.int32, 2: np.int16}[dst_bytes])  # (T)(int64_t)v: the low bytes
    return vals, vals.size, err, vals.size


def run_table(data):
    """One segment per whole run: [(offset, first value index)]."""
    out, vi = [], 0
    for r in runs(data):
        if r.err:
            break
        out.append((r.off, vi))
        vi += r.L
    return out


def table_error(data, segs):
    """None, or the value index at which a decode of every value reports
    SEGMENT_ERROR: a segment's runs must end at the next segment's first byte
    with its first value index."""
    size = {r.off: (r.size, r.L) for r in runs(data) if not r.err}
    bad = []
    for (off, vi), (noff, nvi) in zip(segs, list(segs[1:]) + [(len(data), None)]):
        p = off
        while p < noff:
            if p not in size or p + size[p][0] > noff:
                bad.append(vi)
                break
            vi += size[p][1]
            p += size[p][0]
        else:
            if nvi is not None and vi != nvi:
                bad.append(vi)
    return min(bad) if bad else None


def positions(data, n, stride):
    """Row-index positions every `stride` values: (offset of the run that
    holds the value, values to skip in it)."""
    rs = [r for r in runs(data) if not r.err]
    starts = np.concatenate([[0], np.cumsum([r.L for r in rs])[:-1]]).astype(np.int64)
    g = np.arange(0, n, stride)
    ri = np.searchsorted(starts, g, side="right") - 1
    return np.stack([np.array([r.off for r in rs], dtype=np.int64)[ri], g - starts[ri]], axis=1).astype(np.uint64)


# ---- the serial walk's windows -----------------------------------------------------
class Window:
    """One window of a serial walk: wpos, the stream offset of window byte 0
    (the first unprocessed run's address aligned down 16), the bytes loaded
    (need), and the offsets of the runs it takes."""

    def __init__(self, wpos, need):
        self.wpos, self.need, self.runs = wpos, need, []

    def byte(self, off):
        return off - self.wpos


def serial_windows(data, seg_start, seg_end, addr_mod16, win, win_later=None, cap=SERIAL_RUNS):
    """The windows rlev2_tiled_kernel's serial walk takes over segment
    [seg_start, seg_end) of whole runs, the stream's byte 0 at an address =
    addr_mod16 mod 16. A window loads min(win, the segment's bytes rounded up
    16) bytes; passes of up to `cap` runs take every run that starts in its
    first kChunk = win - kMaxRun bytes, and a run that starts past kChunk only
    if it follows another in its pass and all of its bytes are loaded; the
    first run not taken opens the next window. win_later: the size of the
    windows after the first (a union instance's serial windows)."""
    size = {seg_start + r.off: r.size for r in runs(data[seg_start:seg_end]) if not r.err}
    out, pos = [], seg_start
    end_abs = (addr_mod16 + seg_end + 15) & ~15
    while pos < seg_end:
        kwin = win if not out or win_later is None else win_later
        chunk = kwin - MAX_RUN
        wpos = pos - (addr_mod16 + pos) % 16
        w = Window(wpos, min(kwin, end_abs - addr_mod16 - wpos))
        out.append(w)
        while True:  # passes
            n = 0
            while pos < seg_end and n < cap:
                lp = pos - wpos
                if lp >= chunk and n > 0 and lp + size[pos] > w.need:
                    break
                w.runs.append(pos)
                pos += size[pos]
                n += 1
            if not (pos < wpos + chunk and pos < seg_end):
                break
    return out


def window_of(wins, off):
    """(window index, window byte) of the run at stream offset off."""
    for k, w in enumerate(wins):
        if off in w.runs:
            return k, w.byte(off)
    raise KeyError(off)


# ---- builders ------------------------------------------------------------------------
BIG = 2 + 8 * 512  # a DIRECT W=64 L=512 run


def filler(rng, nbytes):
    """Whole DIRECT runs of exactly nbytes bytes (0, or >= 3): W=64 L=512 runs
    of 4,098 bytes, then W=8 runs of 2 + L bytes for the rest."""
    assert nbytes == 0 or nbytes >= 3
    out, left = [], nbytes
    while left >= BIG + 3 or left == BIG:
        out.append(bytes([0x40 | 31 << 1 | 1, 0xFF]) + rng.bytes(8 * 512))
        left -= BIG
    while left:
        take = min(left, 514)
        if left - take in (1, 2):
            take -= 3
        out.append(_head(DIRECT, 7, take - 2) + rng.bytes(take - 2))
        left -= take
    return b"".join(out)


class Shape:
    """A stream built for one launch: bytes, signedness, the source pointer's
    low four bits it is built for, its segment table, and what it claims
    (marks)."""

    def __init__(self, name, data, signed=True, off=0, segs=None, **marks):
        self.name, self.data, self.signed, self.off = name, bytes(data), signed, off
        self.segs = list(segs) if segs else [(0, 0)]
        self.marks = marks


def concat(name, cases, signed, off=0):
    """The cases' bytes as the segments of one stream; marks names, starts."""
    data, segs, vi = bytearray(), [], 0
    for _, b in cases:
        segs.append((len(data), vi))
        data += b
        vi += sum(r.L for r in runs(b))
    return Shape(name, data, signed, off, segs, names=[c[0] for c in cases], starts=[s[0] for s in segs])


def _wrap(rng, run):
    """A SHORT_REPEAT, the run under test, a SHORT_REPEAT."""
    return sr(1, 3, int(rng.integers(1, 256))) + run + sr(2, 5, int(rng.integers(256, 1 << 16)))


def _payload(rng, how, W, k):
    if how == "ones":
        return [(1 << W) - 1] * k
    if how == "alt":
        return [int("10" * 32, 2) >> (64 - W) if i % 2 else int("01" * 32, 2) >> (64 - W) for i in range(k)]
    return [int(rng.integers(0, 1 << 63)) * 2 + 1 & ((1 << W) - 1) for _ in range(k)]


DIRECT_L = (1, 2, 63, 64, 65, 511, 512)
PATCHED_L = (1, 2, 16, 17, 64, 65, 511, 512)
DELTA_L = (2, 3, 66, 512)
SCAN_W = (24, 26, 28, 32, 64)  # around the W <= 26 switch to 32-bit scans


def sr_cases(rng, signed):
    out = []
    for nb in range(1, 9):
        for L in range(3, 11):
            out.append(("sr nb=%d L=%d" % (nb, L), sr(nb, L, int(rng.integers(1 << (8 * nb - 2), 1 << (8 * nb - 1))) | 1 << (8 * nb - 1))))
    for nb in range(2, 9):  # leading zero bytes
        out.append(("sr padded nb=%d" % nb, sr(nb, 4, int(rng.integers(1, 256)))))
    for raw in (M64, M64 - 1, 0, 1, 1 << 63):  # the extremes of either signedness
        out.append(("sr raw=%x" % raw, sr(8, 10, raw)))
    return out


def direct_cases(rng, signed):
    out = []
    for code in range(32):
        for L in DIRECT_L:
            for how in ("ones", "alt", "random"):
                out.append(("direct W=%d L=%d %s" % (FBS[code], L, how), direct(code, L, _payload(rng, how, FBS[code], L), pad_bits=0xFF)))
    return out


def _escaped(positions, patches, pw):
    """Entries that patch the given (growing) positions: gaps over 255 take
    escape entries (gap 255, patch 0)."""
    ents, at = [], 0
    for pos, patch in zip(positions, patches):
        g = pos - at
        while g > 255:
            ents.append(entry(255, 0, pw))
            g -= 255
        ents.append(entry(g, patch, pw))
        at = pos
    return ents


def patched_cases(rng, signed):
    out = []
    lit = lambda W, L: _payload(rng, "random", W, L)
    # the three walks of a corrupt list that the reference decodes (W=8, L=6,
    # base 5, literals 1..6, pw=8): a later gap of 0, a position >= L, a
    # trailing escape entry; each patches value 2 and stalls
    for name, pgw, ents in (("later gap 0", 3, [(2, 1), (0, 2), (1, 3)]), ("position >= L", 3, [(2, 1), (7, 2), (1, 3)]),
                            ("trailing escape", 8, [(2, 1), (255, 0)])):
        out.append(("patched " + name, patched(7, 6, 1, 5, 7, pgw, [entry(g, q, 8) for g, q in ents], [1, 2, 3, 4, 5, 6])))
    out.append(("patched base 0x80", patched(7, 6, 1, 0x80, 7, 3, [entry(2, 1, 8)], [1, 2, 3, 4, 5, 6])))
    out.append(("patched base 0x85", patched(7, 6, 1, 0x85, 7, 3, [entry(2, 1, 8)], [1, 2, 3, 4, 5, 6])))
    for code in range(32):  # every W, 64 included (the patch shifts by W mod 64)
        W = FBS[code]
        out.append(("patched W=%d" % W, patched(code, 17, 2, 0x1234, 7, 4, [entry(2, 0xA5, 8), entry(9, 0xFF, 8)], lit(W, 17), pad_bits=0xFF)))
    for pc in range(32):  # every (pw, pgw) the reference accepts
        for pgw in range(1, 9):
            pw = FBS[pc]
            if pw + pgw > 64:
                continue
            g = min(5, (1 << pgw) - 1)
            ents = [entry(g, (1 << pw) - 1, pw), entry(1, int(rng.integers(1, 1 << min(pw, 62))), pw)]
            out.append(("patched pw=%d pgw=%d" % (pw, pgw), patched(7, 20, 1, 3, pc, pgw, ents, lit(8, 20), pad_bits=0xFF)))
    for bw in range(1, 9):  # bases: positive, negative, negative zero, the largest magnitude, wrapping past 2^63
        top = 1 << (8 * bw - 1)
        for name, raw in (("pos", top >> 1 | 1), ("neg", top | top >> 1 | 1), ("negzero", top), ("max", top - 1), ("-max", 2 * top - 1)):
            out.append(("patched bw=%d %s" % (bw, name), patched(15, 5, bw, raw, 7, 3, [entry(1, 0xFF, 8)], [0xFFFF] * 5)))
    for L in PATCHED_L:  # patches at values 0, 63, 64, L - 1 and past L
        pos = sorted({p for p in (0, 63, 64, L - 1) if p < L})
        ents = _escaped(pos + [L + 3], [int(rng.integers(1, 256)) for _ in range(len(pos) + 1)], 8)
        out.append(("patched L=%d" % L, patched(11, L, 3, 0x800001, 7, 8, ents, lit(12, L), pad_bits=0xFF)))
    out.append(("patched pl=1", patched(7, 512, 1, 1, 7, 8, [entry(200, 7, 8)], lit(8, 512))))
    out.append(("patched pl=31", patched(7, 512, 1, 1, 7, 8, [entry(int(g), int(q), 8) for g, q in zip(rng.integers(1, 17, 31), rng.integers(1, 256, 31))], lit(8, 512))))
    out.append(("patched pl=31 of 64 bits", patched(31, 512, 8, M64 >> 1, 30, 8, [entry(int(g), int(q), 56) for g, q in zip(rng.integers(1, 17, 31), rng.integers(1, 1 << 56, 31))], lit(64, 512))))
    out.append(("patched L < pl", patched(7, 2, 1, 1, 7, 3, [entry(1, 9, 8)] + [entry(1, k, 8) for k in range(1, 5)], lit(8, 2))))
    esc = entry(255, 0, 8)
    out.append(("patched escape first", patched(7, 300, 1, 1, 7, 8, [esc, entry(3, 9, 8), entry(4, 8, 8)], lit(8, 300))))
    out.append(("patched escape middle", patched(7, 300, 1, 1, 7, 8, [entry(3, 9, 8), esc, entry(4, 8, 8), entry(1, 7, 8)], lit(8, 300))))
    out.append(("patched escape doubled", patched(7, 512, 1, 1, 7, 8, [esc, esc, entry(1, 9, 8)], lit(8, 512))))
    out.append(("patched escape last in L", patched(7, 512, 1, 1, 7, 8, [entry(3, 9, 8), esc], lit(8, 512))))
    out.append(("patched gap 255 patched", patched(7, 512, 1, 1, 7, 8, [entry(255, 5, 8), entry(255, 6, 8), entry(1, 7, 8)], lit(8, 512))))
    return out


def delta_cases(rng, signed):
    out = []
    zz = zigzag if signed else (lambda v: v & M64)
    big = (1 << 63) - 1
    for L in (1, 2, 3, 512):  # fixed deltas
        for name, d in (("+7", 7), ("-7", -7), ("0", 0), ("+max", big), ("-max", -big)):
            base = int(rng.integers(-(1 << 40), 1 << 40)) if signed else int(rng.integers(0, 1 << 63)) * 2 + 1
            out.append(("delta fixed L=%d d=%s" % (L, name), delta(0, L, zz(base), zigzag(d))))
    for code in range(1, 32):
        W = FBS[code]
        for L in DELTA_L:
            d = int(rng.integers(1, 1 << 20)) * (-1 if (code + L) % 2 else 1)
            out.append(("delta W=%d L=%d" % (W, L), delta(code, L, zz(int(rng.integers(0, 1 << 50))), zigzag(d), fields=_payload(rng, "random", W, L - 2), pad_bits=0xFF)))
    for W in SCAN_W:  # all-ones deltas: the sums that a 32-bit scan cannot hold
        for L in (66, 512):
            for d in (1, -1):
                out.append(("delta ones W=%d L=%d %+d" % (W, L, d), delta(FBS.index(W), L, zz(12345), zigzag(d), fields=[(1 << W) - 1] * (L - 2))))
    out.append(("delta base 0 with a width", delta(7, 66, zz(1000), 0, fields=_payload(rng, "random", 8, 64))))
    out.append(("delta W=4 L=2", delta(3, 2, zz(77), zigzag(-5))))
    for n1 in range(1, 11):  # the varints at every padded length, independently
        for n2 in range(1, 11):
            out.append(("delta varints %d %d" % (n1, n2), delta(3 if (n1 + n2) % 2 else 0, 5, int(rng.integers(1, 128)), int(rng.integers(1, 128)), n1, n2,
                                                              fields=[1, 2, 3] if (n1 + n2) % 2 else ())))
    full = M64 if signed else int(rng.integers(1 << 62, 1 << 63)) | 1 << 63  # signed: zigzag of the minimum
    out.append(("delta full base", delta(0, 3, full, zigzag(-1))))
    out.append(("delta full base and delta", delta(15, 4, full, M64, fields=[0xFFFF, 1])))
    for n1, n2 in ((11, 1), (1, 11), (11, 11), (12, 1), (1, 12), (12, 12), (31, 31), (10, 52), (52, 10)):
        out.append(("delta varints %d %d" % (n1, n2), delta(7, 6, full, zigzag(3), n1, n2, fields=[1, 2, 3, 4])))
    return out


FAMILIES = {"sr": sr_cases, "direct": direct_cases, "patched": patched_cases, "delta": delta_cases}


def grammar(family, signed, off=0):
    """Every case of one run kind, each between two SHORT_REPEATs, as the
    segments of one stream."""
    rng = np.random.default_rng([1, sorted(FAMILIES).index(family), int(signed)])
    return concat("%s %s" % (family, "signed" if signed else "unsigned"),
                  [(n, _wrap(rng, b)) for n, b in FAMILIES[family](rng, signed)], signed, off)


def error_cases():
    """(name, bytes, signed): single-segment streams that end in a ParseError,
    each after two good runs; with the cuts that come earlier or later in the
    read order than the corrupt field (the precedence)."""
    rng = np.random.default_rng(3)
    head = sr(1, 3, 9) + direct(7, 4, [1, 2, 3, 4])
    pl0 = patched(7, 6, 2, 5, 7, 3, [], [1, 2, 3, 4, 5, 6])  # pl = 0
    pw64 = patched(7, 6, 2, 5, 31, 1, [1, 2], [1, 2, 3, 4, 5, 6])
    d1 = delta(7, 1, 8, 2)  # L = 1 with a width
    out = [("pl == 0", head + pl0 + sr(1, 3, 1)), ("pl == 0, cut in the base", head + pl0[:5]),
           ("pl == 0, cut before byte 4", head + pl0[:3]), ("pw = 64", head + pw64 + sr(1, 3, 1)),
           ("pw = 64, cut in the literals", head + pw64[:9]), ("pw = 64, cut in the base", head + pw64[:5]),
           ("pw = 64, cut in the list", head + pw64[:len(pw64) - 3]), ("pw = 64 and pl == 0", head + patched(7, 6, 2, 5, 31, 1, [], [1] * 6)),
           ("delta L = 1", head + d1 + sr(1, 3, 1)), ("delta L = 1, cut in the second varint", head + delta(7, 1, 8, 300)[:3]),
           ("delta L = 1, fixed", head + delta(0, 1, 8, 2))]
    for n1, n2 in ((31, 31), (32, 32), (62, 1), (63, 1), (1, 63), (40, 30), (34, 34)):  # a header of 64 bytes is the longest
        out.append(("delta header of %d bytes" % (2 + n1 + n2), head + delta(0, 5, 6, 4, n1, n2) + sr(1, 3, 1)))
    return [(n, b, True) for n, b in out]


def cut_stream():
    """About 150 bytes with one run of each kind, a padded DELTA and a PATCHED
    run with escapes among them, to be cut at every byte."""
    rng = np.random.default_rng(5)
    esc = entry(255, 0, 4)
    data = (sr(3, 7, 0x123456) + direct(10, 9, _payload(rng, "random", 11, 9)) + delta(0, 20, zigzag(-99), zigzag(3), 4, 7)
            + patched(7, 20, 2, 0x8123, 7, 8, [entry(3, 9, 8), entry(4, 1, 8)], _payload(rng, "random", 8, 20))
            + delta(12, 11, zigzag(1 << 40), zigzag(-2), fields=_payload(rng, "random", 13, 9)) + sr(1, 3, 7)
            + patched(3, 300 - 256 + 1, 1, 7, 3, 8, [esc, entry(3, 9, 4)], _payload(rng, "random", 4, 45), pl=2)
            + direct(31, 2, [M64, 1]) + delta(31, 3, M64, 1, 10, 1, fields=[M64]))
    return Shape("cuts", data, True)


def trunc_long(win, win_later):
    """One segment of more than three windows (runs of every size up to 4 KB),
    to be cut around kChunk and the end of each of its first three windows
    (marks cuts)."""
    rng = np.random.default_rng([37, win, win_later])
    data = bytearray(sr(1, 3, 1))
    while len(data) < win + 2 * win_later + 6000:
        data += filler(rng, int(rng.integers(3, 1500))) + short_run(rng, int(rng.integers(0, 6)))
        if rng.random() < 0.2:
            data += filler(rng, BIG)
    s = Shape("cut long %d/%d" % (win, win_later), data, False)
    cuts = set()
    for k, w in enumerate(serial_windows(s.data, 0, len(s.data), 0, win, win_later)[:3]):
        kwin = win_later if k else win
        for e in (kwin - MAX_RUN, kwin):
            cuts.update(w.wpos + e + d for d in (-2, -1, 0, 1, 2))
    s.marks["cuts"] = sorted(c for c in cuts if 0 < c < len(s.data))
    return s


PLACED = ("delta22", "longest", "direct64", "sr", "straddle")


def placed_run(rng, kind):
    """The runs of the placement sweeps: a DELTA run with a 22-byte header,
    the longest legal run, DIRECT W=64 L=512, a SHORT_REPEAT, and a DELTA
    whose 22-byte header is nearly all of it (it straddles an edge at most
    offsets) with a good run after it."""
    if kind == "delta22":
        return delta(27, 512, M64, M64 - 2, 10, 10, fields=_payload(rng, "random", 32, 510))
    if kind == "longest":
        ents = [entry(int(g), int(q), 56) for g, q in zip(rng.integers(1, 17, 31), rng.integers(1, 1 << 56, 31))]
        b = patched(31, 512, 8, int(rng.integers(1, 1 << 63)), 30, 8, ents, _payload(rng, "random", 64, 512))
        assert len(b) == LONGEST_RUN
        return b
    if kind == "direct64":
        return direct(31, 512, _payload(rng, "random", 64, 512))
    if kind == "sr":
        return sr(1, 9, int(rng.integers(1, 256)))
    return delta(7, 3, M64, M64 - 2, 10, 10, fields=[200])


def sweep(win):
    """The window bytes the run under test starts at, for a window of `win`
    bytes, by kind: around kChunk, and around the last byte at which the run
    is still fully loaded."""
    chunk = win - MAX_RUN
    return {k: sorted(set(range(chunk - 80, chunk + 17)) | set(range(win - len(placed_run(np.random.default_rng(0), k)) - 16,
                                                                     win - len(placed_run(np.random.default_rng(0), k)) + 17)))
            for k in PLACED}


def placement(win, win_later, off, kinds=PLACED, step=1, near=20):
    """One segment per (kind, window byte `at`): a SHORT_REPEAT (so that no
    flat DIRECT chain leads the segment), filler runs, the run under test at
    window byte `at` of the segment's last-sized window (the first if
    win_later == win, else the second: a union instance's serial window), a
    SHORT_REPEAT, a DIRECT run of 200 bytes and a SHORT_REPEAT. marks: runs =
    [(kind, at, stream offset, segment index)], window = 0 or 1. step: only
    every step-th byte further than `near` bytes from the two edges."""
    rng = np.random.default_rng([7, win, win_later, off])
    data, segs, marks, vi = bytearray(), [], [], 0
    later = win_later != win
    for kind in kinds:
        size = len(placed_run(np.random.default_rng(0), kind))
        edges = (win_later - MAX_RUN, win_later - size)
        for at in sweep(win_later)[kind]:
            if at % step and min(abs(at - e) for e in edges) > near:
                continue
            start = len(data)
            p0 = (off + start) % 16
            seg = bytearray(sr(1, 3, int(rng.integers(1, 256))))
            if later:
                # fill the first window; the second opens at the first run it does not take
                k = 0
                while 2 + k * BIG < win:
                    k += 1
                pre = bytes(seg) + filler(rng, k * BIG)
                w = serial_windows(pre, 0, len(pre), p0, win, win_later)
                s1 = w[1].runs[0]
                seg = bytearray(pre[:s1])
                lp = s1 - w[1].wpos  # the second window's first run, in window bytes
                seg += filler(rng, at - lp)
            else:
                seg += filler(rng, at - p0 - len(seg))
            marks.append((kind, at, start + len(seg), len(segs)))
            seg += placed_run(rng, kind) + sr(2, 4, int(rng.integers(256, 1 << 16))) + filler(rng, 200) + sr(1, 3, 5)
            segs.append((start, vi))
            vi += sum(r.L for r in runs(bytes(seg)))
            data += seg
    return Shape("placement %d/%d +%d" % (win, win_later, off), data, False, off, segs, runs=marks, window=int(later), win=(win, win_later))


SLICE_AT = tuple(range(180, 331))


def header_slice(off):
    """After a window start, a DELTA run with a 22-byte header and a PATCHED
    run, each at every stream offset 180..330 of a segment (a segment per
    offset and kind, the other kind right behind it): over the walk's 256-byte
    header slice and its reload at kHdrLim bytes before the slice's end.
    Fillers are DIRECT W=8 runs of <= 62 bytes, so that the slice moves on in
    small steps. marks at: (kind of the run at the offset, offset) a segment."""
    rng = np.random.default_rng([11, off])
    cases, marks = [], []
    for at in SLICE_AT:
        for kind in (DELTA, PATCHED):
            b = bytearray(sr(1, 3, 1))
            while len(b) < at:
                take = min(at - len(b), int(rng.integers(20, 63)))
                if at - len(b) - take in (1, 2):
                    take -= 3
                b += direct(7, take - 2, list(rng.bytes(take - 2)))
            assert len(b) == at, (at, len(b))
            d = delta(7, 40, M64, M64 - 2, 10, 10, fields=_payload(rng, "random", 8, 38))
            p = patched(7, 40, 2, 0x8123, 7, 8, [entry(3, 9, 8), entry(30, 1, 8)], _payload(rng, "random", 8, 40))
            b += d + p if kind == DELTA else p + d
            b += sr(1, 3, 2)
            cases.append(("slice %d %s" % (at, "DELTA" if kind == DELTA else "PATCHED"), bytes(b)))
            marks.append((kind, at))
    s = concat("header slice +%d" % off, cases, False, off)
    s.marks["at"] = marks
    return s


def placement_cuts(win, win_later):
    """The longest run, the DELTA run with a 22-byte header and the straddling
    DELTA of the placement sweeps, each starting at kChunk and at the last
    byte at which it is fully loaded, a segment each; marks cuts: stream
    lengths around the run's window's kChunk and end, and around the run's
    own first and last byte."""
    s = placement(win, win_later, 0, kinds=("longest", "delta22", "straddle"), step=1 << 30, near=0)
    size = {r.off: r.size for r in runs(s.data)}
    cuts = set()
    for kind, at, o, seg in s.marks["runs"]:
        start = s.segs[seg][0]
        end = s.segs[seg + 1][0] if seg + 1 < len(s.segs) else len(s.data)
        w = serial_windows(s.data, start, end, 0, win, win_later)[s.marks["window"]]
        for e in (w.wpos + win_later - MAX_RUN, w.wpos + win_later, o, o + size[o]):
            cuts.update(e + d for d in (-1, 0, 1, 2))
    s.marks["cuts"] = sorted(c for c in cuts if 0 < c <= len(s.data))
    return s


def short_run(rng, k):
    """A run of <= kShortL values in 2..14 bytes (k picks the kind)."""
    k %= 6
    if k == 0:
        return sr(int(rng.integers(1, 9)), int(rng.integers(3, 11)), int(rng.integers(1, 1 << 62)))
    if k == 1:
        L = int(rng.integers(1, 11))
        return direct(7, L, list(rng.bytes(L)))
    if k == 2:
        return delta(0, int(rng.integers(1, 17)), zigzag(int(rng.integers(-999, 999))), zigzag(int(rng.integers(-9, 9))))
    if k == 3:
        L = int(rng.integers(3, 10))
        return delta(7, L, int(rng.integers(1, 1 << 35)), zigzag(int(rng.integers(-99, 99))), fields=list(rng.bytes(L - 2)))
    if k == 4:
        L = int(rng.integers(1, 17))
        return direct(3, L, [int(x) & 15 for x in rng.bytes(L)])
    return delta(0, 16, int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 20)))


def short_runs(rng, n):
    return [short_run(rng, int(rng.integers(0, 6))) for _ in range(n)]


def items(off=0):
    """Work items and run tables: 63, 64, 65, 128 and 129 short runs before a
    long one, runs of 16 against 17 values, a PATCHED run of <= 16 values
    among short runs; a segment each."""
    rng = np.random.default_rng([13, off])
    long_run = lambda: direct(15, 300, _payload(rng, "random", 16, 300))
    cases = []
    for n in (63, 64, 65, 128, 129):
        # a long run first: the segment is not a short-run segment to the probes
        cases.append(("%d short runs" % n, long_run() + b"".join(short_runs(rng, n)) + long_run() + sr(1, 3, 1)))
    for L in (16, 17):
        body = b"".join(direct(7, L, list(rng.bytes(L))) + delta(0, L, 5, 6) + delta(3, L, 5, 6, fields=[1] * (L - 2)) for _ in range(40))
        cases.append(("runs of %d" % L, long_run() + body + long_run()))
    p = patched(7, 12, 1, 3, 7, 4, [entry(2, 0xA5, 8), entry(7, 0xFF, 8)], _payload(rng, "random", 8, 12))
    cases.append(("short PATCHED", long_run() + b"".join(short_runs(rng, 30)) + p + b"".join(short_runs(rng, 30)) + p + p + long_run()))
    cases.append(("short PATCHED among short runs", b"".join(short_runs(rng, 30)) + p + b"".join(short_runs(rng, 70)) + p + p + sr(1, 3, 1)))
    return concat("items +%d" % off, cases, True, off)


TABLE_RUNS = (511, 512, 513, 1025)


def tables():
    """511, 512, 513 and 1,025 runs inside one serial window (the serial run
    table holds 512: a second pass over the same window), a segment each:
    DIRECT W=8 runs of 20 values (22 bytes, long to the walk) - and a slab of
    1,024 two-byte SHORT_REPEATs, kDenseRuns, and the same plus one."""
    rng = np.random.default_rng(17)
    cases = []
    for n in TABLE_RUNS:
        cases.append(("%d runs" % n, b"".join(direct(7, 20, list(rng.bytes(20))) for _ in range(n))))
    for n in (DENSE_RUNS, DENSE_RUNS + 1):
        cases.append(("%d two-byte runs" % n, b"".join(sr(1, 3 + i % 8, int(rng.integers(0, 256))) for i in range(n))))
    return concat("tables", cases, True)


def dense_phases(off=0):
    """Runs of every byte size 2..12 at every phase of the dense discovery's
    8-byte blocks, 64-byte super-blocks and 2,048-byte slabs (all counted from
    the pass's first run: here the segment's): for each size s, a segment per
    lead-in run of 2 .. s + 1 bytes, then s-byte runs past the first slab - so
    the run across each edge has 1 .. s - 1 of its bytes before it - as
    SHORT_REPEATs (the second header byte and the payload cross), fixed DELTAs
    with padded varints (a varint crosses) and DIRECT runs (the payload)."""
    rng = np.random.default_rng([19, off])
    cases = []
    for s in range(2, 13):
        for kind in ("sr", "delta", "direct"):
            if (kind == "sr" and s > 9) or (kind == "delta" and s < 4) or (kind == "direct" and s < 3):
                continue
            for lead in range(2, s + 2):
                b = bytearray(sr(1, 3, 7) if lead == 2 else direct(7, lead - 2, list(rng.bytes(lead - 2))))
                k = 0
                while len(b) < SLAB + 40:
                    if kind == "sr":
                        b += sr(s - 1, 3 + k % 8, int(rng.integers(1, 1 << min(8 * (s - 1), 62))) | 1)
                    elif kind == "delta":
                        n1 = 1 + k % (s - 3)
                        b += delta(0, 2 + k % 9, int(rng.integers(1, 128)), int(rng.integers(1, 128)), n1, s - 2 - n1)
                    else:
                        b += direct(7, s - 2, list(rng.bytes(s - 2)))
                    k += 1
                cases.append(("%s of %d bytes after %d" % (kind, s, lead), bytes(b)))
    return concat("dense phases +%d" % off, cases, True, off)


def dense_mixes():
    """Dense passes that end early, full slabs of values, and the density
    thresholds from both sides within one segment."""
    rng = np.random.default_rng(23)
    shorts = lambda n: b"".join(short_runs(rng, n))
    mid = lambda nbytes: direct(7, nbytes - 2, list(rng.bytes(nbytes - 2)))  # a run of nbytes bytes
    p = patched(7, 40, 2, 0x8123, 7, 8, [entry(3, 9, 8), entry(30, 1, 8)], _payload(rng, "random", 8, 40))
    d11 = delta(7, 6, M64, zigzag(3), 11, 1, fields=[1, 2, 3, 4])
    cases = [("an 11-byte varint and a PATCHED run amid short runs", shorts(200) + d11 + shorts(150) + p + shorts(200) + d11 + p + shorts(50)),
             ("slabs of 512-value fixed DELTAs", b"".join(delta(0, 512, int(rng.integers(0, 128)), int(rng.integers(0, 64))) for _ in range(2 * 512 + 7)))]
    for L in (16, 17, 256, 257):
        body = b"".join(shorts(3) + delta(0, L, 5, 6) + direct(0, L, [i & 1 for i in range(L)]) for _ in range(60))
        cases.append(("short runs and runs of %d" % L, body))
    # bytes per run across the thresholds, both ways: 24 and 64 (one pass),
    # 128 and 512 (two passes), sections of 40 runs and more
    for lo, hi in ((23, 25), (60, 70), (120, 136), (500, 514)):
        up = b"".join(mid(lo) for _ in range(60)) + b"".join(mid(hi) for _ in range(60))
        cases.append(("%d then %d bytes a run" % (lo, hi), shorts(100) + up + shorts(100)))
        cases.append(("%d then %d bytes a run" % (hi, lo), b"".join(mid(hi) for _ in range(60)) + b"".join(mid(lo) for _ in range(60)) + shorts(100)))
    return concat("dense mixes", cases, True)


def slices():
    """The second pass's value slices (kSliceMax = 1024 values, kRound = 256
    runs a round): run boundaries at values 1,023 / 1,024 / 1,025 of a
    segment, a variable-width DELTA run and a PATCHED run with patches on both
    sides carried over the slice edge, and 255, 256, 257 and 513 runs in one
    slice; short runs around them keep the segments dense."""
    rng = np.random.default_rng(29)
    cases = []

    def upto(nvalues):  # SHORT_REPEATs of exactly nvalues >= 3 values
        b, left = bytearray(), nvalues
        while left:
            L = left if left <= 10 else int(rng.integers(3, 8))
            b += sr(2, L, int(rng.integers(1, 1 << 16)))
            left -= L
        return bytes(b)

    tail = lambda: upto(1500)
    for edge in (1023, 1024, 1025):
        cases.append(("a run boundary at value %d" % edge, upto(edge) + tail()))
    dv = delta(12, 200, zigzag(5), zigzag(-3), fields=_payload(rng, "random", 13, 198))
    cases.append(("a DELTA run over the slice edge", upto(900) + dv + tail()))
    pv = patched(7, 200, 2, 0x8123, 7, 8, [entry(50, 9, 8), entry(100, 1, 8)], _payload(rng, "random", 8, 200))
    cases.append(("a PATCHED run over the slice edge", upto(950) + pv + tail()))
    for n in SLICE_RUNS:  # exactly n runs in the first 1,024 values
        ls = [SLICE_MAX // n + (k < SLICE_MAX % n) for k in range(n)]
        cases.append(("%d runs in a slice" % n, b"".join(direct(7, L, list(rng.bytes(L))) for L in ls) + tail()))
    return concat("slices", cases, True)


def two_pass_shape(nvalues, nsegs):
    """(slices a segment, values a slice) of a two-pass launch over a segment
    table (rlev2_route.hh seg_value_bound, two_pass_shape; checked against
    them by tests/test_cxx_rlev2_route.py)."""
    avg = (nvalues + nsegs - 1) // max(nsegs, 1)
    n = max(avg + avg // 8 + 512, 1)
    k = min((n + SLICE_MAX - 1) // SLICE_MAX, 256)
    s = (n + k - 1) // k
    return k, min((s + 255) & ~255, SLICE_MAX)


SLICE_RUNS = (255, 256, 257, 513)
RANGE_AT = (0, 1, 63, 64, 65)


def ranges():
    """One long run of each kind between SHORT_REPEATs; marks ranges: (begin,
    count) windows that begin and end inside each run at in-run offsets 0, 1,
    63, 64, 65 and L - 1 (PATCHED: after some of its patches)."""
    rng = np.random.default_rng(31)
    big = lambda W, k: _payload(rng, "random", W, k)
    body = [sr(8, 10, int(rng.integers(1, 1 << 63))), direct(31, 300, big(64, 300)),
            patched(30, 300, 8, int(rng.integers(1, 1 << 63)), 7, 8, _escaped([10, 62, 64, 70, 298], [3, 5, 7, 9, 11], 8), big(56, 300)),
            delta(0, 300, zigzag(-(1 << 62)), zigzag((1 << 55) + 1)), delta(30, 300, zigzag(1 << 61), zigzag(-9), fields=big(56, 298)),
            direct(20, 300, big(21, 300)), sr(3, 5, 0x80FFFF)]
    data = b"".join(body)
    table = run_table(data) + [(len(data), None)]
    first = [v for _, v in table[:-1]] + [sum(r.L for r in runs(data))]
    total, out = first[-1], [(0, first[-1]), (0, 1), (first[-1] - 1, 1)]
    for a, b in zip(first[:-1], first[1:]):
        L = b - a
        ins = sorted({x for x in RANGE_AT + (L - 1,) if x < L})
        for x in ins:
            out.append((a + x, L - x))  # from inside the run to its end
            out.append((a, x + 1))  # from its start to inside
            out.append((a + x, 1))
        out.append((a + 1, L + 3))  # into the next run
    return Shape("ranges", data, True, 0, [(0, 0)], ranges=[(a, c) for a, c in out if c > 0 and a + c <= total], first=first)
