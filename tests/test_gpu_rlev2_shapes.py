"""Every RLEv2 kernel instance against the exact model of tests/rlev2_model.py
at the streams where its steps can go wrong: the whole run grammar as a writer
with every header field free can say it (non-minimal varints and byte counts,
corrupt patch lists the reference still decodes, padding bits, every width),
runs placed at every byte around the serial walk's kChunk and around the last
start at which a run is still fully loaded, for every window size, headers over
the walk's 256-byte slice, work items and run tables at their capacities, runs
over the dense discovery's block, super-block and slab edges at every phase,
the density thresholds from both sides, the second pass's slice edges, output
ranges and widths, row-index positions, segment tables with empty and
misaligned entries, and streams cut at every byte with live bytes after the
cut.

Everything goes through orcg_rlev2_decode_device and
orcg_rlev2_decode_positions_device, so the test sets the segment table, the
output width and range, src_len and the source pointer's low four bits. Many
shapes go into one launch as the segments of one stream: each segment has its
own workgroup, and its first window starts at it. Outputs are pre-filled with
a sentinel and carry guard elements on both sides; every comparison is exact,
and every check runs on every id of orc_amd.rlev2_variants().
tests/test_rlev2_model_cpu.py proves on the CPU that the model agrees with
the oracle on these streams and that each holds its run where it says.

Needs a real MI355X: run with `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

import orc_amd
import rlev2_model as m

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = {8: 0x5A5A5A5A5A5A5A5A, 4: 0x5A5A5A5A, 2: 0x5A5A}
OFFS = (0, 1, 15)


@pytest.fixture(scope="module")
def ctx():
    c = orc_amd.Context(0)
    yield c
    c.set_rlev2_variant(0)


def each_variant(ctx, fn):
    """fn(variant) under every kernel variant; variant 0 is restored. The
    failures of all variants are reported together."""
    bad = []
    try:
        for v in orc_amd.rlev2_variants():
            ctx.set_rlev2_variant(v)
            try:
                fn(v)
            except AssertionError as e:
                bad.append("variant %d (%s): %s" % (v, m.VARIANTS[v][1], str(e)[:600]))
    finally:
        ctx.set_rlev2_variant(0)
    assert not bad, "\n".join(bad)


class Source:
    """A stream in device memory with its byte 0 at an address = off mod 16
    (read from data_ptr() at run time), followed by 64 zero bytes."""

    def __init__(self, data, off=0):
        import torch

        host = np.frombuffer(bytes(data) + bytes(64), dtype=np.uint8).copy()
        self.raw = torch.zeros(host.size + 32, dtype=torch.uint8, device="cuda")
        at = (off - self.raw.data_ptr()) % 16
        self.dev = self.raw[at:at + host.size]
        self.dev.copy_(torch.from_numpy(host))
        assert self.dev.data_ptr() % 16 == off
        self.len = len(data)
        self.tables = {}

    def table(self, segs):
        import torch

        key = tuple(segs)
        if key not in self.tables:
            self.tables[key] = torch.from_numpy(np.array(segs, dtype=np.uint64).reshape(-1, 2).view(np.int64)).cuda()
        return self.tables[key]

    def decode(self, ctx, signed, segs, begin, count, dst_bytes=8, src_len=None, stride=None):
        """(the output range, the error Context.synchronize reports or None,
        the error's value index). stride: segs are row-index positions (run
        offset, values to skip) of row groups of `stride` values."""
        import torch

        L = orc_amd.rle._lib.load()
        src_len = self.len if src_len is None else src_len
        table = self.table(segs)
        dtype = {8: torch.int64, 4: torch.int32, 2: torch.int16}[dst_bytes]
        out = torch.full((count + 2 * GUARD,), SENTINEL[dst_bytes], dtype=dtype, device="cuda")
        vp = ctypes.c_void_p
        ctx.after_torch()
        if stride is None:
            rc = L.orcg_rlev2_decode_device(ctx.handle, vp(self.dev.data_ptr()), src_len, int(signed), vp(table.data_ptr()),
                                            len(segs), begin, count, vp(out.data_ptr() + GUARD * dst_bytes), dst_bytes)
        else:
            rc = L.orcg_rlev2_decode_positions_device(ctx.handle, vp(self.dev.data_ptr()), src_len, int(signed),
                                                      vp(table.data_ptr()), len(segs), stride, begin, count,
                                                      vp(out.data_ptr() + GUARD * dst_bytes), dst_bytes)
        orc_amd.rle.check(rc, ctx.last_error)
        err, at = None, None
        try:
            ctx.synchronize()
        except orc_amd.OrcError as e:
            err, at = e, ctx.last_error_value()
        host = out.cpu().numpy()
        assert (host[:GUARD] == SENTINEL[dst_bytes]).all() and (host[GUARD + count:] == SENTINEL[dst_bytes]).all(), "guards"
        return host[GUARD:GUARD + count], err, at


def same(got, want, label):
    if got.shape != want.shape or not (got == want).all():
        k = int(np.flatnonzero(got != want)[0]) if got.shape == want.shape else -1
        raise AssertionError("%s: value %d of %d is %s, the model's %s (%d differ)" % (
            label, k, want.size, got[k] if k >= 0 else got.shape, want[k] if k >= 0 else want.shape,
            int((got != want).sum()) if k >= 0 else -1))


def check_stream(ctx, src, signed, segs, label, whole, src_len=None):
    """Under every variant: the stream's producible values decode exactly and
    without an error; one more value gives the model's error at the model's
    value index, after the same values, with the sentinel left in its place."""
    src_len = src.len if src_len is None else src_len
    segs = [s for s in segs if s[0] < src_len] or [(0, 0)]
    want, n, text, at = m.decode(whole[:src_len], signed)

    def one(v):
        if n:
            got, err, _ = src.decode(ctx, signed, segs, 0, n, src_len=src_len)
            assert err is None, "%s: %r" % (label, err)
            same(got, want, label)
        got, err, eat = src.decode(ctx, signed, segs, 0, n + 1, src_len=src_len)
        assert isinstance(err, orc_amd.ParseError) and text in str(err) and eat == at, "%s: %r at %s, the model's %r at %d" % (
            label, err, eat, text, at)
        same(got[:n], want, label + " before the error")
        assert got[n] == SENTINEL[8], label + ": a value past the error"

    each_variant(ctx, one)
    return want


def check_shape(ctx, s):
    return check_stream(ctx, Source(s.data, s.off), s.signed, s.segs, s.name, s.data)


# ---- A. the run grammar ---------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("family", sorted(m.FAMILIES))
def test_run_grammar(ctx, family, signed):
    """Every case of the family between two SHORT_REPEATs, a segment each:
    SHORT_REPEAT byte counts and lengths, minimal or not; DIRECT at every
    width and length with the padding bits set; PATCHED_BASE at every W, (pw,
    pgw), bw and base sign, patch positions from 0 to past L, gaps of 0,
    escapes at every place; DELTA fixed and at every width, all-ones deltas
    around the 32-bit scan's limit, varints padded to every length up to a
    64-byte header."""
    check_shape(ctx, m.grammar(family, signed, off=1 if signed else 0))


def test_run_grammar_as_one_segment(ctx):
    """The same runs back to back in one segment (one workgroup walks them
    all), at the third pointer offset."""
    for family in sorted(m.FAMILIES):
        s = m.grammar(family, True, off=15)
        check_stream(ctx, Source(s.data, 15), True, [(0, 0)], s.name + " in one segment", s.data)


@pytest.mark.parametrize("name,data,signed", m.error_cases(), ids=[c[0] for c in m.error_cases()])
def test_parse_errors_and_their_precedence(ctx, name, data, signed):
    """pl == 0, pw + pgw > 64 and a DELTA run of one value with a width, each
    with cuts that come earlier and later in the read order; DELTA headers of
    64 bytes (the longest accepted) and longer ones (a bad read at the run's
    first value, by the rule of include/orcg.h)."""
    check_stream(ctx, Source(data), signed, [(0, 0)], name, data)


# ---- B. placement in the windows ----------------------------------------------------------
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("win", m.WINDOWS, ids=["%d-%d" % w for w in m.WINDOWS])
def test_runs_around_the_window_edges(ctx, win, off):
    """A DELTA run with a 22-byte header, the longest legal run, DIRECT W=64
    L=512, a SHORT_REPEAT and a 23-byte DELTA run that straddles the edge,
    starting at every window byte of kChunk - 80 .. kChunk + 16 and of the 16
    bytes on either side of the last start at which they are fully loaded;
    for each window size of the instances (8704-17152: the second, serial
    window of the union instances)."""
    check_shape(ctx, m.placement(win[0], win[1], off, step=1 if off == 0 else 7))


@pytest.mark.parametrize("off", OFFS)
def test_headers_over_the_header_slice(ctx, off):
    """A 22-byte DELTA header and a PATCHED header, each at every offset
    180..330 after a window start."""
    check_shape(ctx, m.header_slice(off))


# ---- C. tables and items --------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 15))
def test_work_items(ctx, off):
    """63 .. 129 short runs before a long one, runs of 16 against 17 values,
    PATCHED runs of <= 16 values among short runs."""
    check_shape(ctx, m.items(off))


def test_run_tables_at_their_capacity(ctx):
    """511, 512, 513 and 1,025 runs inside one serial window; a slab of
    kDenseRuns two-byte runs, and one more."""
    check_shape(ctx, m.tables())


# ---- D. dense discovery -------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
def test_runs_over_block_and_slab_edges(ctx, off):
    check_shape(ctx, m.dense_phases(off))


def test_dense_passes_and_thresholds(ctx):
    """Passes that end at an 11-byte varint or a PATCHED run, slabs of
    512-value runs, runs of 16 / 17 / 256 / 257 values, and the bytes per run
    across each density threshold in both directions."""
    check_shape(ctx, m.dense_mixes())


# ---- E. the second pass ----------------------------------------------------------------------------
def test_slice_edges(ctx):
    check_shape(ctx, m.slices())


# ---- F. ranges, positions, segment tables -----------------------------------------------------------
@pytest.mark.parametrize("dst_bytes", (8, 4, 2))
def test_output_ranges_and_widths(ctx, dst_bytes):
    s = m.ranges()
    src = Source(s.data)
    want = m.decode(s.data, True, dst_bytes)[0]
    assert len(s.marks["ranges"]) > 80

    def one(v):
        for begin, count in s.marks["ranges"]:
            got, err, _ = src.decode(ctx, True, s.segs, begin, count, dst_bytes=dst_bytes)
            assert err is None, (begin, count, err)
            same(got, want[begin:begin + count], "range %d + %d" % (begin, count))

    each_variant(ctx, one)


@pytest.mark.parametrize("stride", (100, 37))
def test_row_index_positions(ctx, stride):
    """Positions with a non-zero skip into each run kind, whole and as a
    range that starts inside a row group."""
    streams = [m.ranges(), m.grammar("patched", True), m.grammar("delta", False)]

    def one(v):
        for s in streams:
            want, n, _, _ = m.decode(s.data, s.signed)
            pos = m.positions(s.data, n, stride)
            assert (pos[1:, 1] > 0).any()
            src = srcs[s.name]
            for begin, count in ((0, n), (stride + 3, n - stride - 3), (2 * stride - 1, 2)):
                got, err, _ = src.decode(ctx, s.signed, [tuple(p) for p in pos.tolist()], begin, count, stride=stride)
                assert err is None, (s.name, begin, err)
                same(got, want[begin:begin + count], "%s from %d" % (s.name, begin))

    srcs = {s.name: Source(s.data) for s in streams}
    each_variant(ctx, one)


def test_empty_segments(ctx):
    """Table entries repeated: segments that hold nothing."""
    s = m.grammar("sr", True)
    segs = [e for k, e in enumerate(s.segs) for _ in range(1 + (k % 3 == 0) + (k % 5 == 0))]
    assert len(set(segs)) < len(segs)
    check_stream(ctx, Source(s.data), True, segs, "empty segments", s.data)


def test_table_that_is_not_run_aligned_is_reported(ctx):
    """A run-aligned offset whose value index is off by one, and an entry
    inside the previous segment's last run. The context decodes the stream
    afterwards."""
    s = m.grammar("delta", True)
    src = Source(s.data)
    want, n, _, _ = m.decode(s.data, True)
    size = {r.off: r.size for r in m.runs(s.data, True)}
    tables = []
    for k in (1, len(s.segs) // 2):
        for by in (1, -1):
            bad = list(s.segs)
            bad[k] = (bad[k][0], bad[k][1] + by)
            tables.append((bad, n))
        bad = list(s.segs)
        bad[k] = (bad[k][0] - 1, bad[k][1])  # inside the SHORT_REPEAT that ends segment k - 1
        tables.append((bad, bad[k][1]))  # the values asked for end there: the later segment decodes nothing
    for bad, count in tables:
        assert m.table_error(s.data, bad) is not None

    def one(v):
        for bad, count in tables:
            _, err, at = src.decode(ctx, True, bad, 0, count)
            assert isinstance(err, orc_amd.InvalidArgument) and m.SEGMENT_ERROR in str(err), err
            assert at == m.table_error(s.data, bad), (at, m.table_error(s.data, bad))
        got, err, _ = src.decode(ctx, True, s.segs, 0, n)
        assert err is None
        same(got, want, "after the errors")

    each_variant(ctx, one)


# ---- G. cuts ----------------------------------------------------------------------------------------------
def test_small_stream_cut_at_every_byte(ctx):
    """src_len at every byte of a stream that holds every run kind, the rest
    of the stream live behind the cut."""
    s = m.cut_stream()
    src = Source(s.data)
    for cut in range(len(s.data) + 1):
        check_stream(ctx, src, True, s.segs, "cut %d" % cut, s.data, src_len=cut)


@pytest.mark.parametrize("win", m.WINDOWS, ids=["%d-%d" % w for w in m.WINDOWS])
def test_long_stream_cut_around_its_windows_ends(ctx, win):
    s = m.trunc_long(*win)
    src = Source(s.data)
    assert len(s.marks["cuts"]) >= 20
    for cut in s.marks["cuts"]:
        check_stream(ctx, src, False, s.segs, "cut %d" % cut, s.data, src_len=cut)


@pytest.mark.parametrize("win", m.WINDOWS, ids=["%d-%d" % w for w in m.WINDOWS])
def test_placed_runs_cut_around_their_windows_ends(ctx, win):
    """The longest run, the 22-byte-header DELTA and the straddling DELTA at
    kChunk and at the last fully loaded start, with src_len around kChunk and
    the end of their window and around the run's own ends."""
    s = m.placement_cuts(*win)
    src = Source(s.data)
    for cut in s.marks["cuts"]:
        check_stream(ctx, src, False, s.segs, "cut %d" % cut, s.data, src_len=cut)
