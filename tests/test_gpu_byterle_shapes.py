"""byterle_kernel against the exact model of tests/byterle_model.py at the
stream shapes where its steps can go wrong: group headers on the window's
last bytes, groups of every length at every phase of a thread's chunk and
across block ends, windows of as many groups as the tables hold (17 owner-map
rounds), groups around the owner map's dword and round edges, several windows
a segment with every p0, misaligned byte and row ranges, the set-row and
device-side row counts the file reader uses, segment tables with a group a
segment, repeated and wrong entries, and streams cut at every byte and around
the window's end with live bytes after the cut.

Everything goes through orcg_byterle_decode_device, orcg_boolrle_decode_device
and orcg_boolrle_decode_counted_device, so the test sets the segment table,
the range, the destination's alignment and the source pointer's low four
bits. Outputs are pre-filled with a sentinel and carry guard bytes on both
sides; every comparison is exact. tests/test_byterle_model_cpu.py proves on
the CPU that the model agrees with the oracle on these streams and that each
holds its feature where it says.

Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import byterle_model as m
import orc_amd

pytestmark = pytest.mark.gpu

READ_ERROR = "bad read in nextBuffer"
SEGMENT_ERROR = "Stream position is not at a run boundary"
GUARD, SENTINEL, LIVE = 64, 0x5A, 0xA5
ONES0 = 1_000_003  # the set-row counter starts from here


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


class Source:
    """A stream in device memory with its byte 0 at an address = off mod 16
    (read from data_ptr() at run time), up to 15 bytes of the allocation
    before it (the descriptor starts at the address rounded down to 16) and 64
    live, non-zero bytes after it."""

    def __init__(self, data, off=0):
        import torch

        host = np.frombuffer(bytes(data) + bytes([LIVE]) * 64, dtype=np.uint8).copy()
        self.raw = torch.full((host.size + 32,), LIVE, dtype=torch.uint8, device="cuda")
        at = (off - self.raw.data_ptr()) % 16
        self.dev = self.raw[at:at + host.size]
        self.dev.copy_(torch.from_numpy(host))
        assert self.dev.data_ptr() % 16 == off
        self.len = len(data)

    def decode(self, ctx, boolean, segs, begin, count, src_len=None, dst_off=0, entry="counted", row_count=None):
        """(the output range, the error Context.synchronize reports or None,
        the set rows added to the counter: boolean mode through the counted
        entry). dst_off: the destination address mod 8. row_count: the
        device-side row count (count is then the host-side bound)."""
        import torch

        L = orc_amd.rle._lib.load()
        src_len = self.len if src_len is None else src_len
        table = torch.from_numpy(np.array(segs, dtype=np.uint64).reshape(-1, 2).view(np.int64)).cuda()
        out = torch.full((count + 2 * GUARD + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 8 == 0
        at = GUARD + dst_off
        args = (ctx.handle, self.dev.data_ptr(), src_len, table.data_ptr(), len(segs), begin, count)
        ones = None
        ctx.after_torch()
        if not boolean:
            rc = L.orcg_byterle_decode_device(*args, out.data_ptr() + at)
        elif entry == "plain":
            rc = L.orcg_boolrle_decode_device(*args, out.data_ptr() + at)
        else:
            ones = torch.tensor([ONES0], dtype=torch.int64, device="cuda")
            rows = None if row_count is None else torch.tensor([row_count], dtype=torch.int64, device="cuda")
            ctx.after_torch()
            rc = L.orcg_boolrle_decode_counted_device(*args, None if rows is None else rows.data_ptr(),
                                                      out.data_ptr() + at, ones.data_ptr())
        orc_amd.rle.check(rc, ctx.last_error)
        err = None
        try:
            ctx.synchronize()
        except orc_amd.OrcError as e:
            err = e
        host = out.cpu().numpy()
        assert (host[:at] == SENTINEL).all() and (host[at + count:] == SENTINEL).all(), "guards"
        return host[at:at + count], err, None if ones is None else int(ones.cpu()[0]) - ONES0


def check_stream(ctx, src, segs, label, whole, src_len=None, modes=(False, True)):
    """In both modes: what the stream can produce decodes exactly, without an
    error, and the counter gains the set rows; one more value gives the
    reference's error at the model's index, after the same values."""
    src_len = src.len if src_len is None else src_len
    segs = [s for s in segs if s[0] < src_len] or [(0, 0)]
    for boolean in modes:
        want, n = m.decode(whole[:src_len], boolean)
        tag = "%s %s" % (label, "rows" if boolean else "bytes")
        if n:
            got, err, ones = src.decode(ctx, boolean, segs, 0, n, src_len=src_len)
            assert err is None, (tag, err)
            np.testing.assert_array_equal(got, want, err_msg=tag)
            assert ones is None or ones == int(want.sum()), tag
        got, err, _ = src.decode(ctx, boolean, segs, 0, n + 1, src_len=src_len)
        assert isinstance(err, orc_amd.ParseError) and READ_ERROR in str(err), (tag, err)
        assert ctx.last_error_value() == (n // 8 if boolean else n), tag  # the first decoded byte that is missing
        np.testing.assert_array_equal(got[:n], want, err_msg=tag + " before the error")


def check_shape(ctx, s, label):
    check_stream(ctx, Source(s.data, s.off), s.segs, label, s.data)


# ---- window, chunk and block edges -------------------------------------------
@pytest.mark.parametrize("off", m.OFFS)
@pytest.mark.parametrize("kind", m.EDGE_KINDS)
def test_group_header_on_the_windows_last_bytes(ctx, kind, off):
    """A run whose value byte lies in the tail, a 129-byte literal reaching
    window byte 4095 + 129 and a 1-byte literal, with the header at window
    bytes 4096 - 18 .. 4095 and at 4096 (where it opens the next window)."""
    for d in m.EDGE_D:
        check_shape(ctx, m.window_edge(kind, d, off), "%s d=%s off=%d" % (kind, d, off))


@pytest.mark.parametrize("off", m.OFFS)
def test_every_group_length_at_every_chunk_phase(ctx, off):
    """Stream lengths 2 .. 129 from every byte of a 16-byte chunk: groups
    across chunk and block ends, literal payloads at every offset mod 4."""
    for band in range(m.BANDS):
        check_shape(ctx, m.length_phases(band, off), "band %d off=%d" % (band, off))


@pytest.mark.parametrize("off", m.OFFS)
def test_blocks_without_a_group_start(ctx, off):
    check_shape(ctx, m.block_hops(off), "block hops off=%d" % off)


# ---- full tables, the owner map -------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("kind", m.DENSE)
def test_dense_windows(ctx, kind, off):
    """Windows of 2,048 two-byte groups: 1-byte literals, runs of 3, runs of
    130 (266,240 decoded bytes, 17 owner-map rounds), both parities of p0."""
    check_shape(ctx, m.dense(kind, off), "dense %s off=%d" % (kind, off))


@pytest.mark.parametrize("off", m.OFFS)
def test_groups_without_a_whole_dword(ctx, off):
    check_shape(ctx, m.small_groups(off), "small groups off=%d" % off)


@pytest.mark.parametrize("off", m.OFFS)
def test_groups_on_and_across_the_owner_maps_round_edge(ctx, off):
    check_shape(ctx, m.round_edges(off), "round edges off=%d" % off)


@pytest.mark.parametrize("off", m.OFFS)
def test_every_p0_of_a_later_window(ctx, off):
    for ph in range(16):
        check_shape(ctx, m.crossing(ph, off), "crossing %d off=%d" % (ph, off))


# ---- ranges and counts ------------------------------------------------------------
def test_byte_ranges(ctx):
    """value_begin and the destination address at every residue mod 4, counts
    that end inside a dword, ranges that let whole segments return early."""
    s = m.ranged()
    src = Source(s.data)
    want = m.decode(s.data)[0]
    for k, (begin, count) in enumerate(m.byte_ranges(s)):
        for dst_off in {0, k % 4, (k + 1) % 4}:
            got, err, _ = src.decode(ctx, False, s.segs, begin, count, dst_off=dst_off)
            assert err is None, (begin, count, err)
            np.testing.assert_array_equal(got, want[begin:begin + count], "bytes %d + %d to %d" % (begin, count, dst_off))


@pytest.mark.parametrize("entry", ["counted", "plain"])
def test_row_ranges_and_their_counts(ctx, entry):
    """row_begin, nrows and the destination address at every residue mod 8,
    ranges inside one decoded byte; the counter gains the range's set rows."""
    s = m.ranged()
    src = Source(s.data)
    want = m.decode(s.data, True)[0]
    for k, (begin, count) in enumerate(m.bool_ranges(s)):
        for dst_off in {0, k % 8, (-begin) % 8}:
            got, err, ones = src.decode(ctx, True, s.segs, begin, count, dst_off=dst_off, entry=entry)
            assert err is None, (begin, count, err)
            np.testing.assert_array_equal(got, want[begin:begin + count], "rows %d + %d to %d" % (begin, count, dst_off))
            assert ones == (int(want[begin:begin + count].sum()) if entry == "counted" else None), (begin, count, dst_off)


def test_device_side_row_count(ctx):
    """The row count read from device memory, below the host-side bound: the
    rows past it are untouched and uncounted."""
    s = m.ranged()
    src = Source(s.data)
    want = m.decode(s.data, True)[0]
    n = want.size
    for begin, rows, bound in [(0, n, n), (0, n - 1, n), (0, 1, n), (0, 0, 64), (0, 8 * s.segs[2][1] + 3, n), (5, 1001, 4000),
                               (13, 3, 100), (8 * s.segs[1][1], 8, n - 8 * s.segs[1][1])]:
        got, err, ones = src.decode(ctx, True, s.segs, begin, bound, row_count=rows)
        assert err is None, (begin, rows, bound, err)
        np.testing.assert_array_equal(got[:rows], want[begin:begin + rows], "%d rows from %d" % (rows, begin))
        assert (got[rows:] == SENTINEL).all(), (begin, rows, bound)
        assert ones == int(want[begin:begin + rows].sum()), (begin, rows, bound)


# ---- segment tables -------------------------------------------------------------------
@pytest.mark.parametrize("repeat", [False, True], ids=["a group a segment", "repeated entries"])
def test_one_group_per_segment(ctx, repeat):
    data, segs = m.grouped(repeat)
    check_stream(ctx, Source(data), segs, "grouped", data)


def test_table_that_is_not_group_aligned_is_reported(ctx):
    """Error reports, not faults: an entry whose value index is off by one,
    and an entry inside the previous segment's last group (that group runs
    past its segment's end). The segments before decode exactly, and the
    context decodes the stream afterwards."""
    data, segs = m.grouped()
    src = Source(data)
    for boolean in (False, True):
        want, n = m.decode(data, boolean)
        scale = 8 if boolean else 1
        for k in (1, len(segs) // 2):
            for by in (1, -1):
                bad = list(segs)
                bad[k] = (bad[k][0], bad[k][1] + by)
                got, err, _ = src.decode(ctx, boolean, bad, 0, n)
                assert isinstance(err, orc_amd.InvalidArgument) and SEGMENT_ERROR in str(err), (k, by, err)
                good = scale * min(segs[k][1], bad[k][1])
                np.testing.assert_array_equal(got[:good], want[:good])
        sizes = {g[0]: g[3] for g in m.walk(data)}
        for k in (0, 5):
            off, vi = segs[k]
            bad = list(segs)
            bad[k + 1] = (off + sizes[off] // 2, segs[k + 1][1])
            got, err, _ = src.decode(ctx, boolean, bad, 0, scale * segs[k + 1][1])
            assert isinstance(err, orc_amd.InvalidArgument) and SEGMENT_ERROR in str(err), (k, err)
            np.testing.assert_array_equal(got[:scale * vi], want[:scale * vi])
        got, err, ones = src.decode(ctx, boolean, segs, 0, n)
        assert err is None and (ones is None or ones == int(want.sum()))
        np.testing.assert_array_equal(got, want)


# ---- truncation ---------------------------------------------------------------------------
def check_host_decoder(ctx, data, label):
    """orcg_byte_rle_decoder over a host buffer of exactly the cut's length
    (make_byte_plan's count): the producible values, then the error."""
    for boolean in (False, True):
        want, n = m.decode(data, boolean)
        if n:
            np.testing.assert_array_equal(orc_amd.ByteRleDecoder(data, boolean=boolean, ctx=ctx).next(n), want, label)
        dec = orc_amd.ByteRleDecoder(data, boolean=boolean, ctx=ctx)
        with pytest.raises(orc_amd.ParseError, match=READ_ERROR):
            dec.next(n + 1)


def test_small_stream_cut_at_every_byte(ctx):
    """src_len = cut over a device buffer that still holds the rest of the
    stream (live bytes within the descriptor's rounded-up dword and after)."""
    s = m.trunc_small()
    src = Source(s.data)
    for cut in range(len(s.data) + 1):
        check_stream(ctx, src, s.segs, "cut %d" % cut, s.data, src_len=cut)
        check_host_decoder(ctx, s.data[:cut], "cut %d" % cut)


def test_stream_cut_around_the_windows_end(ctx):
    s = m.trunc_window()
    src = Source(s.data)
    for cut in s.marks["cuts"]:
        check_stream(ctx, src, s.segs, "cut %d" % cut, s.data, src_len=cut)
        check_host_decoder(ctx, s.data[:cut], "cut %d" % cut)
