"""rlev1_kernel against the exact model of tests/rlev1_model.py at the
stream shapes where its steps can go wrong: group headers around the window's
kChunk, varints across chunk, block, tail and tail-pass edges, windows of as
many groups or runs as the tables hold, every run length around kLaneRun,
groups longer than a window (the serial path), streams cut at every byte and
around the windows' ends with live bytes after the cut, output ranges and
widths, and segment tables with one group a segment, empty segments and
entries that are not group aligned.

Everything goes through orcg_rlev1_decode_device, so the test sets the
segment table (and with it the chunk width), the output width and range and
the source pointer's low four bits. Outputs are pre-filled with a sentinel and
carry guard elements on both sides; every comparison is exact.
tests/test_rlev1_model_cpu.py proves on the CPU that the model agrees with
the oracle on these streams and that each holds its feature where it says.

Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import orc_amd
import rlev1_model as m

pytestmark = pytest.mark.gpu

READ_ERROR = "bad read in readByte"
SEGMENT_ERROR = "Stream position is not at a run boundary"
GUARD = 64
SENTINEL = {8: 0x5A5A5A5A5A5A5A5A, 4: 0x5A5A5A5A, 2: 0x5A5A}
OFFS = (0, 1, 15)


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


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

    def decode(self, ctx, signed, segs, begin, count, dst_bytes=8, src_len=None):
        """(the output range, the error Context.synchronize reports or None)."""
        import torch

        L = orc_amd.rle._lib.load()
        src_len = self.len if src_len is None else src_len
        table = torch.from_numpy(np.array(segs, dtype=np.uint64).reshape(-1, 2).view(np.int64)).cuda()
        dtype = {8: torch.int64, 4: torch.int32, 2: torch.int16}[dst_bytes]
        out = torch.full((count + 2 * GUARD,), SENTINEL[dst_bytes], dtype=dtype, device="cuda")
        orc_amd.rle.check(L.orcg_rlev1_decode_device(ctx.handle, self.dev.data_ptr(), src_len, int(signed),
                                                     table.data_ptr(), len(segs), begin, count,
                                                     out.data_ptr() + GUARD * dst_bytes, dst_bytes), ctx.last_error)
        err = None
        try:
            ctx.synchronize()
        except orc_amd.OrcError as e:
            err = e
        host = out.cpu().numpy()
        assert (host[:GUARD] == SENTINEL[dst_bytes]).all() and (host[GUARD + count:] == SENTINEL[dst_bytes]).all(), "guards"
        return host[GUARD:GUARD + count], err


def check_stream(ctx, src, signed, segs, label, whole, src_len=None):
    """The stream's producible values decode exactly and without an error;
    one more value gives the reference's error after the same values."""
    src_len = src.len if src_len is None else src_len
    segs = [s for s in segs if s[0] < src_len] or [(0, 0)]
    want, n = m.decode(whole[:src_len], signed)
    if n:
        got, err = src.decode(ctx, signed, segs, 0, n, src_len=src_len)
        assert err is None, (label, err)
        np.testing.assert_array_equal(got, want, err_msg=label)
    got, err = src.decode(ctx, signed, segs, 0, n + 1, src_len=src_len)
    assert isinstance(err, orc_amd.ParseError) and READ_ERROR in str(err), (label, err)
    np.testing.assert_array_equal(got[:n], want, err_msg=label + " before the error")
    assert got[n] == SENTINEL[8], label
    return want


def check_shape(ctx, s, label):
    return check_stream(ctx, Source(s.data, s.off), s.signed, s.segs, label, s.data)


# ---- window, chunk, block and tail edges -----------------------------------
@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("kind", m.EDGE_KINDS)
def test_group_header_around_the_window_edge(ctx, kind, off, cb):
    """A run whose delta and base lie in the tail, a run with a 10-byte base
    and the longest legal group, with the header at window bytes kChunk - 18
    .. kChunk - 1 and at kChunk (where it opens the next window)."""
    for d in m.EDGE_D:
        check_shape(ctx, m.window_edge(kind, d, off, cb), "%s d=%s off=%d cb=%d" % (kind, d, off, cb))


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", (0, 15))
def test_ten_byte_varints_at_every_phase(ctx, off, cb):
    """10-byte literal varints across thread-chunk and block edges, kChunk
    and kChunk + 1024 at each of their nine split points."""
    for j in range(10):
        check_shape(ctx, m.literal_phases(j, off, cb), "phase %d off=%d cb=%d" % (j, off, cb))


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", (0, 15))
@pytest.mark.parametrize("nbytes", m.PADDED)
def test_padded_varints_across_chunk_edges(ctx, nbytes, off, cb):
    """Varints longer than 10 bytes (payload first, bit 63 set): the resume
    from the 16 bytes before a chunk, and the byte loop past 16."""
    check_shape(ctx, m.padded_literals(nbytes, off, cb), "padded %d off=%d cb=%d" % (nbytes, off, cb))


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", (0, 15))
def test_literal_ending_on_a_chunk_edge(ctx, off, cb):
    check_shape(ctx, m.literal_ends(off, cb), "ends off=%d cb=%d" % (off, cb))


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", (0, 15))
@pytest.mark.parametrize("kind", m.DENSE)
def test_dense_windows(ctx, kind, off, cb):
    """Windows of kMaxGroups 2-byte literals, of kMaxRuns 3-byte runs, and of
    as many 130-value runs (the long-run list full)."""
    check_shape(ctx, m.dense(kind, off, cb), "dense %s off=%d cb=%d" % (kind, off, cb))


# ---- runs --------------------------------------------------------------------
@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_run_lengths_deltas_and_bases(ctx, signed, cb):
    """Lengths around kLaneRun and the wave size x deltas -128 .. 127 x bases
    at the extremes (runs wrap mod 2^64), canonical and padded."""
    check_shape(ctx, m.run_matrix(signed, cb), "runs signed=%s cb=%d" % (signed, cb))


@pytest.mark.parametrize("cb", m.WIDTHS)
def test_500_runs_of_10(ctx, cb):
    check_shape(ctx, m.runs_of_10(cb), "runs of 10 cb=%d" % cb)


# ---- groups longer than a window ----------------------------------------------
@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("where", m.LONG_WHERE)
@pytest.mark.parametrize("kind", m.LONG_KINDS)
def test_group_longer_than_a_window(ctx, kind, where, cb):
    """The serial path for a literal and for a run: first in its segment,
    after ordinary groups (the window restarts at it), followed by ordinary
    groups, and cut by the stream's end (the error at the model's index)."""
    check_shape(ctx, m.long_group(kind, where, cb), "long %s %s cb=%d" % (kind, where, cb))


# ---- truncation ------------------------------------------------------------------
def test_small_stream_cut_at_every_byte(ctx):
    """Host buffers of exactly the cut's length, and the device buffer that
    still holds the rest of the stream behind src_len = cut: live terminators
    within the descriptor's rounded-up dword."""
    s = m.trunc_small()
    src = Source(s.data)
    for cut in range(len(s.data) + 1):
        want = check_stream(ctx, src, True, s.segs, "cut %d" % cut, s.data, src_len=cut)
        if want.size:
            np.testing.assert_array_equal(orc_amd.rlev1_decode(s.data[:cut], want.size, True, ctx=ctx), want)
        with pytest.raises(orc_amd.ParseError, match=READ_ERROR):
            orc_amd.rlev1_decode(s.data[:cut], want.size + 1, True, ctx=ctx)


@pytest.mark.parametrize("cb", m.WIDTHS)
def test_long_stream_cut_around_its_windows_ends(ctx, cb):
    s = m.trunc_long(cb)
    src = Source(s.data)
    for cut in s.marks["cuts"]:
        want = check_stream(ctx, src, True, s.segs, "cut %d cb=%d" % (cut, cb), s.data, src_len=cut)
        np.testing.assert_array_equal(orc_amd.rlev1_decode(s.data[:cut], want.size, True, ctx=ctx), want)
        with pytest.raises(orc_amd.ParseError, match=READ_ERROR):
            orc_amd.rlev1_decode(s.data[:cut], want.size + 1, True, ctx=ctx)


# ---- output ranges and widths ------------------------------------------------------
@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("dst_bytes", (8, 4, 2))
def test_output_ranges_and_widths(ctx, dst_bytes, cb):
    s = m.range_stream(cb)
    src = Source(s.data)
    want = m.truncate(m.decode(s.data, True)[0], dst_bytes)
    assert s.marks["ranges"]
    for begin, count in s.marks["ranges"]:
        got, err = src.decode(ctx, True, s.segs, begin, count, dst_bytes=dst_bytes)
        assert err is None, (begin, count, err)
        np.testing.assert_array_equal(got, want[begin:begin + count], err_msg="range %d + %d" % (begin, count))


def test_host_decode_to_int32(ctx):
    s = m.range_stream(16)
    vals = m.decode(s.data, True)[0]
    got = orc_amd.rlev1_decode(s.data, vals.size, True, dtype=np.int32, ctx=ctx)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, m.truncate(vals, 4))
    rng = np.random.default_rng(43)
    nn = (rng.random(vals.size * 2) < 0.5).astype(np.uint8)
    nn[np.flatnonzero(nn)[vals.size:]] = 0
    out = np.full(nn.size, 0x5A5A5A5A, dtype=np.int32)
    got = orc_amd.rlev1_decode(s.data, nn.size, True, not_null=nn, ctx=ctx, out=out)
    np.testing.assert_array_equal(got[nn.astype(bool)], m.truncate(vals[:int(nn.sum())], 4))
    assert (got[~nn.astype(bool)] == 0x5A5A5A5A).all()


# ---- segment tables ---------------------------------------------------------------------
@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("empty", [False, True], ids=["a group a segment", "with empty segments"])
def test_one_group_per_segment(ctx, empty, cb):
    data, segs = m.grouped(cb, empty)
    assert len(data) <= 66_000 and (len(set(segs)) < len(segs)) == empty
    check_stream(ctx, Source(data), True, segs, "cb=%d" % cb, data)


@pytest.mark.parametrize("cb", m.WIDTHS)
def test_table_that_is_not_group_aligned_is_reported(ctx, cb):
    """Error reports, not faults: a group-aligned offset whose value index is
    off by one, and an entry inside the previous segment's last group (the
    values asked for end at that group, so the later segment decodes
    nothing). The context decodes the stream afterwards."""
    data, segs = m.grouped(cb)
    src = Source(data)
    want, n = m.decode(data, True)
    for k in (1, len(segs) // 2):
        for by in (1, -1):
            bad = list(segs)
            bad[k] = (bad[k][0], bad[k][1] + by)
            _, err = src.decode(ctx, True, bad, 0, n)
            assert isinstance(err, orc_amd.InvalidArgument) and SEGMENT_ERROR in str(err), (k, by, err)
    sizes = {g[0]: g[3] for g in m.walk(data)}
    for k in (0, 5):
        off, vi = segs[k]
        assert sizes[off] >= 3
        bad = list(segs)
        bad[k + 1] = (off + sizes[off] // 2, segs[k + 1][1])
        _, err = src.decode(ctx, True, bad, 0, segs[k + 1][1])
        assert isinstance(err, orc_amd.InvalidArgument) and SEGMENT_ERROR in str(err), (k, err)
    got, err = src.decode(ctx, True, segs, 0, n)
    assert err is None
    np.testing.assert_array_equal(got, want)
