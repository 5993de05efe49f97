"""GPU parity tests of the flat DIRECT path's 16-byte form (rlev2_tiled_flat.hh,
kOptFlat16 / flat_expand16): full W=64 runs of a segment's leading chain are
loaded as aligned 16-byte chunks, shifted in registers by the payload's offset
mod 16 and stored two values per lane. Variant 2 (and the default for such
streams) has it, variant 10 is the same instance with the 8-byte form at every
width, variant 9 has no flat path at all.

Streams come from orc_amd.encode_runs, expected values from the CPU oracle on
the same bytes. Every test first proves on the CPU, from the encoded bytes and
the device pointers (`flat64`, a model of the prologue's rules), that it holds
the cases it means to hold, so that no test passes by never entering the path.

Needs a real MI355X: run with `pytest -m gpu`.
"""
import numpy as np
import pytest

from oracle import oracle
from rle_streams import DIRECT, direct_values, positions, walk

pytestmark = pytest.mark.gpu

VARIANTS = (0, 2, 10, 9)
BIG = 1 << 30  # a stride that makes the whole stream one segment
FLAT16_RUNS = 5  # ORCG_FLAT16_RUNS, the shipped runs in flight per wave
GUARD = 2  # output elements before and after the requested values
B64 = 2 + 512 * 8


def direct_stream(rng, spec, signed):
    """A stream of DIRECT runs, spec = [(W, L), ...]: (values, bytes, runs)."""
    import orc_amd

    v = np.concatenate([direct_values(rng, W, L, signed) for W, L in spec])
    data, _ = orc_amd.encode_runs(v, signed, [DIRECT] * len(spec), [L for _, L in spec])
    runs = walk(data)
    assert [(r[1], r[2], r[3]) for r in runs] == [(DIRECT, W, L) for W, L in spec]
    return v, data, runs


def flat64(runs, n, stride, ptr, src_len, begin=0, count=None):
    """The W=64 runs the prologue expands in 16-byte chunks, by its rules: per
    segment the leading chain of equal full DIRECT runs of W >= 40 that lie
    inside the requested values, end at or before the segment's end and (W=64)
    16 bytes or more before the end of the stream rounded up to 4 bytes.
    Returns [(segment, chain index, shift, output index)], shift = the
    payload's address mod 16."""
    end = begin + (n - begin if count is None else count)
    pos = positions(runs, n, stride).astype(np.int64)
    by_off = {r[0]: i for i, r in enumerate(runs)}
    lim = ((ptr + src_len + 3) & ~3) - ptr
    out = []
    for g in range(len(pos)):
        vi = g * stride - pos[g, 1]
        if g + 1 < len(pos):
            seg_end, v_next = min(pos[g + 1, 0], src_len), (g + 1) * stride - pos[g + 1, 1]
        else:
            seg_end, v_next = src_len, 1 << 62
        if vi >= end or v_next <= begin:
            continue
        vstop, i, first, k = min(v_next, end), by_off[pos[g, 0]], None, 0
        while i < len(runs) and vi >= begin:
            off, kind, W, L, size = runs[i]
            if not (kind == DIRECT and L == 512 and W >= 40) or (first is not None and W != first):
                break
            if vi + 512 > vstop or off + size > seg_end or off + size > lim - (16 if W == 64 else 4):
                break
            if W == 64:
                out.append((g, k, (ptr + off + 2) % 16, vi - begin))
            first, vi, i, k = W, vi + 512, i + 1, k + 1
    return out


class Gpu:
    """One stream on the device at byte `src_offset` of its allocation,
    decoded under a pinned variant into an output with guard elements."""

    def __init__(self, data, runs, n, signed, src_offset=0, src_len=None):
        import torch

        self.n, self.signed, self.runs = n, signed, runs
        self.len = int(data.size) if src_len is None else src_len
        buf = torch.zeros(data.size + src_offset + 64, dtype=torch.uint8)
        buf[src_offset:src_offset + data.size] = torch.from_numpy(data)
        self.buf = buf.cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.src = self.buf[src_offset:]
        self.ptr = self.src.data_ptr()
        self.pos = {}

    def flat64(self, stride, begin=0, count=None):
        return flat64(self.runs, self.n, stride, self.ptr, self.len, begin, count)

    def decode(self, variant, stride, value_begin=0, count=None, out_offset=0):
        import torch

        import orc_amd

        count = self.n - value_begin if count is None else count
        if stride not in self.pos:
            self.pos[stride] = torch.from_numpy(positions(self.runs, self.n, stride).view(np.int64)).cuda()
        ctx = orc_amd.default_context(0)
        lo = GUARD + out_offset
        out = torch.full((lo + count + GUARD,), -7, dtype=torch.int64, device="cuda")
        assert out.data_ptr() % 16 == 0
        ctx.set_rlev2_variant(variant)
        try:
            orc_amd.decode_positions_device(ctx, self.src, self.pos[stride], stride, count, self.signed,
                                            out[lo:lo + count], value_begin=value_begin, src_len=self.len)
            ctx.synchronize()
        finally:
            ctx.set_rlev2_variant(0)
        got = out.cpu().numpy()
        assert (got[:lo] == -7).all() and (got[lo + count:] == -7).all()  # both guard regions unchanged
        return got[lo:lo + count]


def test_variant_10_is_listed():
    import orc_amd

    assert {2, 9, 10} <= set(orc_amd.rlev2_variants())


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_every_shift_and_output_alignment(signed):
    """9 W=64 runs in one segment (the payload's shift steps by 2 from run to
    run), the stream at allocation offsets 0-15: every shift 0-15, each with
    the output 16-byte aligned (out[2:]) and 8 mod 16 (out[3:])."""
    rng = np.random.default_rng(41 + signed)
    v, data, runs = direct_stream(rng, [(64, 512)] * 9 + [(64, 77)], signed)
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, signed)
    np.testing.assert_array_equal(want, v)
    shifts = set()
    for src_offset in range(16):
        g = Gpu(data, runs, n, signed, src_offset=src_offset)
        assert g.ptr % 16 == src_offset
        f = g.flat64(BIG)
        assert [x[1] for x in f] == list(range(9))  # all nine runs, one chain
        assert [x[2] for x in f] == [(src_offset + 2 + 2 * k) % 16 for k in range(9)]
        shifts |= {x[2] for x in f}
        for out_offset in (0, 1):
            for variant in VARIANTS:
                got = g.decode(variant, BIG, out_offset=out_offset)
                np.testing.assert_array_equal(
                    got, want, err_msg="src offset %d out offset %d variant %d" % (src_offset, out_offset, variant))
    assert shifts == set(range(16))  # s = 0 (nothing of chunk 256 is used) and s = 15 among them


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_chain_lengths(signed):
    """Chains of 1 .. 4 * R + 1 runs (R runs in flight in each of the 4 waves:
    every mix of full batches, a short batch and no work), cut out of one
    stream by the value count, and one chain of 70 runs (two probes)."""
    rng = np.random.default_rng(43 + signed)
    v, data, runs = direct_stream(rng, [(64, 512)] * 70 + [(64, 77)], signed)
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, signed)
    np.testing.assert_array_equal(want, v)
    g = Gpu(data, runs, n, signed, src_offset=3)
    assert [x[1] for x in g.flat64(BIG)] == list(range(70))
    for variant in VARIANTS:
        np.testing.assert_array_equal(g.decode(variant, BIG), want, err_msg="70 runs, variant %d" % variant)
    for m in range(1, 4 * FLAT16_RUNS + 2):
        for count in (512 * m, 512 * m + 100):  # the chain ends at the output's end / a run that is cut follows
            assert [x[1] for x in g.flat64(BIG, 0, count)] == list(range(m))
            for variant in VARIANTS:
                np.testing.assert_array_equal(g.decode(variant, BIG, count=count), want[:count],
                                              err_msg="%d runs, count %d, variant %d" % (m, count, variant))


def test_reach():
    """The chunk loads read up to 15 bytes past a run: the last full run of a
    stream is taken flat only with 16 bytes or more of stream behind it. The
    stream ends at that run's last byte, or 1, 15, 16 bytes into the next
    run; the stream's end is 4-byte aligned, so the margin is those bytes."""
    import orc_amd

    rng = np.random.default_rng(47)
    v, data, runs = direct_stream(rng, [(64, 512)] * 6 + [(64, 300)], True)
    full = 6 * B64
    assert runs[6][0] == full
    nfull = 6 * 512
    want = oracle.rlev2_decode(data[:full].tobytes(), nfull, True)
    np.testing.assert_array_equal(want, v[:nfull])
    for tail in (0, 1, 15, 16):
        cut = full + tail
        g = Gpu(data[:cut], walk(data[:full]), nfull, True, src_offset=(-cut) % 4, src_len=cut)
        assert (g.ptr + cut) % 4 == 0
        f = g.flat64(BIG)
        assert [x[1] for x in f] == list(range(6 if tail == 16 else 5)), tail  # the last run: flat at 16 only
        for variant in VARIANTS:
            np.testing.assert_array_equal(g.decode(variant, BIG), want, err_msg="tail %d variant %d" % (tail, variant))
        if tail == 0:
            continue
        # one value of the cut run asked for: the same report from every instance
        g.runs, g.n, g.pos = runs, nfull + 1, {}
        status = {}
        for variant in VARIANTS:
            with pytest.raises(orc_amd.OrcError) as dev:
                g.decode(variant, BIG)
            status[variant] = (type(dev.value), str(dev.value))
        assert status[2] == status[10] == status[9] == status[0], tail


def test_mixed_widths():
    """W = 64, 56, 64, 40, 64, 64, 48 and a 511-value W=64 run in one segment:
    the 16-byte and the 8-byte form alternate, chain by chain."""
    rng = np.random.default_rng(53)
    spec = [(64, 512), (56, 512), (64, 512), (40, 512), (64, 512), (64, 512), (48, 512), (64, 511), (64, 512), (64, 9)]
    v, data, runs = direct_stream(rng, spec, True)
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, True)
    np.testing.assert_array_equal(want, v)
    for src_offset in (0, 5):
        g = Gpu(data, runs, n, True, src_offset=src_offset)
        # one segment: the prologue's chain is the first run; run by run (stride 512) each full run is a chain
        assert [x[1] for x in g.flat64(BIG)] == [0]
        assert [x[0] for x in g.flat64(512)] == [0, 2, 4, 5, 8]
        for stride in (BIG, 512, 1_024):
            for out_offset in (0, 1):
                for variant in VARIANTS:
                    got = g.decode(variant, stride, out_offset=out_offset)
                    np.testing.assert_array_equal(got, want, err_msg="stride %d variant %d" % (stride, variant))


def test_value_windows():
    """value_begin / count that start and end inside runs: a flat run's output
    pointer is 8 mod 16 when value_begin is odd."""
    rng = np.random.default_rng(59)
    v, data, runs = direct_stream(rng, [(64, 512)] * 40 + [(64, 77)], True)
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, True)
    g = Gpu(data, runs, n, True, src_offset=1)
    odd = even = 0
    windows = ((700, 5_000), (0, 1_000), (512, 1_024), (10_001, 10_000), (20_479, 1), (0, 1), (9_999, 10_500),
               (1, 20_000), (0, 20_000), (9_728, 6_000))
    for begin, count in windows:
        for stride in (BIG, 10_000):
            assert begin + count <= n
            f = g.flat64(stride, begin, count)
            odd += sum(x[3] % 2 for x in f)
            even += sum(1 - x[3] % 2 for x in f)
            for variant in VARIANTS:
                got = g.decode(variant, stride, value_begin=begin, count=count)
                np.testing.assert_array_equal(got, want[begin:begin + count],
                                              err_msg="begin %d count %d stride %d variant %d" % (begin, count, stride, variant))
    assert odd >= 10 and even >= 10  # flat W=64 runs at both output alignments
