"""GPU parity tests of the flat DIRECT path (rlev2_tiled_flat.hh, kOptFlat): a
segment's leading chain of full 512-value DIRECT runs of one width >= 40 bits
is validated by one header probe and expanded straight from memory, the rest
of the segment goes through the windowed walk. Variant 2 (and the default for
such streams) has the path, variant 9 is the same instance without it.

Streams come from orc_amd.encode_runs / encode_direct, expected values from
the CPU oracle on the same bytes. Every test first checks on the CPU, from
the encoded bytes, that the stream holds the eligible / ineligible runs it
means to hold, so that no test passes by never entering the path.

Needs a real MI355X: run with `pytest -m gpu`.
"""
import numpy as np
import pytest

from oracle import oracle
from rle_streams import DELTA, DIRECT, PATCHED, SR, direct_values, positions, walk

pytestmark = pytest.mark.gpu

VARIANTS = (0, 2, 9)
BIG = 1 << 30  # a stride that makes the whole stream one segment


def eligible(run):
    _, kind, W, L, _ = run
    return kind == DIRECT and L == 512 and W >= 40


def direct_stream(rng, spec, signed):
    """A stream of DIRECT runs, spec = [(W, L), ...]: (values, bytes, runs)."""
    import orc_amd

    v = np.concatenate([direct_values(rng, W, L, signed) for W, L in spec])
    data, _ = orc_amd.encode_runs(v, signed, [DIRECT] * len(spec), [L for _, L in spec])
    runs = walk(data)
    assert [(r[1], r[2], r[3]) for r in runs] == [(DIRECT, W, L) for W, L in spec]
    return v, data, runs


class Gpu:
    """One stream on the device, decoded under a pinned variant."""

    def __init__(self, data, runs, n, signed, src_offset=0):
        import torch

        self.n, self.signed, self.runs, self.len = n, signed, runs, int(data.size)
        buf = torch.zeros(data.size + src_offset + 64, dtype=torch.uint8)
        buf[src_offset:src_offset + data.size] = torch.from_numpy(data)
        self.src = buf.cuda()[src_offset:]
        self.pos = {}

    def decode(self, variant, stride, value_begin=0, count=None, dtype=None, out_offset=0, pos=None, src_len=None):
        import torch

        import orc_amd

        count = self.n - value_begin if count is None else count
        if pos is None:
            if stride not in self.pos:
                self.pos[stride] = torch.from_numpy(positions(self.runs, self.n, stride).view(np.int64)).cuda()
            pos = self.pos[stride]
        ctx = orc_amd.default_context(0)
        out = torch.full((count + out_offset,), -7, dtype=dtype or torch.int64, device="cuda")
        ctx.set_rlev2_variant(variant)
        try:
            orc_amd.decode_positions_device(ctx, self.src, pos, stride, count, self.signed, out[out_offset:],
                                            value_begin=value_begin, src_len=self.len if src_len is None else src_len)
            ctx.synchronize()
        finally:
            ctx.set_rlev2_variant(0)
        got = out.cpu().numpy()
        assert (got[:out_offset] == -7).all()  # nothing stored before the output
        return got[out_offset:]


def test_variant_9_is_listed():
    import orc_amd

    assert {2, 9} <= set(orc_amd.rlev2_variants())


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("W", [40, 48, 56, 64])
def test_periodic(W, signed):
    """70 equal runs: segments that start inside a run (stride 10,000), one
    run per segment (512), one segment of 70 runs (more than one probe)."""
    rng = np.random.default_rng(W + signed)
    v, data, runs = direct_stream(rng, [(W, 512)] * 70, signed)
    n = v.size
    assert n == 35_840 and all(eligible(r) for r in runs)
    B = 2 + 64 * W
    assert [r[0] for r in runs] == [k * B for k in range(70)]  # header k sits at k * B
    p10k = positions(runs, n, 10_000)
    assert (p10k[1:, 1] > 0).all()  # the later segments start inside a run
    assert (np.diff(positions(runs, n, 512)[:, 0].astype(np.int64)) == B).all()
    want = oracle.rlev2_decode(data.tobytes(), n, signed)
    np.testing.assert_array_equal(want, v)
    g = Gpu(data, runs, n, signed)
    for stride in (10_000, 512, BIG):
        for variant in VARIANTS:
            np.testing.assert_array_equal(g.decode(variant, stride), want, err_msg="stride %d variant %d" % (stride, variant))


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_header_change_inside_segment(signed):
    """Widths change from run to run, a run of 511 and one of 300 sit in the
    middle and the last run is partial: the chain stops at each of them."""
    rng = np.random.default_rng(5)
    spec = [(64, 512)] * 3 + [(48, 512)] * 2 + [(64, 512), (56, 512), (56, 512), (64, 511), (64, 512), (64, 512),
                                                   (40, 512), (64, 300), (64, 512), (64, 512), (48, 512), (64, 77)]
    v, data, runs = direct_stream(rng, spec, signed)
    assert sum(eligible(r) for r in runs) == len(spec) - 3
    assert [eligible(r) for r in runs][8] is False and runs[-1][3] == 77
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, signed)
    np.testing.assert_array_equal(want, v)
    g = Gpu(data, runs, n, signed)
    for stride in (BIG, 3_000):
        for variant in VARIANTS:
            np.testing.assert_array_equal(g.decode(variant, stride), want, err_msg="stride %d variant %d" % (stride, variant))


def _mixed_stream(rng):
    """Eligible W=64 runs with one DELTA, PATCHED_BASE, SHORT_REPEAT, 5-value
    DIRECT and W=32 DIRECT run between them."""
    import orc_amd

    def wide(k):
        return [(DIRECT, direct_values(rng, 64, 512, True)) for _ in range(k)]

    delta = np.cumsum(rng.integers(0, 1 << 12, size=512, dtype=np.int64)) + 1_000_000
    patched = rng.integers(0, 1 << 12, size=512, dtype=np.int64)
    patched[0] = 0
    patched[100] += 1 << 41
    parts = (wide(3) + [(DELTA, delta)] + wide(2) + [(PATCHED, patched)] + wide(2) +
             [(SR, np.full(7, -123_456_789, dtype=np.int64))] + wide(1) +
             [(DIRECT, direct_values(rng, 64, 5, True))] + wide(2) + [(DIRECT, direct_values(rng, 32, 512, True))] +
             wide(2))
    v = np.concatenate([p[1] for p in parts])
    data, _ = orc_amd.encode_runs(v, True, [p[0] for p in parts], [p[1].size for p in parts])
    return v, data, walk(data), [p[0] for p in parts]


def test_ineligible_runs_between_eligible_ones():
    rng = np.random.default_rng(9)
    v, data, runs, kinds = _mixed_stream(rng)
    assert [r[1] for r in runs] == kinds
    bad = [r for r in runs if not eligible(r)]
    assert sorted((r[1], r[2] if r[1] == DIRECT else 0, r[3]) for r in bad) == sorted(
        [(DELTA, 0, 512), (PATCHED, 0, 512), (SR, 0, 7), (DIRECT, 64, 5), (DIRECT, 32, 512)])
    assert sum(eligible(r) for r in runs) == 12 and eligible(runs[0]) and eligible(runs[-1])
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, True)
    np.testing.assert_array_equal(want, v)
    g = Gpu(data, runs, n, True)
    for stride in (BIG, 1_500):
        for variant in VARIANTS:
            np.testing.assert_array_equal(g.decode(variant, stride), want, err_msg="stride %d variant %d" % (stride, variant))


def test_false_match_further_on():
    """Runs of W = 64, 56, 64, ...: the bytes at 2 * 4098, where a third W=64
    run would start, are payload of the third run and equal the first header.
    The chain ends at the first mismatch (the second header)."""
    rng = np.random.default_rng(13)
    v, data, runs = direct_stream(rng, [(64, 512), (56, 512), (64, 512), (64, 512), (64, 512)], True)
    data = data.copy()
    at = 2 * 4098
    assert bytes(data[0:2]) == b"\x7f\xff"
    assert runs[1][0] == 4098 and bytes(data[4098:4100]) != b"\x7f\xff"
    assert runs[2][0] + 2 <= at and at + 2 <= runs[2][0] + runs[2][4]  # inside the third run's payload
    data[at], data[at + 1] = 0x7F, 0xFF
    assert [(r[1], r[2], r[3]) for r in walk(data)] == [(r[1], r[2], r[3]) for r in runs]
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, True)
    assert (want != v).sum() == 1  # the payload stays valid: one value changed
    g = Gpu(data, runs, n, True)
    for variant in VARIANTS:
        np.testing.assert_array_equal(g.decode(variant, BIG), want, err_msg="variant %d" % variant)


def test_value_windows():
    """value_begin / nvalues that cut runs: the slice of the full decode."""
    rng = np.random.default_rng(17)
    v, data, runs = direct_stream(rng, [(64, 512)] * 40, True)
    assert all(eligible(r) for r in runs)
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, True)
    g = Gpu(data, runs, n, True)
    for begin, count in ((700, 5_000), (0, 1_000), (512, 1_024), (10_001, 10_000), (20_479, 1)):
        for stride in (BIG, 10_000):
            for variant in VARIANTS:
                got = g.decode(variant, stride, value_begin=begin, count=count)
                np.testing.assert_array_equal(got, want[begin:begin + count],
                                              err_msg="begin %d count %d stride %d variant %d" % (begin, count, stride, variant))


def test_truncated_periodic_stream():
    """A periodic stream cut inside the last run's payload, right after a
    header and one byte into a header: the reference's message from the host
    entry point, and the same status from every instance on the device."""
    import orc_amd

    rng = np.random.default_rng(19)
    v, data, runs = direct_stream(rng, [(64, 512)] * 20, True)
    assert all(eligible(r) for r in runs)
    n = v.size
    last = runs[-1][0]
    ctx = orc_amd.default_context(0)
    for cut in (last + 2 + 1_000, last + 2, last + 1):
        bad = data[:cut].tobytes()
        with pytest.raises(oracle.OracleError) as want:
            oracle.RleDecoderV2(bad, True).next(n)
        status = {}
        for variant in VARIANTS:
            ctx.set_rlev2_variant(variant)
            try:
                with pytest.raises(orc_amd.ParseError) as got:
                    orc_amd.rlev2_decode(bad, n, True)
            finally:
                ctx.set_rlev2_variant(0)
            assert str(got.value) == str(want.value), (cut, variant)
            # the device entry point, the whole stream one segment: the runs
            # before the cut decode, the cut one is reported
            g = Gpu(data[:cut], runs, n, True)
            with pytest.raises(orc_amd.OrcError) as dev:
                g.decode(variant, BIG)
            status[variant] = (type(dev.value), str(dev.value))
        assert status[2] == status[9] == status[0], cut


def test_positions_entry_inside_a_run():
    """A positions table whose second entry points into a run's payload: the
    same outcome with and without the path."""
    import torch

    import orc_amd

    rng = np.random.default_rng(23)
    v, data, runs = direct_stream(rng, [(64, 512)] * 40, True)
    assert all(eligible(r) for r in runs)
    n, stride = v.size, 10_000
    pos = positions(runs, n, stride)
    pos[1, 0] += 1_001  # inside the payload of the run that holds value 10,000
    assert runs[19][0] + 2 < pos[1, 0] < runs[20][0]
    d_pos = torch.from_numpy(pos.view(np.int64)).cuda()
    g = Gpu(data, runs, n, True)
    outcome = {}
    for variant in (2, 9):
        try:
            outcome[variant] = ("ok", g.decode(variant, stride, pos=d_pos).tobytes())
        except orc_amd.OrcError as e:
            outcome[variant] = (type(e).__name__, str(e))
    assert outcome[2] == outcome[9]


@pytest.mark.parametrize("src_offset", [1, 2, 3])
def test_unaligned_pointers(src_offset):
    """The stream at byte offsets 1, 2, 3 of its allocation (src_len passed),
    the output at out[1:]."""
    rng = np.random.default_rng(29 + src_offset)
    v, data, runs = direct_stream(rng, [(64, 512)] * 9 + [(40, 512)] * 9 + [(56, 512)] * 9 + [(48, 512)] * 9, True)
    assert all(eligible(r) for r in runs)
    n = v.size
    want = oracle.rlev2_decode(data.tobytes(), n, True)
    g = Gpu(data, runs, n, True, src_offset=src_offset)
    assert g.src.data_ptr() % 4 == src_offset
    for stride in (BIG, 10_000):
        for variant in VARIANTS:
            got = g.decode(variant, stride, out_offset=1)
            np.testing.assert_array_equal(got, want, err_msg="stride %d variant %d" % (stride, variant))


@pytest.mark.parametrize("dtype", ["int32", "int16"])
def test_narrow_outputs(dtype):
    """int32 / int16 outputs (the path is compiled for int64 outputs only):
    the periodic and the header-change streams still decode, narrowed."""
    import torch

    rng = np.random.default_rng(31)
    tdt = getattr(torch, dtype)
    for spec in ([(64, 512)] * 30, [(64, 512)] * 3 + [(48, 512)] * 2 + [(64, 511), (56, 512), (64, 300), (40, 512), (64, 9)]):
        v, data, runs = direct_stream(rng, spec, True)
        assert sum(eligible(r) for r in runs) >= len(spec) - 3
        n = v.size
        want = oracle.rlev2_decode(data.tobytes(), n, True).astype(dtype)
        g = Gpu(data, runs, n, True)
        for stride in (BIG, 10_000):
            for variant in VARIANTS:
                got = g.decode(variant, stride, dtype=tdt)
                np.testing.assert_array_equal(got, want, err_msg="stride %d variant %d" % (stride, variant))
