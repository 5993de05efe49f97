"""The host stream planners (orcg_rlev2 / rlev1 / byterle_plan_create) against
one cut rule written here: a plan's segments, decodable values and first error
are compared exactly, for whole, truncated and corrupt streams of each format.
The groups of a stream come from the tests' models (rle_streams.walk,
rlev1_model.groups, byterle_model.headers); the rule and its three per-format
policies are `cut_plan` below. No GPU calls are made here."""
import numpy as np
import pytest

import byterle_model as bm
import orc_amd
import rle_streams
import rlev1_model as v1
from orc_amd import _lib
from rlev1_writer import encode as v1_encode

# (max_bytes, max_values); (0, 0) = the defaults
LIMITS = [(512, 700), (1 << 30, 1), (1, 1 << 40), (0, 0)]
V2_READ = "bad read in RleDecoderV2::readByte"
V1_READ = "bad read in readByte"
BYTE_READ = "bad read in nextBuffer"

# What a planner does with the group its walk fails at, when the cut
# condition holds there:
NEVER, ALWAYS, IF_DELIVERS = "never", "always", "if it delivers values"
FORMATS = {
    # RLEv2 cuts only after a run has parsed: a bad run delivers nothing
    "v2": (orc_amd.Plan, 8192, NEVER),
    # RLEv1 cuts before it parses the group, so a bad group has its segment
    "v1": (orc_amd.V1Plan, 8192, ALWAYS),
    # byte RLE cuts at a literal the stream's end cuts only if bytes of it are there
    "byte": (orc_amd.BytePlan, 16384, IF_DELIVERS),
}


def cut_plan(groups, bad, max_bytes, max_values, at_bad):
    """groups: (offset, values) of the whole groups before the first bad one;
    bad: None or (offset, values the cut group still delivers, message).
    Returns (segments, values, error)."""
    segs, vi, seg = [], 0, None

    def due(pos):
        return seg is None or pos - seg[0] >= max_bytes or vi - seg[1] >= max_values

    for off, n in groups:
        if due(off):
            seg = (off, vi)
            segs.append(seg)
        vi += n
    if bad is None:
        return segs, vi, None
    off, partial, msg = bad
    if due(off) and (at_bad == ALWAYS or (at_bad == IF_DELIVERS and partial)):
        segs.append((off, vi))
    vi += partial
    return segs, vi, (_lib.ORCG_PARSE_ERROR, vi, msg)


def check(fmt, data, groups, bad):
    cls, default_values, at_bad = FORMATS[fmt]
    for mb, mv in LIMITS:
        plan = cls(bytes(data), mb, mv)
        segs, values, err = cut_plan(groups, bad, mb or 16 << 10, mv or default_values, at_bad)
        got = [tuple(int(x) for x in s) for s in plan.segments()]
        assert got == segs, (fmt, mb, mv, len(data), bad)
        assert plan.values == values, (fmt, mb, mv, len(data), bad)
        assert plan.error() == err, (fmt, mb, mv, len(data), bad)
        assert values < 10_000


# ---- RLEv2 ------------------------------------------------------------------
def v2_groups(data):
    return [(r[0], r[3]) for r in rle_streams.walk(data)]


def _one_run(rng, kind, n):
    if kind == 0:
        return np.full(n, int(rng.integers(-1000, 1000)), dtype=np.int64)
    if kind == 1:
        return rng.integers(-(1 << 30), 1 << 30, size=n).astype(np.int64)
    if kind == 2:
        x = 1000 + rng.integers(0, 200, size=n).astype(np.int64)
        x[int(rng.integers(0, n))] += 1 << 25
        return x
    return (int(rng.integers(-10 ** 6, 10 ** 6)) + 37 * np.arange(n)).astype(np.int64)


def v2_mixed(seed, nruns):
    """A stream of nruns runs of random kinds, about 20 values each."""
    rng = np.random.default_rng(seed)
    kinds = [int(k) for k in rng.integers(0, 4, size=nruns)]
    lens = [int(rng.integers(3, 11)) if k == 0 else int(rng.integers(20, 40)) for k in kinds]
    v = np.concatenate([_one_run(rng, k, n) for k, n in zip(kinds, lens)])
    return orc_amd.encode_runs(v, True, kinds, lens)[0].tobytes(), kinds, lens


@pytest.fixture(scope="module")
def v2_mix():
    return v2_mixed(3, 40)[0]


LAST_RUNS = {
    "short_repeat": np.full(7, 100_000, dtype=np.int64),
    "direct": np.array([5, -70000, 12, 900, -3, 65000, 1, 77] * 3, dtype=np.int64),
    "patched_base": np.concatenate([np.arange(30) % 50, [1 << 28], np.arange(9)]).astype(np.int64) + 2000,
    "delta": 1_000_000 + np.cumsum(np.concatenate([[0], np.arange(500, 530)])),
    # the first value and the delta base take several bytes each, the deltas none
    "delta_fixed": 10 ** 12 + 70_000 * np.arange(25, dtype=np.int64),
}


def test_rlev2_mix():
    data, kinds, lens = v2_mixed(4, 400)
    groups = v2_groups(data)
    assert [n for _, n in groups] == lens and [r[1] for r in rle_streams.walk(data)] == kinds
    check("v2", data, groups, None)


@pytest.mark.parametrize("last", sorted(LAST_RUNS))
def test_rlev2_truncated_in_the_last_run(v2_mix, last):
    tail, _ = orc_amd.encode_runs(LAST_RUNS[last], True, [last.split("_fixed")[0]], [LAST_RUNS[last].size])
    data = v2_mix + tail.tobytes()
    groups = v2_groups(data)
    assert groups[-1] == (len(v2_mix), LAST_RUNS[last].size)
    assert rle_streams.walk(data)[-1][1] == orc_amd.rle.KIND[last.split("_fixed")[0]]
    if last.startswith("delta"):
        assert data[len(v2_mix) + 3] >= 0x80  # the first varint has several bytes
    check("v2", data, groups, None)
    for cut in range(len(v2_mix) + 1, len(data)):
        check("v2", data[:cut], groups[:-1], (len(v2_mix), 0, V2_READ))


# a PATCHED_BASE run of one 1-bit value, a 1-byte base and one patch entry
# of 64 + 1 bits: the header, base and data are whole
PATCH_WIDE = bytes([0x80, 0x00, 0x1F, 0x01, 0x00, 0x00])
CORRUPT = [
    (bytes([0x8E, 0x09, 0x2B, 0x20]), "Corrupt PATCHED_BASE encoded data (pl==0)!"),
    (PATCH_WIDE, "Corrupt PATCHED_BASE encoded data (patchBitSize + pgw > 64)!"),
    (PATCH_WIDE[:5], V2_READ),  # its data byte is missing: the read fails first
    (bytes([0xC2, 0x00, 0x05, 0x02]), "Illegal run length for delta encoding: 1"),
]


@pytest.mark.parametrize("k", range(len(CORRUPT)))
def test_rlev2_corrupt_run(v2_mix, k):
    run, msg = CORRUPT[k]
    groups = v2_groups(v2_mix)
    check("v2", v2_mix + run, groups, (len(v2_mix), 0, msg))
    check("v2", run, [], (0, 0, msg))  # as the first run: no segment at all
    if msg != V2_READ:  # (bytes after the cut run would complete it)
        check("v2", run + v2_mix, [], (0, 0, msg))


def test_rlev2_empty():
    check("v2", b"", [], None)


# ---- RLEv1 ------------------------------------------------------------------
def v1_parts(data):
    """(whole groups, bad) of a stream from the model's groups."""
    gs = v1.groups(data, False)
    whole = [(g[0], len(g[2])) for g in gs if g[4]]
    bad = [(g[0], len(g[2]), V1_READ) for g in gs if not g[4]]
    return whole, (bad[0] if bad else None)


def test_rlev1_truncated_everywhere():
    data = v1.trunc_small().data
    assert v1_parts(data)[1] is None
    for cut in range(len(data) + 1):
        check("v1", data[:cut], *v1_parts(data[:cut]))


@pytest.mark.parametrize("head", [b"", v1_encode([("lit", [1, -2, 300]), ("run", 7, 1, 20)], True)[0]])
def test_rlev1_cut_groups(head):
    head = bytes(head)
    n = v1.decode(head, False)[1]
    whole = v1_parts(head)[0]
    # a run whose base varint is missing (after the header, after the delta) or unterminated
    for run in (bytes([5]), bytes([5, 1]), bytes([5, 1, 0x80]), bytes([5, 1, 0xFF, 0xFF])):
        check("v1", head + run, whole, (len(head), 0, V1_READ))
    # a literal group cut after k of its varints: err_at = values = its first value + k
    varints = [v1.varint(x) for x in (1, 300, 1 << 40, 5, 1 << 63, 77)]
    for k in (0, 1, len(varints) - 1):
        for rest in (b"", varints[k][:-1]):  # at a varint's end, and inside the next
            data = head + bytes([256 - len(varints)]) + b"".join(varints[:k]) + rest
            assert v1_parts(data) == (whole, (len(head), k, V1_READ))
            check("v1", data, whole, (len(head), k, V1_READ))
            plan = orc_amd.V1Plan(data)
            assert plan.error()[1] == plan.values == n + k


def test_rlev1_first_group_bad_keeps_its_segment():
    plan = orc_amd.V1Plan(bytes([5, 1, 0x80]))
    assert plan.segments().tolist() == [[0, 0]] and plan.values == 0 and plan.error()[1] == 0


def test_rlev1_overlong_varint():
    data = v1.run_bytes(10, -1, v1.padded_varint(12345, 40)) + v1.lit_bytes([v1.padded_varint(9, 25), v1.varint(3)])
    data += v1.run_bytes(3, 0, v1.varint(1))
    whole, bad = v1_parts(data)
    assert bad is None and [n for _, n in whole] == [10, 2, 3]
    check("v1", data, whole, None)
    for cut in (20, 41, 42, 43, 60, len(data) - 1):
        check("v1", data[:cut], *v1_parts(data[:cut]))


def test_rlev1_empty():
    check("v1", b"", [], None)


# ---- byte RLE ---------------------------------------------------------------
def byte_parts(data):
    whole = [(g[0], g[2]) for g in bm.walk(data)]
    hs = bm.headers(data)
    if not hs or hs[-1][0] + hs[-1][3] <= len(data):
        return whole, None
    off, kind = hs[-1][0], hs[-1][1]
    return whole, (off, len(data) - off - 1 if kind == bm.LIT else 0, BYTE_READ)


def test_byterle_truncated_everywhere():
    data = bm.trunc_small().data
    assert byte_parts(data)[1] is None
    for cut in range(len(data) + 1):
        check("byte", data[:cut], *byte_parts(data[:cut]))


@pytest.mark.parametrize("head", [b"", bm.lit(b"\x01\x02\x03") + bm.run(40, 9)])
def test_byterle_cut_groups(head):
    """With `head` the cut condition holds at the cut group under the limits
    (1 << 30, 1) and (1, 1 << 40) and not under the others; without it the
    group opens the stream and it holds under all."""
    whole = byte_parts(head)[0]
    n = sum(k for _, k in whole)
    # a run header as the last byte fails at its first value
    check("byte", head + bytes([7]), whole, (len(head), 0, BYTE_READ))
    assert orc_amd.BytePlan(head + bytes([7])).error()[1] == n
    payload = bytes(range(10, 30))
    for have in (0, 1, len(payload) - 1):
        data = head + bytes([256 - len(payload)]) + payload[:have]
        check("byte", data, whole, (len(head), have, BYTE_READ))
        for mb, mv in LIMITS:
            holds = not head or (mb, mv) in LIMITS[1:3]
            segs = orc_amd.BytePlan(data, mb, mv).segments().tolist()
            assert ([len(head), n] in segs) == (have > 0 and holds), (have, mb, mv)


def test_byterle_empty():
    check("byte", b"", [], None)
