"""Stream-shape edges of the DECIMAL varint decode (decimal_kernels.hip)
against tests/decimal_model.py, an exact Python-int model written apart from
the kernel (tests/test_decimal_model_cpu.py holds it to the reference's known
answers and to the C oracle).

The kernel cuts the DATA stream blindly into 4096-byte tiles of 256 threads x
16 bytes; a varint belongs to the thread that holds its terminator and is
rebuilt from a 64-byte LDS look-back, past that from global memory; ranks
come from a wave scan plus a tile scan; up to 4096 values a tile are staged
in LDS. The shapes below sit on each of those edges. Every comparison is
exact, every output is allocated with 64 sentinel elements past nvalues, and
the scales array is exactly nvalues long and ends where its device allocation
ends, with poison before it.

The C ABI reports an error's message, not its value index, so "the first bad
value's error" is pinned by decoding prefixes: up to the bad value decodes,
one value more raises.
"""
import decimal
import re

import numpy as np
import pytest

import decimal_model as dm
from oracle import oracle

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3)
N_BIG = 3 * dm.TILE + 5
SLACK = 64
SENTINEL = 0x5A5A5A5A5A5A5A5A
POISON_SCALE = 1 << 20  # a scale no column is within 18 digits of
# torch hands out device blocks above 10 MiB as allocations of their own,
# rounded to 2 MiB: the last element of such a tensor is the allocation's last
TAIL_BYTES = 12 << 20
_tail = {}


def _scales_at_end(scales):
    import torch

    buf = _tail.get("buf")
    if buf is None:
        buf = _tail["buf"] = torch.full((TAIL_BYTES // 8,), POISON_SCALE, dtype=torch.int64, device="cuda")
        assert buf.untyped_storage().nbytes() == TAIL_BYTES
    sc = np.ascontiguousarray(scales, dtype=np.int64)
    n = sc.size
    buf[buf.numel() - n - 64:] = POISON_SCALE
    view = buf[buf.numel() - n:]
    if n:
        view.copy_(torch.from_numpy(sc))
    assert view.data_ptr() + 8 * n == buf.data_ptr() + TAIL_BYTES
    return view


def _run(data, scales, n, col_scale, mode):
    """One device decode: int64[n] / int64[n, 2] (and keep uint8[n] in mode
    3). Raises what the decode raises; asserts the sentinels past n."""
    import torch

    import orc_amd

    assert len(scales) == n
    ctx = orc_amd.default_context(0)
    d_src = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8).cuda()
    d_sc = _scales_at_end(scales)
    width = 2 if mode else 1
    out = torch.full(((n + SLACK) * width,), SENTINEL, dtype=torch.int64, device="cuda")
    keep = torch.full((n + SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    if mode < 2:
        orc_amd.decimal_decode_device(ctx, d_src, d_sc, n, 18 if mode == 0 else 38, col_scale, out, src_len=len(data))
    else:
        L = orc_amd._lib.load()
        ctx.after_torch()
        orc_amd._lib.check(L.orcg_hive11_decimal_decode_device(
            ctx.handle, d_src.data_ptr(), len(data), d_sc.data_ptr(), n, col_scale, int(mode == 2), out.data_ptr(),
            keep.data_ptr() if mode == 3 else None), ctx.last_error)
    got, k = out.cpu().numpy(), keep.cpu().numpy()
    assert (got[n * width:] == SENTINEL).all(), "values written past nvalues"
    if mode == 3:
        assert (k[n:] == 0xA5).all(), "keep written past nvalues"
    else:
        assert (k == 0xA5).all(), "keep written in a mode without one"
    got = got[:n * width].reshape((n, 2) if mode else (n,))
    return (got, k[:n]) if mode == 3 else got


def _assert_equal(got, want, mode, ctx=""):
    if mode == 3:
        assert set(np.unique(got[1])) <= {0, 1}, ctx
        np.testing.assert_array_equal(got[1], want[1], err_msg=ctx)
        got, want = got[0], want[0]
    np.testing.assert_array_equal(got, want, err_msg=ctx)


def _check(data, scales, n, col_scale, mode, witness=False, ctx=""):
    """The device gives what the model gives: the same arrays ("equal") or
    the same error message ("raised")."""
    import orc_amd

    try:
        want = dm.decode(data, scales, n, col_scale, mode)
    except dm.ModelError as e:
        with pytest.raises(orc_amd.ParseError, match=re.escape(str(e))):
            _run(data, scales, n, col_scale, mode)
        return "raised"
    _assert_equal(_run(data, scales, n, col_scale, mode), want, mode, ctx)
    if witness:
        o = oracle.decimal_decode_keep(data, scales, n, col_scale) if mode == 3 else \
            oracle.decimal_decode(data, scales, n, col_scale, mode)
        _assert_equal(o, want, mode, ctx + " (oracle)")
    return "equal"


def _scales(n, col_scale, mode, rng):
    """Spread scales; mode 2 gets divides only, so that a stream whose
    unscaled values are in range decodes instead of raising."""
    if mode == 2:
        return (col_scale + rng.integers(0, 41, size=n)).astype(np.int64)
    return dm.spread_scales(n, col_scale, mode, rng)


def _mixed(n, mode, rng):
    """mixed(); for the Hive modes a stream they accept (at most 17 bytes of
    payload, zeros of at most 19 bytes)."""
    if mode >= 2:
        return dm.mixed(n, True, rng, max_len=17, max_pad=18)
    return dm.mixed(n, mode == 1, rng)


@pytest.mark.parametrize("n", [dm.TILE - 1, dm.TILE, dm.TILE + 1, N_BIG])
@pytest.mark.parametrize("mode", MODES)
def test_dense_tiles(mode, n):
    """Tiles full of one-byte varints: 4096 values a tile, every LDS stage
    slot and all 16 preloaded scales of every thread in use."""
    data = dm.dense(n)
    rng = np.random.default_rng(n + mode)
    assert _check(data, np.full(n, 2, dtype=np.int64), n, 2, mode, witness=True) == "equal"
    assert _check(data, _scales(n, 2, mode, rng), n, 2, mode, witness=True) == "equal"
    if mode >= 2:  # scaled up by as much as 10^40: overflows (raise / keep 0)
        _check(data, dm.spread_scales(n, 40, mode, rng), n, 40, mode, witness=True)


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("mode", MODES)
def test_tile_edge_lengths(mode, k):
    """Streams of 4096k - 1, 4096k and 4096k + 1 bytes. Once the last varint
    is one byte ending at len; once it is a 6-byte varint ending at len, which
    at 4096k + 1 straddles the last tile edge with one byte in a tile of its
    own, at 4096k ends flush with the tile and at 4096k - 1 one byte short."""
    rng = np.random.default_rng(10 * k + mode)
    body = _mixed(dm.TILE * k // 2 + 600, mode, rng)
    assert len(body) > dm.TILE * k + 1
    for delta in (-1, 0, 1):
        length = dm.TILE * k + delta
        for last in (dm.filler(3), dm.varint(int(rng.integers(1 << 35, 1 << 42)), 6)):
            data = dm.with_length(body, length, last)
            assert len(data) == length and data.endswith(last)
            n = len(dm.terminators(data))
            sc = _scales(n, 2, mode, rng)
            sc[-1] = 3
            assert _check(data, sc, n, 2, mode, ctx="len %d last %d" % (length, len(last))) == "equal"


@pytest.mark.parametrize("mode", MODES)
def test_varint_straddles_tile_edge_by_every_split(mode):
    wide = mode >= 1
    rng = np.random.default_rng(mode)
    for split in range(1, 19 if wide else 10):
        data = dm.straddle(split, wide)
        n = len(dm.terminators(data))
        at = dm.TILE - split  # the straddling value: one digit down, so it stays in range and visible
        end = dm.TILE - split + (19 if wide else 10) - 1  # its terminator
        assert n == at + 41 and data[at - 1] < 0x80 and data[end] < 0x80 and min(data[at:end]) >= 0x80
        sc = _scales(n, 2, mode, rng)
        sc[at] = 3
        assert _check(data, sc, n, 2, mode, witness=True, ctx="split %d" % split) == "equal"
        if mode == 3:
            assert _run(data, sc, n, 2, mode)[1][at] == 1


@pytest.mark.parametrize("k", dm.LONG_BACK_K)
@pytest.mark.parametrize("mode", MODES)
def test_varint_longer_than_the_look_back(mode, k):
    """A value padded with zero payload to k bytes, ending in the first byte,
    a middle thread and the last byte of a tile. Its payload is in its first
    byte: past the 64-byte LDS look-back (66 bytes and more at a tile's first
    byte) only the scan-back through global memory finds it, and at 4100
    bytes it crosses a tile that holds no terminator. The Hive modes call a
    varint of 20 bytes or more too long whatever its payload."""
    import orc_amd

    rng = np.random.default_rng(k + mode)
    for where in dm.LONG_BACK_AT:
        data = dm.long_back(k, where)
        n = len(dm.terminators(data))
        at = n - 41  # the long varint's value index
        sc = _scales(n, 2, mode, rng)
        sc[at] = 2
        ctx = "k %d %s" % (k, where)
        if mode == 2:
            with pytest.raises(dm.ModelError) as e:
                dm.decode(data, sc, n, 2, mode)
            assert e.value.index == at and str(e.value) == dm.HIVE_OVERFLOW
            with pytest.raises(orc_amd.ParseError, match="Hive 0.11 decimal was more than 38 digits"):
                _run(data, sc, n, 2, mode)
            # a later value is too long as well: the first bad value is still `at`
            data2, sc2 = data + dm.padded_zero(25), np.append(sc, 2)
            with pytest.raises(dm.ModelError) as e:
                dm.decode(data2, sc2, n + 1, 2, mode)
            assert e.value.index == at
            with pytest.raises(orc_amd.ParseError, match="Hive 0.11 decimal was more than 38 digits"):
                _run(data2, sc2, n + 1, 2, mode)
            _assert_equal(_run(data2, sc2[:at], at, 2, mode), dm.decode(data2, sc2[:at], at, 2, mode), mode, ctx)
            with pytest.raises(orc_amd.ParseError, match="Hive 0.11 decimal was more than 38 digits"):
                _run(data2, sc2[:at + 1], at + 1, 2, mode)
            continue
        assert _check(data, sc, n, 2, mode, witness=True, ctx=ctx) == "equal"
        if mode < 2:
            assert dm.decode_ints(data, sc, n, 2, mode)[0][at] == -43, ctx
        if mode == 3:
            keep = _run(data, sc, n, 2, mode)[1]
            assert keep[at] == 0 and keep[at - 1] == 1 and keep[at + 1] == 1, ctx
        if mode == 0:
            # a bad scale after the long varint: the error is that value's, the prefix before it decodes
            sc[at + 3] = 2 + 19
            assert _check(data, sc, n, 2, mode, ctx=ctx) == "raised"
            assert _check(data, sc[:at + 3], at + 3, 2, mode, ctx=ctx) == "equal"
            assert _check(data, sc[:at + 4], at + 4, 2, mode, ctx=ctx) == "raised"


@pytest.mark.parametrize("scales", [(0, 0), (0, 1), (0, 18), (0, 19), (0, 38), (0, 39), (1, 0), (18, 0), (38, 0),
                                    (40, 0)], ids=lambda s: "col%d_val%d" % s)
@pytest.mark.parametrize("mode", (1, 2, 3))
def test_extreme_128_bit_encodings(mode, scales):
    """-2^127, 2^127 - 1, +-(10^38 - 1), +-10^38, 2^126 | 1 and the 19-byte
    varints ending in 3 and 4, multiplied and divided in one and in several
    steps. Mode 2 decodes each alone as well: those that raise must raise,
    the others must come out."""
    col_scale, cur = scales
    ex = dm.extremes()
    n = len(ex)
    _check(b"".join(ex), np.full(n, cur, dtype=np.int64), n, col_scale, mode, witness=True)
    if mode == 2:
        got = {_check(e, [cur], 1, col_scale, mode, witness=True, ctx="extreme %d" % i) for i, e in enumerate(ex)}
        assert got == {"equal", "raised"}


def test_mode3_nulls_at_size():
    """Hive 0.11 NULL-on-overflow over 3 * 4096 + 5 values: overflowing and
    too-long values in every tile (the kernel's 4 KB s_bad stage), some
    values overflowing only after the rescale."""
    rng = np.random.default_rng(11)
    data = dm.hive_mixed(N_BIG, rng)
    col = 12
    sc = np.full(N_BIG, col, dtype=np.int64)
    pick = rng.random(N_BIG)
    sc[pick < 0.02] = 0  # 10^12 up: past 38 digits for the longer values
    sc[pick > 0.9] = col + rng.integers(1, 30, size=int((pick > 0.9).sum()))
    want, keep = dm.decode(data, sc, N_BIG, col, 3)
    tiles = dm.terminators(data) // dm.TILE
    assert set(tiles[keep == 0]) == set(range((len(data) + dm.TILE - 1) // dm.TILE))
    assert 0.02 < np.mean(keep == 0) < 0.10
    _, keep_unscaled = dm.decode(data, np.full(N_BIG, col, dtype=np.int64), N_BIG, col, 3)
    assert ((keep == 0) & (keep_unscaled == 1)).sum() >= 10, "no value overflows through the rescale alone"
    assert _check(data, sc, N_BIG, col, 3, witness=True) == "equal"
    assert _check(data, sc, N_BIG, col, 2) == "raised"


@pytest.mark.parametrize("mode", MODES)
def test_prefix_decode_and_write_bounds(mode):
    """Fewer values requested than the stream holds: nothing is written past
    nvalues (sentinels, checked in _run) and no scale is read past nvalues
    (the array ends with its allocation); one value too many raises."""
    rng = np.random.default_rng(20 + mode)
    data = _mixed(N_BIG, mode, rng)
    T = len(dm.terminators(data))
    assert T == N_BIG and len(data) > 5 * dm.TILE
    sc = _scales(T, 2, mode, rng)
    want = dm.decode(data, sc, T, 2, mode)
    for n in (1, T - dm.TILE, T - 1, T):
        w = (want[0][:n], want[1][:n]) if mode == 3 else want[:n]
        _assert_equal(_run(data, sc[:n], n, 2, mode), w, mode, "nvalues %d" % n)
    assert _check(data, np.append(sc, 2), T + 1, 2, mode) == "raised"
    with pytest.raises(dm.ModelError, match="Read past end of stream"):
        dm.decode(data, np.append(sc, 2), T + 1, 2, mode)


@pytest.mark.parametrize("mode", MODES)
def test_repeated_launch_on_one_context(mode):
    """Back-to-back decodes of streams with different tile counts on one
    context: the tile-count and tile-base scratch is reused, not stale."""
    rng = np.random.default_rng(30 + mode)
    a = _mixed(2 * dm.TILE, mode, rng)
    b = dm.dense(dm.TILE + 7)
    c = dm.with_length(_mixed(dm.TILE, mode, rng), dm.TILE, dm.filler(1))
    runs = []
    for data in (a, b, c, a):
        n = len(dm.terminators(data))
        sc = _scales(n, 2, mode, rng)
        runs.append((data, sc, n, dm.decode(data, sc, n, 2, mode)))
    for i, (data, sc, n, want) in enumerate(runs):
        _assert_equal(_run(data, sc, n, 2, mode), want, mode, "launch %d" % i)


# ---- files: several decimal columns of different tile counts in one stripe ----

ROWS = 4096
NAMES = ["a", "b", "c", "d", "e", "f"]
PREC = {"a": (18, 2), "b": (18, 2), "c": (18, 2), "d": (38, 10), "e": (38, 10), "f": (18, 2)}


def _columns(present):
    """{name: (DATA bytes, scales, not-null mask or None)}: a dense, exactly
    one tile; b 4095 one-byte values and one two-byte value split by the tile
    edge (4097 bytes); c mixed; d mixed wide; e dense; f one value repeated
    with a scale change midway. Values stay within the declared precision.
    With `present`, b and d have ~30 % nulls, rows 0 and n - 1 among them."""
    rng = np.random.default_rng(5 + present)
    nn = {}
    for name in NAMES:
        nn[name] = None
        if present and name in "bd":
            m = rng.random(ROWS) >= 0.3
            m[0] = m[-1] = False
            nn[name] = m
    cnt = {name: ROWS if nn[name] is None else int(nn[name].sum()) for name in NAMES}
    cols = {}
    cols["a"] = (dm.dense(cnt["a"]), np.full(cnt["a"], 2, dtype=np.int64))
    cols["b"] = (dm.dense(cnt["b"] - 1) + dm.varint(dm.zigzag(-4321), 2), rng.integers(0, 5, size=cnt["b"]))
    cols["c"] = (dm.mixed(cnt["c"], False, rng, max_len=7), rng.integers(0, 5, size=cnt["c"]))  # |v| < 2^48, x 100
    cols["d"] = (dm.mixed(cnt["d"], True, rng, max_len=15), rng.integers(6, 15, size=cnt["d"]))  # |v| < 2^104, x 10^4
    cols["e"] = (dm.dense(cnt["e"]), rng.integers(0, 30, size=cnt["e"]))
    half = cnt["f"] // 2 - 3
    cols["f"] = (dm.varint(dm.zigzag(-123456789012)) * cnt["f"],
                 np.array([2] * half + [5] * (cnt["f"] - half), dtype=np.int64))
    if not present:
        assert len(cols["a"][0]) == dm.TILE and len(cols["b"][0]) == dm.TILE + 1
        tiles = {(len(cols[x][0]) + dm.TILE - 1) // dm.TILE for x in "abcf"}
        assert len(tiles) >= 3, "the batched launch wants columns of different tile counts"
    return {name: (cols[name][0], np.asarray(cols[name][1], dtype=np.int64), nn[name]) for name in NAMES}


def _file(cols, rows=ROWS):
    import orc_amd
    from orc_craft import DATA, PRESENT, SECONDARY, CraftColumn, bool_rle, decimal_type, struct_file

    craft = []
    for name in NAMES:
        data, sc, nn = cols[name]
        sec, _ = orc_amd.encode_direct(sc, True, aligned=True)
        streams = [] if nn is None else [(PRESENT, bool_rle(nn.astype(int)))]
        craft.append(CraftColumn(streams + [(DATA, data), (SECONDARY, sec.tobytes())]))
    return struct_file(NAMES, [decimal_type(*PREC[name]) for name in NAMES], [(rows, craft)], 0)


def _exact_decimal(v, scale):
    """v * 10^-scale without the context's rounding (28 digits by default)."""
    return decimal.Decimal((int(v < 0), tuple(int(c) for c in str(abs(v))), -scale))


def _model_rows(cols):
    per = {}
    for name in NAMES:
        data, sc, nn = cols[name]
        p, s = PREC[name]
        vals, _ = dm.decode_ints(data, sc, len(sc), s, int(p > 18))
        assert all(abs(v) < 10 ** p for v in vals), name
        it = iter(vals)
        per[name] = [_exact_decimal(next(it), s) if nn is None or nn[r] else None for r in range(ROWS)]
    return [{name: per[name][r] for name in NAMES} for r in range(ROWS)]


def _row_reader_rows(r, cap):
    rr = r.create_row_reader()
    batch = rr.create_row_batch(cap)
    rows = []
    while rr.next(batch):
        rows += batch.to_pylist()
    return rows


@pytest.mark.parametrize("present", [False, True], ids=["non_nullable", "nullable"])
def test_decimal_columns_of_one_stripe(tmp_path, present):
    """Six decimal columns in one stripe, read with stream batching (one
    varint_decimal_multi_kernel launch per width, the workgroups finding
    their column by tile), without it (one launch a column) and through the
    RowReader. Nullable columns leave the batch for the per-column kernel and
    the 8- / 16-byte scatter while their siblings stay in it."""
    import orc_amd

    cols = _columns(present)
    p = str(tmp_path / "decimals.orc")
    with open(p, "wb") as f:
        f.write(_file(cols))
    want = _model_rows(cols)
    # more digits than decimal's default context keeps
    assert any(w["d"] is not None and len(w["d"].as_tuple().digits) > 28 for w in want)
    if present:
        assert want[0]["b"] is None and want[-1]["d"] is None and want[0]["a"] is not None
        assert 0.2 < sum(w["b"] is None for w in want) / ROWS < 0.4

    r = orc_amd.Reader(p, orc_amd.default_context(0))
    assert r.num_rows == ROWS and r.num_stripes == 1
    got = r.read_stripe(0).to_pylist()
    assert r.last_stream_stats()["batched"] > 0
    assert got == want
    r.set_stream_batching(False)
    got_single = r.read_stripe(0).to_pylist()
    assert r.last_stream_stats()["batched"] == 0
    assert got_single == want
    r.set_stream_batching(True)
    for cap in (1000, ROWS):
        assert _row_reader_rows(r, cap) == want, cap

    po = pytest.importorskip("pyarrow.orc")
    assert po.ORCFile(p).read().to_pylist() == want


def test_error_is_the_first_columns_in_both_batching_modes(tmp_path):
    """A short DATA stream in column a and a bad scale in column c, row 10:
    the error raised is column a's, batched or not."""
    import orc_amd

    cols = _columns(False)
    data, sc, nn = cols["a"]
    cols["a"] = (data[:-1], sc, nn)
    data, sc, nn = cols["c"]
    sc = sc.copy()
    sc[10] = 2 + 38
    cols["c"] = (data, sc, nn)
    with pytest.raises(dm.ModelError, match=dm.PAST_END):
        dm.decode(cols["a"][0], cols["a"][1], ROWS, 2, 0)
    with pytest.raises(dm.ModelError, match=dm.BAD_SCALE) as e:
        dm.decode(cols["c"][0], cols["c"][1], ROWS, 2, 0)
    assert e.value.index == 10
    p = str(tmp_path / "bad.orc")
    with open(p, "wb") as f:
        f.write(_file(cols))
    r = orc_amd.Reader(p, orc_amd.default_context(0))
    for batching in (True, False):
        r.set_stream_batching(batching)
        with pytest.raises(orc_amd.ParseError, match="Read past end of stream in Decimal64ColumnReader column 1 ") as e:
            r.read_stripe(0)
        assert "scale out of range" not in str(e.value)
