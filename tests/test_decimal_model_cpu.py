"""tests/decimal_model.py (exact Python ints) against the two other CPU
references of the DECIMAL decode: the reference's own asserted values
(tests/golden/kat_decimal.json) and the C oracle, on every stream builder the
GPU tests use. The oracle was written beside the kernel; the model was not,
so an agreement here is what makes either fit to judge the kernel."""
import numpy as np
import pytest

import decimal_model as dm
from conftest import load_golden
from oracle import oracle

DECIMAL = [f for f in load_golden("kat_decimal.json") if f["kind"] == "decimal"]
MODES = (0, 1, 2, 3)
N_BIG = 3 * dm.TILE + 5


def _col_scales(mode):
    return (0, 2, 18) if mode == 0 else (0, 2, 18, 38)


def _oracle(data, scales, n, col_scale, mode):
    if mode == 3:
        return oracle.decimal_decode_keep(data, scales, n, col_scale)
    return oracle.decimal_decode(data, scales, n, col_scale, mode)


def _same(data, scales, n, col_scale, mode):
    """Model and oracle give the same arrays, or raise the same message."""
    try:
        want = dm.decode(data, scales, n, col_scale, mode)
    except dm.ModelError as e:
        with pytest.raises(oracle.OracleError) as o:
            _oracle(data, scales, n, col_scale, mode)
        assert str(o.value) == str(e)
        return "raised"
    got = _oracle(data, scales, n, col_scale, mode)
    if mode == 3:
        np.testing.assert_array_equal(got[1], want[1])
        got, want = got[0], want[0]
    np.testing.assert_array_equal(got, want)
    return "equal"


def _sweep(data, mode, seed):
    n = len(dm.terminators(data))
    for col_scale in _col_scales(mode):
        rng = np.random.default_rng(seed * 64 + col_scale)
        _same(data, dm.spread_scales(n, col_scale, mode, rng), n, col_scale, mode)
    _same(data, np.zeros(n, dtype=np.int64), n, 0, mode)


@pytest.mark.parametrize("fx", DECIMAL, ids=[f["name"] for f in DECIMAL])
def test_model_reproduces_reference_known_answers(fx):
    n = len(fx["expected"])
    scales = oracle.RleDecoderV1(bytes.fromhex(fx["secondary"]), True).next(n)
    data = bytes.fromhex(fx["data"])
    mode = 2 if fx["precision"] == 0 else int(fx["precision"] > 18)
    if fx.get("error"):
        with pytest.raises(dm.ModelError, match=fx["error"]):
            dm.decode_ints(data, scales, n, fx["scale"], mode)
        return
    if fx.get("throw_on_overflow") is False:
        vals, keep = dm.decode_ints(data, scales, n, fx["scale"], 3)
        assert [v if k else None for v, k in zip(vals, keep)] == fx["expected"]
        assert all(v == 0 for v, k in zip(vals, keep) if not k)
        with pytest.raises(dm.ModelError, match="more than 38 digits"):
            dm.decode_ints(data, scales, n, fx["scale"], 2)
        return
    vals, _ = dm.decode_ints(data, scales, n, fx["scale"], mode)
    assert vals == fx["expected"]


@pytest.mark.parametrize("mode", MODES)
def test_dense_matches_oracle(mode):
    for n in (1, dm.TILE, N_BIG):
        _sweep(dm.dense(n), mode, n)


@pytest.mark.parametrize("mode", MODES)
def test_mixed_matches_oracle(mode):
    rng = np.random.default_rng(mode)
    data = dm.mixed(N_BIG, mode >= 1, rng)
    assert len(data) > 10 * dm.TILE
    _sweep(data, mode, 1)
    if mode >= 2:  # a stream the Hive modes accept (divides only): values compared in mode 2 as well
        data = dm.mixed(N_BIG, True, rng, max_len=17, max_pad=18)
        n = len(dm.terminators(data))
        assert _same(data, 6 + rng.integers(0, 41, size=n), n, 6, mode) == "equal"


@pytest.mark.parametrize("mode", MODES)
def test_straddle_and_long_back_match_oracle(mode):
    wide = mode >= 1
    for split in range(1, 19 if wide else 10):
        _sweep(dm.straddle(split, wide), mode, split)
    for k in dm.LONG_BACK_K:
        for where in dm.LONG_BACK_AT:
            data = dm.long_back(k, where)
            thread, byte = dm.LONG_BACK_AT[where]
            end = len(data) - 41
            assert data[end] == 0 and data[end - k + 2:end] == b"\x80" * (k - 2) and data[end - k] < 0x80
            assert data[end - k + 1] == 0x80 | dm.LONG_BACK_RAW
            assert end % dm.TILE == thread * dm.PER_THREAD + byte
            _sweep(data, mode, k)


@pytest.mark.parametrize("mode", (1, 2, 3))
def test_extremes_match_oracle(mode):
    ex = dm.extremes()
    assert [len(e) for e in ex[:4]] == [19] * 4 and ex[0][-1] == 3 and ex[-2][-1] == 3 and ex[-1][-1] == 4
    outcomes = set()
    for col_scale, cur in ((0, 0), (0, 1), (0, 18), (0, 19), (0, 38), (0, 39), (0, 40), (1, 0), (18, 0), (38, 0),
                           (40, 0)):
        data = b"".join(ex)
        _same(data, np.full(len(ex), cur, dtype=np.int64), len(ex), col_scale, mode)
        for e in ex:  # alone, so that mode 2 compares the values that do not raise
            outcomes.add(_same(e, [cur], 1, col_scale, mode))
    assert outcomes == ({"equal", "raised"} if mode == 2 else {"equal"})
    # -2^127 one digit down: truncated toward zero
    vals, _ = dm.decode_ints(ex[0], [1], 1, 0, 1)
    assert vals == [-17014118346046923173168730371588410572]


def test_hive_mixed_matches_oracle_and_fills_every_tile():
    rng = np.random.default_rng(11)
    data = dm.hive_mixed(N_BIG, rng)
    scales = np.full(N_BIG, 6, dtype=np.int64)
    assert _same(data, scales, N_BIG, 6, 3) == "equal"
    assert _same(data, scales, N_BIG, 6, 2) == "raised"
    _, keep = dm.decode(data, scales, N_BIG, 6, 3)
    tiles = dm.terminators(data) // dm.TILE
    assert set(tiles[keep == 0]) == set(range(len(data) // dm.TILE + 1))
    assert 0.02 < np.mean(keep == 0) < 0.08


def test_short_stream_and_bad_scale_raise_the_same():
    for mode in MODES:
        with pytest.raises(dm.ModelError, match=dm.PAST_END) as e:
            dm.decode(bytes([6, 0x80]), [2, 2], 2, 2, mode)
        assert e.value.index == 1
        assert _same(bytes([6, 0x80]), [2, 2], 2, 2, mode) == "raised"
        assert _same(dm.dense(5), [0] * 6, 6, 0, mode) == "raised"
    for cur, col in ((22, 2), (0, 19), (-1, 18)):
        with pytest.raises(dm.ModelError, match=dm.BAD_SCALE):
            dm.decode(bytes([6, 8]), [col, cur], 2, col, 0)
        assert _same(bytes([6, 8]), [col, cur], 2, col, 0) == "raised"
    # Decimal128 has no range error
    assert _same(bytes([6]), [22], 1, 2, 1) == "equal"
