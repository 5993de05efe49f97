"""The schema-evolution conversion kernel (orc_amd/csrc/convert_kernels.hip)
through orcg_convert_column_device, against the exact model of the
reference's rules (tests/convert_model.py), for every source and target pair
in scope. Every comparison is exact: data by bit pattern, the mask, the count
of rows the conversion nulled.

Counts lie around a wave (63, 64, 65), around a thread's stride (255, 256,
257) and around a workgroup's 1,024 values, with a ragged last workgroup
(3 * 1024 + 17). Values come from each pair's boundary set in a seeded order;
where a pair can overflow, an overflowing value sits in every 64-row group,
so every wave of every workgroup adds to the nulled count."""
import numpy as np
import pytest
import torch

import convert_model as M
import orc_amd
from convert_cases import reference_tests

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 17]
NMAX = max(COUNTS)
KIND = {"boolean": 0, "tinyint": 1, "smallint": 2, "int": 3, "bigint": 4, "float": 5, "double": 6, "decimal": 14}
INT_RANGE = {"boolean": (0, 1), "tinyint": (-128, 127), "smallint": (-(1 << 15), (1 << 15) - 1),
             "int": (-(1 << 31), (1 << 31) - 1), "bigint": (M.INT64_MIN, M.INT64_MAX)}
DEC_TARGETS = ["decimal(3,2)", "decimal(10,4)", "decimal(18,0)", "decimal(18,18)", "decimal(20,3)", "decimal(38,0)",
               "decimal(38,19)", "decimal(38,38)"]
DEC_SOURCES = ["decimal(10,2)", "decimal(18,0)", "decimal(18,18)", "decimal(30,3)", "decimal(38,19)", "decimal(38,37)"]
# decimal -> decimal: scale differences 0, 1, 18, 19, 37 (and 38) both ways, across the 64 / 128 boundary
DEC_PAIRS = [("decimal(10,2)", "decimal(18,4)"), ("decimal(10,2)", "decimal(9,2)"), ("decimal(10,2)", "decimal(30,20)"),
             ("decimal(10,2)", "decimal(5,1)"), ("decimal(18,0)", "decimal(38,19)"), ("decimal(18,0)", "decimal(38,37)"),
             ("decimal(18,18)", "decimal(18,0)"), ("decimal(18,18)", "decimal(38,37)"), ("decimal(18,18)", "decimal(20,19)"),
             ("decimal(30,3)", "decimal(38,6)"), ("decimal(30,3)", "decimal(18,2)"), ("decimal(30,3)", "decimal(30,21)"),
             ("decimal(30,3)", "decimal(10,3)"), ("decimal(38,19)", "decimal(38,0)"), ("decimal(38,19)", "decimal(38,1)"),
             ("decimal(38,19)", "decimal(18,18)"), ("decimal(38,19)", "decimal(38,38)"), ("decimal(38,37)", "decimal(38,0)"),
             ("decimal(38,37)", "decimal(18,18)"), ("decimal(38,37)", "decimal(20,0)"), ("decimal(38,38)", "decimal(5,0)"),
             ("decimal(20,1)", "decimal(38,38)"), ("decimal(38,0)", "decimal(18,0)"), ("decimal(38,0)", "decimal(19,0)")]

PAIRS = [(s, d) for s in M.NUMERIC for d in M.NUMERIC if s != d]
PAIRS += [(s, d) for s in M.NUMERIC for d in DEC_TARGETS]
PAIRS += [(s, d) for s in DEC_SOURCES for d in M.NUMERIC]
PAIRS += DEC_PAIRS


def src_class(t):
    k, p, _ = M.parse(t)
    if k == "decimal":
        return orc_amd.rle.CONVERT_DECIMAL64 if p <= 18 else orc_amd.rle.CONVERT_DECIMAL128
    return {"float": orc_amd.rle.CONVERT_FLOAT, "double": orc_amd.rle.CONVERT_DOUBLE}.get(k, orc_amd.rle.CONVERT_INT64)


def _near(xs, spread=(-1, 0, 1)):
    return [x + d for x in xs for d in spread]


def boundary_values(src, dst, rng):
    """The pair's boundary set: values of the source type at which the rules
    change their answer, and a few seeded ordinary ones."""
    sk, sp, ss = M.parse(src)
    dk, dp, ds = M.parse(dst)
    powers = [1 << 7, 1 << 15, 1 << 31, 1 << 63]
    ints = _near(powers + [-p for p in powers]) + [0, 1, -1, (1 << 24) + 1, (1 << 53) + 1, (1 << 62) + 112312,
                                                    (1 << 53) + (1 << 29) + 1, -((1 << 24) + 1), -((1 << 53) + 1)]
    if dk == "decimal":
        # the bound of the target at the source's scale: 10^(p - s) and neighbours
        ints += _near([10 ** (dp - ds), -(10 ** (dp - ds)), 10 ** dp, -(10 ** dp)])
    ints += [int(x) for x in rng.integers(-(1 << 62), 1 << 62, size=16)] + [int(x) for x in rng.integers(-300, 300, size=16)]
    if sk in M.INTEGERS:
        lo, hi = INT_RANGE[sk]
        return [v for v in ints if lo <= v <= hi] + [lo, hi]
    if sk in ("float", "double"):
        T = np.float32 if sk == "float" else np.float64
        big = T(2.0 ** 63)
        vals = [0.0, -0.0, 0.5, -0.5, -0.9, 0.9, 1.0, -1.0, 1e35, -1e35, np.inf, -np.inf, np.nan, 127.9, 128.0, -128.9,
                -129.0, 32767.5, 32768.0, 2147483647.5, 2147483648.0, -2147483648.9, -2147483649.0, 9.9999, -9.9999,
                0.7, 0.005, 0.015, 0.025, 1.5, 2.5, 1e9 + 7, 2.0 ** 64, 2.0 ** 64 + 2.0 ** 41, 2.0 ** 100, -(2.0 ** 100),
                2.0 ** 127, -(2.0 ** 127), 1e-30, 1e18, 1e19, 123456789.987654321, 12345678910.1234]
        vals = [T(v) for v in vals]
        vals += [big, -big, np.nextafter(big, T(0)), np.nextafter(big, T(np.inf)), np.nextafter(-big, T(0)),
                 np.nextafter(-big, T(-np.inf)), np.nextafter(T(2.0 ** 127), T(0)), np.nextafter(T(-2.0 ** 127), T(0))]
        if dk == "decimal":
            edge = float(10 ** (dp - ds))
            vals += [T(edge), T(-edge), np.nextafter(T(edge), T(0)), np.nextafter(T(edge), T(np.inf)), T(edge - 0.5),
                     T(edge / 10 + 0.05)]
        vals += [T(x) for x in rng.standard_normal(16) * 1e3] + [T(x) for x in rng.standard_normal(8) * 1e17]
        if sk == "double":
            vals += [np.float64(3.4e38), np.float64(3.5e38), np.float64(1e39), np.float64(1e-46), np.float64(1e-39),
                     np.float64(16777217.0), np.float64(-16777219.0)]
        return vals
    # a decimal source: |v| <= the digits its width holds
    cap = M.INT64_MAX if sp <= 18 else M.INT128_MAX
    vals = list(ints) + _near([10 ** k for k in (1, 2, 3, 9, 10, 17, 18, 19, 20, 30, 37, 38)])
    vals += _near([(1 << 64), -(1 << 64), (1 << 64) + (1 << 11), (1 << 100), -(1 << 100), M.INT128_MAX - 1,
                   M.INT128_MIN + 2])
    # the integer part at int64's ends, with and without a fraction
    vals += _near([M.INT64_MAX * 10 ** ss, M.INT64_MIN * 10 ** ss, (M.INT64_MAX + 1) * 10 ** ss,
                   (M.INT64_MIN - 1) * 10 ** ss, 128 * 10 ** ss, -129 * 10 ** ss, (1 << 31) * 10 ** ss])
    if dk == "decimal":
        delta = ss - ds
        if delta > 0:
            # remainders exactly at, just under and just over half, around the target's bound
            half = 10 ** delta // 2
            for q in (0, 1, 2, 10 ** dp - 2, 10 ** dp - 1, 10 ** dp, 10 ** dp + 1, 12345):
                for r in (half - 1, half, half + 1, 0, 10 ** delta - 1):
                    vals += [q * 10 ** delta + r, -(q * 10 ** delta + r)]
        else:
            vals += _near([10 ** (dp + delta) if dp + delta >= 0 else 1, 10 ** dp, -(10 ** dp)])
    vals += [int(x) * 10 ** int(k) for x, k in zip(rng.integers(-10 ** 9, 10 ** 9, size=24), rng.integers(0, 29, size=24))]
    return [v for v in vals if -cap <= v <= cap]


def build_column(src, dst, seed):
    """NMAX values of the pair's boundary set in a seeded order, an overflowing
    one (if the pair has any) in every 64-row group, with the model's answers."""
    rng = np.random.default_rng(seed)
    cand = boundary_values(src, dst, rng)
    model = [M.convert(v, src, dst) for v in cand]
    over = [i for i, m in enumerate(model) if m is None]
    pick = rng.integers(0, len(cand), size=NMAX)
    pick[:len(cand)] = rng.permutation(len(cand))[:NMAX]  # every boundary value at least once
    if over:
        for g in range(0, NMAX, 64):
            pick[min(g + (g // 64 * 7) % 64, NMAX - 1)] = over[(g // 64) % len(over)]
    return [cand[i] for i in pick], [model[i] for i in pick], bool(over)


def masks(n):
    """(name, mask or None): none, all set, nulls at lanes 0 / 63 / 64, at the
    last row of a workgroup and the first of the next, one whole wave nulled"""
    out = [("none", None), ("all-set", np.ones(n, dtype=np.uint8))]
    for name, rows in (("lanes-0-63-64", [0, 63, 64]), ("workgroup-edge", [1023, 1024, 2047, 2048]),
                       ("one-wave", list(range(64, 128)) + list(range(1024 + 192, 1024 + 256)))):
        m = np.ones(n, dtype=np.uint8)
        rows = [r for r in rows if r < n]
        if rows:
            m[rows] = 0
            out.append((name, m))
    return out


def run(ctx, values, src, dst, mask, throw=False):
    dk, dp, ds = M.parse(dst)
    _, _, ss = M.parse(src)
    data = torch.from_numpy(M.pack(values, src)).cuda()
    nn = None if mask is None else torch.from_numpy(mask).cuda()
    nn_before = None if nn is None else nn.clone()
    out, out_nn, nulled = orc_amd.convert_column_device(ctx, data, src_class(src), KIND[dk], dp, ds, ss, nn, throw)
    if nn is not None:
        assert torch.equal(nn, nn_before), "the incoming mask was written"
    return out.cpu().numpy(), out_nn.cpu().numpy(), nulled


def expect(model, dst, mask):
    vals = [m if (mask is None or mask[i]) else None for i, m in enumerate(model)]
    nulled = sum(1 for i, m in enumerate(model) if m is None and (mask is None or mask[i]))
    return M.pack(vals, dst), np.array([v is not None for v in vals], dtype=np.uint8), nulled


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.default_context(0)


@pytest.mark.parametrize("src,dst", PAIRS, ids=["%s->%s" % p for p in PAIRS])
def test_pair_against_model(ctx, src, dst):
    values, model, has_overflow = build_column(src, dst, seed=PAIRS.index((src, dst)))
    for n in COUNTS:
        for name, mask in masks(n) if n in (65, 1025, NMAX) else [("none", None), ("all-set", np.ones(n, dtype=np.uint8))]:
            got, got_nn, nulled = run(ctx, values[:n], src, dst, mask)
            want, want_nn, want_nulled = expect(model[:n], dst, mask)
            where = "%s -> %s, n = %d, mask %s" % (src, dst, n, name)
            assert np.array_equal(got_nn, want_nn), where
            bad = np.flatnonzero((got.view(np.int64) != want.view(np.int64)).reshape(n, -1).any(axis=1)) if n else []
            assert len(bad) == 0, "%s: row %d, value %r: got %r, want %r" % (where, bad[0], values[bad[0]], got[bad[0]],
                                                                            want[bad[0]])
            assert nulled == want_nulled, where
    if has_overflow:
        # the same pair with no overflowing value at all
        keep = [i for i, m in enumerate(model) if m is not None][:1025]
        got, got_nn, nulled = run(ctx, [values[i] for i in keep], src, dst, None)
        want, want_nn, _ = expect([model[i] for i in keep], dst, None)
        assert nulled == 0 and got_nn.all() and same_bits(got, want)


@pytest.mark.parametrize("name", sorted(reference_tests()))
def test_reference_tests_on_the_device(ctx, name):
    """the reference's own test inputs (tests/convert_cases.py) and what its tests assert for them"""
    for col in reference_tests()[name]:
        got, got_nn, _ = run(ctx, col.values, col.src, col.dst, None)
        want, want_nn, _ = expect([M.convert(v, col.src, col.dst) for v in col.values], col.dst, None)
        assert np.array_equal(got_nn, want_nn) and same_bits(got, want), "%s %s -> %s" % (name, col.src, col.dst)
        dk, dp, _ = M.parse(col.dst)
        for i in range(len(col.values)):
            if not got_nn[i]:
                v = None
            elif dk == "decimal" and dp > 18:
                v = (int(got[i, 0]) << 64) | (int(got[i, 1]) & ((1 << 64) - 1))
            elif dk in ("float", "double"):
                v = np.float64(got[i])
            else:
                v = int(got[i])
            assert col.check(i, v), "%s %s -> %s row %d: %r" % (name, col.src, col.dst, i, v)


THROW = [("bigint", "int", 5, 1 << 40, "Overflow when convert from bigint to int"),
         ("double", "decimal(10,2)", 1.5, 1e30, "Overflow when convert from double to decimal(10,2)"),
         ("decimal(30,3)", "decimal(10,3)", 123456, 10 ** 25,
          "Overflow when convert from decimal(38,3) to decimal(10,3)")]


@pytest.mark.parametrize("src,dst,fine,over,text", THROW, ids=[t[0] + "->" + t[1] for t in THROW])
def test_throw_reports_the_first_overflowing_row(ctx, src, dst, fine, over, text):
    n = 3 * 1024
    # an overflow in two workgroups: the lower row is reported, whichever ran first
    values = [fine] * n
    values[2 * 1024 + 100] = over
    values[1024 + 700] = over
    with pytest.raises(orc_amd.ParseError, match="^" + text.replace("(", r"\(").replace(")", r"\)") + "$"):
        run(ctx, values, src, dst, None, throw=True)
    assert ctx.last_error_value() == 1024 + 700
    # the context's error record is clear again, and masked-out overflows raise nothing
    mask = np.ones(n, dtype=np.uint8)
    mask[[1024 + 700, 2 * 1024 + 100]] = 0
    got, got_nn, nulled = run(ctx, values, src, dst, mask, throw=True)
    assert nulled == 0 and np.array_equal(got_nn, mask)
    want, _, _ = expect([M.convert(v, src, dst) for v in values], dst, mask)
    assert same_bits(got, want)


def test_more_tiles_than_workgroups(ctx):
    """The grid is capped at 1,024 workgroups: past 1,024 tiles of 1,024 values
    a workgroup takes several tiles, and a wave adds the nulled rows of all of
    them with one atomic. bigint -> int here is the rule itself in numpy: cast
    to 32 bits and compare back."""
    n = 1024 * 1024 * 2 + 1024 + 5
    rng = np.random.default_rng(12)
    v = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64)
    big = rng.random(n) < 0.05
    v[big] <<= 6
    mask = (rng.random(n) >= 0.1).astype(np.uint8)
    fits = v.astype(np.int32).astype(np.int64) == v
    keep = fits & (mask != 0)
    out, out_nn, nulled = orc_amd.convert_column_device(ctx, torch.from_numpy(v).cuda(), orc_amd.rle.CONVERT_INT64,
                                                        KIND["int"], not_null=torch.from_numpy(mask).cuda())
    assert np.array_equal(out_nn.cpu().numpy(), keep.astype(np.uint8))
    assert np.array_equal(out.cpu().numpy(), np.where(keep, v, 0))
    assert nulled == int(((mask != 0) & ~fits).sum())


def test_bad_arguments(ctx):
    d = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(orc_amd.InvalidArgument):
        orc_amd.convert_column_device(ctx, d, 0, KIND["decimal"], 39, 0)
    with pytest.raises(orc_amd.InvalidArgument):
        orc_amd.convert_column_device(ctx, d, 0, KIND["decimal"], 10, 11)
    with pytest.raises(orc_amd.InvalidArgument):
        orc_amd.convert_column_device(ctx, d, 0, 7)  # string
    with pytest.raises(orc_amd.InvalidArgument):
        orc_amd.convert_column_device(ctx, d, 9, KIND["int"])
