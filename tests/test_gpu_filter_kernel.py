"""The row-level filter kernels (orc_amd/csrc/filter_kernels.hip) through
orcg_filter_columns_device and orcg_filter_gather_device, against the exact
model of the truth rules (tests/filter_model.py). Every comparison is exact:
the selected row indices, their order, the gathered values and masks.

The combine and select kernels work on tiles of T = 1,024 rows (256 lanes x 4
rows); neither has a grid cap (a workgroup per tile, up to 2^31 tiles). Row
counts lie around a wave (63, 64, 65) and around the tile (T - 1, T, T + 1,
2 T + 3); one count of 8,192 T + 5 rows crosses from launch_exclusive_scan's
single-workgroup scan of the tile counts to its look-back scan (8,192 inputs),
checked against numpy there (the model's loop over 8.4 M rows would take
minutes; the rule is one int64 compare)."""
import datetime
import decimal

import numpy as np
import pytest
import torch

import filter_model as M
import orc_amd
from orc_amd import reader as R
from orc_amd import sarg as S

pytestmark = pytest.mark.gpu

T = 1024
COUNTS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
NAN, INF = float("nan"), float("inf")
EPOCH = datetime.date(1970, 1, 1)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.default_context(0)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def mask_of(values):
    if all(v is not None for v in values):
        return None
    return dev(np.array([v is not None for v in values], dtype=np.uint8))


def int_col(cid, kind, values, junk=0, **typ):
    """int64 layout: integers, boolean, date, decimal of precision <= 18; a
    null slot holds `junk`"""
    d = dict(id=cid, kind=kind, not_null=mask_of(values),
             data=dev(np.array([junk if v is None else v for v in values], dtype=np.int64)))
    d.update(typ)
    return d


def f64_col(cid, values, kind=R.DOUBLE):
    return dict(id=cid, kind=kind, not_null=mask_of(values),
                data=dev(np.array([7.25 if v is None else v for v in values], dtype=np.float64)))


def dec128_col(cid, values, precision=30, scale=4):
    words = np.zeros(2 * len(values), dtype=np.int64)
    for i, v in enumerate(values):
        v = 12345 if v is None else v
        words[2 * i] = v >> 64
        words[2 * i + 1] = ((v & ((1 << 64) - 1)) ^ (1 << 63)) - (1 << 63)
    return dict(id=cid, kind=R.DECIMAL, precision=precision, scale=scale, not_null=mask_of(values), data=dev(words))


def direct_col(cid, values, kind=R.STRING):
    """start / length / blob; a null row's start and length point far outside the blob"""
    blob = b"\xee" + b"".join(v for v in values if v is not None)
    start, length, at = [], [], 1
    for v in values:
        if v is None:
            start.append(1 << 40)
            length.append(1 << 40)
        else:
            start.append(at)
            length.append(len(v))
            at += len(v)
    return dict(id=cid, kind=kind, not_null=mask_of(values), data=dev(np.array(start, dtype=np.int64)),
                length=dev(np.array(length, dtype=np.int64)), blob=dev(np.frombuffer(blob, dtype=np.uint8)))


def dict_col(cid, values, entries=None, eager=False, kind=R.STRING):
    """index / dict_offsets / blob; a null row's index is out of range"""
    if entries is None:
        entries = sorted({v for v in values if v is not None}) or [b"unused"]
    at = {e: i for i, e in enumerate(entries)}
    offs = np.zeros(len(entries) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(e) for e in entries])
    blob = b"".join(entries) or b"\x00"
    idx = np.array([10 ** 9 if v is None else at[v] for v in values], dtype=np.int64)
    d = dict(id=cid, kind=kind, not_null=mask_of(values), index=dev(idx), dict_offsets=dev(offs),
             blob=dev(np.frombuffer(blob, dtype=np.uint8)))
    if eager:  # the decoded starts and lengths too, as with lazy decoding off
        d["data"] = dev(np.array([0 if v is None else offs[at[v]] for v in values], dtype=np.int64))
        d["length"] = dev(np.array([0 if v is None else len(v) for v in values], dtype=np.int64))
    return d


def selected(ctx, leaves, program, cols, n):
    """the filter's selected rows as np.int64 (read back through an identity gather)"""
    p, cnt = S.filter_columns_device(ctx, S.SearchArgument(leaves, program), cols, n)
    if cnt == 0:
        return np.zeros(0, dtype=np.int64)
    out8, _, _, _ = S.gather_device(ctx, p, cnt, n, [torch.arange(n, dtype=torch.int64, device=DEV)])
    got = out8[0].cpu().numpy()
    assert np.all(np.diff(got) > 0), "selected[] is not strictly ascending"
    return got


def check(ctx, leaves, model_leaves, program, cols, model_cols, n, what=""):
    got = selected(ctx, leaves, program, cols, n)
    want = M.select(model_leaves, program, model_cols, n)
    assert got.tolist() == want, what


def spread(pool, n, rng, nulls):
    vals = [pool[i] for i in rng.integers(0, len(pool), size=n)]
    if nulls == "all":
        return [None] * n
    if nulls:
        for i in np.flatnonzero(rng.random(n) < nulls):
            vals[i] = None
    return vals


LEAF0 = [(M.LEAF, 0)]


@pytest.mark.parametrize("n", COUNTS)
def test_row_counts_and_selections(ctx, n):
    """none, all, only row 0, only the last row, alternating"""
    values = [(i % 2) * 10 + (100 if i == 0 else 0) + (-100 if i == n - 1 and n > 1 else 0) for i in range(n)]
    cols, model = [int_col(1, R.LONG, values)], {1: values}
    for op, lits in [(M.LESS_THAN, [-1000]), (M.LESS_THAN, [1000]), (M.EQUALS, [100]), (M.EQUALS, [-100 + (n - 1) % 2 * 10]),
                     (M.EQUALS, [10]), (M.IN, [[0, 100, -100]])]:
        lits = lits[0] if op == M.IN else lits
        check(ctx, [(op, 1, S.LONG, lits)], [(op, 1, lits)], LEAF0, cols, model, n, (op, lits))


@pytest.mark.parametrize("nulls", [0, 0.37, "all"], ids=["no-mask", "37pct", "all-null"])
def test_masks(ctx, nulls):
    n = 2 * T + 3
    rng = np.random.default_rng(3)
    values = spread([-5, 0, 3, 9], n, rng, nulls)
    cols, model = [int_col(1, R.LONG, values, junk=3)], {1: values}
    for op, lits in [(M.EQUALS, [3]), (M.LESS_THAN_EQUALS, [3]), (M.IS_NULL, []), (M.BETWEEN, [0, 3])]:
        for prog in (LEAF0, LEAF0 + [(M.NOT, 0)]):
            check(ctx, [(op, 1, S.LONG, lits)], [(op, 1, lits)], prog, cols, model, n, (op, prog))


def days(d):
    return EPOCH + datetime.timedelta(days=d)


def dec(u, scale):
    return decimal.Decimal(u).scaleb(-scale, decimal.Context(prec=60))


X = (1 << 70) + 12345
# name: (column builder, value pool (model values), literal type, model literal -> API literal,
#        single literals, BETWEEN pairs, IN lists), literals in model form
CLASSES = {
    "long": (lambda v: int_col(1, R.LONG, v, junk=7), [-(1 << 63), -5, -1, 0, 1, 2, 7, 100, (1 << 63) - 1], S.LONG,
             lambda x: x, [7, -(1 << 63), (1 << 63) - 1], [(-1, 7), (7, -1)], [[7, 100, -5, 12345, 7]]),
    "boolean": (lambda v: int_col(1, R.BOOLEAN, v, junk=1), [0, 1], S.BOOLEAN, bool, [0, 1], [(0, 1), (1, 1)],
                [[1], [0, 1]]),
    "date": (lambda v: int_col(1, R.DATE, v, junk=18000), [-1, 0, 18000, 19000], S.DATE, days, [0, 18000, 5],
             [(-1, 18000)], [[19000, -1, 3]]),
    "double": (lambda v: f64_col(1, v), [NAN, -INF, -1.5, -0.0, 0.0, 1.5, 2.5, INF, 5e-324], S.FLOAT, float,
               [0.0, -0.0, NAN, 1.5, INF, -INF], [(-0.0, 2.5), (NAN, 1.0), (-INF, INF), (0.0, NAN)],
               [[NAN, 1.5], [0.0], [-0.0], [INF, -INF, 3.0, 2.5]]),
    "float": (lambda v: f64_col(1, v, R.FLOAT), [float(np.float32(0.1)), 0.5, -0.0, NAN], S.FLOAT, float,
              [0.1, float(np.float32(0.1)), 0.5], [(0.0, 0.2)], [[float(np.float32(0.1))], [0.1]]),
    "decimal64": (lambda v: int_col(1, R.DECIMAL, v, junk=150, precision=10, scale=2),
                  [-(10 ** 9), -200, -150, 0, 150, 151, 10 ** 9], S.DECIMAL, None,
                  [(15, 1), (150, 2), (-2, 0), (0, 0)], [((-2, 0), (15, 1))], [[(15, 1), (150, 2), (-2, 0), (7, 2)]]),
    # values that differ only in the high word, and in the low word's top bit
    "decimal128": (lambda v: dec128_col(1, v), [X, X + (1 << 64), X - (1 << 64), -X, 0, 15000, -(1 << 100), 1 << 100,
                                               1 << 63, (1 << 63) - 1, -(1 << 63)], S.DECIMAL, None,
                   [(X, 4), (X + (1 << 64), 4), (15, 1), (0, 0), (1 << 63, 4)],
                   [((-X, 4), (X, 4)), ((X, 4), (X + (1 << 64), 4))],
                   [[(X, 4), (15, 1), (-(1 << 100), 4), (5, 0), (X - (1 << 64), 4)]]),
}
STRINGS = [b"", b"a", b"ab", b"abc", b"b", b"\x7f", b"\x80", b"\xff\x00", b"ab\x00", b"abd"]
STRING_LITS = ([b"ab", b"", b"\x80", b"abcd", b"\x7f"], [(b"a", b"abc"), (b"\x7f", b"\xff"), (b"b", b"a")],
               [[b"", b"\x80", b"zz", b"ab", b"ab"], [b"abcd"]])
for _name, _build in (("direct string", lambda v: direct_col(1, v)), ("dictionary string", lambda v: dict_col(1, v)),
                      ("eager dictionary char", lambda v: dict_col(1, v, eager=True, kind=R.CHAR))):
    CLASSES[_name] = (_build, STRINGS, S.STRING, lambda x: x) + STRING_LITS


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_every_operator_on_every_leaf_class(ctx, name):
    build, pool, typ, conv, singles, ranges, lists = CLASSES[name]
    n = T + 5
    rng = np.random.default_rng(11)
    values = spread(pool, n, rng, 0.37)
    cols, model = [build(values)], {1: values}
    if typ == S.DECIMAL:
        scale = cols[0]["scale"]
        api = lambda x: dec(*x)  # noqa: E731
        mod = lambda x: M.rescale(x[0], x[1], scale)  # noqa: E731
    else:
        api, mod = conv, lambda x: x  # noqa: E731
    cases = [(op, [x]) for x in singles for op in (M.EQUALS, M.LESS_THAN, M.LESS_THAN_EQUALS)]
    cases += [(M.BETWEEN, list(r)) for r in ranges] + [(M.IN, list(x)) for x in lists] + [(M.IS_NULL, [])]
    for op, lits in cases:
        for prog in (LEAF0, LEAF0 + [(M.NOT, 0)]):
            check(ctx, [(op, 1, typ, [api(x) for x in lits])], [(op, 1, [mod(x) for x in lits])], prog, cols, model, n,
                  (name, op, lits, prog))


def test_long_rows_and_long_literals(ctx):
    """a 100 KB row against a literal that shares its first 30,000 bytes, and
    literals longer than every other row (a filter's string literals total at
    most 64 KB)"""
    big = bytes(range(256)) * 400  # 102,400 bytes
    values = [b"", big, big[:30000], None, big[:29999] + b"\xff", b"\x00", big[:30001], big]
    lit = big[:30000]
    model = {1: values}
    for build in (direct_col, dict_col):
        cols = [build(1, values)]
        for op, lits in [(M.EQUALS, [lit]), (M.LESS_THAN, [lit]), (M.LESS_THAN_EQUALS, [lit]),
                         (M.BETWEEN, [lit, big[:30001]]), (M.IN, [lit, b"\x00"])]:
            check(ctx, [(op, 1, S.STRING, lits)], [(op, 1, lits)], LEAF0, cols, model, len(values), (build.__name__, op))


@pytest.mark.parametrize("entries", [1, 5000])
def test_dictionary_sizes(ctx, entries):
    """one evaluation per entry, a lookup per row; null rows carry index 10^9"""
    words = [b"w%05d" % i for i in range(entries)]
    n = 2 * T + 3
    rng = np.random.default_rng(entries)
    values = spread(words, n, rng, 0.2)
    cols, model = [dict_col(1, values, entries=words)], {1: values}
    for op, lits in [(M.EQUALS, [words[-1]]), (M.LESS_THAN, [b"w02500"]), (M.IN, [words[0], words[entries // 2], b"none"]),
                     (M.BETWEEN, [b"w00001", b"w04000"]), (M.IS_NULL, [])]:
        for prog in (LEAF0, LEAF0 + [(M.NOT, 0)]):
            check(ctx, [(op, 1, S.STRING, lits)], [(op, 1, lits)], prog, cols, model, n, (op, prog))


def test_three_columns_stack_depth_16_and_64_leaf_or(ctx):
    n = T + 77
    rng = np.random.default_rng(5)
    a = spread(list(range(-40, 40)), n, rng, 0.3)
    b = spread([NAN, -1.0, 0.0, 0.5, 2.0], n, rng, 0.3)
    c = spread([b"x", b"yy", b"", b"zzz"], n, rng, 0.3)
    cols = [int_col(1, R.LONG, a), f64_col(2, b), dict_col(5, c)]
    model = {1: a, 2: b, 5: c}
    # a flat OR of 64 leaves (what an expanded IN produces), and its negation:
    # the host folds an n-ary op as it emits it, so width costs no stack
    leaves = [(M.EQUALS, 1, S.LONG, [k - 40]) for k in range(64)]
    mleaves = [(M.EQUALS, 1, [k - 40]) for k in range(64)]
    prog = [(M.LEAF, k) for k in range(64)] + [(M.OR, 64)]
    check(ctx, leaves, mleaves, prog, cols, model, n, "64-leaf OR")
    check(ctx, leaves, mleaves, prog + [(M.NOT, 0)], cols, model, n, "NOT of a 64-leaf OR")
    # a 63-leaf AND of negated leaves with one nullable OR inside
    prog = [(M.LEAF, k) for k in range(62)] + [(M.LEAF, 62), (M.LEAF, 63), (M.OR, 2), (M.AND, 63), (M.NOT, 0)]
    check(ctx, leaves, mleaves, prog, cols, model, n, "NOT of a 63-operand AND")
    # stack depth 16 is nesting: l0 op (l1 op (l2 ... l15)), AND and OR alternating, NOTs over nulls
    leaves = [(M.LESS_THAN, 1, S.LONG, [0]), (M.LESS_THAN_EQUALS, 2, S.FLOAT, [0.5]), (M.EQUALS, 5, S.STRING, [b"yy"]),
              (M.IS_NULL, 2, S.LONG, []), (M.IN, 5, S.STRING, [b"", b"zzz"])]
    mleaves = [(op, col, lits) for op, col, _, lits in leaves]

    def nested(depth):
        prog = [(M.LEAF, k % 5) for k in range(depth)]
        for k in range(depth - 1):
            prog += [(M.AND if k % 2 else M.OR, 2)] + ([(M.NOT, 0)] if k % 5 == 3 else [])
        return prog

    check(ctx, leaves, mleaves, nested(16), cols, model, n, "depth 16")
    with pytest.raises(orc_amd.InvalidArgument, match="nests to a stack of 17, deeper than 16"):
        S.SearchArgument(leaves, nested(17)).handle(orc_amd._lib.load(), int)
    # a three-leaf AND / OR over the three columns, and its negation
    prog = [(M.LEAF, 0), (M.LEAF, 1), (M.AND, 2), (M.LEAF, 2), (M.OR, 2)]
    for p in (prog, prog + [(M.NOT, 0)]):
        check(ctx, leaves, mleaves, p, cols, model, n, p)


def test_refusals_carry_their_text(ctx):
    cols = [int_col(1, R.LONG, [1, 2, 3])]
    with pytest.raises(orc_amd.InvalidArgument, match="column 1 is bigint: it takes a LONG literal, not FLOAT"):
        selected(ctx, [(M.EQUALS, 1, S.FLOAT, [1.0])], LEAF0, cols, 3)
    with pytest.raises(orc_amd.InvalidArgument, match="column 2 was not decoded"):
        selected(ctx, [(M.IS_NULL, 2, S.LONG, [])], LEAF0, cols + [int_col(3, R.LONG, [1, 2, 3])], 3)
    with pytest.raises(orc_amd.InvalidArgument, match="NULL_SAFE_EQUALS is not supported"):
        selected(ctx, [(M.NULL_SAFE_EQUALS, 1, S.LONG, [1])], LEAF0, cols, 3)
    # views the run cannot read
    with pytest.raises(orc_amd.InvalidArgument, match="column 1 has no string layout"):
        selected(ctx, [(M.EQUALS, 1, S.STRING, [b"x"])], LEAF0, [dict(id=1, kind=R.STRING)], 3)
    with pytest.raises(orc_amd.InvalidArgument, match="column 1 has nulls and no mask"):
        selected(ctx, [(M.EQUALS, 1, S.LONG, [1])], LEAF0, [dict(cols[0], has_nulls=True)], 3)
    with pytest.raises(orc_amd.InvalidArgument, match="column 1 has no values"):
        selected(ctx, [(M.EQUALS, 1, S.LONG, [1])], LEAF0, [dict(id=1, kind=R.LONG)], 3)
    big = [b"x" * 40000, b"y" * 25537]
    with pytest.raises(orc_amd.InvalidArgument, match="at most 65536 bytes of string literals, not 65537"):
        selected(ctx, [(M.IN, 1, S.STRING, big)], LEAF0, [dict(id=1, kind=R.STRING)], 3)
    with pytest.raises(orc_amd.InvalidArgument, match="an IN list has at most 1024 literals, not 3000"):
        selected(ctx, [(M.IN, 1, S.LONG, list(range(3000)))], LEAF0, cols, 3)


def test_scan_of_more_than_8192_tiles(ctx):
    n = 8192 * T + 5
    rng = np.random.default_rng(1)
    v = rng.integers(-1000, 1000, size=n, dtype=np.int64)
    got = selected(ctx, [(M.LESS_THAN, 1, S.LONG, [-990])], LEAF0, [dict(id=1, kind=R.LONG, data=dev(v))], n)
    assert np.array_equal(got, np.flatnonzero(v < -990))


@pytest.mark.parametrize("n,keep", [(1, "all"), (65, "odd"), (2 * T + 3, "odd"), (2 * T + 3, "non-null"),
                                    (T, "none")])
def test_gather_against_numpy_indexing(ctx, n, keep):
    """8-byte and 16-byte values, string (start, length) pairs and masks; the
    gathered null count is 0 when only non-null rows are selected"""
    rng = np.random.default_rng(n)
    nn = (rng.random(n) >= 0.37).astype(np.uint8)
    sel = {"all": np.arange(n), "odd": np.arange(1, n, 2), "non-null": np.flatnonzero(nn),
           "none": np.zeros(0, np.int64)}[keep].astype(np.int64)
    v8 = rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
    start = rng.integers(0, 1 << 40, size=n, dtype=np.int64)
    length = rng.integers(0, 1 << 20, size=n, dtype=np.int64)
    f8 = rng.standard_normal(n)
    v16 = rng.integers(-(1 << 62), 1 << 62, size=2 * n, dtype=np.int64)
    d_sel = dev(sel if sel.size else np.zeros(1, np.int64))
    out8, out16, out_nn, nulls = S.gather_device(ctx, d_sel, int(sel.size), n, [dev(v8), dev(start), dev(length)],
                                                 dev(v16), dev(nn))
    assert np.array_equal(out8[0].cpu().numpy(), v8[sel])
    assert np.array_equal(out8[1].cpu().numpy(), start[sel]) and np.array_equal(out8[2].cpu().numpy(), length[sel])
    assert np.array_equal(out16.cpu().numpy().reshape(-1, 2), v16.reshape(-1, 2)[sel])
    assert np.array_equal(out_nn.cpu().numpy(), nn[sel])
    assert nulls == int((nn[sel] == 0).sum())
    if keep == "non-null":
        assert nulls == 0
    out8, out16, out_nn, nulls = S.gather_device(ctx, d_sel, int(sel.size), n, [dev(f8)])
    assert np.array_equal(out8[0].cpu().numpy(), f8[sel]) and out_nn is None and nulls == 0
