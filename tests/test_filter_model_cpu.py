"""tests/filter_model.py, the exact model the filter kernels are tested
against, checked itself against pyarrow.compute on the same data (less,
less_equal, equal, is_null, and_kleene, or_kleene, invert, is_in), its NOT
push-down against its own unpushed evaluation, and its decimal rescaling
against decimal.Decimal.

Where pyarrow differs, the adaptor is written out here:
  * is_in gives false, not null, for a null row: the model's NULL there is
    compared with "the row is null";
  * is_in's NaN / -0.0 matching is pinned by test_pyarrow_is_in_float_matching
    (it matches NaN with NaN and tells -0.0 from 0.0, which is Double.compare's
    rule and the model's), not assumed."""
import decimal
import random

import pyarrow as pa
import pyarrow.compute as pc
import pytest

import filter_model as M

NAN = float("nan")
INF = float("inf")


def truth_of(x):
    """a pyarrow boolean scalar's value as a model truth"""
    return M.NULL if x is None else (M.YES if x else M.NO)


INTS = [None, -(1 << 63), -5, -1, 0, 1, 2, 7, 7, (1 << 63) - 1, None, 3]
FLOATS = [None, NAN, -INF, -1.5, -0.0, 0.0, 1.5, 2.5, INF, 1e300, None, 5e-324]
BYTES = [None, b"", b"a", b"ab", b"abc", b"b", b"\x7f", b"\x80", b"\xff\x00", b"ab\x00", None, b"abd"]
CASES = [
    ("int", INTS, pa.int64(), [(-1,), (7,), ((1 << 63) - 1,), (-(1 << 63),)], [(0, 7), (7, 0), (-5, -5)],
     [[7, 0, -5], [100]]),
    ("float", FLOATS, pa.float64(), [(0.0,), (-0.0,), (NAN,), (INF,), (1.5,)],
     [(-0.0, 1.5), (-INF, INF), (NAN, 1.0), (0.0, NAN)], [[NAN, 1.5], [0.0], [-0.0], [INF, -INF, 3.0]]),
    ("bytes", BYTES, pa.binary(), [(b"",), (b"ab",), (b"\x80",), (b"abc",)], [(b"a", b"abc"), (b"\x7f", b"\xff")],
     [[b"", b"\x80", b"zz"], [b"ab"]]),
]


@pytest.mark.parametrize("name,values,typ,singles,ranges,lists", CASES, ids=[c[0] for c in CASES])
def test_leaves_match_pyarrow(name, values, typ, singles, ranges, lists):
    arr = pa.array(values, type=typ)
    for (lit,) in singles:
        s = pa.scalar(lit, type=typ)
        for op, fn in ((M.EQUALS, pc.equal), (M.LESS_THAN, pc.less), (M.LESS_THAN_EQUALS, pc.less_equal)):
            want = [truth_of(x) for x in fn(arr, s).to_pylist()]
            got = [M.leaf_truth(op, v, [lit]) for v in values]
            assert got == want, (name, op, lit)
    for lo, hi in ranges:
        a, b = pa.scalar(lo, type=typ), pa.scalar(hi, type=typ)
        want = [truth_of(x) for x in pc.and_kleene(pc.less_equal(a, arr), pc.less_equal(arr, b)).to_pylist()]
        got = [M.leaf_truth(M.BETWEEN, v, [lo, hi]) for v in values]
        assert got == want, (name, lo, hi)
    for lits in lists:
        raw = pc.is_in(arr, value_set=pa.array(lits, type=typ)).to_pylist()
        # the adaptor: pyarrow says false for a null row, the filter NULL
        want = [M.NULL if v is None else truth_of(x) for v, x in zip(values, raw)]
        got = [M.leaf_truth(M.IN, v, lits) for v in values]
        assert got == want, (name, lits)
    want = [truth_of(x) for x in pc.is_null(arr).to_pylist()]
    assert [M.leaf_truth(M.IS_NULL, v, []) for v in values] == want


def test_pyarrow_is_in_float_matching():
    """What the adaptor above relies on, pinned: is_in matches NaN with NaN,
    keeps -0.0 and 0.0 apart, and gives false for a null row."""
    arr = pa.array([NAN, 0.0, -0.0, None])
    assert pc.is_in(arr, value_set=pa.array([NAN])).to_pylist() == [True, False, False, False]
    assert pc.is_in(arr, value_set=pa.array([0.0])).to_pylist() == [False, True, False, False]
    assert pc.is_in(arr, value_set=pa.array([-0.0])).to_pylist() == [False, False, True, False]
    # and the IEEE operators do not: -0.0 = 0.0, NaN equals nothing
    assert pc.equal(arr, 0.0).to_pylist() == [False, True, True, None]
    assert M.double_compare(-0.0, 0.0) == -1 and M.double_compare(NAN, NAN) == 0
    assert M.double_compare(INF, NAN) == -1 and M.double_compare(NAN, -NAN) == 0


def random_tree(rng, nleaves, depth):
    """a postfix program over leaves [0, nleaves)"""
    if depth == 0 or rng.random() < 0.3:
        return [(M.LEAF, rng.randrange(nleaves))]
    kind = rng.choice([M.AND, M.OR, M.NOT])
    if kind == M.NOT:
        return random_tree(rng, nleaves, depth - 1) + [(M.NOT, 0)]
    n = rng.randint(1, 4)
    out = []
    for _ in range(n):
        out += random_tree(rng, nleaves, depth - 1)
    return out + [(kind, n)]


def arrow_eval(program, leaf_arrays):
    st = []
    for op, arg in program:
        if op == M.LEAF:
            st.append(leaf_arrays[arg])
        elif op == M.NOT:
            st.append(pc.invert(st.pop()))
        else:
            acc = st.pop()
            for _ in range(arg - 1):
                acc = (pc.and_kleene if op == M.AND else pc.or_kleene)(st.pop(), acc)
            st.append(acc)
    return st[0]


def test_expressions_match_pyarrow_kleene_and_push_down():
    rng = random.Random(7)
    nleaves, rows = 5, 40
    truths = [[rng.choice([M.YES, M.NO, M.NULL]) for _ in range(nleaves)] for _ in range(rows)]
    to_arrow = {M.YES: True, M.NO: False, M.NULL: None}
    arrays = [pa.array([to_arrow[truths[r][k]] for r in range(rows)], type=pa.bool_()) for k in range(nleaves)]
    for _ in range(200):
        prog = random_tree(rng, nleaves, 4)
        want = [truth_of(x) for x in arrow_eval(prog, arrays).to_pylist()]
        got = [M.eval_program(prog, truths[r]) for r in range(rows)]
        assert got == want, prog
        pushed = M.push_down_not(prog)
        assert all(item[0] != "not" for item in pushed)
        assert [M.eval_pushed(pushed, truths[r]) for r in range(rows)] == got, prog


def test_decimal_rescale_matches_decimal():
    ctx = decimal.Context(prec=80)
    for text, column_scale in [("1.5", 2), ("-0.001", 3), ("12345678901234567890.12", 4), ("0", 10), ("-7", 0),
                               ("99999999999999999999999999999999999", 3)]:
        d = decimal.Decimal(text)
        sign, digits, exp = d.as_tuple()
        u = int("".join(map(str, digits))) * (-1 if sign else 1)
        got = M.rescale(u, -exp, column_scale)
        assert decimal.Decimal(got).scaleb(-column_scale, ctx) == d
        assert got == int(d.scaleb(column_scale, ctx))
    with pytest.raises(ValueError, match="exceeds"):
        M.rescale(15, 3, 2)
    with pytest.raises(ValueError, match="128 bits"):
        M.rescale(10 ** 37, 0, 2)
    assert M.rescale(10 ** 37, 0, 1) == 10 ** 38  # < 2^127


def test_select_is_the_yes_rows():
    col = {1: [1, None, 3, 4], 2: [b"a", b"b", None, b"a"]}
    leaves = [(M.LESS_THAN, 1, [4]), (M.EQUALS, 2, [b"a"])]
    assert M.select(leaves, [(M.LEAF, 0), (M.LEAF, 1), (M.AND, 2)], col, 4) == [0]
    assert M.select(leaves, [(M.LEAF, 0), (M.LEAF, 1), (M.OR, 2)], col, 4) == [0, 2, 3]
    # a negated leaf never selects a null row
    assert M.select(leaves, [(M.LEAF, 0), (M.NOT, 0)], col, 4) == [3]
