"""Row-level filters through the reader: Reader.read_stripe(i, filter=sarg),
filter_stripe and filtered_column over files written with pyarrow (two
stripes, row-index stride 1,000, 6,000 rows), against pyarrow's own
read_stripe(i).filter(expression) -- Kleene logic, a null result drops the row
-- and, under a read type (which pyarrow cannot read), against the model
(tests/filter_model.py) over the converted values."""
import datetime
import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.orc as pa_orc
import pytest

import filter_model as M
import orc_amd
from conftest import GOLDEN
from orc_amd import SearchArgumentBuilder as B

pytestmark = pytest.mark.gpu

ROWS = 6000
D = decimal.Decimal


def with_nulls(values, rng, p=0.2):
    return [None if rng.random() < p else v for v in values]


def make_table():
    rng = np.random.default_rng(42)
    i = rng.integers(-50, 50, size=ROWS).tolist()
    d = (rng.integers(-40, 40, size=ROWS) / 4.0).tolist()
    days = rng.integers(18000, 18100, size=ROWS).tolist()
    d10 = [D(int(x)).scaleb(-2) for x in rng.integers(-10 ** 6, 10 ** 6, size=ROWS)]
    d30 = [D(int(x) * 10 ** 15 + 7).scaleb(-4) for x in rng.integers(-10 ** 9, 10 ** 9, size=ROWS)]
    direct = ["row-%06d-%s" % (k, "x" * int(k % 7)) for k in rng.permutation(ROWS)]
    words = ["", "apple", "banana", "cherry", "éclair", "fig"]
    dic = [words[k] for k in rng.integers(0, len(words), size=ROWS)]
    sx = rng.integers(0, 10, size=ROWS).tolist()
    struct_rows = [None if rng.random() < 0.1 else {"x": (None if rng.random() < 0.2 else x), "y": w}
                   for x, w in zip(sx, dic)]
    dates = [datetime.date(1970, 1, 1) + datetime.timedelta(days=x) for x in days]
    small = rng.integers(-100, 100, size=ROWS).tolist()
    f32 = (rng.integers(-40, 40, size=ROWS) / 8.0).tolist()  # exact in float32
    flags = (rng.random(ROWS) < 0.3).tolist()
    extra = {
        # the same kinds without nulls (no PRESENT stream: views with no mask) ...
        "d0": pa.array(d, pa.float64()),
        "dt0": pa.array(dates, pa.date32()),
        "d10_0": pa.array(d10, pa.decimal128(10, 2)),
        "d30_0": pa.array(d30, pa.decimal128(30, 4)),
        # ... and the kinds the binding maps onto the int64 and double layouts
        "b": pa.array(with_nulls(flags, rng), pa.bool_()),
        "i8": pa.array(with_nulls(small, rng), pa.int8()),
        "i16": pa.array([100 * x for x in small], pa.int16()),
        "f32": pa.array(with_nulls(f32, rng), pa.float32()),
    }
    return pa.table({
        "i": pa.array(with_nulls(i, rng), pa.int64()),
        "i0": pa.array(i, pa.int32()),
        "d": pa.array(with_nulls(d, rng), pa.float64()),
        "dt": pa.array(with_nulls([datetime.date(1970, 1, 1) + datetime.timedelta(days=x) for x in days], rng),
                       pa.date32()),
        "d10": pa.array(with_nulls(d10, rng), pa.decimal128(10, 2)),
        "d30": pa.array(with_nulls(d30, rng), pa.decimal128(30, 4)),
        "sd": pa.array(with_nulls(direct, rng), pa.string()),
        "sd0": pa.array(direct, pa.string()),
        "sk": pa.array(with_nulls(dic, rng), pa.string()),
        "sk0": pa.array(dic, pa.string()),
        "st": pa.array(struct_rows, pa.struct([("x", pa.int64()), ("y", pa.string())])),
        **extra,
    })


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("filter") / "f.orc")
    t = make_table()
    pa_orc.write_table(t, path, compression="zlib", stripe_size=1024, batch_size=ROWS // 2, row_index_stride=1000,
                       dictionary_key_size_threshold=0.5)
    f = pa_orc.ORCFile(path)
    assert f.nstripes == 2
    return path, [pa.Table.from_batches([f.read_stripe(k)]) for k in range(2)]


DAY = datetime.date(1970, 1, 1) + datetime.timedelta(days=18050)
F = pc.field
IN_DIRECT = ["row-%06d-%s" % (k, "x" * (k % 7)) for k in range(0, ROWS, 40)] + ["nope"]
# (name, builder -> sarg, pyarrow expression)
CASES = [
    ("int <", lambda: B().less_than("i", -45).build(), F("i") < -45),
    ("int not <=", lambda: B().start_not().less_than_equals("i", 40).end().build(), ~(F("i") <= 40)),
    ("int no nulls in", lambda: B().is_in("i0", [3, -7, 3, 49]).build(), F("i0").isin([3, -7, 49])),
    ("int is null", lambda: B().is_null("i").build(), F("i").is_null()),
    ("double between", lambda: B().between("d", -0.5, 0.25).build(), (F("d") >= -0.5) & (F("d") <= 0.25)),
    ("double =", lambda: B().equals("d", 0.0).build(), F("d") == 0.0),
    ("date <=", lambda: B().less_than_equals("dt", DAY).build(), F("dt") <= DAY),
    ("decimal(10,2) <", lambda: B().less_than("d10", D("-9000.5")).build(), F("d10") < D("-9000.50")),
    ("decimal(30,4) between", lambda: B().between("d30", D("-1e23"), D("1e23")).build(),
     (F("d30") >= D("-1e23")) & (F("d30") <= D("1e23"))),
    ("direct string <", lambda: B().less_than("sd", "row-000300").build(), F("sd") < "row-000300"),
    ("direct string no nulls in", lambda: B().is_in("sd0", IN_DIRECT).build(), F("sd0").isin(IN_DIRECT)),
    ("dictionary string =", lambda: B().equals("sk", "éclair").build(), F("sk") == "éclair"),
    ("dictionary string not in", lambda: B().start_not().is_in("sk0", ["", "fig"]).end().build(),
     ~F("sk0").isin(["", "fig"])),
    ("double no nulls between", lambda: B().between("d0", -0.5, 0.25).build(), (F("d0") >= -0.5) & (F("d0") <= 0.25)),
    ("double no nulls not <", lambda: B().start_not().less_than("d0", 9.0).end().build(), ~(F("d0") < 9.0)),
    ("date no nulls <=", lambda: B().less_than_equals("dt0", DAY).build(), F("dt0") <= DAY),
    ("date no nulls in", lambda: B().is_in("dt0", [DAY, DAY + datetime.timedelta(days=3)]).build(),
     F("dt0").isin([DAY, DAY + datetime.timedelta(days=3)])),
    ("decimal(10,2) no nulls <", lambda: B().less_than("d10_0", D("-9000.5")).build(), F("d10_0") < D("-9000.50")),
    ("decimal(30,4) no nulls between", lambda: B().between("d30_0", D("-1e19"), D("1e19")).build(),
     (F("d30_0") >= D("-1e19")) & (F("d30_0") <= D("1e19"))),
    ("decimal(30,4) no nulls not <=", lambda: B().start_not().less_than_equals("d30_0", D("9e19")).end().build(),
     ~(F("d30_0") <= D("9e19"))),
    ("boolean =", lambda: B().equals("b", True).build(), F("b") == True),  # noqa: E712
    ("boolean not =", lambda: B().start_not().equals("b", True).end().build(), ~(F("b") == True)),  # noqa: E712
    ("tinyint between", lambda: B().between("i8", -5, 20).build(), (F("i8") >= -5) & (F("i8") <= 20)),
    ("smallint no nulls <", lambda: B().less_than("i16", -9000).build(), F("i16") < -9000),
    ("float <=", lambda: B().less_than_equals("f32", -4.125).build(), F("f32") <= -4.125),
    ("float in", lambda: B().is_in("f32", [0.125, 0.0, 4.875]).build(), F("f32").isin([0.125, 0.0, 4.875])),
    ("and / or over three columns",
     lambda: B().start_or().start_and().less_than("i", 0).equals("sk", "apple").end().less_than("d", -9.0).end().build(),
     ((F("i") < 0) & (F("sk") == "apple")) | (F("d") < -9.0)),
]


def rows_equal(batch, table):
    got, want = batch.to_pylist(), table.to_pylist()
    assert len(got) == len(want)
    assert got == want


@pytest.mark.parametrize("lazy", [False, True], ids=["eager-dict", "lazy-dict"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_filtered_stripe_matches_pyarrow(written, case, lazy):
    path, stripes = written
    _, build, expr = case
    r = orc_amd.open_reader(path)
    r.set_lazy_dictionary(lazy)
    sarg = build()
    for k in range(2):
        want = stripes[k].filter(expr)
        batch = r.read_stripe(k, filter=sarg)
        assert 0 < want.num_rows < stripes[k].num_rows
        rows_equal(batch, want)
    # the dictionary column is dictionary-encoded, the direct one direct
    ids = dict(zip(r.types[0].field_names, r.types[0].subtypes))
    assert r.stripe_column_view(0, ids["sk"]).encoding in (1, 3) and r.stripe_column_view(0, ids["sd"]).encoding in (0, 2)


def test_struct_child_leaf_read_stripes_and_has_nulls(written):
    path, stripes = written
    r = orc_amd.open_reader(path)
    st = r.types[0].subtypes[r.types[0].field_names.index("st")]
    x = r.types[st].subtypes[0]
    sarg = B().less_than(x, 3).build()
    r.read_stripes_device(0, 2)
    for k in (1, 0):
        tab = stripes[k]
        xs = tab.column("st").combine_chunks().field("x")
        want = np.flatnonzero(np.array(pc.fill_null(pc.less(xs, 3), False).to_pylist()) &
                              np.array(tab.column("st").is_valid().to_pylist()))
        got = r.filter_stripe(k, sarg)
        assert got.dtype == np.int64 and got.tolist() == want.tolist() and len(want) > 0
        col = r.filtered_column(k, x)
        assert col.num_elements == len(want) and col.not_null is None  # only non-null rows were selected
        assert col.data.tolist() == [xs[int(j)].as_py() for j in want]
        # the struct and a sibling column with nulls, gathered by the same selection
        assert r.filtered_column(k, st).not_null is None
        i_id = r.types[0].subtypes[0]
        ci = r.filtered_column(k, i_id)
        wi = [tab.column("i")[int(j)].as_py() for j in want]
        assert [None if ci.not_null is not None and not ci.not_null[j] else int(ci.data[j])
                for j in range(len(want))] == wi
        assert (ci.not_null is not None) == (None in wi)


def test_no_null_columns_filter_and_gather_without_a_mask(written):
    """the F64, int64 (date, decimal64) and decimal128 leaf classes with no
    mask, and their filtered views: has_nulls = 0, not_null = NULL"""
    path, stripes = written
    r = orc_amd.open_reader(path)
    ids = dict(zip(r.types[0].field_names, r.types[0].subtypes))
    sarg = B().start_and().less_than("d0", 5.0).less_than_equals("dt0", DAY).less_than("d10_0", D("5000"))\
        .less_than("d30_0", D("5e19")).end().build()
    expr = (F("d0") < 5.0) & (F("dt0") <= DAY) & (F("d10_0") < D("5000")) & (F("d30_0") < D("5e19"))
    r.read_stripe_device(1)
    for name in ("d0", "dt0", "d10_0", "d30_0"):
        v = r.stripe_column_view(0, ids[name])
        assert v.decoded and not v.has_nulls, name
    want = stripes[1].filter(expr)
    got = r.filter_stripe(0, sarg)
    assert 0 < len(got) == want.num_rows < stripes[1].num_rows
    for name in ("d0", "dt0", "d10_0", "d30_0"):
        v = r.filtered_column_view(0, ids[name])
        assert v.num_elements == len(got) and not v.has_nulls and not v.not_null, name
    rows_equal(r.read_stripe(1, filter=sarg), want)


def test_golden_varchar_column():
    """orc_index_int_string.orc: struct<_col0:int,_col1:varchar(4)>"""
    path = os.path.join(GOLDEN, "files", "orc_index_int_string.orc")
    f = pa_orc.ORCFile(path)
    r = orc_amd.open_reader(path)
    assert r.type_string() == "struct<_col0:int,_col1:varchar(4)>"
    tab = f.read()
    lit = sorted(set(x for x in tab.column("_col1").to_pylist() if x is not None))
    lit = lit[len(lit) // 3]
    sarg = B().start_and().less_than_equals("_col1", lit).start_not().less_than("_col0", 100).end().end().build()
    total = 0
    for k in range(f.nstripes):
        t = pa.Table.from_batches([f.read_stripe(k)])
        want = t.filter((F("_col1") <= lit) & ~(F("_col0") < 100))
        rows_equal(r.read_stripe(k, filter=sarg), want)
        total += want.num_rows
    assert 0 < total < tab.num_rows


def test_leaf_under_a_read_type(tmp_path):
    """int -> bigint passes values through; bigint -> decimal(6,1) nulls what
    does not fit: such a row is NULL for the leaf, negated or not"""
    rng = np.random.default_rng(9)
    a = rng.integers(-100, 100, size=ROWS).tolist()
    b = [int(v) for v in rng.integers(-200000, 200000, size=ROWS)]
    b = [None if k % 11 == 0 else v for k, v in enumerate(b)]
    path = str(tmp_path / "rt.orc")
    pa_orc.write_table(pa.table({"a": pa.array(a, pa.int32()), "b": pa.array(b, pa.int64())}), path,
                       stripe_size=1024, batch_size=ROWS // 2, row_index_stride=1000)
    r = orc_amd.open_reader(path)
    assert r.num_stripes == 2
    r.set_read_type("struct<a:bigint,b:decimal(6,1)>")
    conv = [None if v is None or abs(v) >= 10 ** 5 else v * 10 for v in b]  # unscaled at scale 1
    assert any(v is not None and abs(v) >= 10 ** 5 for v in b)
    sargs = [(B().less_than("b", D("100.5")).build(), [(M.LESS_THAN, 2, [1005])], [(M.LEAF, 0)]),
             (B().start_not().less_than("b", D("100.5")).end().build(), [(M.LESS_THAN, 2, [1005])],
              [(M.LEAF, 0), (M.NOT, 0)]),
             (B().start_and().less_than("a", 0).is_null("b").end().build(),
              [(M.LESS_THAN, 1, [0]), (M.IS_NULL, 2, [])], [(M.LEAF, 0), (M.LEAF, 1), (M.AND, 2)])]
    for sarg, leaves, prog in sargs:
        at = 0
        for k in range(2):
            n = r.stripe(k)["num_rows"]
            cols = {1: a[at:at + n], 2: conv[at:at + n]}
            want = M.select(leaves, prog, cols, n)
            batch = r.read_stripe(k, filter=sarg)
            assert r.filter_stripe(0, sarg).tolist() == want and len(want) > 0
            assert batch.to_pylist() == [{"a": cols[1][j], "b": None if cols[2][j] is None else D(cols[2][j]).scaleb(-1)}
                                         for j in want]
            at += n
    with pytest.raises(orc_amd.InvalidArgument, match="column 2 is decimal: it takes a DECIMAL literal, not LONG"):
        r.read_stripe(0, filter=B().less_than("b", 5).build())


def test_list_schema_and_unselected_leaf(tmp_path):
    rng = np.random.default_rng(2)
    a = rng.integers(0, 100, size=ROWS).tolist()
    lists = [None if k % 13 == 0 else list(range(k % 4)) for k in range(ROWS)]
    s = ["s%d" % (k % 50) for k in range(ROWS)]
    path = str(tmp_path / "l.orc")
    t = pa.table({"a": pa.array(a, pa.int64()), "l": pa.array(lists, pa.list_(pa.int32())), "s": pa.array(s)})
    pa_orc.write_table(t, path, stripe_size=1024, batch_size=ROWS // 2, row_index_stride=1000)
    r = orc_amd.open_reader(path)
    assert r.type_string() == "struct<a:bigint,l:array<int>,s:string>"
    sarg = B().start_and().less_than("a", 10).equals("s", "s7").end().build()
    f = pa_orc.ORCFile(path)
    tab = pa.Table.from_batches([f.read_stripe(1)])
    mask = pc.and_kleene(pc.less(tab.column("a"), 10), pc.equal(tab.column("s"), "s7"))
    want = np.flatnonzero(np.array(mask.to_pylist()))
    batch = r.read_stripe(1, filter=sarg)
    assert r.filter_stripe(0, sarg).tolist() == want.tolist() and len(want) > 0
    for tid in (2, 3):
        with pytest.raises(orc_amd.InvalidArgument, match="column %d is not filtered: nested" % tid):
            r.filtered_column(0, tid)
    assert sorted(batch.columns) == [0, 1, 4]  # the siblings gather, the list is left out
    assert [batch.value(1, j) for j in range(len(want))] == [a[ROWS // 2 + int(j)] for j in want]
    assert [batch.value(4, j) for j in range(len(want))] == ["s7"] * len(want)
    # a leaf under the list, and a leaf on a column that was not selected
    with pytest.raises(orc_amd.InvalidArgument, match="column 3 is under a list, map or union"):
        r.read_stripe(0, filter=B().equals(3, 1).build())
    r.select([1])
    with pytest.raises(orc_amd.InvalidArgument, match="column 4 was not decoded"):
        r.read_stripe(0, filter=sarg)
    assert r.read_stripe(0, filter=B().less_than("a", 10).build()).num_rows > 0


def test_filter_none_is_todays_read(written):
    path, _ = written
    r = orc_amd.open_reader(path)
    a, b = r.read_stripe(1), r.read_stripe(1, filter=None)
    assert sorted(a.columns) == sorted(b.columns)
    for tid, ca in a.columns.items():
        cb = b.columns[tid]
        for name in ("not_null", "data", "length", "offsets", "index", "dict_offsets", "secondary", "tags"):
            x, y = getattr(ca, name), getattr(cb, name)
            assert (x is None) == (y is None) and (x is None or (x.dtype == y.dtype and x.tobytes() == y.tobytes()))
        assert ca.blob == cb.blob and ca.num_elements == cb.num_elements and ca.encoding == cb.encoding


def test_golden_predicate_pushdown_file():
    path = os.path.join(GOLDEN, "files", "TestOrcFile.testPredicatePushdown.orc")
    f = pa_orc.ORCFile(path)
    r = orc_amd.open_reader(path)
    name = r.types[0].field_names[0]
    assert r.types[r.types[0].subtypes[0]].kind == orc_amd.reader.INT
    # testPredicatePushdown writes int1 = 300 i: the rows its own test keeps, [300 * 1000, 300 * 2000)
    sarg = B().start_and().start_not().less_than(name, 300000).end().less_than(name, 600000).end().build()
    total = 0
    for k in range(f.nstripes):
        tab = pa.Table.from_batches([f.read_stripe(k)])
        want = tab.filter((pc.field(name) >= 300000) & (pc.field(name) < 600000))
        batch = r.read_stripe(k, filter=sarg)
        rows_equal(batch, want)
        total += want.num_rows
    assert total == 1000
