"""Schema evolution through the file reader and the row reader
(Reader.set_read_type, RowReaderOptions::setReadType): files written at test
time with pyarrow, read under another type, compared exactly with the model of
the reference's rules (tests/convert_model.py) and with what the reference's
own tests assert (tests/convert_cases.py)."""
import decimal

import numpy as np
import pytest

import convert_model as M
import orc_amd
from convert_cases import reference_tests

import pyarrow as pa
from pyarrow import orc as pa_orc

pytestmark = pytest.mark.gpu

DECIMAL = 14
_CTX = decimal.Context(prec=60)


def arrow_type(t):
    k, p, s = M.parse(t)
    return {"boolean": pa.bool_(), "tinyint": pa.int8(), "smallint": pa.int16(), "int": pa.int32(),
            "bigint": pa.int64(), "float": pa.float32(), "double": pa.float64()}.get(k) or pa.decimal128(p, s)


def arrow_values(values, t):
    k, _, s = M.parse(t)
    if k == "decimal":
        return [None if v is None else decimal.Decimal(v).scaleb(-s, _CTX) for v in values]
    if k == "boolean":
        return [None if v is None else bool(v) for v in values]
    if k in ("float", "double"):
        return [None if v is None else float(v) for v in values]
    return values


def write(path, columns, **kw):
    """columns: [(name, type string, values)] -> an ORC file; the file's type string"""
    arrays = [pa.array(arrow_values(v, t), type=arrow_type(t)) for _, t, v in columns]
    pa_orc.write_table(pa.table(arrays, names=[n for n, _, _ in columns]), str(path), **kw)
    return "struct<%s>" % ",".join("%s:%s" % (n, t) for n, t, _ in columns)


def norm(batch, tid, i):
    """a value as the model gives it: unscaled int for a decimal, 0 / 1 for a
    boolean, float64 for float / double, None for NULL"""
    v = batch.value(tid, i)
    t = batch.types[tid]
    if v is None:
        return None
    if t.kind == DECIMAL:
        return int(v.scaleb(t.scale, _CTX))
    if isinstance(v, float):
        return np.float64(v)
    return int(v)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, np.floating) or isinstance(b, np.floating):
        return np.float64(a).view(np.int64) == np.float64(b).view(np.int64)
    return a == b


def model_column(values, src, dst):
    return [None if v is None else M.convert(v, src, dst) for v in values]


def read_columns(r, ncols, row_reader=False, capacity=1000, **kw):
    """per top-level column the values of the whole file, by read_stripe or by a row reader"""
    out = [[] for _ in range(ncols)]
    if row_reader:
        rr = r.create_row_reader(**kw)
        b = rr.create_row_batch(capacity)
        while rr.next(b):
            for c in range(ncols):
                out[c] += [norm(b, c + 1, i) for i in range(b.num_rows)]
        rr.close()
    else:
        for s in range(r.num_stripes):
            b = r.read_stripe(s)
            for c in range(ncols):
                out[c] += [norm(b, c + 1, i) for i in range(b.num_rows)]
    return out


def read_type_of(cols):
    return "struct<%s>" % ",".join("c%d:%s" % (i, d) for i, d in enumerate(cols))


def _holding(src, values):
    """The reference's TestConvertDecimalToDecimal stores 10^20 + i in a
    decimal(20,4) column, which its writer does not check and pyarrow refuses:
    such a column is written with the precision its values need (21). The
    conversion rules do not read the file precision beyond the 64 / 128 split."""
    k, p, s = M.parse(src)
    if k != "decimal":
        return src
    digits = max(len(str(abs(v))) for v in values)
    assert digits <= p or p > 18
    return "decimal(%d,%d)" % (max(p, digits), s)


@pytest.mark.parametrize("row_reader", [False, True], ids=["reader", "row-reader"])
@pytest.mark.parametrize("name", sorted(reference_tests()))
def test_reference_tests_end_to_end(tmp_path, name, row_reader):
    cols = [c._replace(src=_holding(c.src, c.values)) for c in reference_tests()[name]]
    p = tmp_path / "f.orc"
    write(p, [("c%d" % i, c.src, c.values) for i, c in enumerate(cols)])
    r = orc_amd.open_reader(str(p))
    r.set_read_type(read_type_of([c.dst for c in cols]))
    got = read_columns(r, len(cols), row_reader)
    for ci, c in enumerate(cols):
        want = model_column(c.values, c.src, c.dst)
        for i, (g, w) in enumerate(zip(got[ci], want)):
            assert same(g, w), "%s %s -> %s row %d: got %r, want %r" % (name, c.src, c.dst, i, g, w)
            assert c.check(i, g), "%s %s -> %s row %d: %r" % (name, c.src, c.dst, i, g)
        assert len(got[ci]) == len(c.values)


def test_nulls_are_the_files_plus_the_overflows(tmp_path):
    n = 3000
    rng = np.random.default_rng(5)
    base = [int(x) for x in rng.integers(-1000, 1000, size=n)]
    nullable = [None if i % 7 == 0 else (1 << 40 if i % 11 == 0 else v) for i, v in enumerate(base)]
    overflow_only = [1 << 40 if i % 13 == 0 else v for i, v in enumerate(base)]
    p = tmp_path / "f.orc"
    write(p, [("a", "bigint", nullable), ("b", "bigint", overflow_only), ("c", "bigint", base)])
    r = orc_amd.open_reader(str(p))
    # without a read type: b and c have no nulls
    r.read_stripe_device(0)
    assert r.column_view(1).has_nulls and not r.column_view(2).has_nulls and not r.column_view(3).has_nulls
    r.set_read_type("struct<a:int,b:int,c:int>")
    got = read_columns(r, 3)
    for ci, vals in enumerate((nullable, overflow_only, base)):
        want = model_column(vals, "bigint", "int")
        assert all(same(g, w) for g, w in zip(got[ci], want)) and len(got[ci]) == n
    assert got[0].count(None) == sum(1 for i in range(n) if i % 7 == 0 or i % 11 == 0)
    # has_nulls turns true only through the overflows; none: it stays false and the mask NULL
    va, vb, vc = (r.column_view(i) for i in (1, 2, 3))
    assert va.has_nulls and vb.has_nulls and vb.not_null
    assert not vc.has_nulls and not vc.not_null
    assert (va.kind, vb.kind, vc.kind) == (3, 3, 3) and r.types[1].kind == 4
    # null slots hold 0
    b = r.read_stripe(0)
    assert all(int(b.columns[2].data[i]) == 0 for i in range(0, n, 13))


def test_overflow_in_the_second_stripe_only(tmp_path):
    n = 8000
    rng = np.random.default_rng(6)
    vals = [int(x) for x in rng.integers(-(1 << 30), 1 << 30, size=n)]
    vals[-3] = 1 << 35
    p = tmp_path / "f.orc"
    write(p, [("a", "bigint", vals)], stripe_size=16 * 1024, batch_size=1024, row_index_stride=1000,
          compression="uncompressed")
    r = orc_amd.open_reader(str(p))
    assert r.num_stripes >= 2 and r.row_index_stride == 1000
    r.set_read_type("struct<a:int>")
    want = model_column(vals, "bigint", "int")
    for rows in (read_columns(r, 1)[0], read_columns(r, 1, row_reader=True, capacity=777)[0]):
        assert len(rows) == n and all(same(g, w) for g, w in zip(rows, want))
    r.read_stripes_device()
    flags = [bool(r.stripe_column_view(k, 1).has_nulls) for k in range(r.num_stripes)]
    assert flags == [False] * (r.num_stripes - 1) + [True]


def test_children_of_a_nullable_struct_and_of_a_list(tmp_path):
    n = 2500
    rng = np.random.default_rng(7)
    structs = [None if i % 5 == 0 else {"a": (1 << 33) if i % 9 == 0 else int(rng.integers(-100, 100)),
                                         "d": decimal.Decimal(int(rng.integers(-10 ** 6, 10 ** 6))).scaleb(-2)}
               for i in range(n)]
    lists = [None if i % 6 == 0 else [float(x) for x in rng.standard_normal(i % 4) * 1e3] + ([1e30] if i % 10 == 0 else [])
             for i in range(n)]
    t = pa.table({"s": pa.array(structs, type=pa.struct([("a", pa.int64()), ("d", pa.decimal128(10, 2))])),
                  "l": pa.array(lists, type=pa.list_(pa.float64()))})
    p = tmp_path / "f.orc"
    pa_orc.write_table(t, str(p))
    r = orc_amd.open_reader(str(p))
    assert r.type_string() == "struct<s:struct<a:bigint,d:decimal(10,2)>,l:array<double>>"
    r.set_read_type("struct<s:struct<a:int,d:decimal(6,1)>,l:array<int>>")
    assert r.read_type_string() == "struct<s:struct<a:int,d:decimal(6,1)>,l:array<int>>"

    def want_row(i):
        s = structs[i]
        if s is not None:
            s = {"a": M.convert(s["a"], "bigint", "int"),
                 "d": M.convert(int(s["d"].scaleb(2)), "decimal(10,2)", "decimal(6,1)")}
            s["d"] = None if s["d"] is None else decimal.Decimal(s["d"]).scaleb(-1)
        li = lists[i]
        if li is not None:
            li = [M.convert(np.float64(x), "double", "int") for x in li]
        return {"s": s, "l": li}

    for rows in (r.read(), _row_reader_rows(r)):
        assert len(rows) == n
        for i, row in enumerate(rows):
            assert row == want_row(i), "row %d: %r vs %r" % (i, row, want_row(i))


def _row_reader_rows(r, **kw):
    rr = r.create_row_reader(**kw)
    b = rr.create_row_batch(600)
    rows = []
    while rr.next(b):
        rows += b.to_pylist()
    rr.close()
    return rows


def test_batched_streams_and_one_launch_per_stream_agree(tmp_path):
    n = 6000
    rng = np.random.default_rng(8)
    cols = [("a", "bigint", [int(x) for x in rng.integers(-(1 << 40), 1 << 40, size=n)]),
            ("b", "int", [int(x) for x in rng.integers(-(1 << 20), 1 << 20, size=n)]),
            ("d", "decimal(30,3)", [int(x) * 10 ** 9 for x in rng.integers(-(1 << 60), 1 << 60, size=n)])]
    p = tmp_path / "f.orc"
    write(p, cols, row_index_stride=1000)
    dsts = ["int", "smallint", "decimal(38,6)"]
    want = [model_column(v, s, d) for (_, s, v), d in zip(cols, dsts)]
    r = orc_amd.open_reader(str(p))
    r.set_read_type("struct<a:int,b:smallint,d:decimal(38,6)>")
    got = read_columns(r, 3)
    assert r.last_stream_stats()["batched"] > 0
    r.set_stream_batching(False)
    unbatched = read_columns(r, 3)
    assert r.last_stream_stats()["batched"] == 0
    for g, u, w in zip(got, unbatched, want):
        assert len(g) == n and all(same(x, y) for x, y in zip(g, w)) and all(same(x, y) for x, y in zip(u, w))


def test_equal_read_type_and_clearing(tmp_path):
    n = 2000
    rng = np.random.default_rng(9)
    cols = [("a", "int", [None if i % 17 == 0 else int(x) for i, x in enumerate(rng.integers(-1000, 1000, size=n))]),
            ("f", "float", [float(np.float32(x)) for x in rng.standard_normal(n)]),
            ("d", "decimal(10,2)", [int(x) for x in rng.integers(-10 ** 9, 10 ** 9, size=n)])]
    p = tmp_path / "f.orc"
    file_type = write(p, cols)
    r = orc_amd.open_reader(str(p))
    assert r.type_string() == file_type
    plain = r.read_stripe(0)
    views = [(r.column_view(i).kind, bool(r.column_view(i).has_nulls)) for i in (1, 2, 3)]
    # a read type equal to the file's: every column passes through, byte for byte
    r.set_read_type(file_type)
    assert r.read_type_string() == file_type
    again = r.read_stripe(0)
    for tid in (1, 2, 3):
        assert again.columns[tid].data.tobytes() == plain.columns[tid].data.tobytes()
        a, b = again.columns[tid].not_null, plain.columns[tid].not_null
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    # another one, then cleared: the file's kinds are back
    r.set_read_type("struct<a:bigint,f:double,d:decimal(18,4)>")
    conv = r.read_stripe(0)
    assert [r.column_view(i).kind for i in (1, 2, 3)] == [4, 6, 14]
    assert conv.value(3, 5) == plain.value(3, 5) and str(conv.value(3, 5)).endswith("00")
    r.set_read_type(None)
    assert r.read_type_string() == file_type
    back = r.read_stripe(0)
    assert [(r.column_view(i).kind, bool(r.column_view(i).has_nulls)) for i in (1, 2, 3)] == views
    assert all(back.columns[t].data.tobytes() == plain.columns[t].data.tobytes() for t in (1, 2, 3))


def test_throw_names_the_first_overflowing_column(tmp_path):
    n = 3000
    a = list(range(n))
    b = list(range(n))
    c = list(range(n))
    b[2500] = 1 << 40
    b[700] = 1 << 41
    c[10] = 1 << 20  # overflows smallint at an earlier row, in a later column
    p = tmp_path / "f.orc"
    write(p, [("a", "bigint", a), ("b", "bigint", b), ("c", "bigint", c)])
    r = orc_amd.open_reader(str(p))
    r.set_read_type("struct<a:int,b:int,c:smallint>", throw_on_overflow=True)
    with pytest.raises(orc_amd.ParseError, match="^Overflow when convert from bigint to int$"):
        r.read_stripe(0)
    rr = r.create_row_reader()
    with pytest.raises(orc_amd.ParseError, match="^Overflow when convert from bigint to int$"):
        rr.next(rr.create_row_batch(100))
    rr.close()
    # b read as it is: c is the first
    r.set_read_type("struct<a:int,b:bigint,c:smallint>")
    with pytest.raises(orc_amd.ParseError, match="^Overflow when convert from bigint to smallint$"):
        r.read_stripe(0)
    # off again: NULLs
    r.set_read_type("struct<a:int,b:int,c:smallint>", throw_on_overflow=False)
    got = read_columns(r, 3)
    assert got[1].count(None) == 2 and got[2].count(None) == 1 and got[0].count(None) == 0


REFUSED = [
    ("struct<a:string,s:string,t:date>", "Conversion from int to string is not supported"),
    ("struct<a:varchar(5),s:string,t:date>", "Conversion from int to varchar(5) is not supported"),
    ("struct<a:timestamp,s:string,t:date>", "Conversion from int to timestamp is not supported"),
    ("struct<a:date,s:string,t:date>", "Cannot convert from int to date"),
    ("struct<a:binary,s:string,t:date>", "Cannot convert from int to binary"),
    ("struct<a:array<int>>", "Cannot convert from struct<a:int,s:string,t:date> to struct<a:array<int>>"),
    ("struct<a:int,s:int,t:date>", "Conversion from string to int is not supported"),
    ("struct<a:int,s:varchar(3),t:date>", "Conversion from string to varchar(3) is not supported"),
    ("struct<a:int,s:string,t:bigint>", "Cannot convert from date to bigint"),
    ("struct<a:int,s:string>", "Cannot convert from struct<a:int,s:string,t:date> to struct<a:int,s:string>"),
    ("struct<a:decimal(39,0),s:string,t:date>", "Invalid decimal precision or scale in the read type decimal(39,0)"),
]


def test_refused_read_types(tmp_path):
    import datetime

    p = tmp_path / "f.orc"
    pa_orc.write_table(pa.table({"a": pa.array([1, 2], pa.int32()), "s": pa.array(["x", "y"]),
                                 "t": pa.array([datetime.date(2020, 1, 1)] * 2)}), str(p))
    r = orc_amd.open_reader(str(p))
    assert r.type_string() == "struct<a:int,s:string,t:date>"
    for read_type, text in REFUSED:
        with pytest.raises(orc_amd.InvalidArgument) as e:
            r.set_read_type(read_type)
        assert str(e.value) == text, read_type
    for bad in ("struct<a:int", "struct<a:integer,s:string,t:date>", "struct<a:decimal(10),s:string,t:date>"):
        with pytest.raises(orc_amd.InvalidArgument):
            r.set_read_type(bad)
    # a refused read type leaves the reader as it was; field names are not compared
    assert r.read_type_string() == "struct<a:int,s:string,t:date>"
    r.set_read_type("struct<x:bigint,y:string,z:date>")
    assert r.read_type_string() == "struct<a:bigint,s:string,t:date>"
    assert r.read()[1] == {"a": 2, "s": "y", "t": datetime.date(2020, 1, 1)}


def test_a_row_reader_keeps_the_setting_of_its_creation(tmp_path):
    n = 2000
    vals = [(1 << 33) if i % 100 == 0 else i for i in range(n)]
    p = tmp_path / "f.orc"
    write(p, [("a", "bigint", vals)])
    r = orc_amd.open_reader(str(p))
    before = r.create_row_reader()
    r.set_read_type("struct<a:int>")
    under = r.create_row_reader()
    r.set_read_type(None)
    own = r.create_row_reader(read_type="struct<a:smallint>")
    assert r.read_type_string() == "struct<a:bigint>"  # the option did not stay on the reader
    tight = r.create_row_reader(read_type="struct<a:int>", tight_numeric=True)

    def rows(rr):
        b = rr.create_row_batch(512)
        out, dtypes = [], set()
        while rr.next(b):
            out += [norm(b, 1, i) for i in range(b.num_rows)]
            dtypes.add(b.columns[1].data.dtype)
        return out, dtypes

    assert rows(before)[0] == vals
    assert rows(under)[0] == model_column(vals, "bigint", "int")
    assert rows(own)[0] == model_column(vals, "bigint", "smallint")
    got, dtypes = rows(tight)
    assert got == model_column(vals, "bigint", "int") and dtypes == {np.dtype(np.int32)}
    assert [x["a"] for x in r.read()] == vals
    for rr in (before, under, own, tight):
        rr.close()
