"""Decoded stripes exported as Arrow arrays (Reader.read_stripe_arrow,
read_arrow, arrow_device_buffers over include/orcg_arrow.h) against pyarrow's
own ORC reader (ORC C++ on the CPU), which reads the same file into the same
Arrow types: the same schema, validate(full=True), and equals() per stripe
(values under null slots do not take part in equals)."""
import io

import numpy as np
import pytest

import orc_amd
from file_parity import CORRUPT_FILES, path
from test_arrow_schema_cpu import PLAIN, UNION_FILES, char_file

pa = pytest.importorskip("pyarrow")
po = pytest.importorskip("pyarrow.orc")

pytestmark = pytest.mark.gpu

CORRUPT = [c[0] for c in CORRUPT_FILES]
# pyarrow builds without the codec refuse it ("Compression type not supported
# by Arrow"); this reader decodes it. Where pyarrow reads it, it is the oracle
# as for every other file; where not, the export is checked against the
# reader's own host batch
NO_ORACLE = ["TestVectorOrcFile.testLzo.orc"]
# Files whose stripes name no writer time zone: the reference assumes the
# machine's /etc/localtime, this reader leaves their TIMESTAMP columns
# undecoded (include/orcg_reader.h), so the export refuses them by name
NO_WRITER_ZONE = ["orc-file-11-format.orc", "orc_split_elim.orc", "over1k_bloom.orc"]
FILES = [f for f in PLAIN if f not in CORRUPT + NO_ORACLE + NO_WRITER_ZONE]


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def same_batch(got, want, what):
    assert got.schema.equals(want.schema, check_metadata=False), "%s\n%s\n-- pyarrow --\n%s" % (what, got.schema,
                                                                                               want.schema)
    got.validate(full=True)
    assert got.num_rows == want.num_rows, what
    for name, g, w in zip(got.schema.names, got.columns, want.columns):
        assert g.equals(w), "%s column %s" % (what, name)
    assert got.equals(want), what


def test_the_lists_name_golden_files():
    for f in CORRUPT + NO_ORACLE + NO_WRITER_ZONE:
        assert f in PLAIN, f


@pytest.mark.parametrize("name", FILES)
def test_every_stripe_equals_pyarrow(ctx, name):
    r = orc_amd.Reader(path(name), ctx)
    f = po.ORCFile(path(name))
    assert r.num_stripes == f.nstripes
    for i in range(r.num_stripes):
        same_batch(r.read_stripe_arrow(i), f.read_stripe(i), "%s stripe %d" % (name, i))


@pytest.mark.parametrize("name", ["TestOrcFile.testSeek.orc", "TestOrcFile.emptyFile.orc", "decimal.orc",
                                  "TestOrcFile.testDate1900.orc", "nulls-at-end-snappy.orc"])
def test_read_arrow_equals_pyarrow_read(ctx, name):
    got = orc_amd.Reader(path(name), ctx).read_arrow()
    want = po.ORCFile(path(name)).read()
    assert got.schema.equals(want.schema, check_metadata=False)
    got.validate(full=True)
    assert got.equals(want.replace_schema_metadata(None).cast(got.schema))


@pytest.mark.parametrize("name", NO_ORACLE)
def test_a_codec_pyarrow_may_not_read(ctx, name):
    r = orc_amd.Reader(path(name), ctx)
    f = po.ORCFile(path(name))
    rows = 0
    for i in range(r.num_stripes):
        b = r.read_stripe_arrow(i)
        b.validate(full=True)
        assert b.schema.equals(f.schema)
        try:
            want = f.read_stripe(i)
        except Exception as e:
            assert "not supported" in str(e)
            want = None
        if want is not None:
            same_batch(b, want, "%s stripe %d" % (name, i))
        # the same values as the reader's own host batch
        hb = r.read_stripe(i)
        for tid, col in zip(r.types[0].subtypes, b.columns):
            assert np.array_equal(col.to_numpy(zero_copy_only=False), hb.columns[tid].data)
        rows += b.num_rows
    assert rows == r.num_rows


@pytest.mark.parametrize("name,messages", CORRUPT_FILES)
def test_corrupt_files_fail_the_read_before_the_export(ctx, name, messages):
    r = orc_amd.Reader(path(name), ctx)
    with pytest.raises(orc_amd.ParseError) as ei:
        for i in range(r.num_stripes):
            r.read_stripe_arrow(i)
    assert any(m in str(ei.value) for m in messages), str(ei.value)
    with pytest.raises(Exception):
        f = po.ORCFile(path(name))
        for i in range(f.nstripes):
            f.read_stripe(i)


@pytest.mark.parametrize("name", NO_WRITER_ZONE)
def test_an_undecoded_column_fails_the_export_by_name(ctx, name):
    r = orc_amd.Reader(path(name), ctx)
    f = po.ORCFile(path(name))
    root = r.types[0]
    ts = [s for s in root.subtypes if r.types[s].kind == orc_amd.reader.TIMESTAMP]
    assert ts
    with pytest.raises(orc_amd.InvalidArgument, match="column %d was not decoded" % ts[0]):
        r.read_stripe_arrow(0)
    keep = [(s, n) for s, n in zip(root.subtypes, root.field_names) if s not in ts]
    r.select([s for s, _ in keep])
    for i in range(r.num_stripes):
        same_batch(r.read_stripe_arrow(i), f.read_stripe(i, columns=[n for _, n in keep]), "%s stripe %d" % (name, i))


# ---- files written with pyarrow.orc.write_table ----

CODECS = ["uncompressed", "zlib", "snappy", "lz4", "zstd"]
ROWS = 6000


def table(n=ROWS, seed=0):
    """Nulls in every column; nested list / map / struct; `low` is
    low-cardinality (dictionary-encoded), `high` all distinct (direct), `mixed`
    low-cardinality in the first stripe and distinct in the second."""
    import datetime
    import decimal

    rng = np.random.default_rng(seed)

    def nulls(values, typ=None, p=0.1):
        m = rng.random(n) < p
        return pa.array([None if x else v for v, x in zip(values, m)], type=typ)

    low = ["alpha", "", "beta-gamma", "x" * 40, "delta"]
    pick = rng.integers(0, len(low), n)
    ints = rng.integers(-2 ** 31, 2 ** 31, n)
    return pa.table({
        "b": nulls([bool(x) for x in rng.integers(0, 2, n)], pa.bool_()),
        "i8": nulls([int(x) for x in rng.integers(-128, 128, n)], pa.int8()),
        "i16": nulls([int(x) for x in rng.integers(-2 ** 15, 2 ** 15, n)], pa.int16()),
        "i32": nulls([int(x) for x in ints], pa.int32()),
        "i64": nulls([int(x) for x in rng.integers(-2 ** 62, 2 ** 62, n)], pa.int64()),
        "f32": nulls([float(np.float32(x)) for x in rng.standard_normal(n)], pa.float32()),
        "f64": nulls([float(x) for x in rng.standard_normal(n)], pa.float64()),
        "d64": nulls([decimal.Decimal(int(x)).scaleb(-3) for x in rng.integers(-10 ** 11, 10 ** 11, n)],
                     pa.decimal128(12, 3)),
        "d128": nulls([decimal.Decimal(int(x) * 10 ** 14 + 7).scaleb(-5) for x in rng.integers(-10 ** 15, 10 ** 15, n)],
                      pa.decimal128(30, 5)),
        "date": nulls([datetime.date(1970, 1, 1) + datetime.timedelta(days=int(x))
                       for x in rng.integers(-40000, 40000, n)], pa.date32()),
        "ts": nulls([int(x) for x in rng.integers(-2 ** 60, 2 ** 60, n)], pa.timestamp("ns")),
        "low": nulls([low[k] for k in pick], pa.string()),
        "high": nulls(["row-%d-%s" % (k, "y" * (k % 23)) for k in range(n)], pa.string()),
        "mixed": nulls([low[pick[k]] if k < n // 2 else "unique-%d" % k for k in range(n)], pa.string()),
        "bin": nulls([bytes([k % 251]) * (k % 9) for k in range(n)], pa.binary()),
        "list": nulls([[int(v) for v in ints[k:k + k % 4]] + ([None] if k % 11 == 0 else []) for k in range(n)],
                      pa.list_(pa.int32())),
        "map": nulls([[("k%d" % j, float(k + j)) for j in range(k % 3)] for k in range(n)],
                     pa.map_(pa.string(), pa.float64())),
        "struct": nulls([{"x": int(k), "y": None if k % 5 == 0 else low[k % 5]} for k in range(n)],
                        pa.struct([("x", pa.int64()), ("y", pa.string())])),
    })


_written = {}


def written(codec):
    """(file bytes, its table): written once per codec."""
    if codec not in _written:
        t = table()
        buf = io.BytesIO()
        po.write_table(t, buf, compression=codec, stripe_size=1024, batch_size=ROWS // 2,
                       dictionary_key_size_threshold=0.5)
        _written[codec] = (buf.getvalue(), t)
    return _written[codec]


@pytest.mark.parametrize("codec", CODECS)
def test_written_file_equals_pyarrow(ctx, codec):
    data, t = written(codec)
    f = po.ORCFile(io.BytesIO(data))
    assert f.nstripes == 2
    r = orc_amd.Reader(data, ctx)
    for i in range(2):
        same_batch(r.read_stripe_arrow(i), f.read_stripe(i), "%s stripe %d" % (codec, i))
    got = r.read_arrow()
    assert got.equals(f.read()) and got.equals(t.cast(got.schema))


def _ids(r):
    return dict(zip(r.types[0].field_names, r.types[0].subtypes))


def test_dictionary_export_round_trips(ctx):
    data, _ = written("zlib")
    r = orc_amd.Reader(data, ctx)
    ids = _ids(r)
    kinds = []
    for i in range(2):
        plain = r.read_stripe_arrow(i)
        d = r.read_stripe_arrow(i, dictionary=True)
        d.validate(full=True)
        assert d.schema.equals(r.arrow_schema(dictionary=True))
        for name in ("low", "high", "mixed"):
            col = d.column(name)
            is_dict = pa.types.is_dictionary(col.type)
            # the stripe's own encoding decides (DICTIONARY_V2 = 3)
            assert is_dict == (r.column_view(ids[name]).encoding == 3), (i, name)
            if is_dict:
                assert col.type == pa.dictionary(pa.int32(), pa.string())
                col = col.dictionary_decode()
            assert col.equals(plain.column(name)), (i, name)
            kinds.append((i, name, is_dict))
        # (nested strings -- struct.y, the map's keys -- are dictionaries too)
        assert pa.types.is_dictionary(d.column("struct").type.field("y").type)
        assert d.column("struct").field("y").dictionary_decode().equals(plain.column("struct").field("y"))
        strings = ["low", "high", "mixed", "struct", "map"]
        assert d.drop_columns(strings).equals(plain.drop_columns(strings))
    # low is dictionary-encoded, high (all distinct) direct; the ORC C++ writer
    # decides once a file, at its first row group, so `mixed` follows stripe 0
    assert [k for k in kinds if k[1] != "mixed"] == [(0, "low", True), (0, "high", False), (1, "low", True),
                                                     (1, "high", False)]


def _rle2(values):
    v = np.asarray(values, dtype=np.int64)
    lens = [min(512, v.size - i) for i in range(0, v.size, 512)]
    data, _ = orc_amd.encode_runs(v, False, np.ones(len(lens), np.uint8), np.array(lens, np.uint32))
    return bytes(data)


def test_a_column_that_changes_encoding_between_stripes(ctx):
    """A crafted file: column s is DICTIONARY_V2 in stripe 0 and DIRECT_V2 in
    stripe 1. With dictionary=True the first exports dictionary<int32,
    string>, the second plain string."""
    from orc_craft import (DATA, DICTIONARY_DATA, ENC_DICTIONARY_V2, ENC_DIRECT_V2, LENGTH, T_STRING, CraftColumn,
                           struct_file)

    entries = [b"", b"pear", b"fig", b"clementine-" * 3]
    idx = np.arange(1000) % 4
    dict_col = CraftColumn([(DATA, _rle2(idx)), (LENGTH, _rle2([len(e) for e in entries])),
                            (DICTIONARY_DATA, b"".join(entries))], encoding=ENC_DICTIONARY_V2,
                           dictionary_size=len(entries))
    rows = [b"row%d" % k for k in range(700)]
    direct_col = CraftColumn([(DATA, b"".join(rows)), (LENGTH, _rle2([len(x) for x in rows]))], encoding=ENC_DIRECT_V2)
    data = struct_file(["s"], [T_STRING], [(1000, [dict_col]), (700, [direct_col])], 0)
    f = po.ORCFile(io.BytesIO(data))
    r = orc_amd.Reader(data, ctx)
    for i, is_dict in ((0, True), (1, False)):
        want = f.read_stripe(i)
        same_batch(r.read_stripe_arrow(i), want, "stripe %d" % i)
        d = r.read_stripe_arrow(i, dictionary=True)
        d.validate(full=True)
        col = d.column("s")
        assert pa.types.is_dictionary(col.type) == is_dict
        assert d.schema.equals(r.arrow_schema(dictionary=True))
        if is_dict:
            assert col.dictionary.to_pylist() == [e.decode() for e in entries]
            col = col.dictionary_decode()
        assert col.equals(want.column("s"))
    assert r.read_arrow().equals(f.read())


def test_lazy_dictionary_reads_export_the_same(ctx):
    data, _ = written("snappy")
    r = orc_amd.Reader(data, ctx)
    want = r.read_stripe_arrow(0)
    r.set_lazy_dictionary(True)
    assert r.read_stripe_arrow(0).equals(want)
    assert r.read_stripe_arrow(0, dictionary=True).column("low").dictionary_decode().equals(want.column("low"))


def test_read_type_exports_the_read_kind(ctx):
    name = "TestOrcFile.testSnappy.orc"  # struct<int1:int,string1:string>
    r = orc_amd.Reader(path(name), ctx)
    want = po.ORCFile(path(name)).read_stripe(0)
    r.set_read_type("struct<int1:bigint,string1:string>")
    got = r.read_stripe_arrow(0)
    assert got.schema.field("int1").type == pa.int64()
    got.validate(full=True)
    assert got.column("int1").equals(want.column("int1").cast(pa.int64()))
    assert got.column("string1").equals(want.column("string1"))
    r.set_read_type("struct<int1:tinyint,string1:string>")  # values that do not fit read as NULL
    got = r.read_stripe_arrow(0)
    got.validate(full=True)
    v = want.column("int1").to_numpy(zero_copy_only=False)
    fits = (v >= -128) & (v <= 127)
    assert got.column("int1").equals(pa.array(v.astype(np.int8), mask=~fits))


def test_select_exports_the_selected_fields_only(ctx):
    data, _ = written("lz4")
    f = po.ORCFile(io.BytesIO(data))
    r = orc_amd.Reader(data, ctx)
    ids = _ids(r)
    names = ["i8", "low", "map", "struct"]
    r.select([ids[n] for n in names])
    same_batch(r.read_stripe_arrow(1), f.read_stripe(1, columns=names), "selected")
    r.select(None)
    assert r.read_stripe_arrow(1).num_columns == len(ids)


@pytest.mark.parametrize("name,tid,field", UNION_FILES)
def test_union_refusal_and_success_once_deselected(ctx, name, tid, field):
    r = orc_amd.Reader(path(name), ctx)
    f = po.ORCFile(path(name))
    with pytest.raises(orc_amd.InvalidArgument, match="union column %d is not exported to Arrow" % tid):
        r.read_stripe_arrow(0)
    root = r.types[0]
    keep = [(s, n) for s, n in zip(root.subtypes, root.field_names) if n != field]
    r.select([s for s, _ in keep])
    for i in range(r.num_stripes):
        same_batch(r.read_stripe_arrow(i), f.read_stripe(i, columns=[n for _, n in keep]), "%s stripe %d" % (name, i))


def test_char_column_exports_as_string(ctx):
    f = char_file()
    got = orc_amd.Reader(f, ctx).read_stripe_arrow(0)
    same_batch(got, po.ORCFile(io.BytesIO(f)).read_stripe(0), "char")
    assert got.column("c").to_pylist() == ["abc", "de ", "f  "]


def _flat_buffers(arr, path, out):
    """(path, buffer index, bytes) of a pyarrow array, depth first in the
    order Reader.arrow_device_buffers walks the device export."""
    for k, b in enumerate(arr.buffers()[:_nbuf(arr.type)]):
        out.append((path, k, None if b is None else b.to_pybytes()))
    if pa.types.is_dictionary(arr.type):
        _flat_buffers(arr.dictionary, path + "/dictionary", out)
    elif pa.types.is_struct(arr.type):
        for k in range(arr.type.num_fields):
            _flat_buffers(arr.field(k), path + "/" + arr.type.field(k).name, out)  # (field(): no slicing, offset 0)
    elif pa.types.is_map(arr.type):
        _flat_buffers(pa.StructArray.from_arrays([arr.keys, arr.items], names=["key", "value"]), path + "/entries", out)
    elif pa.types.is_list(arr.type):
        _flat_buffers(arr.values, path + "/item", out)


def _nbuf(t):
    if pa.types.is_struct(t):
        return 1
    if pa.types.is_list(t) or pa.types.is_map(t) or pa.types.is_dictionary(t):
        return 2
    return 3 if (pa.types.is_string(t) or pa.types.is_binary(t)) else 2


@pytest.mark.parametrize("dictionary", [False, True])
def test_device_export_holds_the_host_exports_bytes(ctx, dictionary):
    data, _ = written("zstd")
    r = orc_amd.Reader(data, ctx)
    batch = r.read_stripe_arrow(0, dictionary=dictionary)
    bufs, (device_type, device_id) = r.arrow_device_buffers(dictionary=dictionary)
    assert device_type == 10 and device_id == 0  # ARROW_DEVICE_ROCM
    want = [("", 0, None)]
    for name, col in zip(batch.schema.names, batch.columns):
        _flat_buffers(col, "/" + name, want)
    assert [(p, k) for p, k, _, _ in bufs] == [(p, k) for p, k, _ in want]
    checked = 0
    for (p, k, ptr, size), (_, _, raw) in zip(bufs, want):
        assert (ptr is None) == (raw is None), (p, k)
        if raw is None:
            continue
        assert ptr % 64 == 0 or size == 0 or k == 2 or p.endswith("/dictionary"), (p, k)
        got = r._host(ptr, size, np.uint8).tobytes() if size else b""
        assert got == raw[:size], (p, k)
        checked += 1
    assert checked > 40
