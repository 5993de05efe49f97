"""The Arrow schema of a file (orcg_reader_arrow_schema, Reader.arrow_schema)
against pyarrow's own ORC reader, which maps the same file to Arrow types on
the CPU (pyarrow.orc.ORCFile(f).schema). Host only: the readers are opened
without a device context. Field and schema metadata (ORC type attributes,
user metadata) are not exported, so schemas compare without metadata."""
import glob
import io
import os

import numpy as np
import pytest

import orc_amd
from file_parity import FILES, path
from orc_craft import DATA, ENC_DIRECT_V2, LENGTH, CraftColumn, field_varint, struct_file, type_msg

pa = pytest.importorskip("pyarrow")
po = pytest.importorskip("pyarrow.orc")

# Files pyarrow does not open as a table, by name: the top level is not a
# struct ("Only ORC files with a top-level struct can be handled"), or the file
# is empty bytes
NOT_A_STRUCT = ["TestOrcFile.testTimestamp.orc", "TestOrcFile.testWithoutCompressionBlockSize.orc"]
NOT_A_FILE = ["zero.orc"]
# Files with a union column (checked with pyarrow: the one golden file whose
# schema holds a sparse_union): (file, the union's type id, its field name)
UNION_FILES = [("TestOrcFile.testUnionAndTimestamp.orc", 2, "union")]

ALL = sorted(os.path.basename(f) for f in glob.glob(os.path.join(FILES, "*.orc")))
PLAIN = [f for f in ALL if f not in NOT_A_STRUCT + NOT_A_FILE + [u[0] for u in UNION_FILES]]


def test_the_lists_name_golden_files():
    for f in NOT_A_STRUCT + NOT_A_FILE + [u[0] for u in UNION_FILES]:
        assert f in ALL, f
    assert len(PLAIN) >= 40
    # no other golden file holds a union
    for f in PLAIN:
        assert not any(pa.types.is_union(fld.type) for fld in po.ORCFile(path(f)).schema), f


@pytest.mark.parametrize("name", PLAIN)
def test_schema_matches_pyarrow(name):
    want = po.ORCFile(path(name)).schema
    r = orc_amd.Reader(path(name))  # no device context
    got = r.arrow_schema()
    assert isinstance(got, pa.Schema)
    assert got.equals(want, check_metadata=False), "%s\n%s\n-- pyarrow --\n%s" % (name, got, want)
    # no stripe was decoded: the dictionary flag changes nothing
    assert r.arrow_schema(dictionary=True).equals(want, check_metadata=False)


@pytest.mark.parametrize("name", NOT_A_STRUCT)
def test_top_level_must_be_a_struct(name):
    with pytest.raises(Exception, match="top-level struct"):
        po.ORCFile(path(name)).schema
    r = orc_amd.Reader(path(name))
    with pytest.raises(orc_amd.InvalidArgument, match="top level is not a struct"):
        r.arrow_schema()


@pytest.mark.parametrize("name,tid,field", UNION_FILES)
def test_union_is_refused_until_deselected(name, tid, field):
    want = po.ORCFile(path(name)).schema
    assert pa.types.is_union(want.field(field).type)
    r = orc_amd.Reader(path(name))
    assert orc_amd.reader.KIND_NAMES[r.types[tid].kind] == "uniontype"
    with pytest.raises(orc_amd.InvalidArgument, match="union column %d is not exported to Arrow" % tid):
        r.arrow_schema()
    root = r.types[0]
    r.select([s for s, n in zip(root.subtypes, root.field_names) if n != field])
    got = r.arrow_schema()
    assert got.equals(want.remove(want.get_field_index(field)), check_metadata=False), got
    r.select(None)
    with pytest.raises(orc_amd.InvalidArgument, match="union column %d" % tid):
        r.arrow_schema()


def test_selection_and_nesting():
    r = orc_amd.Reader(path("TestOrcFile.test1.orc"))
    want = po.ORCFile(path("TestOrcFile.test1.orc")).schema
    ids = dict(zip(r.types[0].field_names, r.types[0].subtypes))
    r.select([ids["map"], ids["byte1"]])
    got = r.arrow_schema()
    assert got.names == ["byte1", "map"]
    assert got.field("map").equals(want.field("map")) and got.field("byte1").equals(want.field("byte1"))
    m = got.field("map").type
    assert pa.types.is_map(m) and not m.key_field.nullable and m.item_field.nullable


def test_schema_under_a_read_type():
    name = "TestOrcFile.testSnappy.orc"  # struct<int1:int,string1:string>
    r = orc_amd.Reader(path(name))
    assert r.arrow_schema().field("int1").type == pa.int32()
    r.set_read_type("struct<a:bigint,string1:string>")
    got = r.arrow_schema()
    # the read kind, the file's field names
    assert got.equals(pa.schema([("int1", pa.int64()), ("string1", pa.string())]))
    r.set_read_type("struct<a:decimal(20,2),string1:string>")
    assert r.arrow_schema().field("int1").type == pa.decimal128(20, 2)
    r.set_read_type(None)
    assert r.arrow_schema().equals(po.ORCFile(path(name)).schema)


def test_hive11_decimal_follows_the_forced_scale():
    r = orc_amd.Reader(path("orc_split_elim.orc"))
    assert r.types[4].kind == 14 and r.types[4].precision == 0  # a Hive 0.11 decimal
    assert r.arrow_schema().field("decimal1").type == pa.decimal128(38, 6)
    r.set_hive11_decimal(forced_scale=4)
    assert r.arrow_schema().field("decimal1").type == pa.decimal128(38, 4)


def _rle2(values):
    v = np.asarray(values, dtype=np.int64)
    data, _ = orc_amd.encode_runs(v, False, np.ones(1, np.uint8), np.array([v.size], np.uint32))
    return bytes(data)


def char_file():
    """struct<c:char(3),v:varchar(5)>, three rows, direct encoding."""
    char_t = type_msg(17) + field_varint(4, 3)
    varchar_t = type_msg(16) + field_varint(4, 5)
    c = CraftColumn([(DATA, b"abcde f  "), (LENGTH, _rle2([3, 3, 3]))], encoding=ENC_DIRECT_V2)
    v = CraftColumn([(DATA, b"xyzuvw"), (LENGTH, _rle2([1, 2, 3]))], encoding=ENC_DIRECT_V2)
    return struct_file(["c", "v"], [char_t, varchar_t], [(3, [c, v])], 0)


def test_char_and_varchar_are_strings():
    """No golden file has a char column: a crafted one. pyarrow reads char(n)
    as string (not fixed_size_binary), and so does the export."""
    f = char_file()
    want = po.ORCFile(io.BytesIO(f)).schema
    r = orc_amd.Reader(f)
    assert r.type_string() == "struct<c:char(3),v:varchar(5)>"
    got = r.arrow_schema()
    assert got.equals(want) and got.field("c").type == pa.string() and got.field("v").type == pa.string()
