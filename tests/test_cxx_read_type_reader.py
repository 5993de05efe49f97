"""Schema evolution through the C++ RowReader adapter (GpuRowReader.hh:
RowReaderOptions::setReadType / throwOnSchemaEvolutionOverflow) with tight
numeric vectors: tests/cxx/read_type_reader_test.cpp reads files written here
with pyarrow under a read type; every cell is compared with the model of the
reference's rules (tests/convert_model.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import convert_model as M
from conftest import ROOT
from convert_cases import reference_tests

SRC = os.path.join(ROOT, "tests", "cxx", "read_type_reader_test.cpp")
OUT = os.path.join(ROOT, "tests", "cxx", "build", "read_type_reader_test")
TIGHT_CLASS = {"boolean": "byte", "tinyint": "byte", "smallint": "short", "int": "int", "bigint": "long",
               "float": "float", "double": "double"}


def build_program():
    from orc_amd import build as orc_build

    orc_build.build()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SRC, "-o", OUT,
        "-L" + os.path.join(ROOT, "orc_amd"), "-lorcgpu", "-Wl,-rpath," + os.path.join(ROOT, "orc_amd"),
        "-Wl,-rpath,/opt/rocm/lib",
    ])
    return OUT


def test_read_type_adapter_compiles_and_links():
    assert os.access(build_program(), os.X_OK)


def class_of(t):
    k, p, _ = M.parse(t)
    return ("decimal64" if p <= 18 else "decimal128") if k == "decimal" else TIGHT_CLASS[k]


def cell(v, t):
    """a model value as read_type_reader_test prints it"""
    k, _, s = M.parse(t)
    if v is None:
        return "N"
    if k == "decimal":
        return "%d@%d" % (v, s)
    if k == "float":
        return "f%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]
    if k == "double":
        return "d%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    return str(int(v))


def run(path, read_type, *args):
    r = subprocess.run([build_program(), str(path), read_type] + [str(a) for a in args], capture_output=True,
                       text=True, timeout=120)
    return r.returncode, r.stdout.splitlines(), r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(reference_tests()))
def test_reference_tests_through_the_adapter(tmp_path, name):
    from test_gpu_read_type import _holding, read_type_of, write

    cols = [c._replace(src=_holding(c.src, c.values)) for c in reference_tests()[name]]
    p = tmp_path / "f.orc"
    write(p, [("c%d" % i, c.src, c.values) for i, c in enumerate(cols)])
    rc, lines, err = run(p, read_type_of([c.dst for c in cols]), "--batch", 300)
    assert rc == 0, (rc, lines[-3:], err[-2000:])
    # batches are built from the read type; a row reader without one keeps the file's
    assert lines[0].split() == ["#classes"] + [class_of(c.dst) for c in cols]
    assert lines[1].split() == ["#plain"] + [class_of(c.src) for c in cols]
    want = [[cell(M.convert(v, c.src, c.dst), c.dst) for v in c.values] for c in cols]
    rows = [ln.split() for ln in lines[2:]]
    assert len(rows) == len(cols[0].values)
    for i, row in enumerate(rows):
        assert row == [w[i] for w in want], "row %d" % i


@pytest.mark.gpu
def test_tight_vector_exception_and_throw_mode(tmp_path):
    from test_gpu_read_type import write

    p = tmp_path / "f.orc"
    write(p, [("a", "bigint", [1, 2, 1 << 40, 4]), ("b", "double", [0.5, 1e30, 2.5, -1.0])])
    read_type = "struct<a:int,b:decimal(10,2)>"
    rc, lines, _ = run(p, read_type, "--loose")
    assert rc == 2 and lines == ["#error SchemaEvolution only support tight vector, please create ColumnVectorBatch "
                                 "with option useTightNumericVector"]
    rc, lines, _ = run(p, read_type, "--throw")
    assert rc == 2 and lines[-1] == "#error Overflow when convert from bigint to int"
    rc, lines, _ = run(p, read_type)
    assert rc == 0 and lines[2:] == ["1 50@2", "2 N", "N 250@2", "4 -100@2"]
    rc, lines, _ = run(p, "struct<a:string,b:double>")
    assert rc == 2 and lines == ["#error Conversion from bigint to string is not supported"]
