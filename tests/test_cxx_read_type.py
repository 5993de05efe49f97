"""orc_amd/csrc/read_type.hh, the host side of schema evolution: the
type-string parser (the inverse of Reader.type_string) and the check of a
file type against a read type. A host program (tests/cxx/read_type_test.cpp)
round-trips type strings, refuses malformed ones and compares the check for
every pair of kinds with a table written out by hand; built with
-fsanitize=address,undefined and run on its own."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_read_type_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "read_type_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cxx", "read_type_test.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    assert p.stdout == "read types ok\n"
