"""orc_amd/csrc/inflate_plan.hh, the LZ4 size walk and chunk planner: a byte
walk over untrusted input. A host program (tests/cxx/lz4_plan_test.cpp) runs it
over every truncation and every single-byte corruption of a short multi-chunk
stream, each in a buffer of exactly its length, checks the tables' invariants
and decodes every chunk the walk accepts into a buffer of exactly its size;
built with -fsanitize=address,undefined and run on its own."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_lz4_plan_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "lz4_plan_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cxx", "lz4_plan_test.cpp"),
                    os.path.join(ROOT, "orc_amd", "csrc", "inflate_plan.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    assert p.stdout == "lz4 plans ok\n"
