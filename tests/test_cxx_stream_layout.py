"""orc_amd/csrc/reader_layout.hh, the one description of which streams each
column kind reads (order, coding, signedness, count source): a host program
(tests/cxx/stream_layout_test.cpp) checks it against lists written out by
hand, built with -fsanitize=address,undefined and run on its own."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_stream_layout_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "stream_layout_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cxx", "stream_layout_test.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    assert p.stdout == "stream layouts ok\n"
