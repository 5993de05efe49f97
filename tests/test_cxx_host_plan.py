"""orc_amd/csrc/host_plan.hh, the host stream planners and the seek lookup:
pure byte walks over untrusted input. A host program
(tests/cxx/host_plan_test.cpp) runs them over every truncation of a short mixed
stream of each format and every single-byte corruption of its first 64 bytes,
each stream in a buffer of exactly its length, and checks the plans'
invariants; built with -fsanitize=address,undefined and run on its own."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_host_plan_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "host_plan_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cxx", "host_plan_test.cpp"),
                    os.path.join(ROOT, "orc_amd", "csrc", "host_plan.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    assert p.stdout == "host plans ok\n"
