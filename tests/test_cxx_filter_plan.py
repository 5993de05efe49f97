"""orc_amd/csrc/filter_plan.hh, the row-level filter's host half: a host
program (tests/cxx/filter_plan_test.cpp, its own main, no HIP) runs malformed
programs, every limit at its edge and one past, every refusal with its text,
the NOT push-down, and IN sorting and de-duplication; built once plain and once
with -fsanitize=address,undefined, and each run on its own."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SANITIZE], ids=["plain", "sanitized"])
def test_filter_plan_program(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "filter_plan_test")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags +
                   [os.path.join(ROOT, "tests", "cxx", "filter_plan_test.cpp"),
                    os.path.join(ROOT, "orc_amd", "csrc", "filter_plan.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    assert p.stdout == "filter plans ok\n"
