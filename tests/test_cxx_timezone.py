"""RowReaderOptions::setTimezoneName / getTimezoneName of the C++ adapter
(orc_amd/csrc/GpuRowReader.hh; c++/include/orc/Reader.hh:349-354): a small
program (tests/cxx/timezone_test.cpp) reads a US/Pacific file in a named zone
and prints its first timestamps; zone rules come from tests/golden/tz."""
import os
import subprocess

import pytest

import tz_model
from conftest import GOLDEN, ROOT
from file_parity import path

SRC = os.path.join(ROOT, "tests", "cxx", "timezone_test.cpp")
OUT = os.path.join(ROOT, "tests", "cxx", "build", "timezone_test")
TZ = os.path.join(GOLDEN, "tz")


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


def test_timezone_program_compiles_and_links():
    assert os.access(build_program(), os.X_OK)


def _zone(name):
    with open(os.path.join(TZ, name), "rb") as f:
        return tz_model.Zone(name, f.read())


@pytest.mark.gpu
def test_set_timezone_name_prints_three_rows():
    import orc_amd

    exe = build_program()
    name = "TestOrcFile.testDate1900.orc"
    env = dict(os.environ, TZDIR=TZ)
    # the writer's own wall-clock seconds: read in the writer's zone
    r = orc_amd.Reader(path(name), orc_amd.default_context(0))
    r.set_zone_rules("America/Los_Angeles", open(os.path.join(TZ, "America/Los_Angeles"), "rb").read())
    r.set_timezone("US/Pacific")
    tid = [i for i, t in enumerate(r.types) if t.kind == 9][0]
    c = r.read_stripe(0).columns[tid]
    la = _zone("America/Los_Angeles")
    for zone in ("GMT", "America/New_York", "Asia/Kolkata"):
        target = _zone(zone)
        p = subprocess.run([exe, path(name), zone, "3"], capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        want = ["%d %d" % (tz_model.convert(la, target, int(c.data[i])), int(c.secondary[i])) for i in range(3)]
        assert p.stdout.split("\n")[:3] == want, zone
    p = subprocess.run([exe, path(name), "Mars/Olympus_Mons"], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 1 and "Mars/Olympus_Mons" in p.stderr
