"""orc_amd/csrc/rlev2_route.hh, the RLEv2 launch routing: a host program
(tests/cxx/rlev2_route_test.cpp, its own main, no HIP) pins the density rule,
the segments-per-CU test, the two-pass shape, its addressing limits and the
grouping of multi-stream launches; built once plain and once with
-fsanitize=address,undefined, and each run on its own. The same program then
answers for every RLE stream of the crafted files M, S and F, and its answers
must be those of the rules' Python restatements (multi_stream_files
density_class and seg_value_bound, rlev2_model.two_pass_shape), which the
crafted-file tests reason with."""
import os
import shutil
import subprocess

import pytest

import multi_stream_files as msf
import rlev2_model
from conftest import ROOT

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g"] + SANITIZE}


@pytest.fixture(scope="module", params=list(BUILDS))
def program(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rlev2_route_" + request.param) / "rlev2_route_test")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                   [os.path.join(ROOT, "tests", "cxx", "rlev2_route_test.cpp"),
                    os.path.join(ROOT, "orc_amd", "csrc", "rlev2_route.cpp"), "-o", exe], check=True)
    return exe


def run(exe, args=(), stdin=""):
    p = subprocess.run([exe] + list(args), input=stdin, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    return p.stdout


def test_rlev2_route_program(program):
    assert run(program) == "rlev2 routes ok\n"


def crafted_streams():
    """(src_len, values, nsegs) of every RLE stream of M, S and F, with the
    segments the reader cuts them into: a row group each where the row index
    has positions for the stream, else one."""
    out = []
    for f in (msf.file_m(), msf.file_s(), msf.file_f()):
        for k, (n, _) in enumerate(f.stripes):
            groups = (n + f.stride - 1) // f.stride
            out += [(len(s.data), s.values.size, groups if s.indexed else 1) for _, s in f.rle_streams(k)]
    return out


def test_the_python_restatements_are_the_routing_units(program):
    streams = crafted_streams()
    assert len(streams) == 11 + 3 * 11 + 3
    got = [tuple(map(int, ln.split())) for ln in run(program, ["streams"], "".join("%d %d %d\n" % s for s in streams)).splitlines()]
    want = [(msf.density_class(b, v), msf.seg_value_bound(v, g)) + rlev2_model.two_pass_shape(v, g) for b, v, g in streams]
    assert got == want
    assert {c for c, _, _, _ in got} == {2, 3, 6}  # the files reach every class (test_density_classes_and_job_order)
