"""tests/snappy_model.py proved against pyarrow's raw Snappy codec, on random
and repetitive buffers and on every built stream of the GPU tests
(tests/snappy_cases.py); orcg_snappy_plan equals the model's plan exactly. No
GPU."""
import numpy as np
import pyarrow as pa
import pytest

import orc_amd
import snappy_cases as C
import snappy_model as M

R, THREADS = orc_amd.snappy_device_info()
CODEC = pa.Codec("snappy")


def pa_decode(block, size):
    return pa.decompress(block, decompressed_size=size, codec="snappy", asbytes=True)


def _buffers():
    rng = np.random.default_rng(5)
    yield b""
    yield b"a"
    yield rng.integers(0, 256, 10000, dtype=np.uint8).tobytes()             # incompressible: literals
    yield b"abc" * 5000                                                     # overlapping copies
    yield bytes(70000)                                                      # offset 1
    yield rng.integers(0, 4, 100000, dtype=np.uint8).tobytes()              # short matches
    words = [rng.integers(97, 123, int(k), dtype=np.uint8).tobytes() for k in rng.integers(2, 12, 200)]
    yield b" ".join(words[int(i)] for i in rng.integers(0, 200, 30000))     # text: copy-1 and copy-2
    yield rng.integers(0, 256, 70000, dtype=np.uint8).tobytes() * 3         # matches 70,000 back


def test_device_info():
    assert R >= 64 and R & (R - 1) == 0 and THREADS == 64


@pytest.mark.parametrize("i", range(8))
def test_model_decodes_pyarrow_blocks(i):
    data = list(_buffers())[i]
    block = CODEC.compress(data, asbytes=True)
    assert M.decode(block) == data
    assert M.decode(block, cap=len(data)) == data
    if data:
        assert M.decode(block, cap=len(data) - 1) == M.TOO_LARGE


def test_pyarrow_blocks_use_literals_and_short_copies():
    # (the compressor works in 64 KB fragments and never emits a copy-4: those
    # come from the built streams, which pyarrow decodes below)
    kinds = set()
    for data in _buffers():
        block = CODEC.compress(data, asbytes=True)
        _, p = M.preamble(block)
        while p < len(block):
            tag = block[p]
            kinds.add(tag & 3)
            if tag & 3 == 0:
                ln = (tag >> 2) + 1
                nb = ln - 60 if ln > 60 else 0
                if nb:
                    ln = int.from_bytes(block[p + 1:p + 1 + nb], "little") + 1
                p += 1 + nb + ln
            else:
                p += (0, 2, 3, 5)[tag & 3]
    assert kinds >= {0, 1, 2}


def test_pyarrow_decodes_built_streams():
    for name, chunks in C.good_cases(R).items():
        for body, stored in chunks:
            if stored:
                continue
            want = M.decode(body, C.BLOCK)
            assert isinstance(want, bytes), (name, want)
            if want:
                assert pa_decode(body, len(want)) == want, name


def test_built_streams_decode_to_what_they_were_built_from():
    s = M.Stream(3).literal(100).copy(64, 3, kind=2).copy(11, 100, kind=1).copy(64, 170, kind=4).literal(61)
    assert M.decode(s.block()) == bytes(s.out) and len(s.out) == 300
    for extra, n in ((0, 60), (1, 61), (2, 300), (3, 70000), (4, 5)):
        data = M.Stream(n)._fill(n)
        e = M.literal(data, extra)
        assert len(e) == 1 + extra + n
        assert M.decode(M.varint(n) + e) == data


def test_ring_cases_reach_what_they_name():
    cases = C.good_cases(R)
    for total in (R - 1, R, R + 1, 2 * R + 1):
        for reach in (R - 1, R, R + 1):
            if reach < total:
                (body, _), = cases["ring_%d_reach_%d" % (total, reach)]
                assert len(M.decode(body, C.BLOCK)) == total
    (body, _), = cases["far_copy"]
    assert len(body) > 262144 - 200 and len(M.decode(body, C.BLOCK)) == 262144
    assert len(cases["chunks_257"]) == 257 and len(cases["chunks_2"]) == 2 and len(cases["chunks_1"]) == 1
    assert [len(M.decode(b, C.BLOCK)) for b, _ in cases["sizes"]] == [0, 1, 63, 64, 65, 4095, 4096, 4097]


def test_crafted_chunks_fail_their_check():
    for name, (chunks, index, text) in C.bad_cases().items():
        framed = b"".join(M.frame(b, st) for b, st in chunks)
        out, err = M.decode_framed(framed, C.BLOCK)
        assert out is None and err == (index, text), name
        assert isinstance(M.plan(framed, C.BLOCK), tuple), name  # the preambles are sound
    # pyarrow refuses them too
    for name, (chunks, index, text) in C.bad_cases().items():
        if len(chunks) == 1:
            with pytest.raises(Exception):
                pa_decode(chunks[0][0], M.preamble(chunks[0][0])[0])


def _assert_plan_equal(framed, block):
    want = M.plan(framed, block)
    if isinstance(want, str):
        with pytest.raises(orc_amd.ParseError) as e:
            orc_amd.snappy_plan(framed, block)
        assert str(e.value) == want
    else:
        table, total = orc_amd.snappy_plan(framed, block)
        assert total == want[1]
        assert table.tolist() == [list(r) for r in want[0]]


def _text(r):
    return r if isinstance(r, str) else "ok"


def test_library_plan_equals_model_plan():
    for name, chunks in list(C.good_cases(R).items()) + [(k, v[0]) for k, v in C.bad_cases().items()]:
        _assert_plan_equal(b"".join(M.frame(b, st) for b, st in chunks), C.BLOCK)
    _assert_plan_equal(b"", 1024)


def test_library_plan_errors_equal_model():
    a = M.Stream(1).literal(100).copy(30, 7).block()
    framed = M.frame(a) + M.frame(b"stored bytes", True) + M.frame(M.Stream(2).literal(2000).block())
    seen = set()
    for cut in range(len(framed)):
        _assert_plan_equal(framed[:cut], 1024)
    for block in (99, 100, 129, 130, 1999, 2000):
        _assert_plan_equal(framed, block)
        seen.add(_text(M.plan(framed, block)))
    # preambles: cut, overlong, too many bytes
    for pre in (b"", b"\x80", b"\x80\x80\x80\x80\x80\x80", b"\xff\xff\xff\xff\xff\x01", b"\xff\xff\xff\xff\x7f",
                b"\x80\x80\x80\x80\x80\x00"):
        f = M.frame(pre)
        seen.add(_text(M.plan(f, 1 << 40)))
        _assert_plan_equal(f, 1 << 40)
        _assert_plan_equal(f, 1024)
    assert {M.BAD_LENGTH, M.TOO_LARGE, "ok"} <= seen
