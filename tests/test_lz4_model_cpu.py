"""tests/lz4_model.py proved against pyarrow's raw LZ4 codec (liblz4), on
compressed random and repetitive buffers, on every built stream of the GPU
tests that liblz4 accepts too (tests/lz4_cases.py), and on 24,000 mutated
blocks; orcg_lz4_plan equals the model's plan exactly, errors included. No GPU.

pyarrow's decompress returns a buffer of the capacity it was given, whatever
liblz4 wrote: at a capacity above a block's size only the leading bytes are
compared."""
import numpy as np
import pyarrow as pa
import pytest

import orc_amd
import lz4_cases as C
import lz4_model as M

R, THREADS = orc_amd.lz4_device_info()


def pa_decode(block, cap):
    return pa.decompress(block, decompressed_size=cap, codec="lz4_raw", asbytes=True)


def pa_accepts(block, cap):
    try:
        return pa_decode(block, cap)
    except Exception:  # pyarrow raises OSError / ArrowInvalid by version
        return None


def _buffers():
    rng = np.random.default_rng(5)
    yield b""
    yield b"a"
    yield rng.integers(0, 256, 10000, dtype=np.uint8).tobytes()             # incompressible: literals
    yield b"abc" * 5000                                                     # overlapping matches
    yield bytes(70000)                                                      # offset 1, a long match
    yield rng.integers(0, 4, 100000, dtype=np.uint8).tobytes()              # short matches
    words = [rng.integers(97, 123, int(k), dtype=np.uint8).tobytes() for k in rng.integers(2, 12, 200)]
    yield b" ".join(words[int(i)] for i in rng.integers(0, 200, 30000))     # text
    yield rng.integers(0, 256, 65000, dtype=np.uint8).tobytes() * 3         # matches 65,000 back
    yield rng.integers(0, 3, 300000, dtype=np.uint8).tobytes()


def test_device_info():
    assert R == 65536 and THREADS == 64  # every LZ4 offset lies inside the history


@pytest.mark.parametrize("i", range(9))
def test_model_decodes_pyarrow_blocks(i):
    data = list(_buffers())[i]
    block = pa.compress(data, codec="lz4_raw", asbytes=True)
    assert M.decode(block, len(data)) == data
    assert M.decode(block, C.BLOCK * 2) == data
    assert M.size(block, len(data)) == len(data)
    if data:
        assert M.decode(block, len(data) - 1) == M.CORRUPT
        assert M.size(block, len(data) - 1) == M.CORRUPT


def test_model_equals_pyarrow_on_built_streams():
    refused = set()
    for name, chunks in C.good_cases(R).items():
        for body, stored in chunks:
            if stored:
                continue
            want = M.decode(body, C.BLOCK)
            assert isinstance(want, bytes), name
            assert M.size(body, C.BLOCK) == len(want) == M.size(body, len(want)), name
            got = pa_accepts(body, len(want))
            if got is None:
                refused.add(name)
            else:
                assert got == want, name
    # liblz4 refuses only blocks that end closer to a match than its margins allow
    assert refused <= C.RULES_ONLY, refused - C.RULES_ONLY
    assert {"only_these_rules_final_0", "only_these_rules_final_1"} <= refused


def test_built_streams_decode_to_what_they_were_built_from():
    s = M.Stream(3).literal(100).match(64, 3).match(11, 100).match(300, 170).literal(61)
    assert M.decode(s.block(), C.BLOCK) == bytes(s.out) and len(s.out) == 536
    for n in (0, 14, 15, 269, 270, 271, 70000):
        data = M.Stream(n)._fill(n)
        e = M.sequence(data)
        assert len(e) == 1 + n + (0 if n < 15 else (n - 15) // 255 + 1)
        assert M.decode(e, C.BLOCK) == data
    assert M.sequence(b"") == b"\x00" and M.decode(b"\x00", 0) == b""


def test_cases_hold_what_they_name():
    cases = C.good_cases(R)
    assert [len(M.decode(b, C.BLOCK)) for b, _ in cases["match_ends_block"]] == [R - 1, R, R + 1, 65535 + 64, 2 * R + 1]
    assert [len(M.decode(b, C.BLOCK)) for b, _ in cases["ring_sizes"]] == [2 * R - 1, 2 * R, 2 * R + 1, R - 1, R, R + 1]
    assert len(cases["chunks_257"]) == 257 and len(cases["chunks_2"]) == 2 and len(cases["chunks_1"]) == 1
    assert [len(M.decode(b, C.BLOCK)) for b, _ in cases["sizes"]] == [0, 1, 63, 64, 65, 4095, 4096, 4097]
    (body, _), = cases["match_300_extension_bytes"]
    assert body.count(b"\xff") >= 299 and len(body) < 340
    (body, _), = cases["long_match_off_65535"]
    assert len(M.decode(body, C.BLOCK)) == 65535 + 150000 + C.END
    assert max(len(M.decode(b, C.BLOCK)) if not st else len(b) for ch in cases.values() for b, st in ch) <= C.BLOCK


def test_crafted_chunks_fail_with_the_one_text():
    for name, (chunks, index) in C.bad_cases().items():
        fails = [i for i, (b, st, dst) in enumerate(chunks) if not st and M.decode_exact(b, dst) == M.CORRUPT]
        assert fails and fails[0] == index, name
        if len(chunks) == 1:
            (b, _, dst), = chunks
            # the walk itself fails, or (an edited table) ends elsewhere than the table says
            assert M.size(b, dst) != dst, name
    assert M.CORRUPT == "Corrupt lz4 compressed block"


def _assert_plan_equal(framed, block):
    want = M.plan(framed, block)
    if isinstance(want, str):
        with pytest.raises(orc_amd.ParseError) as e:
            orc_amd.lz4_plan(framed, block)
        assert str(e.value) == want
    else:
        table, total = orc_amd.lz4_plan(framed, block)
        assert total == want[1]
        assert table.tolist() == [list(r) for r in want[0]]


def _text(r):
    return r if isinstance(r, str) else "ok"


def test_library_plan_equals_model_plan():
    for name, chunks in C.good_cases(R).items():
        _assert_plan_equal(b"".join(M.frame(b, st) for b, st in chunks), C.BLOCK)
    for name, (chunks, _) in C.bad_cases().items():
        _assert_plan_equal(b"".join(M.frame(b, st) for b, st, _ in chunks), C.BLOCK)
    _assert_plan_equal(b"", 1024)


def test_library_plan_errors_equal_model():
    a = M.Stream(1).literal(100).match(30, 7).literal(C.END).block()
    framed = M.frame(a) + M.frame(b"stored bytes", True) + M.frame(M.Stream(2).literal(2000).block())
    seen = set()
    for cut in range(len(framed)):  # a cut frame header, a cut body
        _assert_plan_equal(framed[:cut], 4096)
        seen.add(_text(M.plan(framed[:cut], 4096)))
    for block in (141, 142, 143, 1999, 2000, 1 << 31, 1 << 40):  # an oversize block
        _assert_plan_equal(framed, block)
        seen.add(_text(M.plan(framed, block)))
    for at in range(len(framed)):  # a corrupt body (or header)
        for v in (0x00, 0xFF, framed[at] ^ 0x10):
            _assert_plan_equal(framed[:at] + bytes([v]) + framed[at + 1:], 4096)
    assert {M.PAST_EOF, M.CORRUPT, "ok"} <= seen
    assert M.plan(framed, 141) == M.CORRUPT and isinstance(M.plan(framed, 2000), tuple)


def _mutants(count):
    """liblz4-compressed word soup with 0-3 byte edits, truncations and
    appended bytes, each with a capacity from exact to generous."""
    rng = np.random.default_rng(77)
    words = [rng.integers(97, 123, int(k), dtype=np.uint8).tobytes() for k in rng.integers(1, 9, 60)]
    made = 0
    while made < count:
        n = int(rng.integers(1, 400))
        data = b" ".join(words[int(i)] for i in rng.integers(0, 60, n))[:int(rng.integers(1, 1500))]
        block = bytearray(pa.compress(data, codec="lz4_raw", asbytes=True))
        for _ in range(12):
            b = bytearray(block)
            for _ in range(int(rng.integers(0, 4))):
                b[int(rng.integers(0, len(b)))] = int(rng.choice([0, 0xFF, int(rng.integers(0, 256))]))
            shape = int(rng.integers(0, 6))
            if shape == 0:
                b = b[:int(rng.integers(0, len(b) + 1))]
            elif shape == 1:
                b += rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8).tobytes()
            cap = len(data) + int(rng.choice([0, 0, 1, 7, 64, 5000]))
            made += 1
            yield bytes(b), cap


def test_model_contains_liblz4_on_mutated_blocks():
    total = both = zero = only_model = 0
    for block, cap in _mutants(24000):
        total += 1
        got = pa_accepts(block, cap)
        want = M.decode(block, cap, why=True)
        if got is None:
            only_model += isinstance(want, bytes)
            continue
        if want == M.ZERO_OFFSET:
            zero += 1  # liblz4 1.9.3 does not check it: the documented difference
            continue
        # whatever liblz4 accepts these rules accept, with its bytes
        assert isinstance(want, bytes), (block, cap, want)
        assert got[:len(want)] == want, (block, cap)
        assert M.size(block, cap) == len(want)
        both += 1
    assert total >= 20000
    assert both * 3 >= total, (both, total)
    assert zero * 20 < total, (zero, total)
    print("blocks %d, both %d, zero offsets %d, these rules only %d" % (total, both, zero, only_model))
