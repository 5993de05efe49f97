"""The built LZ4 streams of tests/test_gpu_lz4_shapes.py, shared with
tests/test_lz4_model_cpu.py (which proves the model on them). A good case is a
list of chunks, each (body bytes, stored?); a bad case's chunks carry the
table's dst_bytes as well, since a corrupt block has no plan. The edge shapes
derive from R, the kernel's history size (orcg_lz4_device_info).

A block that ends with a literal run of at least END bytes keeps liblz4's
end-of-block margins, so liblz4 accepts it too; the cases named in RULES_ONLY
hold blocks that end closer to a match, which only this project's rules
accept."""
import functools

import lz4_model as M

BLOCK = 262144  # the largest ORC compression block
END = 12        # liblz4: a literal that is not the last ends 12 bytes before the output's end
MAX_OFF = 65535


def _mixed(total, seed):
    """A block of `total` output bytes: literals and matches, near and far,
    short and extended. Ends as the byte count falls (often on a match)."""
    s = M.Stream(seed)
    step = 0
    while s.o < total:
        left = total - s.o
        step += 1
        if s.o == 0 or step % 3 == 1 or left < 4:
            s.literal(min(left, 1 + (step * 37) % 90))
        elif step % 3 == 2:
            s.match(min(left, 4 + (step * 11) % 70), 1 + (step * 7) % min(s.o, 3000))
        else:
            s.match(min(left, 4 + step % 8), 1 + (step * 5) % min(s.o, 60))
    assert s.o == total
    return s


def _ring_edge(total, R):
    """Filler, a match at reach 65,535 placed at o == 65,535 where the block is
    long enough, and a match at the farthest reach that ends the block at
    `total` (a final literal run of 0 bytes)."""
    s = M.Stream(total * 31)
    if total >= MAX_OFF + 64 + 64:
        s.fill_to(MAX_OFF).match(64, MAX_OFF)  # off == o
    ln = min(64, total - max(s.o, 4))
    reach = min(MAX_OFF, total - ln)
    s.fill_to(total - ln).match(ln, reach)
    assert s.o == total
    return s


RULES_ONLY = {"only_these_rules_final_0", "only_these_rules_final_1", "sizes", "stored_mixed", "chunks_1", "chunks_2",
              "chunks_257", "match_ends_block"}


@functools.lru_cache(maxsize=None)
def good_cases(R):
    """name -> [(body, stored)], every chunk valid."""
    cases = {}

    def one(name, *streams):
        cases[name] = [(s.block(), False) for s in streams]

    lits = (0, 1, 14, 15, 16, 269, 270, 271, 525, 4095, 4096, 4097, R + 1)
    one("literal_only", *[M.Stream(n).literal(n) for n in lits])  # 0: the one-byte block 00
    one("literal_then_match", *[M.Stream(n + 1).literal(n).match(4, 1 + n % min(n, 3)).literal(END) for n in lits if n])
    big = M.Stream(5).literal(65550)
    assert len(M.sequence(big.pending)) - 65550 - 1 > 256  # more extension bytes than a slice holds
    one("literal_65550", big, M.Stream(6).literal(70001).match(9, 65000).literal(END))
    for ln in (4, 5, 18, 19, 20, 63, 64, 65, 127, 128, 129, 273, 274, 275, 4100):
        one("match_len_%d" % ln, *[M.Stream(off).literal(max(off, 3)).match(ln, off).literal(END)
                                   for off in (1, 3, 7, 64, 100, 300)])
    ext = M.Stream(7).literal(1).match(4 + 15 + 299 * 255 + 7, 1).literal(END)
    assert len(ext.block()) < 340 and ext.o > 76000
    one("match_300_extension_bytes", ext)
    offs = list(range(1, 9)) + [15, 16, 17, 63, 64, 65, 255, 256, 4095, 4096, R - 65, R - 64, R - 63, MAX_OFF]
    for ln in (4, 64, 65, 200):
        # off = 3, len = 200: the phase crosses three steps
        one("offsets_len_%d" % ln, *[M.Stream(off).literal(off).match(ln, off).literal(END) for off in offs])
    one("match_placement",
        M.Stream(1).literal(10).match(10, 10).literal(END),                  # off == o
        M.Stream(2).literal(64).match(64, 64).literal(END),                  # off == o, a whole step
        M.Stream(3).literal(7).match(7, 7).match(7, 7).literal(END),         # what literal, then match, just wrote
        M.Stream(4).literal(5).match(5, 5).match(10, 10).match(20, 20).match(40, 40).match(64, 64).literal(END),
        M.Stream(5).literal(1).match(64, 1).match(64, 1).literal(3).match(64, 2).literal(END))
    chain = M.Stream(6).literal(4)
    prev = 4
    for i in range(300):
        ln = 4 + (i * 29) % 61
        chain.match(ln, prev)  # reads exactly the bytes of the element before
        prev = ln
    one("chain_300", chain.literal(END))
    one("match_ends_block", *[_ring_edge(total, R) for total in (R - 1, R, R + 1, MAX_OFF + 64, 2 * R + 1)])
    one("ring_sizes", *[M.Stream(total).fill_to(MAX_OFF).match(64, MAX_OFF).fill_to(total - 64 - END)
                        .match(64, MAX_OFF).literal(END) for total in (2 * R - 1, 2 * R, 2 * R + 1)],
        *[M.Stream(total).fill_to(total - 4 - END).match(4, total - 4 - END).literal(END)
          for total in (R - 1, R, R + 1)])
    # longer than the ring and the flush threshold
    one("long_match_off_1", M.Stream(8).literal(1).match(150000, 1).literal(END))
    one("long_match_off_65535", M.Stream(9).literal(MAX_OFF).match(150000, MAX_OFF).literal(END))
    one("long_match_off_63_64_65", *[M.Stream(off).literal(off).match(70000, off).literal(END) for off in (63, 64, 65)])
    one("sizes", *[_mixed(n, n + 1) for n in (0, 1, 63, 64, 65, 4095, 4096, 4097)])
    cases["stored_mixed"] = [(_mixed(300, 1).block(), False), (M.Stream(2)._fill(100), True),
                             (_mixed(65, 3).block(), False), (b"", True), (M.Stream(4)._fill(5000), True),
                             (M.Stream(5)._fill(1), True), (_mixed(1000, 6).block(), False),
                             (M.Stream(8)._fill(70001), True)]
    one("chunks_1", _mixed(777, 9))
    one("chunks_2", _mixed(777, 10), _mixed(130, 11))
    one("chunks_257", *[_mixed(20 + (i * 13) % 200, i) for i in range(257)])
    # blocks only these rules accept (liblz4 wants 5 literal bytes and more after the last match)
    one("only_these_rules_final_0", M.Stream(10).literal(30).match(8, 30))
    one("only_these_rules_final_1", M.Stream(11).literal(30).match(8, 30).literal(1))
    return cases


def _bad_chunks():
    """rule -> [(crafted body, dst_bytes)], each failing that rule first."""
    base = M.Stream(1).literal(20).match(4, 5).block(last=False)  # o == 24
    sound = M.Stream(2).literal(20).match(4, 5).literal(END)      # 36 bytes
    return {
        "empty_body": [(b"", 0), (b"", 10)],
        "literal_extension_cut": [(base + bytes([0xF0, 0xFF]), 100), (base + bytes([0xF0]), 100)],
        "literal_past_input": [
            (base + bytes([0xA0]) + b"abcde", 100),                          # 10 bytes announced, 5 present
            (base + bytes([0xF0]) + b"\xff" * 40 + b"\x01" + b"xy", 100000),    # 10,216 announced
        ],
        "literal_past_dst": [
            (sound.block(), 30),                                              # the table says 30, the block holds 36
            (sound.block(), 35),
            (base + bytes([0xF0]) + b"\xff" * 300, 100),                      # the run is left once the block is lost
        ],
        "one_offset_byte": [(base + bytes([0x30]) + b"abc" + bytes([5]), 100)],
        "match_extension_cut": [(base + bytes([0x0F, 1, 0, 0xFF]), 100000), (base + bytes([0x0F, 1, 0]), 100)],
        "zero_offset": [(base + bytes([0x00, 0, 0, 0x00]), 100)],
        "offset_past_output": [(base + bytes([0x00, 25, 0, 0x00]), 100), (base + bytes([0x00, 0xFF, 0xFF, 0x00]), 100)],
        "match_first": [(bytes([0x00, 1, 0, 0x00]), 100)],
        "match_past_dst": [
            (M.Stream(3).literal(20).match(50, 5).block(), 40),
            (M.Stream(3).literal(20).match(50, 5).block(), 69),
            (base + bytes([0x0F, 1, 0]) + b"\xff" * 600 + b"\x00\x00", 100),
        ],
        "ends_short_of_dst": [(sound.block(), 37), (bytes([0x00]), 1), (sound.block(), 100)],
        "ends_after_match": [(base, 24)],                                   # no final literal run, not even of 0 bytes
    }


@functools.lru_cache(maxsize=None)
def bad_cases():
    """name -> (chunks [(body, stored, dst_bytes)], index of the first failing
    chunk): each crafted chunk alone, and launches in which two chunks fail."""
    bad = _bad_chunks()
    good = []
    for body, stored in [(_mixed(200, 20).block(), False), (M.Stream(21)._fill(50), True),
                         (_mixed(4097, 22).block(), False)]:
        good.append((body, stored, len(body) if stored else M.size(body, BLOCK)))
    cases = {}
    rules = list(bad)
    for r, bodies in bad.items():
        for i, (b, dst) in enumerate(bodies):
            cases["%s_%d" % (r, i)] = ([(b, False, dst)], 0)
        first = (bodies[0][0], False, bodies[0][1])
        o = bad[rules[(rules.index(r) + 1) % len(rules)]][0]
        other = (o[0], False, o[1])
        # two failing chunks among good ones: the lower index is reported
        cases["%s_first_of_two" % r] = ([good[0], good[1], first, good[2], other], 2)
        cases["%s_second_of_two" % r] = ([good[0], other, first] + good[1:], 1)
    return cases
