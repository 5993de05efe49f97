"""The built Snappy streams of tests/test_gpu_snappy_shapes.py, shared with
tests/test_snappy_model_cpu.py (which proves the model on them). A case is a
list of chunks, each (body bytes, stored?); the edge shapes derive from R, the
kernel's history size (orcg_snappy_device_info)."""
import functools

import snappy_model as M

BLOCK = 262144  # the largest ORC compression block


def _mixed(total, seed):
    """A block of `total` output bytes: literals and copies of every kind."""
    s = M.Stream(seed)
    step = 0
    while s.o < total:
        left = total - s.o
        step += 1
        if s.o == 0 or step % 3 == 1:
            s.literal(min(left, 1 + (step * 37) % 90))
        elif step % 3 == 2:
            s.copy(min(left, 1 + (step * 11) % 64), 1 + (step * 7) % min(s.o, 3000), kind=2)
        else:
            ln = min(left, 4 + step % 8)
            s.copy(ln, 1 + (step * 5) % min(s.o, 2047)) if ln >= 4 else s.literal(ln)
    assert s.o == total
    return s


def _ring_edge(total, reach, R):
    """Filler, then a copy reaching exactly `reach` back that ends the block at
    `total` (or, when the block is long enough, one at o == reach in the
    middle as well)."""
    s = M.Stream(total * 31 + reach)
    if total >= reach + 64 + 64:
        s.fill_to(reach).copy(64, reach, kind=4 if reach >= 65536 else 2)  # off == o
    ln = min(64, total - max(s.o, reach))
    s.fill_to(total - ln).copy(ln, reach, kind=4 if reach >= 65536 else 2)
    assert s.o == total
    return s


@functools.lru_cache(maxsize=None)
def good_cases(R):
    """name -> [(body, stored)], every chunk valid."""
    cases = {}

    def one(name, *streams):
        cases[name] = [(s.block(), False) for s in streams]

    for n in (1, 60, 61, 64, 65, 256, 257, 65536 + 1):
        one("literal_%d" % n, M.Stream(n).literal(n))
    # every length form, also longer than the length needs
    one("literal_forms", *[M.Stream(e).literal(n, extra=e)
                          for e, n in ((0, 1), (0, 60), (1, 5), (1, 256), (2, 7), (2, 257), (2, 65536), (3, 9),
                                       (3, 65537), (4, 11), (4, 300))])
    offs = list(range(1, 9)) + [63, 64, 65]
    for ln in (1, 4, 11, 63, 64):
        one("copy_len_%d" % ln, *[M.Stream(off).literal(max(off, 3)).copy(ln, off, kind=2) for off in offs])
    one("copy1", *[M.Stream(off).literal(max(off, 3)).copy(ln, off, kind=1).literal(2)
                   for off in offs + [2047] for ln in (4, 11)])
    one("copy4_near", *[M.Stream(off).literal(max(off, 3)).copy(ln, off, kind=4) for off in (1, 5, 64, 300)
                        for ln in (1, 64)])
    one("copy_placement",
        M.Stream(1).literal(10).copy(10, 10),               # off == o
        M.Stream(2).literal(64).copy(64, 64, kind=2),       # off == o, a whole step
        M.Stream(3).literal(7).copy(7, 7).copy(7, 7),       # what the literal, then the copy, just wrote
        M.Stream(4).literal(5).copy(5, 5).copy(10, 10).copy(20, 20).copy(40, 40).copy(64, 64),
        M.Stream(5).literal(1).copy(64, 1, kind=2).copy(64, 1, kind=2).literal(3).copy(64, 2, kind=2))
    chain = M.Stream(6).literal(3)
    prev = 3
    for i in range(300):
        ln = 1 + (i * 29) % 64
        chain.copy(ln, prev, kind=2)  # reads exactly the bytes of the element before
        prev = ln
    one("chain_300", chain)
    for total in (R - 1, R, R + 1, 2 * R + 1):
        for reach in (R - 1, R, R + 1):
            if reach < total:
                one("ring_%d_reach_%d" % (total, reach), _ring_edge(total, reach, R))
    one("ring_%d_reach_%d" % (R - 1, R - 2), _ring_edge(R - 1, R - 2, R))
    far = M.Stream(7).fill_to(250000).copy(64, 200000, kind=4).copy(33, 200000 + 64, kind=4).fill_to(262144 - 64)
    far.copy(64, 262144 - 64, kind=4)
    assert far.o == 262144 and 200000 > R
    one("far_copy", far)
    one("sizes", *[_mixed(n, n + 1) for n in (0, 1, 63, 64, 65, 4095, 4096, 4097)])
    cases["stored_mixed"] = [(_mixed(300, 1).block(), False), (M.Stream(2)._fill(100), True),
                             (_mixed(65, 3).block(), False), (b"", True), (M.Stream(4)._fill(5000), True),
                             (M.Stream(5)._fill(1), True), (_mixed(1000, 6).block(), False),
                             (M.Stream(8)._fill(70001), True)]
    one("chunks_1", _mixed(777, 9))
    one("chunks_2", _mixed(777, 10), _mixed(130, 11))
    one("chunks_257", *[_mixed(20 + (i * 13) % 200, i) for i in range(257)])
    return cases


def _bad_chunks():
    """text -> [crafted bodies], each failing exactly that check first."""
    lit = M.Stream(1).literal(20)
    return {
        M.LITERAL_TRUNCATED: [
            lit.block(ulen=100) + bytes([61 << 2, 0x10]),           # two length bytes announced, one present
            lit.block(ulen=100) + bytes([63 << 2, 1, 2, 3]),        # four announced, three present
        ],
        M.LITERAL_RANGE: [
            lit.block(ulen=100) + bytes([9 << 2]) + b"abcde",       # 10 bytes announced, 5 present
            lit.block(ulen=22) + M.literal(b"abc"),                 # would pass the stated length
            lit.block(ulen=100) + bytes([63 << 2, 0xFF, 0xFF, 0xFF, 0xFF]) + b"xy",  # 2^32 bytes announced
        ],
        M.COPY_TRUNCATED: [
            lit.block(ulen=100) + bytes([1 | (3 << 2)]),            # copy-1 without its offset byte
            lit.block(ulen=100) + bytes([2 | (3 << 2), 5]),         # copy-2 with one offset byte
            lit.block(ulen=100) + bytes([3 | (3 << 2), 5, 0, 0]),   # copy-4 with three
        ],
        M.COPY_RANGE: [
            lit.block(ulen=100) + M.copy2(4, 21),                   # off > o
            lit.block(ulen=100) + M.copy2(4, 0),                    # off == 0
            lit.block(ulen=100) + M.copy1(4, 0),
            lit.block(ulen=100) + M.copy4(64, 0xFFFFFFFF),
            lit.block(ulen=23) + M.copy2(4, 20),                    # would pass the stated length
            M.varint(10) + M.copy2(4, 1),                           # a copy first: o == 0
        ],
        M.LENGTH_MISMATCH: [
            lit.block(ulen=21),
            M.varint(1),                                            # no elements
            lit.block(ulen=100) + M.copy2(64, 20),
        ],
    }


@functools.lru_cache(maxsize=None)
def bad_cases():
    """name -> (chunks, index of the first failing chunk, its text): each
    crafted chunk alone, and launches in which two chunks fail."""
    bad = _bad_chunks()
    good = [(_mixed(200, 20).block(), False), (M.Stream(21)._fill(50), True), (_mixed(4097, 22).block(), False)]
    cases = {}
    texts = list(bad)
    for t, bodies in bad.items():
        key = t.split(": ")[1].replace(" ", "_")
        for i, b in enumerate(bodies):
            cases["%s_%d" % (key, i)] = ([(b, False)], 0, t)
        other = bad[texts[(texts.index(t) + 1) % len(texts)]][0]
        # two failing chunks among good ones: the lower index is reported
        cases["%s_first_of_two" % key] = ([good[0], good[1], (bodies[0], False), good[2], (other, False)], 2, t)
        cases["%s_second_of_two" % key] = ([good[0], (other, False), (bodies[0], False)] + good[1:], 1,
                                           M.decode(other, BLOCK))
    return cases
