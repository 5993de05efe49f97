"""CPU checks of tests/byterle_model.py, before any GPU is involved: the exact
model and the oracle (oracle/orc_oracle.c, ByteRLE.cc restated) agree byte for
byte, in both modes, on the known-answer vectors and on every stream of
tests/test_gpu_byterle_shapes.py, and on the producible count of every cut;
every shape holds the feature it means to hold at the window byte or decoded
offset it names, read back through walk() / windows(); and the crafted files
of tests/byterle_files.py read identically through the oracle and pyarrow.
No GPU."""
import os

import numpy as np
import pytest

import byterle_model as m
from conftest import load_golden
from oracle import oracle

BYTE = load_golden("kat_byterle.json")
BOOL = load_golden("kat_boolrle.json")
READ_ERROR = "bad read in nextBuffer"


def agree(data, boolean=None):
    """Model == oracle on what the stream can produce, and the oracle fails on
    one more (boolean None: both modes)."""
    if boolean is None:
        agree(data, True)
        boolean = False
    vals, count = m.decode(data, boolean)
    if count:
        np.testing.assert_array_equal(oracle.ByteRleDecoder(data, boolean=boolean).next(count), vals)
    with pytest.raises(oracle.OracleError, match=READ_ERROR):
        oracle.ByteRleDecoder(data, boolean=boolean).next(count + 1)
    return vals, count


def agree_shape(s):
    agree(s.data)
    table = dict(m.group_table(s.data))
    for off, vi in s.segs:  # the table is group aligned
        assert table[off] == vi
    assert len(s.data) <= 17_000


@pytest.mark.parametrize("fx", BYTE + BOOL, ids=[f["kind"] + "-" + f["name"] for f in BYTE + BOOL])
def test_model_on_known_answers(fx):
    data, exp = bytes.fromhex(fx["data"]), fx["expected"]
    if fx.get("not_null") is None:
        vals, count = m.decode(data, fx in BOOL)
        assert count >= len(exp) and [int(v) for v in vals[:len(exp)]] == exp
    agree(data)


def test_the_cut_literal_of_the_issue():
    """02 07 F6 01 02 03 04: a run of 5, then a literal of 10 with 4 of its
    bytes: 9 values, the tenth fails."""
    data = bytes.fromhex("0207f601020304")
    vals, count = agree(data, False)
    assert count == 9 and vals.tolist() == [7] * 5 + [1, 2, 3, 4]
    assert m.walk(data) == [(0, m.RUN, 5, 2)] and m.headers(data)[1] == (2, m.LIT, 10, 11)
    assert m.decode(data[:3], False)[1] == 5 and m.decode(data[:1], False)[1] == 0  # a header alone gives nothing
    assert agree(bytes.fromhex("0207f6"), True)[1] == 40


def test_positions():
    rng = np.random.default_rng(5)
    data = m.filler(rng, 3000)
    w = m.walk(data)
    first = dict(m.group_table(data))
    n = m.decode(data)[1]
    for stride in (100, 1000):
        for g, (off, skip) in enumerate(m.positions(w, n, stride)):
            assert first[off] + skip == g * stride and skip < 130
        pos = m.positions(w, 8 * n, stride, boolean=True)
        assert len(pos) == (8 * n + stride - 1) // stride
        for g, (off, skip, bits) in enumerate(pos):
            assert 8 * (first[off] + skip) + bits == g * stride and bits < 8 and skip < 130
            dec = oracle.ByteRleDecoder(data, boolean=True)
            dec.seek(off, skip, bits)
            k = min(stride, 8 * n - g * stride)
            np.testing.assert_array_equal(dec.next(k), m.decode(data, True)[0][g * stride:g * stride + k])
    assert any(p[2] for p in m.positions(w, 8 * n, 100, boolean=True))


def test_windows_of_a_plain_stream():
    """The schedule's rules on a stream long enough for three windows."""
    rng = np.random.default_rng(6)
    data = m.filler(rng, 10_000)
    for off in m.OFFS:
        w = m.windows(data, [(0, 0)], off)
        assert len(w) == 3 and w[0].wpos == -off and w[0].p0 == off and w[0].vi == 0
        assert sum(len(x.groups) for x in w) == len(m.walk(data)) and sum(x.dec for x in w) == m.decode(data)[1]
        for a, b in zip(w, w[1:]):
            assert a.lim == m.CHUNK and a.byte(a.nxt) >= m.CHUNK and a.byte(a.groups[-1]) < m.CHUNK
            assert (b.wpos + off) % 16 == 0 and b.p0 < 16 and b.wpos + b.p0 == a.nxt and b.vi == a.vi + a.dec
        # a pass stops once enough bytes are decoded
        assert len(m.windows(data, [(0, 0)], off, 0, w[0].dec)) == 1
        assert len(m.windows(data, [(0, 0)], off, 0, w[0].dec + 1)) == 2
        assert len(m.windows(data, [(0, 0)], off, 0, 8 * w[0].dec, boolean=True)) == 1
        assert len(m.windows(data, [(0, 0)], off, 0, 8 * w[0].dec + 1, boolean=True)) == 2


@pytest.mark.parametrize("off", m.OFFS)
@pytest.mark.parametrize("kind", m.EDGE_KINDS)
def test_window_edge_placements(kind, off):
    size = {"run": 2, "lit128": 129, "lit1": 2}[kind]
    p0s = set()
    for d in m.EDGE_D:
        s = m.window_edge(kind, d, off)
        agree_shape(s)
        w = s.windows()
        sizes = {g[0]: g[3] for g in m.walk(s.data)}
        assert sizes[s.marks["a"]] == sizes[s.marks["b"]] == size
        first = [x for x in w if x.seg == 1][0]
        p0s.add(first.p0)
        assert w[0].p0 == off and w[0].wpos == -off and first.p0 == (s.segs[1][0] + off) % 16
        for seg, mark in ((0, "a"), (1, "b")):
            sg, k, b = m.window_of(w, s.marks[mark])
            head = [x for x in w if x.seg == seg][0]
            if d is None:  # a header at CHUNK opens the next window
                assert (sg, k, b) == (seg, 1, 0) and head.byte(s.marks[mark]) == m.CHUNK
            else:
                assert (sg, k, b) == (seg, 0, m.CHUNK - 1 - d)
        if kind == "lit128" and d == 0:
            assert w[0].byte(s.marks["a"] + size) == m.CHUNK - 1 + 129  # the longest group's reach
    assert len(p0s) > 4


@pytest.mark.parametrize("off", m.OFFS)
def test_length_phase_placements(off):
    seen, cross_chunk, cross_block, payload_mod4 = set(), 0, 0, set()
    for band in range(m.BANDS):
        s = m.length_phases(band, off)
        agree_shape(s)
        w = s.windows()
        sizes = {g[0]: g[1:] for g in m.walk(s.data)}
        for a, size in s.marks["heads"]:
            _, _, b = m.window_of(w, a)
            assert sizes[a][2] == size
            seen.add((size, b % 16))
            cross_chunk += b // 16 != (b + size - 1) // 16
            cross_block += b // m.BLOCK != (b + size - 1) // m.BLOCK
            if sizes[a][0] == m.LIT:
                payload_mod4.add((b + 1) % 4)
    assert seen == {(size, ph) for size in range(2, 130) for ph in range(16)}
    assert cross_chunk > 1500 and cross_block > 500 and payload_mod4 == {0, 1, 2, 3}


@pytest.mark.parametrize("off", m.OFFS)
def test_block_hop_placements(off):
    s = m.block_hops(off)
    agree_shape(s)
    w = s.windows()
    assert len(w) == 1
    starts = {w[0].byte(a) // m.BLOCK for a in w[0].groups}
    for a in s.marks["heads"]:
        b = w[0].byte(a)
        assert b % m.BLOCK == m.BLOCK - 1 and b // m.BLOCK + 1 not in starts  # the next block lies inside the literal
    assert len(s.marks["heads"]) == 12


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("kind", m.DENSE)
def test_dense_window_placements(kind, off):
    s = m.dense(kind, off)
    agree_shape(s)
    w = s.windows()
    dec = {"lit1": 1, "run3": 3, "run130": 130}[kind]
    assert {g[1:] for g in m.walk(s.data)} == {(m.LIT if kind == "lit1" else m.RUN, dec, 2)}
    assert len(w) == 2 and [x.p0 for x in w] == [off, off]  # both parities of p0 over the two offsets
    assert all(len(x.groups) == m.SLOTS and x.dec == m.SLOTS * dec for x in w)
    assert w[0].rounds == {"lit1": 1, "run3": 1, "run130": 17}[kind]


@pytest.mark.parametrize("off", m.OFFS)
def test_small_group_placements(off):
    s = m.small_groups(off)
    agree_shape(s)
    w = m.walk(s.data)
    f = m.firsts(w)
    assert {(g[2], v % 4) for g, v in zip(w, f) if g[1] == m.LIT and g[2] <= 3} == {(k, r) for k in (1, 2, 3) for r in range(4)}
    assert {v % 4 for g, v in zip(w, f) if g[1] == m.RUN and g[2] == 3} == {0, 1, 2, 3}
    assert [(g[1], v) for g, v in zip(w, f)][:3] == [(m.RUN, 0), (m.LIT, 5), (m.RUN, 7)] and s.marks["mixed"] == 4
    assert m.decode(s.data)[0][4:8].tolist() == [0x11, 0x22, 0x33, 0x44]
    # dwords no group owns whole, in runs of several groups
    assert sum(g[2] for g in w[3:]) / len(w[3:]) < 4.5


@pytest.mark.parametrize("off", m.OFFS)
def test_round_edge_placements(off):
    s = m.round_edges(off)
    agree_shape(s)
    w = s.windows()
    assert len(w) == len(s.segs) == 16  # one window a segment
    first = dict(m.group_table(s.data))
    kinds = {g[0]: g[1:] for g in m.walk(s.data)}
    seen = set()
    for seg, a, d in s.marks["feats"]:
        assert first[a] - s.segs[seg][1] == d and w[seg].seg == seg and a in w[seg].groups
        assert kinds[a][1] == 100 and w[seg].rounds == d // m.ROUND + 1 + (d % m.ROUND > 0)
        seen.add((kinds[a][0], -d % m.ROUND, (d + 3) // m.ROUND))
    assert seen == {(k, b, r) for k in (m.RUN, m.LIT) for b in m.ROUND_BEFORE for r in (1, 2)}


@pytest.mark.parametrize("off", m.OFFS)
def test_crossing_placements(off):
    p0s = set()
    for ph in range(16):
        s = m.crossing(ph, off)
        agree_shape(s)
        w = s.windows()
        assert len(w) == 3 and [x.p0 for x in w] == [off, ph, ph]
        assert all(x.byte(x.nxt) == m.CHUNK + ph for x in w[:2])
        p0s.add(ph)
    assert p0s == set(range(16))


def test_range_stream():
    s = m.ranged()
    agree_shape(s)
    n = m.decode(s.data)[1]
    assert len(s.segs) == 5
    br, lr = m.byte_ranges(s), m.bool_ranges(s)
    assert {a % 4 for a, _ in br} == {(a + c) % 4 for a, c in br} == {0, 1, 2, 3}
    assert {a % 8 for a, _ in lr} == {c % 8 for _, c in lr} == set(range(8))
    assert any(a // 8 == (a + c - 1) // 8 and a % 8 and (a + c) % 8 for a, c in lr)  # inside one decoded byte
    # ranges that make whole segments return early, at either end
    nw = len(s.windows())
    assert any(len(s.windows(begin=a, count=c)) < nw and a >= s.segs[2][1] for a, c in br)
    assert any(len(s.windows(begin=a, count=c)) < nw and a + c <= s.segs[2][1] for a, c in br)
    assert any(len(s.windows(begin=a, count=c, boolean=True)) < nw and a >= 8 * s.segs[2][1] for a, c in lr)
    assert any(len(s.windows(begin=a, count=c, boolean=True)) < nw and a + c <= 8 * s.segs[2][1] for a, c in lr)
    f = s.marks["first"]
    assert any(f[k] < a and a + c < f[k + 1] for a, c in br for k in range(len(f) - 1))
    assert all(a + c <= n for a, c in br) and all(a + c <= 8 * n for a, c in lr)


@pytest.mark.parametrize("repeat", [False, True])
def test_grouped_tables(repeat):
    data, segs = m.grouped(repeat)
    agree(data)
    first = dict(m.group_table(data))
    assert all(first[off] == vi for off, vi in segs) and segs == sorted(segs)
    assert (len(set(segs)) < len(segs)) == repeat and len(set(segs)) == 300
    sizes = {g[0]: g[3] for g in m.walk(data)}
    assert all(sizes[segs[k][0]] >= 2 for k in (0, 5))


def test_every_cut_of_the_small_stream():
    s = m.trunc_small()
    vals, n = agree(s.data, False)
    kinds = set()
    for cut in range(len(s.data) + 1):
        for boolean in (False, True):
            got, count = agree(s.data[:cut], boolean)
            np.testing.assert_array_equal(got, m.decode(s.data, boolean)[0][:count])
        hs = m.headers(s.data[:cut])
        if hs and hs[-1][0] + hs[-1][3] > cut:
            kinds.add((hs[-1][1], cut - hs[-1][0] - 1 > 0))
    # a header alone (run, literal), and a literal with some of its bytes
    assert kinds == {(m.RUN, False), (m.LIT, False), (m.LIT, True)}


def test_cuts_around_the_window_end():
    s = m.trunc_window()
    agree_shape(s)
    assert len(s.windows()) == 2 and s.marks["cuts"][0] == m.CHUNK - 20 and s.marks["cuts"][-1] == m.CHUNK + 140
    whole = {b: m.decode(s.data, b)[0] for b in (False, True)}
    kinds = set()
    for cut in s.marks["cuts"]:
        for boolean in (False, True):
            got, count = agree(s.data[:cut], boolean)
            np.testing.assert_array_equal(got, whole[boolean][:count])
        hs = m.headers(s.data[:cut])
        if hs[-1][0] + hs[-1][3] > cut:
            kinds.add((hs[-1][1], cut - hs[-1][0] - 1 > 0, hs[-1][0] < m.CHUNK <= cut))
    assert (m.LIT, True, True) in kinds and (m.RUN, False, False) in kinds and (m.LIT, False, False) in kinds


# ---- the crafted files (tests/byterle_files.py) -------------------------------
import byterle_files as bf  # noqa: E402

FILES = {"A": bf.file_a, "B": bf.file_b, "C": bf.file_c, "A0": lambda: bf.file_a(stride=0), "AS": bf.file_as,
         "A-padding": lambda: bf.file_a(cut="padding")}


def expected_units(c, s):
    """What stream s of column c decodes to: rows (boolean) or bytes."""
    if s is c.present:
        return c.bits
    if c.kind == bf.oc.T_BOOLEAN:
        return np.array(c.values, dtype=np.uint8)
    return np.array(c.values, dtype=np.int8).view(np.uint8)


@pytest.mark.parametrize("name", list(FILES))
def test_pyarrow_reads_the_crafted_files(name, tmp_path):
    """(A-padding: the PRESENT stream ends inside its last literal, after the
    last row's byte. pyarrow, which is the reference's reader, and the oracle
    agree on it and on the cut one byte shorter; had they disagreed on a
    corrupt file, the oracle would decide.)"""
    po = pytest.importorskip("pyarrow.orc")
    f = FILES[name]()
    p = tmp_path / "crafted.orc"
    p.write_bytes(f.data)
    o = po.ORCFile(str(p))
    assert o.nrows == sum(n for n, _ in f.stripes) and o.nstripes == len(f.stripes)
    assert o.row_index_stride == f.stride and o.compression == "UNCOMPRESSED"
    assert [x.name for x in o.schema] == f.names and [str(x.type) for x in o.schema] == ["bool", "int8", "int64"]
    for k in range(len(f.stripes)):
        assert o.read_stripe(k).to_pylist() == f.rows(k), (name, k)


def test_pyarrow_reads_its_own_file_to_the_generated_rows():
    po = pytest.importorskip("pyarrow.orc")
    o = po.ORCFile(bf.P_PATH)
    assert o.nrows == bf.P_ROWS and o.nstripes == 1 and o.row_index_stride == bf.P_STRIDE and o.compression == "UNCOMPRESSED"
    rows = bf.pyarrow_rows()
    assert o.read().to_pylist() == rows
    assert o.read().equals(bf.pyarrow_table())
    s = [r["s"] for r in rows]
    assert 0.1 < sum(x is None for x in s) / len(s) < 0.4
    for child in ("big", "flag", "tiny"):
        assert any(x is not None and x[child] is None for x in s) and any(x is not None and x[child] is not None for x in s)
    assert os.path.getsize(bf.P_PATH) < 64 << 10


@pytest.mark.parametrize("name", list(FILES))
def test_oracle_decodes_every_stream_of_the_crafted_files(name):
    """Every byte / boolean RLE stream through the oracle and the model, from
    its start and from every row-index position (the nullable column's DATA
    pair counts non-null values)."""
    f = FILES[name]()
    for k, (n, cols) in enumerate(f.stripes):
        assert [c.name for c in cols] == f.names
        for c, s in f.byte_streams(k):
            want = expected_units(c, s)
            assert want.size == n
            np.testing.assert_array_equal(oracle.ByteRleDecoder(s.data, boolean=s.boolean).next(n), want)
            np.testing.assert_array_equal(m.decode(s.data, s.boolean)[0][:n], want)
        for c in cols:
            cc = c.craft(f.stride)
            if not f.stride:
                assert cc.positions is None
                continue
            rows = list(range(0, n, f.stride))
            assert len(cc.positions) == len(rows)
            s = c.present if c.present is not None else c.data
            want = expected_units(c, s)
            width = 3 if s.boolean else 2
            first = dict(m.group_table(s.full))
            for g, e in zip(rows, cc.positions):
                assert len(e) == width + (2 if c.present is not None else 0)
                assert (8 if s.boolean else 1) * (first[e[0]] + e[1]) + (e[2] if s.boolean else 0) == g
                dec = oracle.ByteRleDecoder(s.data, boolean=s.boolean)
                dec.seek(*[int(x) for x in e[:width]])
                np.testing.assert_array_equal(dec.next(min(f.stride, n - g)), want[g:g + f.stride])
                if c.present is not None:
                    vi = int(c.bits[:g].sum())
                    dec = oracle.RleDecoderV1(c.data.data, True)
                    dec.seek(int(e[3]), int(e[4]))
                    k2 = int(c.bits[g:g + f.stride].sum())
                    np.testing.assert_array_equal(dec.next(k2), c.data.values[vi:vi + k2])


def test_makeup_of_the_crafted_files():
    a, b, c = bf.file_a(), bf.file_b(), bf.file_c()
    for f in (a, b, c):
        n, cols = f.stripes[0]
        flag, tiny, nullable = cols
        for col, s in f.byte_streams():
            assert {g[1] for g in s.groups} == {m.RUN, m.LIT}, (f.stride, col.name)
        assert min(tiny.values) == -128 and max(tiny.values) == 127 and 0 < sum(v < 0 for v in tiny.values) < n
        assert 0 < int(nullable.bits.sum()) < n and 0 < sum(flag.values) < n
        last = m.headers(nullable.present.full)[-1]
        assert last[1] == m.LIT and last[0] + last[3] == len(nullable.present.full)
        assert m.decode(nullable.present.full)[1] == (n + 7) // 8 + bf.PAD
    per_group = lambda f, s: np.diff([p[0] for p in s.positions(f.stripes[0][0], f.stride)] + [len(s.data)])
    assert (a.stripes[0][0] + a.stride - 1) // a.stride == 4 and a.stripes[0][0] % a.stride == 1
    assert all(per_group(a, s).max() <= 2048 for _, s in a.byte_streams())  # the row index is kept
    assert len(c.stripes[0][1][1].data.data) // 4 > 2048 and per_group(c, c.stripes[0][1][1].data)[:3].min() > 2048  # 4 KB host plans
    # B: positions with bits, several row groups starting in one group, skips into runs
    for col, s in b.byte_streams():
        pos = s.positions(b.stripes[0][0], b.stride)
        offs = [p[0] for p in pos]
        kinds = {g[0]: g[1] for g in s.groups}
        # (a byte run holds 130 values at the most: two row groups; a boolean run 1,040 rows)
        assert len(set(offs)) < len(offs) * (0.8 if s.boolean else 0.9) and max(p[1] for p in pos) > 50, col.name
        assert any(kinds[p[0]] == m.RUN and p[1] for p in pos)
        if s.boolean:
            assert {p[2] for p in pos} == {0, 4}  # 100 rows = 12 bytes and 4 bits
    assert [len(x[1]) for x in bf.file_as().stripes] == [3, 3, 3]


def test_cut_present_streams_against_the_oracle_and_pyarrow(tmp_path):
    """padding: the stream ends inside its last literal with every row's byte
    still there: the oracle and pyarrow read all rows. short: one byte less:
    both raise "bad read in nextBuffer". The positions are the whole file's."""
    po = pytest.importorskip("pyarrow.orc")
    whole = bf.file_a()
    n, cols = whole.stripes[0]
    full = cols[2].present.full
    for cut, ok in (("padding", True), ("short", False)):
        f = bf.file_a(cut=cut)
        c = f.stripes[0][1][2]
        s = c.present
        assert s.full == full and len(s.data) == len(full) - bf.PAD - (not ok)
        last = m.headers(s.data)[-1]
        assert last[1] == m.LIT and last[0] + 1 < len(s.data) < last[0] + last[3]  # cut inside its last literal
        assert m.decode(s.data, True)[1] == (n + 7) // 8 * 8 - (0 if ok else 8)
        assert c.craft(f.stride).positions == cols[2].craft(f.stride).positions
        p = tmp_path / (cut + ".orc")
        p.write_bytes(f.data)
        if ok:
            np.testing.assert_array_equal(oracle.ByteRleDecoder(s.data, boolean=True).next(n), c.bits)
            assert po.ORCFile(str(p)).read().to_pylist() == whole.rows()
        else:
            with pytest.raises(oracle.OracleError, match=READ_ERROR):
                oracle.ByteRleDecoder(s.data, boolean=True).next(n)
            with pytest.raises(OSError, match=READ_ERROR):
                po.ORCFile(str(p)).read()
