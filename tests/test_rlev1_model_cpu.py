"""CPU checks of tests/rlev1_model.py, before any GPU is involved: the exact
model, the oracle (oracle/orc_oracle.c, RLEv1.cc restated) and the writer's
values agree bit for bit on the known-answer vectors, random mixes and every
shape of tests/test_gpu_rlev1_shapes.py, and on the producible count of every
cut; and every shape holds the feature it means to hold at the window byte it
names, read back through walk() / windows(). No GPU."""
import numpy as np
import pytest

import rlev1_model as m
from conftest import load_golden
from oracle import oracle
from rlev1_writer import encode, random_groups

RLEV1 = load_golden("kat_rlev1.json")
OFFS = (0, 1, 15)


def oracle_count(data, signed):
    """Values the oracle produces before it throws, by probing."""
    dec, n = oracle.RleDecoderV1(data, signed), 0
    while True:
        try:
            dec.next(1)
            n += 1
        except oracle.OracleError as e:
            assert str(e) == "bad read in readByte"
            return n


def agree(data, signed, n=None):
    """Model == oracle on the whole stream (n: the count, when it is known
    that the stream ends on a group's end)."""
    vals, count = m.decode(data, signed)
    assert n is None or n == count
    np.testing.assert_array_equal(oracle.RleDecoderV1(data, signed).next(count), vals)
    if count:
        with pytest.raises(oracle.OracleError, match="bad read in readByte"):
            oracle.RleDecoderV1(data, signed).next(count + 1)
    return vals, count


def agree_shape(s):
    agree(s.data, s.signed)
    assert m.v1_chunk(len(s.data), len(s.segs)) == s.cb
    table = dict(m.group_table(s.data))
    for off, vi in s.segs:  # the table is group aligned
        assert table[off] == vi


@pytest.mark.parametrize("fx", RLEV1, ids=[f["name"] for f in RLEV1])
def test_model_on_known_answers(fx):
    data, exp = bytes.fromhex(fx["data"]), fx["expected"]
    if fx.get("not_null") is None:
        vals, count = m.decode(data, fx["signed"], len(exp))
        assert count >= len(exp) and [int(v) for v in vals] == exp
    for sk in fx.get("seeks", []):
        off, skip = sk["position"]
        vals, _ = m.decode(data[off:], fx["signed"], skip + len(sk["expected"]))
        assert [int(v) for v in vals[skip:]] == sk["expected"]


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("max_bits", [7, 35, 64])
def test_model_on_random_mixes(signed, max_bits):
    rng = np.random.default_rng(max_bits + int(signed))
    gs = random_groups(rng, 20_000, signed, max_bits)
    data, vals = encode(gs, signed)
    got, count = agree(data, signed, vals.size)
    np.testing.assert_array_equal(got, vals)
    w = m.walk(data)
    assert [(g[1], g[2]) for g in w] == [(g[0], g[3] if g[0] == "run" else len(g[1])) for g in gs]
    assert sum(g[3] for g in w) == len(data)


def test_truncate_and_padded_varints():
    v = [0, -1, 1 << 31, (1 << 31) - 1, -(1 << 31) - 1, 0x12345_8000, -(1 << 63), (1 << 63) - 1]
    np.testing.assert_array_equal(m.truncate(v, 4), np.array(v, dtype=np.int64).astype(np.int32))
    np.testing.assert_array_equal(m.truncate(v, 2), np.array(v, dtype=np.int64).astype(np.int16))
    np.testing.assert_array_equal(m.truncate(v, 8), np.array(v, dtype=np.int64))
    for u, nb in ((0x7F, 1), (0x80, 2), (0x80, 5), (m.M64, 10), (m.M64, 40), (1 << 63, 2600)):
        b = m.padded_varint(u, nb)
        assert len(b) == nb and all(x >= 0x80 for x in b[:-1]) and b[-1] < 0x80
        assert m.decode(bytes([0xFF]) + b, False)[0].tolist() == [m.signed64(u)]
        assert oracle.RleDecoderV1(bytes([0xFF]) + b, False).next(1).tolist() == [m.signed64(u)]
        assert b[:len(m.varint(u))].replace(b"\x80", b"") != b"" or u == 0  # the payload comes first


def test_positions_are_those_of_rle_streams():
    rng = np.random.default_rng(5)
    data, vals = encode(random_groups(rng, 5000, True, 30), True)
    w = m.walk(data)
    first = dict(m.group_table(data))
    for stride in (100, 1000, 0x7FFFFFFF):
        pos = m.positions(w, vals.size, stride)
        for g, (off, skip) in enumerate(pos.tolist()):
            assert first[off] + skip == g * stride and skip < 130
    assert (m.positions(w, vals.size, 100)[:, 1] > 0).any()


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("kind", m.EDGE_KINDS)
def test_window_edge_placements(kind, off, cb):
    chunk, win, _ = m.geo(cb)
    for d in m.EDGE_D:
        s = m.window_edge(kind, d, off, cb)
        agree_shape(s)
        w = s.windows()
        assert w[0].p0 == off and w[0].wpos == -off
        (ka, ba), (kb, bb) = m.window_of(w, s.marks["a"]), m.window_of(w, s.marks["b"])
        if d is None:  # a header at kChunk opens the next window
            assert ka == 1 and ba == w[1].p0 and w[0].byte(s.marks["a"]) == chunk and w[0].how == "next"
            assert kb > 1 and bb == w[kb].p0 and w[kb - 1].byte(s.marks["b"]) == chunk and w[kb - 1].how == "next"
        else:
            assert (ka, ba) == (0, chunk - 1 - d) and kb >= 1 and bb == chunk - 1 - d
        size = {g[0]: g[3] for g in m.walk(s.data)}
        want = {"run": 4, "run10": 12, "lit128": 1281}[kind]
        assert size[s.marks["a"]] == size[s.marks["b"]] == want
        assert all(x.how in ("next", "end") for x in w)
        if kind == "lit128" and d == 0:
            assert w[0].byte(s.marks["a"] + want) == chunk + 1280  # the longest legal group's reach


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", (0, 15))
def test_literal_phase_placements(off, cb):
    chunk, win, block = m.geo(cb)
    at_chunk, at_pass, at_cb, at_block = set(), set(), set(), set()
    for j in range(10):
        s = m.literal_phases(j, off, cb)
        agree_shape(s)
        assert m.window_of(s.windows(), s.marks["a"]) == (0, chunk - 51 - j)
        at_chunk |= m.crossing_phases(s, 1 << 30, chunk)
        at_pass |= m.crossing_phases(s, 1 << 30, chunk + 1024)
        at_cb |= m.crossing_phases(s, cb)
        at_block |= m.crossing_phases(s, block)
    every = set(range(1, 10))
    assert at_chunk == at_pass == at_cb == at_block == every


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", (0, 15))
@pytest.mark.parametrize("nbytes", m.PADDED)
def test_padded_literal_placements(nbytes, off, cb):
    s = m.padded_literals(nbytes, off, cb)
    agree_shape(s)
    w = s.windows()
    size = {g[0]: g[3] for g in m.walk(s.data)}
    assert all(x.how in ("next", "end") for x in w)
    phases, longest = set(), 0
    for h in s.marks["heads"]:
        assert size[h] == 1 + 20 * nbytes
        k, b = m.window_of(w, h)
        phases.add(b % cb)
        for i in range(20):
            start = b + 1 + i * nbytes
            c0 = (start + nbytes - 1) // cb * cb  # the chunk holding the terminator
            longest = max(longest, c0 - start)
    assert phases == set(range(cb))
    # bytes of one varint before the chunk that ends it: the register resume
    # covers 16, the byte loop the rest
    assert longest == nbytes - 1 and (longest > 16) == (nbytes >= 18)
    vals = m.decode(s.data, False)[0]
    assert (vals < 0).sum() >= 20 * 16  # payloads with bit 63 set: no all-zero varints


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", (0, 15))
def test_literal_end_placements(off, cb):
    s = m.literal_ends(off, cb)
    agree_shape(s)
    w = s.windows()
    size = {g[0]: g[3] for g in m.walk(s.data)}
    for name, rem in (("last", cb - 1), ("first", 0)):
        for a in s.marks[name]:
            k, b = m.window_of(w, a)
            assert k == 0 and (b + size[a] - 1) % cb == rem


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("off", (0, 15))
@pytest.mark.parametrize("kind", m.DENSE)
def test_dense_window_placements(kind, off, cb):
    chunk = m.geo(cb)[0]
    s = m.dense(kind, off, cb)
    agree_shape(s)
    w = s.windows()
    assert len(w) >= 3 and all(x.how in ("next", "end") for x in w)
    per = max(len(x.groups) for x in w)
    kinds = {g[1:] for g in m.walk(s.data[:s.segs[1][0] if len(s.segs) > 1 else len(s.data)])}
    if kind == "lit2":
        assert kinds == {(m.LIT, 1, 2)}
        assert per == chunk // 2 and sum(len(x.groups) == per for x in w) >= 2  # kMaxGroups
    else:
        assert kinds == {(m.RUN, 3 if kind == "run3" else 130, 3)}
        assert per == chunk // 3 + 1 if off == 0 else per >= chunk // 3  # kMaxRuns (a window whose p0 = 0)


@pytest.mark.parametrize("cb", m.WIDTHS)
def test_run_shapes(cb):
    for signed in (True, False):
        s = m.run_matrix(signed, cb)
        agree_shape(s)
        w = [g for g in m.walk(s.data) if g[0] < (s.segs[1][0] if len(s.segs) > 1 else len(s.data))]
        gs = m.groups(s.data, signed)[:len(w)]
        assert {g[2] for g in w} == set(m.RUN_LENGTHS) and all(g[1] == m.RUN for g in w)
        assert {(g[2][1] - g[2][0]) for g in gs} >= {-1, 0, 1, 127, -128}
        sizes = {g[3] for g in w}
        assert sizes >= {3, 12} and max(sizes) > 12  # canonical bases of 1 and 10 bytes, padded ones past 10
        lo, hi = (-(1 << 63), (1 << 63) - 1)
        ends = [g for g in gs if lo in g[2][1:] or hi in g[2][1:]]  # runs that wrap mod 2^64
        assert len(ends) >= 8
    s = m.runs_of_10(cb)
    agree_shape(s)
    assert [g[1:3] for g in m.walk(s.data)[:500]] == [(m.RUN, 10)] * 500


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("where", m.LONG_WHERE)
@pytest.mark.parametrize("kind", m.LONG_KINDS)
def test_long_group_placements(kind, where, cb):
    win = m.geo(cb)[1]
    s = m.long_group(kind, where, cb)
    vals, count = m.decode(s.data, False)
    assert oracle_count(s.data, False) == count
    np.testing.assert_array_equal(oracle.RleDecoderV1(s.data, False).next(count), vals)
    assert m.v1_chunk(len(s.data), len(s.segs)) == cb
    a = s.marks["a"]
    seg = max(i for i, (off, _) in enumerate(s.segs) if off <= a)
    w = s.windows(seg)
    k = [i for i, x in enumerate(w) if x.how == "serial"]
    assert len(k) == 1 and w[k[0]].wpos + w[k[0]].p0 == a and w[k[0]].groups == []
    g = [x for x in m.groups(s.data, False) if x[0] == a][0]
    assert g[3] > win or not g[4]
    if where == "first":
        assert k == [0] and a == 0 and len(w) > 1 and w[1].groups
    elif where == "after":
        assert k[0] >= 1 and w[k[0] - 1].how == "restart" and w[k[0] - 1].groups and w[k[0] + 1].groups
    else:
        assert not g[4] and len(s.data) - a > win
        assert count == m.decode(s.data[:a], False)[1] + (0 if kind == "runwin" else (win + 49) // 45)


def test_every_cut_of_the_small_stream():
    s = m.trunc_small()
    vals, n = agree(s.data, True)
    kinds = set()
    for cut in range(len(s.data) + 1):
        got, count = m.decode(s.data[:cut], True)
        assert oracle_count(s.data[:cut], True) == count
        np.testing.assert_array_equal(got, vals[:count])
        gs = m.groups(s.data[:cut], True)
        if gs and not gs[-1][4]:
            kinds.add((gs[-1][1], len(gs[-1][2]) > 0))
    assert kinds == {(m.RUN, False), (m.LIT, False), (m.LIT, True)}


@pytest.mark.parametrize("cb", m.WIDTHS)
def test_cuts_of_the_long_stream(cb):
    s = m.trunc_long(cb)
    agree_shape(s)
    vals = m.decode(s.data, True)[0]
    assert len(s.windows(len(s.segs) - 1)) >= 4 and len(s.marks["cuts"]) >= 25
    for cut in s.marks["cuts"]:
        got, count = m.decode(s.data[:cut], True)
        assert oracle_count(s.data[:cut], True) == count
        np.testing.assert_array_equal(got, vals[:count])
        assert m.v1_chunk(cut, len(s.segs)) == cb


@pytest.mark.parametrize("cb", m.WIDTHS)
def test_range_stream(cb):
    s = m.range_stream(cb)
    agree_shape(s)
    w = m.walk(s.data)[:7]
    assert [(g[1], g[2]) for g in w] == [(m.LIT, 50), (m.RUN, 20), (m.RUN, 100), (m.LIT, 128), (m.RUN, 32), (m.RUN, 33),
                                         (m.LIT, 5)]
    f = s.marks["first"]
    for k in range(7):  # a range starts and ends strictly inside every group
        assert any(f[k] < a < f[k + 1] and f[k] < a + c < f[k + 1] for a, c in s.marks["ranges"])
    vals = m.decode(s.data, True)[0]
    assert (m.truncate(vals[:f[-1]], 4) != vals[:f[-1]]).mean() > 0.9


@pytest.mark.parametrize("cb", m.WIDTHS)
@pytest.mark.parametrize("empty", [False, True])
def test_grouped_tables(empty, cb):
    data, segs = m.grouped(cb, empty)
    agree(data, True)
    assert m.v1_chunk(len(data), len(segs)) == cb and len(data) <= 66_000
    first = dict(m.group_table(data))
    assert all(first[off] == vi for off, vi in segs) and segs == sorted(segs)
    assert (len(set(segs)) < len(segs)) == empty
    sizes = {g[0]: g[3] for g in m.walk(data)}
    assert sizes[segs[0][0]] >= 3 and sizes[segs[5][0]] >= 3 or empty  # a byte strictly inside groups 0 and 5


# ---- the crafted files (tests/rlev1_files.py) ---------------------------------
import orc_craft as oc  # noqa: E402
import rlev1_files as vf  # noqa: E402

FILES = {"V": vf.file_v, "W": vf.file_w, "R": vf.file_r, "V0": lambda: vf.file_v(stride=0), "VS": vf.file_vs}


@pytest.mark.parametrize("name", list(FILES))
def test_pyarrow_reads_the_crafted_files(name, tmp_path):
    po = pytest.importorskip("pyarrow.orc")
    f = FILES[name]()
    p = tmp_path / "crafted.orc"
    p.write_bytes(f.data)
    o = po.ORCFile(str(p))
    assert o.nrows == sum(n for n, _ in f.stripes) and o.nstripes == len(f.stripes)
    assert o.row_index_stride == f.stride and o.compression == "UNCOMPRESSED"
    assert [x.name for x in o.schema] == f.names
    for k in range(len(f.stripes)):
        assert o.read_stripe(k).to_pylist() == f.rows(k), (name, k)


@pytest.mark.parametrize("name", list(FILES))
def test_oracle_decodes_every_stream_of_the_crafted_files(name):
    f = FILES[name]()
    for k, (n, cols) in enumerate(f.stripes):
        assert [c.name for c in cols] == f.names
        for c in cols:
            for s in c.rle:
                got, count = m.decode(s.data, s.signed)
                assert count == s.values.size == sum(g[2] for g in s.groups)
                np.testing.assert_array_equal(got, s.values)
                np.testing.assert_array_equal(oracle.RleDecoderV1(s.data, s.signed).next(count), s.values)
            data = [s for s in c.rle if s.slot != "LENGTH" or c.blob is not None][0]
            assert data.values.size == (n if c.present is None else int(c.present.sum()))
            if c.present is not None:
                bits = oracle.ByteRleDecoder(oc.bool_rle(c.present), boolean=True).next(n)
                np.testing.assert_array_equal(bits, c.present)
                assert 0 < c.present.sum() < n



def _first_values(s):
    return dict(m.group_table(s.data))


@pytest.mark.parametrize("name", ["V", "W", "R", "VS"])
def test_positions_of_the_crafted_files(name):
    """Every RLEv1 pair points at a group header, and header + skip is the row
    group's first value (its first non-null value under PRESENT); the oracle
    seeks there and reads the row group's values."""
    f = FILES[name]()
    for k, (n, cols) in enumerate(f.stripes):
        for c in cols:
            cc = c.craft(f.stride)
            rows = list(range(0, n, f.stride))
            assert len(cc.positions) == len(rows)
            s = [x for x in c.rle if x.indexed][0]
            first = _first_values(s)
            before = np.concatenate([[0], np.cumsum(c.present)]) if c.present is not None else np.arange(n + 1)
            for g, e in zip(rows, cc.positions):
                off, skip = int(e[-2]), int(e[-1])
                vi = int(before[g])
                if vi == s.values.size and off == len(s.data):
                    continue
                assert first[off] + skip == vi and 0 <= skip < 130, (name, k, c.name, g)
                dec = oracle.RleDecoderV1(s.data, s.signed)
                dec.seek(off, skip)
                k2 = min(int(before[min(g + f.stride, n)]) - vi, s.values.size - vi)
                np.testing.assert_array_equal(dec.next(k2), s.values[vi:vi + k2])
            assert len(cc.positions[0]) == 2 + (1 if c.blob is not None else 0) + (3 if c.present is not None else 0)
            if c.present is not None:
                for g, e in zip(rows, cc.positions):
                    dec = oracle.ByteRleDecoder(oc.bool_rle(c.present), boolean=True)
                    dec.seek(*[int(x) for x in e[:3]])
                    np.testing.assert_array_equal(dec.next(min(f.stride, n - g)), c.present[g:g + f.stride])


def test_makeup_of_the_crafted_files():
    v = vf.file_v()
    n, cols = v.stripes[0]
    by = {c.name: c for c in cols}
    assert (n + v.stride - 1) // v.stride == 4 and n % v.stride == 1  # the last row group has 1 row
    seg = lambda s: np.diff(np.concatenate([s.positions(v.stride)[:, 0], [len(s.data)]]).astype(np.int64))
    tiny, wide, runs = by["tiny"].rle[0], by["wide"].rle[0], by["runs"].rle[0]
    assert {g[1:] for g in tiny.groups[:-1]} == {(m.LIT, 128, 129)} and seg(tiny)[:3].max() <= 2048  # kCB = 4
    assert {g[1:] for g in wide.groups[:-1]} == {(m.LIT, 128, 1281)} and seg(wide)[:3].min() > 2048  # kCB = 16
    assert all(g[1] == m.RUN for g in runs.groups) and (runs.positions(v.stride)[1:, 1] > 0).all()
    assert runs.positions(v.stride)[:, 1].tolist() == [0, 90, 50, 10]
    mix = by["mix"].rle[0]
    assert {g[1] for g in mix.groups} == {m.RUN, m.LIT} and (mix.positions(v.stride)[1:, 1] > 0).any()
    small = by["small"].rle[0].values
    assert small.min() >= -(1 << 15) and small.max() < (1 << 15) and np.abs(small).max() > 1 << 12
    length, data = by["dict"].rle
    assert not length.indexed and length.values.tolist() == [3, 5, 1] and not data.signed
    assert {g[1] for g in data.groups} == {m.RUN, m.LIT} and set(data.values.tolist()) == {0, 1, 2}
    assert {g[1] for g in by["str"].rle[0].groups} == {m.RUN, m.LIT} and by["str"].rle[0].values.min() >= 0
    assert len(v.rle_streams()) == 9
    # V's streams are small streams (host plans); W's and R's keep the row index
    assert max(len(s.data) for _, s in v.rle_streams()) <= vf.SMALL_STREAM
    w = vf.file_w()
    for c in w.stripes[0][1]:
        s = c.rle[0]
        pos = s.positions(w.stride)
        assert len(s.data) > vf.SMALL_STREAM and np.diff(pos[:, 0].astype(np.int64)).max() <= 2048  # kCB = 4
        if c.name != "tiny":
            assert {g[1:] for g in s.groups[1:-1]} == {(m.RUN, 130, 64)}
            offs = pos[:, 0].tolist()
            assert len(set(offs)) < len(offs) * 0.8  # several row groups start in one run: empty segments
            assert pos[:, 1].max() > 100
    r = vf.file_r()
    for c in r.stripes[0][1]:
        s = c.rle[0]
        pos = np.array([e[-2:] for e in c.craft(r.stride).positions], dtype=np.int64)
        assert len(s.data) > vf.SMALL_STREAM and np.diff(pos[:, 0]).min() > 2048  # kCB = 16
        assert (pos[1:, 1] > 0).any() and (pos[1:, 0] > 0).all()
    assert {g[1:3] for g in r.stripes[0][1][1].rle[0].groups[:-1]} <= {(m.RUN, 3), (m.RUN, 4), (m.RUN, 5)}
    assert [len(x[1]) for x in vf.file_vs().stripes] == [8, 8, 8]


@pytest.mark.parametrize("cut", [(2,), (5,), (2, 5)])
def test_cut_files_are_rejected_by_the_oracle_and_pyarrow(cut, tmp_path):
    po = pytest.importorskip("pyarrow.orc")
    f, whole = vf.file_v(cut=cut), vf.file_v()
    for cid, c in enumerate(f.stripes[0][1], start=1):
        s, w = c.rle[-1], whole.stripes[0][1][cid - 1].rle[-1]
        if cid in cut:
            last = s.groups[-1]
            assert last[0] < len(s.data) < last[0] + last[3] and s.full == w.data
            assert m.decode(s.data, True)[1] < s.values.size
            with pytest.raises(oracle.OracleError, match="bad read in readByte"):
                oracle.RleDecoderV1(s.data, True).next(s.values.size)
            assert c.craft(f.stride).positions == whole.stripes[0][1][cid - 1].craft(f.stride).positions
            assert all(p[0] < len(s.data) for p in c.craft(f.stride).positions)
        else:
            assert s.data == w.data
    p = tmp_path / "cut.orc"
    p.write_bytes(f.data)
    with pytest.raises(OSError, match="bad read in readByte"):
        po.ORCFile(str(p)).read()
