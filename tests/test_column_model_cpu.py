"""tests/column_model.py checked by something that is not the model: the
dictionary job against the C oracle's gather, the scan against Python
big-integer arithmetic, the row-group segments, the scatter and the union
against row-by-row loops, flatten() by rebuilding the rows from its arrays,
and every crafted file of tests/nested_files.py against pyarrow's ORC reader
(the reference's C++ reader) and the oracle's stream decoders.

Who vouches for which crafted file:
  N1, N2 (16 / 4096 / 4097 entries), N5, N6, N7 (65,536 / 65,537), N8:
      pyarrow reads every row equal to the rows the file was built from.
  N9: the same (its union's values compared without their tags).
  N3, N4: pyarrow (unions come as sparse_union: the values equal the rows',
      the type codes equal flatten()'s tags on the non-null rows).
  Every file with a row index: the oracle's RleDecoderV2 / ByteRleDecoder,
      sought to every row group's positions, decode the values flatten() has
      there (pyarrow's whole-file read never seeks).
  Bad N2 (16 / 4097), bad N7 (both), N8 one byte short, N9-index (bad keys
      and t one byte short: the keys' error, column 5 before column 11):
      pyarrow raises the reference's error.
  N9-tag, N9-tag-short: bad union tags, which pyarrow cannot take (below): the
      oracle reads the crafted tags back; the order of the three errors is
      StructColumnReader::next's, field by field (m, then u, then t).
  Bad N3, N8 negative, N8 wrap: pyarrow 25's bundled ORC reader predates the
      reference's checks (getCheckedUnionTag, computeSize's addLength) and
      crashes the process on them, so it is not run on these: the oracle's
      decoders read the crafted tags / lengths back, and the model says what
      the reference's checks see in them."""
import numpy as np
import pytest

import column_model as cm
import nested_files as nf
from oracle import oracle

M64 = (1 << 64) - 1


def _signed(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


@pytest.mark.parametrize("n", [0, 1, 2, 1000])
@pytest.mark.parametrize("kind", ["clean", "negative", "wrap", "huge"])
def test_scan_against_big_integers(n, kind):
    rng = np.random.default_rng(n)
    x = rng.integers(0, 1 << 20, size=n, dtype=np.int64)
    if n >= 3 and kind == "negative":
        x[n // 2] = -5
    if n >= 3 and kind == "wrap":
        x[n // 2 - 1:n // 2 + 2] = (1 << 63) - 1
    if n >= 3 and kind == "huge":
        x[[0, n // 2, n - 1]] = [-(1 << 63), (1 << 63) - 1, -1]
    total, neg, wrap, want = 0, 0, 0, [0]
    for v in x.tolist():
        neg |= v < 0
        start = total
        total = (total + (v & M64)) & M64  # the kernels add the value's 64 bits unsigned
        wrap |= total < start
        want.append(_signed(total))
    off, got_neg, got_wrap, got_total = cm.scan(x)
    assert off.dtype == np.int64 and off.tolist() == want
    assert (got_neg, got_wrap, got_total) == (int(neg), int(wrap), total)
    if n >= 3:
        assert (got_neg, got_wrap) == {"clean": (0, 0), "negative": (1, 1), "wrap": (0, 1), "huge": (1, 1)}[kind]


@pytest.mark.parametrize("D,n,masked", [(1, 1, False), (16, 300, True), (17, 2049, False), (4096, 5000, True)])
def test_dict_job_against_the_oracle_gather(D, n, masked):
    rng = np.random.default_rng(D)
    lengths = rng.integers(0, 50, size=D, dtype=np.int64)
    idx = rng.integers(0, D, size=n, dtype=np.int64)
    nn = (rng.random(n) < 0.6).astype(np.uint8) if masked else None
    if masked:
        idx[nn == 0] = D + 3  # never read
    off, summary, start, ln, err = cm.dict_job(lengths, idx, nn, n)
    want_start, want_len = oracle.dict_gather(idx, lengths, nn)  # zero-initialised: null rows are (0, 0)
    assert err is None
    np.testing.assert_array_equal(start, want_start)
    np.testing.assert_array_equal(ln, want_len)
    assert off.tolist() == [0] + np.cumsum(lengths).tolist()
    assert summary.tolist() == [int(lengths.sum()), 0]


def test_dict_job_errors_and_negative_lengths():
    lengths = np.array([3, -(1 << 40), 5], dtype=np.int64)
    idx = np.array([0, 3, 1, -1, 7, 2], dtype=np.int64)
    nn = np.array([1, 0, 9, 1, 1, 1], dtype=np.uint8)
    before = np.arange(100, 106, dtype=np.int64)
    off, summary, start, ln, err = cm.dict_job(lengths, idx, nn, 6, start_before=before, len_before=before + 50)
    assert off.tolist() == [0, 3, 3 - (1 << 40), 8 - (1 << 40)]
    assert summary.tolist() == [(8 - (1 << 40)) & M64, 1]
    assert err == 3  # the lowest bad row that is not null: -1 as uint64; row 1 is null
    assert start.tolist() == [0, 0, 3, 103, 104, 3 - (1 << 40)]
    assert ln.tolist() == [3, 0, -(1 << 40), 153, 154, 5]
    with pytest.raises(oracle.OracleError):
        oracle.dict_gather(idx, lengths, nn)
    assert cm.dict_job(lengths, idx, None, 1)[4] is None and cm.dict_job(lengths, idx, None, 2)[4] == 1


@pytest.mark.parametrize("G", [1, 7, 70])
@pytest.mark.parametrize("boolean", [0, 1])
def test_rg_segments_row_by_row(G, boolean):
    rng = np.random.default_rng(G + boolean)
    sizes = rng.integers(0, 30, size=G)
    rows = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    n = max(int(sizes.sum()) - 20, 0) if G > 1 else int(sizes.sum())  # the last row groups start past n
    mask = ((rng.random(n) < 0.5) * rng.integers(1, 256, size=n)).astype(np.uint8)
    trip = np.stack([rng.integers(0, 1 << 40, size=G), rng.integers(-3, 12, size=G), rng.integers(0, 8, size=G)],
                    axis=1)
    prefix, seg = cm.rg_segments(mask, n, rows, trip, boolean)
    seen, want_prefix, want_seg, negative = 0, [], [], 0
    for g in range(G):
        want_prefix.append(seen)
        if boolean:
            v = int((seen - int(trip[g, 2])) / 8.0) - int(trip[g, 1])  # float division, then int(): toward zero
        else:
            v = seen - int(trip[g, 1])
        negative += v < 0
        want_seg.append([int(trip[g, 0]), max(v, 0)])
        end = int(rows[g + 1]) if g + 1 < G else n
        for r in range(min(int(rows[g]), n), min(end, n)):
            seen += mask[r] != 0
    assert prefix.tolist() == want_prefix + [seen]
    assert seg.tolist() == want_seg
    assert seen == int((mask != 0).sum()) and (G == 1 or negative > 0)


def test_rg_segments_truncates_toward_zero():
    # prefix 3, bits 7: (3 - 7) / 8 is 0 in C (floor gives -1); skip -1 shows it past the clamp
    mask = np.ones(3, dtype=np.uint8)
    prefix, seg = cm.rg_segments(mask, 3, [0, 3], [[10, 0, 0], [20, -1, 7]], 1)
    assert prefix.tolist() == [0, 3, 3] and seg.tolist() == [[10, 0], [20, 1]]


@pytest.mark.parametrize("cols", [None, 2])
def test_scatter_row_by_row(cols):
    rng = np.random.default_rng(3)
    nn = ((rng.random(50) < 0.5) * rng.integers(1, 256, size=50)).astype(np.uint8)
    k = int((nn != 0).sum())
    shape = lambda m: (m,) if cols is None else (m, cols)
    dense = rng.integers(-99, 99, size=shape(k))
    before = np.full(shape(50), 77)
    for fill in (None, -9, 4):
        want, j = before.copy(), 0
        for r in range(50):
            if nn[r]:
                want[r] = dense[j]
                j += 1
            elif fill is not None:
                want[r] = fill if cols is None else [-1 if fill < 0 else 0, fill]
        np.testing.assert_array_equal(cm.scatter(dense, nn, before, fill=fill), want)
    np.testing.assert_array_equal(before, 77)


def test_union_row_by_row():
    tags = np.array([0, 2, 2, 1, 5, 0, 2, 255, 1], dtype=np.uint8)
    off, counts, bad = cm.union(tags, 3, offsets_before=np.full(9, -4))
    assert off.tolist() == [0, 0, 1, 0, -4, 1, 2, -4, 1]
    assert counts.tolist() == [2, 2, 3] and bad == (4 << 8) | 5
    assert cm.union(tags[:4], 3)[2] is None and cm.union(tags, 256)[2] is None
    assert cm.union(tags[:0], 2)[1].tolist() == [0, 0]


# ---- nested values and the crafted files -----------------------------------------------
@pytest.mark.parametrize("name", list(nf.GOOD))
def test_flatten_round_trips(name):
    f = nf.GOOD[name]()
    assert cm.rebuild(f.cols) == f.rows
    for c in f.cols:
        assert c.not_null.size == c.n
        if c.present is not None:
            assert c.present.size == (c.n if c.incoming is None else int((c.incoming != 0).sum()))
        if c.node.kind in ("list", "map"):
            assert all(ch.n == c.offsets[-1] == c.lengths.sum() for ch in c.children)
        if c.node.kind == "union":
            assert [ch.n for ch in c.children] == c.counts.tolist() and c.tags.size == c.nonnull


def test_flatten_of_a_small_tree():
    tree = cm.Node("struct", [cm.Node("list", [cm.Node("union", [cm.Node("long"), cm.Node("string", nullable=True)])],
                                      nullable=True), cm.Node("boolean", nullable=True)], ["l", "b"], nullable=True)
    rows = [{"l": [(0, 5), (1, "x")], "b": None}, None, {"l": None, "b": True}, {"l": [(1, None), (0, 6), (1, "y")], "b": False}]
    root, lst, un, lng, st, bo = cm.flatten(tree, rows)
    assert root.present.tolist() == [1, 0, 1, 1] and lst.present.tolist() == [1, 0, 1] and lst.n == 4
    assert lst.not_null.tolist() == [1, 0, 0, 1] and lst.lengths.tolist() == [2, 3]
    assert lst.offsets.tolist() == [0, 2, 2, 2, 5]
    assert un.n == 5 and un.present is None and un.tags.tolist() == [0, 1, 1, 0, 1]
    assert un.offsets.tolist() == [0, 0, 1, 1, 2] and un.counts.tolist() == [2, 3]
    assert lng.dense.tolist() == [5, 6] and st.dense == [b"x", b"y"] and st.not_null.tolist() == [1, 0, 1]
    assert bo.incoming.tolist() == [1, 0, 1, 1] and bo.present.tolist() == [0, 1, 1] and bo.dense.tolist() == [1, 0]
    assert cm.rebuild([root, lst, un, lng, st, bo]) == rows


def _plain(v):
    """A row as pyarrow's to_pylist gives it: a union value without its tag."""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], int) and not isinstance(v[0], bool) \
            and not isinstance(v[1], tuple):
        return _plain(v[1])
    if isinstance(v, list):
        return [(_plain(x[0]), _plain(x[1])) if isinstance(x, tuple) and isinstance(x[0], str) else _plain(x) for x in v]
    return v


def _read(f, tmp_path):
    import pyarrow.orc as po

    p = tmp_path / "crafted.orc"
    p.write_bytes(f.data)
    return po.ORCFile(str(p)).read()


@pytest.mark.parametrize("name", list(nf.GOOD))
def test_pyarrow_reads_the_rows_the_file_was_built_from(name, tmp_path):
    f = nf.GOOD[name]()
    t = _read(f, tmp_path)
    got, want = t.to_pylist(), [_plain(r) for r in f.pylist()]
    assert len(got) == len(want) == len(f.rows)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s row %d" % (name, i)
    if name == "N3":
        u = t.column("u").combine_chunks()
        codes = np.asarray(u.type_codes)
        np.testing.assert_array_equal(codes[f.cols[1].not_null != 0], f.cols[1].tags)
    if name == "N4":
        u = t.column("l").combine_chunks().values
        assert len(u) == f.cols[2].n
        np.testing.assert_array_equal(np.asarray(u.type_codes)[f.cols[2].not_null != 0], f.cols[2].tags)


@pytest.mark.parametrize("name", [n for n in nf.GOOD if n != "N6"])
def test_oracle_decoders_sought_to_every_row_group(name):
    """The row index of every column: the reference's decoders, sought to a
    row group's positions, give the values that follow the column's value
    count at the parent row group's first row."""
    f = nf.GOOD[name]()
    sought = 0
    for c in f.cols:
        for s, at in c.seeks:
            assert len(at) == (len(f.rows) + f.stride - 1) // f.stride
            for v in at:
                k = min(12, s.values.size - v)
                if isinstance(s, nf.IntStream):
                    d = oracle.RleDecoderV2(s.data, s.signed)
                else:
                    d = oracle.ByteRleDecoder(s.data, boolean=s.boolean)
                d.seek(*s.at(v))
                np.testing.assert_array_equal(d.next(k), s.values[v:v + k], err_msg="%s column %d" % (name, c.id))
                sought += 1
    assert sought > 0


PYARROW_RAISES = ["N2-16-index", "N2-4097-index", "N7-65536-negative", "N7-65537-negative", "N8-short", "N9-index"]


@pytest.mark.parametrize("name", PYARROW_RAISES)
def test_pyarrow_raises_the_reference_error(name, tmp_path):
    make, text = nf.BAD[name]
    with pytest.raises(OSError) as e:
        _read(make(), tmp_path)
    # pyarrow's bundled reader words the dictionary check without the column
    assert text.replace(" for column 1", "") in str(e.value)


def test_bad_files_the_bundled_reader_cannot_take():
    """What the reference's checks see in bad N3 and the bad lengths of N8,
    from the oracle's decode of the crafted streams."""
    f = nf.n3(bad=True)
    u = f.cols[1]
    tags = oracle.ByteRleDecoder(f.crafted[1].streams[1][1]).next(u.tags.size)
    np.testing.assert_array_equal(tags, u.tags)
    a, b = nf.N3_BAD
    assert np.flatnonzero(tags >= 3).tolist() == [a, b, tags.size - 1]
    assert cm.union(tags, 3)[2] == (a << 8) | 3 and nf.UNION_TAG == "Invalid union tag 3 for union with 3 children"
    # bad N9's tags (N9-tag, N9-tag-short); in N9-tag the keys' bad indices, which pyarrow raises for
    # N9-index, belong to column 5, read before the union (column 7)
    for name in ("N9-tag", "N9-tag-short"):
        f = nf.BAD[name][0]()
        u = f.cols[nf.N9_UNION]
        tags = oracle.ByteRleDecoder(f.crafted[nf.N9_UNION].streams[1][1]).next(u.tags.size)
        np.testing.assert_array_equal(tags, u.tags)
        assert np.flatnonzero(tags >= 2).tolist() == list(nf.N9_BAD_TAGS)
        assert cm.union(tags, 2)[2] == (nf.N9_BAD_TAGS[0] << 8) | 3
        assert nf.BAD["N9-tag-short"][1] == "Invalid union tag 3 for union with 2 children"
    keys = nf.BAD["N9-tag"][0]().cols[nf.N9_KEYS]
    assert np.flatnonzero(keys.dense >= len(keys.entries)).tolist() == list(nf.N9_BAD_KEYS) and nf.N9_KEYS < nf.N9_UNION
    last_tile = 2 * 4096
    for bad, flags in (("negative", (1, None)), ("wrap", (0, 1))):
        f = nf.n8(bad)
        lens = oracle.RleDecoderV2(f.crafted[1].streams[1][1], False).next(nf.N8_ROWS)
        np.testing.assert_array_equal(lens, f.cols[1].value_lengths)
        _, neg, wrap, _ = cm.scan(lens)
        assert neg == flags[0] and (flags[1] is None or wrap == flags[1])
        assert cm.scan(lens[:last_tile])[1:3] == (0, 0)  # nothing before the last tile
        assert len(f.crafted[1].streams[0][1]) == sum(len(r["s"]) for r in f.rows)
    assert len(nf.n8("short").crafted[1].streams[0][1]) == len(nf.n8().crafted[1].streams[0][1]) - 1
