"""CPU self-checks of the crafted files of tests/multi_stream_files.py, before
any GPU is involved: every stream decodes on the oracle (and the file in
pyarrow's ORC reader) to the generated values, holds the runs it means to
hold, its row-index positions point at run headers, and the files reach the
launch planner's cases (density classes, job re-ordering, the 78-run segment,
the segment past the two-pass bound, the stream of src_len / 2 runs) that
tests/test_gpu_multi_stream.py aims at. No GPU."""
import numpy as np
import pytest

import multi_stream_files as msf
from multi_stream_files import M_ROWS, M_STRIDE, density_class, seg_value_bound, segment_values
from oracle import oracle
from rle_streams import DELTA, DIRECT, PATCHED, SR

FILES = {"M": msf.file_m, "F": msf.file_f, "S": msf.file_s, "M-no-index": lambda: msf.file_m(stride=0)}
READ_ERROR = "bad read in RleDecoderV2::readByte"


def _col(f, name, stripe=0):
    return f.stripes[stripe][1][f.names.index(name)]


@pytest.mark.parametrize("name", list(FILES))
def test_oracle_decodes_every_stream_to_the_generated_values(name):
    f = FILES[name]()
    for k, (n, cols) in enumerate(f.stripes):
        for c in cols:
            for s in c.rle:
                got = oracle.rlev2_decode(s.data.tobytes(), s.values.size, s.signed)
                np.testing.assert_array_equal(got, s.values, err_msg="%s stripe %d %s %s" % (name, k, c.name, s.slot))
            if c.dictionary is None and c.blob is None:
                assert c.rle[0].values.size == n and c.values is c.rle[0].values


@pytest.mark.parametrize("name", list(FILES))
def test_pyarrow_reads_the_generated_values(name, tmp_path):
    po = pytest.importorskip("pyarrow.orc")
    f = FILES[name]()
    p = tmp_path / "crafted.orc"
    p.write_bytes(f.data)
    o = po.ORCFile(str(p))
    assert o.nrows == sum(n for n, _ in f.stripes) and o.nstripes == len(f.stripes)
    assert o.row_index_stride == f.stride and o.compression == "UNCOMPRESSED"
    assert [x.name for x in o.schema] == f.names
    for k, (n, cols) in enumerate(f.stripes):
        t = o.read_stripe(k)
        assert t.num_rows == n
        for c in cols:
            got = t.column(c.name)
            assert got.null_count == 0
            if isinstance(c.values, list):
                assert got.to_pylist() == c.values, (name, k, c.name)
            else:
                np.testing.assert_array_equal(got.to_numpy().astype(np.int64), c.values, err_msg="%s %d %s" % (name, k, c.name))


def test_reader_metadata_of_the_crafted_files():
    import orc_amd

    for name, make in FILES.items():
        f = make()
        r = orc_amd.Reader(f.data)  # metadata only
        assert r.num_rows == sum(n for n, _ in f.stripes) and r.num_stripes == len(f.stripes)
        assert r.row_index_stride == f.stride and r.compression == "NONE"
        assert [r.stripe(k)["num_rows"] for k in range(r.num_stripes)] == [n for n, _ in f.stripes]
        assert all((r.stripe(k)["index_length"] > 0) == (f.stride > 0) for k in range(r.num_stripes))


def _shape(s):
    return [(r[1], r[2], r[3]) for r in s.runs]


def test_run_makeup_of_m():
    f = msf.file_m()
    assert (M_ROWS + M_STRIDE - 1) // M_STRIDE == 4 and M_ROWS % M_STRIDE == 1  # 4 row groups, the last of 1 row
    assert sum(len(s.data) for _, s in f.rle_streams()) + len(_col(f, "str").blob) < 2_000_000
    wide = _col(f, "wide").rle[0]
    assert _shape(wide) == [(DIRECT, 64, 512)] * 58 + [(DIRECT, 64, 305)]
    assert (wide.positions(M_STRIDE)[1:, 1] > 0).all()  # the later segments start inside a run
    chain = _shape(_col(f, "chain").rle[0])
    assert chain[:11] == [(DIRECT, 48, 512)] * 5 + [(DIRECT, 48, 511)] + [(DIRECT, 56, 512)] * 3 + \
        [(DIRECT, 40, 512), (DIRECT, 40, 300)]
    assert chain[11:-1] == [(DIRECT, 64, 512)] * 48 and chain[-1] == (DIRECT, 64, 6)
    # the chain of equal full runs ends inside segment 0 (row group 0 holds
    # the 511- and the 300-value run)
    assert 5 * 512 + 511 < M_STRIDE and sum(r[2] for r in chain[:11]) < M_STRIDE
    assert _shape(_col(f, "w24").rle[0]) == [(DIRECT, 24, 512)] * 58 + [(DIRECT, 24, 305)]
    assert _shape(_col(f, "w16x5").rle[0]) == [(DIRECT, 16, 5)] * 6000 + [(DIRECT, 16, 1)]
    sr = _col(f, "sr").rle[0]
    assert all(r[1] == SR and r[2] == 8 and 3 <= r[3] <= 10 and r[4] == 2 for r in sr.runs)
    assert {r[3] for r in sr.runs} == set(range(3, 11))
    # exactly src_len / 2 runs: the job's run-table range is used to its end
    assert len(sr.data) % 2 == 0 and len(sr.runs) == len(sr.data) // 2
    d = _col(f, "delta").rle[0]
    assert all(r[1] == DELTA for r in d.runs)
    for fixed in (True, False):
        lens = {r[3] for r in d.runs if (r[2] == 0) == fixed}
        assert 512 in lens and lens - {512} == set(range(3, 17)), (fixed, lens)
    p = _col(f, "patched").rle[0]
    assert {r[1] for r in p.runs} == {DIRECT, PATCHED}
    assert all(r[3] <= 20 for r in p.runs if r[1] == DIRECT) and all(r[3] == 512 for r in p.runs if r[1] == PATCHED)
    lists = [p.data[r[0] + 3] & 0x1F for r in p.runs if r[1] == PATCHED]  # patch-list lengths
    assert len(lists) >= 6 and lists == [msf.PATCH_LIST[i % 3] for i in range(len(lists))]
    gap390 = [r for r in p.runs if r[1] == PATCHED][2]  # (10, 400): gap 390 = an escape entry (255, 0) + 135
    assert (p.data[gap390[0] + 3] >> 5) + 1 == 8  # 8-bit gaps
    kinds = [p.runs[i][1] for i in range(len(p.runs))]
    assert all(kinds[i - 1] == DIRECT and kinds[i + 1] == DIRECT for i in range(len(kinds)) if kinds[i] == PATCHED)
    small = _col(f, "small").rle[0]
    assert {r[1] for r in small.runs} == {SR, DIRECT, PATCHED, DELTA}
    assert len({r[2] for r in small.runs}) >= 10 and len({r[3] for r in small.runs}) >= 40
    assert small.values.min() >= -(1 << 15) and small.values.max() < (1 << 15)
    length, data = _col(f, "dict").rle
    assert _shape(length) == [(DIRECT, 3, 3)] and not length.indexed and length.values.tolist() == [3, 5, 1]
    assert _shape(data) == [(DIRECT, 2, 512)] * 58 + [(DIRECT, 2, 305)] and not data.signed
    ln = _col(f, "str").rle[0]
    assert {r[1] for r in ln.runs} == {SR, DIRECT} and max(r[3] for r in ln.runs) <= 20 and not ln.signed
    assert ln.values.min() == 0 and ln.values.max() == 40
    assert len(f.rle_streams()) == 11


def test_run_makeup_of_f():
    f = msf.file_f()
    for name, W in (("w64", 64), ("w56", 56)):
        s = _col(f, name).rle[0]
        assert _shape(s) == [(DIRECT, W, 512)] * 156 + [(DIRECT, W, 129)]
        pos = s.positions(msf.F_STRIDE)
        # segment 0 holds 78 whole runs: more than one 64-run header probe
        assert sum(1 for r in s.runs if r[0] < pos[1, 0]) == 78 and pos[1, 0] == 78 * (2 + 64 * W)
        assert pos[1, 1] == msf.F_STRIDE - 78 * 512 and pos[2, 1] == 2 * msf.F_STRIDE - 156 * 512
    sr = _col(f, "sr").rle[0]
    assert all(r[1] == SR and r[4] == 2 for r in sr.runs) and len(sr.runs) == len(sr.data) // 2
    assert (msf.F_ROWS + msf.F_STRIDE - 1) // msf.F_STRIDE == 3 and msf.F_ROWS % msf.F_STRIDE == 1
    assert len(f.rle_streams()) == 3


@pytest.mark.parametrize("name", ["M", "F", "S"])
def test_positions_point_at_run_headers(name):
    f = FILES[name]()
    for k, (n, cols) in enumerate(f.stripes):
        for c in cols:
            cc = c.craft(f.stride)
            assert len(cc.positions) == (n + f.stride - 1) // f.stride
            for s in c.rle:
                if not s.indexed:
                    continue
                starts = {r[0]: v0 for r, v0 in zip(s.runs, np.cumsum([0] + [r[3] for r in s.runs]))}
                for g, e in enumerate(cc.positions):
                    off, skip = int(e[-2]), int(e[-1])  # the RLE pair comes last
                    assert off in starts, (name, k, c.name, g)
                    assert skip == g * f.stride - starts[off] and 0 <= skip < 512
            if c.blob is not None:
                starts = np.concatenate([[0], np.cumsum(c.rle[0].values)])
                assert [int(e[0]) for e in cc.positions] == [int(starts[g * f.stride]) for g in range(len(cc.positions))]
                assert all(len(e) == 3 for e in cc.positions)
            else:
                assert all(len(e) == 2 for e in cc.positions)


def _classes(f, stripe=0):
    return [density_class(len(s.data), s.values.size) for _, s in f.rle_streams(stripe)]


def test_density_classes_and_job_order():
    """default_variant's routing rule restated: M (and every stripe of S) has
    streams in each class, and the planner's stable sort by stream bytes per
    value moves jobs away from column order."""
    m = msf.file_m()
    by_col = dict(zip([(cid, s.slot) for cid, s in m.rle_streams()], _classes(m)))
    assert by_col[(1, "DATA")] == 2 and by_col[(2, "DATA")] == 2
    assert by_col[(3, "DATA")] == 3 and by_col[(4, "DATA")] == 3
    assert by_col[(5, "DATA")] == 6 and by_col[(6, "DATA")] == 6 and by_col[(9, "DATA")] == 6
    s = msf.file_s()
    for f, stripes in ((m, 1), (s, 3), (msf.file_m(stride=0), 1)):
        for k in range(stripes):
            assert set(_classes(f, k)) == {2, 3, 6}
            jobs = [(len(x.data), x.values.size) for _, x in f.rle_streams(k)]
            order = sorted(range(len(jobs)), key=lambda i: -jobs[i][0] / jobs[i][1])  # stable
            assert order != list(range(len(jobs)))
            for c in (2, 3, 6):  # within each default launch too, where it has more than one job
                mine = [i for i in range(len(jobs)) if density_class(*jobs[i]) == c]
                if c != 2:
                    assert [i for i in order if i in mine] != mine, c
    f = msf.file_f()
    assert _classes(f) == [2, 2, 6]
    # the tiny job (3 values, one segment) sits between jobs of 30,001 values
    sizes = [x.values.size for _, x in m.rle_streams()]
    assert sizes[8] == 3 and sizes[7] == sizes[9] == M_ROWS


def test_two_pass_bound():
    """seg_value_bound restated: F's segments are longer than the bound of any
    launch its streams join (and, its last row group holding one row, so are
    M's full row groups: 10,000 values against 8,950)."""
    f = msf.file_f()
    bounds = [seg_value_bound(s.values.size, 3) for _, s in f.rle_streams()]
    assert bounds == [30_512] * 3  # avg 26,667
    sr = _col(f, "sr").rle[0]
    assert segment_values(sr, f.stride)[:2].min() >= msf.F_STRIDE > max(bounds)
    m = msf.file_m()
    bound = max(seg_value_bound(s.values.size, 4 if s.indexed else 1) for _, s in m.rle_streams())
    assert bound == 8_950  # avg 7,501
    for _, s in m.rle_streams():
        if s.indexed:
            assert M_STRIDE <= segment_values(s, m.stride)[:3].min() and segment_values(s, m.stride).max() < M_STRIDE + 512


@pytest.mark.parametrize("cut", [(2,), (6,), (2, 6)])
def test_cut_streams_are_rejected_by_the_oracle_and_pyarrow(cut, tmp_path):
    po = pytest.importorskip("pyarrow.orc")
    f = msf.file_m(cut=cut)
    whole = msf.file_m()
    for cid, c in enumerate(f.stripes[0][1], start=1):
        s, w = c.rle[0], whole.stripes[0][1][cid - 1].rle[0]
        if cid in cut:
            last = s.runs[-1]
            assert last[0] < len(s.data) < last[0] + last[4] and len(s.full) == len(w.data)
            with pytest.raises(oracle.OracleError) as e:
                oracle.RleDecoderV2(s.data.tobytes(), True).next(M_ROWS)
            assert str(e.value) == READ_ERROR
            # the positions are those of the whole stream and stay inside the cut one
            assert c.craft(f.stride).positions == whole.stripes[0][1][cid - 1].craft(f.stride).positions
            assert all(p[0] < len(s.data) for p in c.craft(f.stride).positions)
        else:
            assert bytes(s.data) == bytes(w.data)
    p = tmp_path / "cut.orc"
    p.write_bytes(f.data)
    with pytest.raises(OSError, match=READ_ERROR):  # the reference C++ reader: the oracle's message
        po.ORCFile(str(p)).read()
