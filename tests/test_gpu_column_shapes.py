"""The column kernels (orc_amd/csrc/column_kernels.hip) against the exact
model of tests/column_model.py, at the sizes where their tiles, waves, trips
and look-back rounds end: the null scatter (4,096-row tiles of 256-row chunks
of 64-row waves; 16-byte mask loads with a byte path), the scan's negative /
wrap flags and total (1,024-value trips of one workgroup up to 8,192 values,
then 4,096-value tiles with 64-tile look-back rounds), the batched dictionary
launch (2,048 rows a workgroup, dictionaries up to 4,096 entries), the two
device forms of the row-group prefix / segment table, and the UNION tag
kernels (a grid stride of 256 x 8,192 rows). Every output is padded by 64
sentinel elements on both sides, which must stay untouched; every comparison
is exact."""
import ctypes

import numpy as np
import pytest

import column_model as cm
import orc_amd
from orc_amd import _lib

pytestmark = pytest.mark.gpu

PAD = 64
vp, u64 = ctypes.c_void_p, ctypes.c_uint64


@pytest.fixture(scope="module")
def ctx():
    c = orc_amd.Context(0)
    yield c
    c.close()


class DebugDictJob(ctypes.Structure):
    """orcg_debug_dict_job (orc_amd/csrc/debug_api.cpp)."""

    _fields_ = [("lengths", vp), ("dict_size", u64), ("offsets", vp), ("summary", vp), ("idx", vp), ("nn", vp),
                ("n", u64), ("start", vp), ("len", vp), ("err", vp)]


def _hooks():
    L = _lib.load()
    L.orcg_debug_exclusive_scan_flags.argtypes = [vp, vp, u64, vp, vp, vp]
    L.orcg_debug_dict_multi.argtypes = [vp, ctypes.POINTER(DebugDictJob), ctypes.c_uint32]
    L.orcg_debug_rg_segments.argtypes = [vp, vp, u64, vp, u64, vp, ctypes.c_int, ctypes.c_int, vp, vp]
    L.orcg_debug_union.argtypes = [vp, vp, u64, ctypes.c_uint32, vp, vp, vp]
    return L


class Padded:
    """A device tensor of `n` elements (rows of `cols` for 2-D) between two
    runs of PAD sentinel elements."""

    def __init__(self, n, dtype, sentinel, cols=None, before=None):
        import torch

        shape = (n + 2 * PAD,) if cols is None else (n + 2 * PAD, cols)
        self.host = np.full(shape, sentinel, dtype=dtype)
        if before is not None:
            self.host[PAD:PAD + n] = before
        self.n = n
        self.t = torch.from_numpy(self.host.copy()).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + PAD * self.host[0:1].nbytes

    def get(self):
        """The n elements, after asserting that the padding is untouched."""
        got = self.t.cpu().numpy()
        np.testing.assert_array_equal(got[:PAD], self.host[:PAD])
        np.testing.assert_array_equal(got[PAD + self.n:], self.host[PAD + self.n:])
        return got[PAD:PAD + self.n]


def _dev(a):
    """A host array on the device, never a null pointer (one spare element)."""
    import torch

    a = np.ascontiguousarray(a)
    spare = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
    return torch.from_numpy(np.concatenate([a, spare])).cuda()


# ---- null scatter -------------------------------------------------------------
SCATTER_N = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]
SCATTER_PATTERNS = ["random", "all", "none", "alternating", "null64", "null256", "null4096", "set64", "set256",
                    "set4096", "random_bytes"]
MASK_OFFSETS = [0, 1, 8, 15]
NP_OF_WIDTH = {8: np.int64, 4: np.int32, 2: np.int16, 1: np.int8}


def _mask(pattern, n, rng):
    if pattern == "random":
        return (rng.random(n) < 0.5).astype(np.uint8)
    if pattern == "all":
        return np.ones(n, dtype=np.uint8)
    if pattern == "none":
        return np.zeros(n, dtype=np.uint8)
    if pattern == "alternating":
        return (np.arange(n) % 2).astype(np.uint8)
    if pattern == "random_bytes":  # a set row is any non-zero byte
        return ((rng.random(n) < 0.5) * rng.integers(1, 256, size=n)).astype(np.uint8)
    k = int(pattern[4:] if pattern.startswith("null") else pattern[3:])
    m = (np.arange(n) >= k) if pattern.startswith("null") else (np.arange(n) < k)
    return m.astype(np.uint8)


@pytest.mark.parametrize("width", [16, 8, 4, 2, 1])
def test_scatter_tile_wave_and_alignment_edges(ctx, width):
    """Every (width, n) pair with every mask pattern; the mask pointer's
    offset (0, 1, 8, 15 bytes past a 16-byte boundary: load16's aligned and
    byte paths, which tile_count_kernel and scatter_kernel both take) and the
    fill (none / -9) rotate so that each value of each axis meets each n."""
    import torch

    rng = np.random.default_rng(width)
    step = 0
    for n in SCATTER_N:
        for pattern in SCATTER_PATTERNS:
            off = MASK_OFFSETS[step % 4]
            fill = None if (step // 4) % 2 == 0 else -9
            step += 1
            nn = _mask(pattern, n, rng)
            k = int((nn != 0).sum())
            if width == 16:
                dense = rng.integers(-(1 << 62), 1 << 62, size=(k, 2), dtype=np.int64)
                out = Padded(n, np.int64, 0x5555, cols=2)
                d_dense = _dev(dense).view(torch.complex128)
                d_out = out.t.view(torch.complex128)[PAD:PAD + n]
            else:
                dt = NP_OF_WIDTH[width]
                dense = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, size=k, dtype=dt, endpoint=True)
                out = Padded(n, dt, 0x55)
                d_dense = _dev(dense)
                d_out = out.t[PAD:PAD + n]
            assert d_out.element_size() == width
            d_nn = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
            assert d_nn.data_ptr() % 16 == 0
            d_nn[off:off + n] = torch.from_numpy(nn).cuda()
            orc_amd.scatter_not_null_device(ctx, d_dense, d_nn[off:off + n], d_out, fill=fill)
            ctx.synchronize()
            want = cm.scatter(dense, nn, out.host[PAD:PAD + n], fill=fill)
            np.testing.assert_array_equal(out.get(), want, err_msg="n=%d %s offset=%d fill=%r" % (n, pattern, off, fill))
    assert step >= 4 * len(SCATTER_N)


# ---- scan flags / total -------------------------------------------------------
BIG = (1 << 63) - 1  # three of them wrap the unsigned total, none is negative


def _scan_flags(ctx, x, preset=(0, 0)):
    L = _hooks()
    n = x.size
    d_in = _dev(x)
    out = Padded(n + 1, np.int64, -7)
    flags = Padded(2, np.uint64, 0xAA, before=np.array(preset, dtype=np.uint64))
    total = Padded(1, np.uint64, 0xBB)
    ctx.after_torch()
    orc_amd.rle.check(L.orcg_debug_exclusive_scan_flags(ctx.handle, d_in.data_ptr(), n, out.ptr, flags.ptr, total.ptr),
                      ctx.last_error)
    ctx.synchronize()
    return out.get(), flags.get(), int(total.get()[0])


@pytest.mark.parametrize("n,unit", [(1, 1024), (1024, 1024), (1025, 1024), (8192, 1024), (8193, 4096),
                                    (4096 * 65, 4096), (4096 * 66 + 1, 4096), (4096 * 130 + 5, 4096)])
def test_scan_flags_and_total(ctx, n, unit):
    """StringDirect's computeSize checks fused into the scan: clean input, one
    negative value, one wrap of the unsigned running total (three values of
    2^63 - 1), each in the first, a middle and the last trip (`unit` 1,024,
    one workgroup) or tile (4,096, the look-back kernel over one, just over
    one and two 64-tile rounds, with 2^46 + 3 in tile 0 to carry through the
    rounds). The flags are OR-ed in: pre-set to [1, 1] they stay set."""
    rng = np.random.default_rng(n)
    base = rng.integers(0, 1 << 20, size=n, dtype=np.int64)
    if n > 4096 * 64:
        base[17] = (1 << 46) + 3
    last = (n - 1) // unit
    units = sorted({0, last // 2, last})
    cases = [("clean", None, None)]
    for u in units:
        lo, hi = u * unit, min(n, (u + 1) * unit)
        cases.append(("neg", int(rng.integers(lo, hi)), None))
        if hi - lo >= 3:
            cases.append(("wrap", None, int(rng.integers(lo + 2, hi))))
    for kind, neg_at, wrap_at in cases:
        x = base.copy()
        if neg_at is not None:
            x[neg_at] = -(1 << 33) - 7
        if wrap_at is not None:
            x[wrap_at - 2:wrap_at + 1] = BIG
        off, neg, wrap, tot = cm.scan(x)
        assert (neg, wrap) == {"clean": (0, 0), "wrap": (0, 1)}.get(kind, (1, wrap))
        got_off, got_flags, got_total = _scan_flags(ctx, x)
        msg = "%s neg_at=%r wrap_at=%r" % (kind, neg_at, wrap_at)
        np.testing.assert_array_equal(got_off, off, err_msg=msg)
        assert [int(f) for f in got_flags] == [neg, wrap], msg
        assert got_total == tot, msg
    got_off, got_flags, got_total = _scan_flags(ctx, base, preset=(1, 1))
    np.testing.assert_array_equal(got_off, cm.scan(base)[0])
    assert [int(f) for f in got_flags] == [1, 1]
    assert got_total == cm.scan(base)[3]


# ---- batched dictionary launch -------------------------------------------------
class DictCase:
    """One job's device buffers and its expectation."""

    def __init__(self, rng, D, n, masked, neg=False, idx_edit=None, all_null=False, own_err=True):
        self.D, self.n = D, n
        self.lengths = rng.integers(0, 40, size=D, dtype=np.int64)
        if neg:
            self.lengths[D // 2] = -(1 << 35) - 1
        self.nn = None
        if masked:
            self.nn = np.zeros(n, dtype=np.uint8) if all_null else \
                ((rng.random(n) < 0.7) * rng.integers(1, 256, size=n)).astype(np.uint8)
        self.idx = rng.integers(0, max(D, 1), size=n, dtype=np.int64)
        if masked:  # what a null row holds is never read as an index
            self.idx[self.nn == 0] = D + 5
        if idx_edit:
            idx_edit(self)
        self.d_lengths, self.d_idx = _dev(self.lengths), _dev(self.idx)
        self.d_nn = None if self.nn is None else _dev(self.nn)
        self.offsets = Padded(D + 1, np.int64, -3)
        self.summary = Padded(2, np.uint64, 0xCC)
        self.start = Padded(n, np.int64, -11)
        self.len = Padded(n, np.int64, -13)
        self.err = Padded(1, np.uint64, 0xDD, before=np.array([cm.M64], dtype=np.uint64)) if own_err else None

    def job(self):
        return DebugDictJob(self.d_lengths.data_ptr() if self.D else None, self.D, self.offsets.ptr, self.summary.ptr,
                            self.d_idx.data_ptr() if self.n else None,
                            None if self.d_nn is None else self.d_nn.data_ptr(), self.n,
                            self.start.ptr if self.n else None, self.len.ptr if self.n else None,
                            None if self.err is None else self.err.ptr)

    def check(self):
        off, summary, start, ln, err = cm.dict_job(self.lengths, self.idx, self.nn, self.n,
                                                   start_before=self.start.host[PAD:PAD + self.n],
                                                   len_before=self.len.host[PAD:PAD + self.n])
        msg = "D=%d n=%d masked=%s" % (self.D, self.n, self.nn is not None)
        np.testing.assert_array_equal(self.offsets.get(), off, err_msg=msg)
        np.testing.assert_array_equal(self.summary.get(), summary, err_msg=msg)
        np.testing.assert_array_equal(self.start.get(), start, err_msg=msg)
        np.testing.assert_array_equal(self.len.get(), ln, err_msg=msg)
        if self.err is not None:
            assert int(self.err.get()[0]) == (cm.M64 if err is None else (err << 8) | 7), msg  # 7: kErrDictIndex
        return err

    def check_per_column(self, ctx):
        """The per-column path on the same inputs: dict_offsets_device, then
        dict_gather_device with int64 and with int32 indices (offsets, and the
        rows that are not null)."""
        import torch

        off = Padded(self.D + 1, np.int64, -3)
        orc_amd.dict_offsets_device(ctx, self.d_lengths[:self.D], off.t[PAD:PAD + self.D + 1])
        ctx.synchronize()
        np.testing.assert_array_equal(off.get(), self.offsets.get())
        if self.n == 0:
            return
        rows = np.ones(self.n, dtype=bool) if self.nn is None else self.nn != 0
        for d_idx in (self.d_idx[:self.n], self.d_idx[:self.n].to(torch.int32)):
            start, ln = Padded(self.n, np.int64, -11), Padded(self.n, np.int64, -13)
            orc_amd.dict_gather_device(ctx, d_idx, off.t[PAD:PAD + self.D + 1], start.t[PAD:PAD + self.n],
                                       ln.t[PAD:PAD + self.n],
                                       not_null=None if self.d_nn is None else self.d_nn[:self.n])
            ctx.synchronize()
            np.testing.assert_array_equal(start.get()[rows], self.start.get()[rows])
            np.testing.assert_array_equal(ln.get()[rows], self.len.get()[rows])


def _dict_launch(ctx, cases):
    L = _hooks()
    jobs = (DebugDictJob * len(cases))(*[c.job() for c in cases])
    ctx.after_torch()
    orc_amd.rle.check(L.orcg_debug_dict_multi(ctx.handle, jobs, len(cases)), ctx.last_error)
    ctx.synchronize()


def test_dict_multi_jobs_of_many_shapes(ctx):
    """One launch of jobs with every D of {0, 1, 15, 16, 17, 4095, 4096} and
    every n of {0, 1, 2047, 2048, 2049, 6145}, with and without a mask (a set
    row is any non-zero byte; D = 0 only with every row null), one with a
    negative entry length: offsets, {blob bytes, negative length} summary,
    (start, length) with (0, 0) on null rows, no error record."""
    rng = np.random.default_rng(5)
    shapes = [(0, 0, False), (0, 2049, True), (1, 1, False), (1, 2048, True), (15, 2047, True), (15, 0, False),
              (16, 2048, False), (16, 1, True), (17, 2049, True), (17, 6145, False), (4095, 6145, False),
              (4095, 2047, True), (4096, 6145, True), (4096, 0, False), (4096, 2049, False)]
    cases = [DictCase(rng, D, n, masked, all_null=(D == 0)) for D, n, masked in shapes]
    cases.append(DictCase(rng, 16, 2049, False, neg=True))
    cases.append(DictCase(rng, 4096, 2048, True, neg=True))
    _dict_launch(ctx, cases)
    for c in cases:
        assert c.check() is None
        c.check_per_column(ctx)
    assert [int(c.summary.get()[1]) for c in cases[-2:]] == [1, 1]


def _set(rows, value, null_rows=()):
    def edit(c):
        for r in rows:
            c.idx[r] = value
            if c.nn is not None:
                c.nn[r] = 1
        for r in null_rows:
            c.nn[r] = 0
    return edit


@pytest.mark.parametrize("D", [16, 4096])
def test_dict_multi_reports_the_lowest_bad_row(ctx, D):
    """An index == D at row 2047 (the last of the first workgroup's tile) and
    at row 2048: the lower row is reported, and a row in error is left as it
    was; at row 2048 alone; a negative index; and an index out of range on a
    null row, which is no error."""
    rng = np.random.default_rng(D)
    c = DictCase(rng, D, 6145, False, idx_edit=_set([2047, 2048, 6000], D))
    _dict_launch(ctx, [c])
    assert c.check() == 2047
    c = DictCase(rng, D, 6145, True, idx_edit=_set([2048, 4100], D))
    _dict_launch(ctx, [c])
    assert c.check() == 2048
    c = DictCase(rng, D, 6145, False, idx_edit=_set([5], -1))
    _dict_launch(ctx, [c])
    assert c.check() == 5
    c = DictCase(rng, D, 6145, True, idx_edit=_set([2047], D, null_rows=[2047]))
    _dict_launch(ctx, [c])
    assert c.check() is None
    # through the context's own error record: the reference's text and the row
    c = DictCase(rng, D, 6145, False, idx_edit=_set([2047, 2048], D), own_err=False)
    with pytest.raises(orc_amd.ParseError, match="Entry index out of range in StringDictionaryColumn"):
        _dict_launch(ctx, [c])
    assert ctx.last_error_value() == 2047


def test_dict_multi_refuses_4097_entries(ctx):
    """kDictLds + 1 entries go to the per-column path: the batch refuses them
    before any launch."""
    c = DictCase(np.random.default_rng(1), 4097, 10, False)
    with pytest.raises(orc_amd.InvalidArgument, match="dictionary too large for a batch"):
        _dict_launch(ctx, [c])
    np.testing.assert_array_equal(c.offsets.get(), c.offsets.host[PAD:PAD + 4098])


# ---- row-group prefix and segment table ---------------------------------------
def _rg_layout(kind, G, rng):
    """(rows[G], n) of G row groups."""
    if kind == "small":
        sizes = rng.integers(1, 41, size=G)
    elif kind == "16":
        sizes = np.full(G, 16)
    elif kind == "4096":
        sizes = np.full(G, 4096)
    else:  # empty groups among them, and row groups that start past n
        sizes = rng.integers(0, 41, size=G) * (rng.random(G) < 0.6)
    rows = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    n = int(np.sum(sizes))
    if kind == "mixed" and G > 2:
        n = int(rows[(4 * G) // 5]) + 3
        if rows[-1] <= n:
            rows[-1] = n + 9
    return rows, n


@pytest.mark.parametrize("G", [1, 2, 64, 65, 66, 130, 300])
def test_rg_segments_fused_and_unfused_match_the_model(ctx, G):
    """rg_prefix_segtab_kernel (look-back over the row groups: G = 65 is one
    full 64-predecessor round, 66 one more, 130 and 300 several) and
    rg_count_kernel + scan + rg_segtab_kernel both equal the model, so each
    other: row groups of 1..40 rows, of exactly 16 and 4,096, and mixed with
    empty groups and starts past n; random, all-set and all-clear masks at
    pointer offsets 0 and 5 (the 16-byte middle and the byte head / tail);
    plain and boolean value indices whose skips and bits go below zero before
    the clamp (negative skips tell truncation from flooring). The fused form
    runs twice: its ticket counter resets itself."""
    import torch

    L = _hooks()
    rng = np.random.default_rng(G)
    step = 0
    for kind in ("small", "16", "4096", "mixed"):
        rows, n = _rg_layout(kind, G, rng)
        d_rows = _dev(rows)
        for mask_kind in ("random", "all", "none"):
            for boolean in (0, 1):
                off = (0, 5)[step % 2]
                step += 1
                mask = {"random": ((rng.random(n) < 0.5) * rng.integers(1, 256, size=n)).astype(np.uint8),
                        "all": np.ones(n, dtype=np.uint8), "none": np.zeros(n, dtype=np.uint8)}[mask_kind]
                trip = np.stack([rng.integers(0, 1 << 40, size=G), rng.integers(-3, 30, size=G),
                                 rng.integers(0, 8 if boolean else 1, size=G)], axis=1).astype(np.int64)
                if boolean:
                    trip[::7, 2] = 7  # bits above a small prefix
                d_mask = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
                d_mask[off:off + n] = torch.from_numpy(mask).cuda()
                d_trip = _dev(trip.reshape(-1))
                prefix, seg = cm.rg_segments(mask, n, rows, trip, boolean)
                for fused in (1, 0, 1):
                    got_prefix, got_seg = Padded(G + 1, np.int64, -5), Padded(G, np.uint64, 0xEE, cols=2)
                    ctx.after_torch()
                    orc_amd.rle.check(L.orcg_debug_rg_segments(ctx.handle, d_mask.data_ptr() + off, n,
                                                               d_rows.data_ptr(), G, d_trip.data_ptr(), boolean, fused,
                                                               got_prefix.ptr, got_seg.ptr), ctx.last_error)
                    ctx.synchronize()
                    msg = "%s %s boolean=%d fused=%d offset=%d" % (kind, mask_kind, boolean, fused, off)
                    np.testing.assert_array_equal(got_prefix.get(), prefix, err_msg=msg)
                    np.testing.assert_array_equal(got_seg.get(), seg, err_msg=msg)


# ---- UNION tags ----------------------------------------------------------------
STRIDE = 256 * 8192  # union_check_kernel's grid stride


def _union(ctx, tags, nchildren):
    L = _hooks()
    n = tags.size
    d_tags = _dev(tags)
    offsets = Padded(n, np.int64, -17)
    counts = Padded(nchildren, np.int64, -19)
    bad = Padded(1, np.uint64, 0xFF)
    ctx.after_torch()
    orc_amd.rle.check(L.orcg_debug_union(ctx.handle, d_tags.data_ptr() if n else None, n, nchildren,
                                         offsets.ptr if n else None, counts.ptr, bad.ptr), ctx.last_error)
    ctx.synchronize()
    want_off, want_counts, first_bad = cm.union(tags, nchildren, offsets_before=offsets.host[PAD:PAD + n])
    np.testing.assert_array_equal(offsets.get(), want_off)
    np.testing.assert_array_equal(counts.get(), want_counts)
    assert int(bad.get()[0]) == (cm.M64 if first_bad is None else first_bad)
    return first_bad


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, STRIDE + 3])
def test_union_offsets_counts_and_lowest_bad_tag(ctx, n):
    """Tags in long runs and random, 1, 2, 3 and (n <= 257) 256 children:
    per-row offsets, the rows each child reads, no bad tag. Then two bad
    tags: the lowest index is reported with its tag, also when the higher
    index is the second grid-stride position of a lower thread."""
    rng = np.random.default_rng(n)
    for nch in (1, 2, 3, 256):
        if nch == 256 and n > 257:
            continue
        random_tags = rng.integers(0, nch, size=n).astype(np.uint8)
        runs = np.repeat(rng.integers(0, nch, size=n // 37 + 1), 37)[:n].astype(np.uint8)
        for tags in (random_tags, runs):
            assert _union(ctx, tags, nch) is None
            if nch == 256 or n < 2:
                continue
            lo, hi = (700, STRIDE + 1) if n > STRIDE else (n // 3, n - 1)
            bad = tags.copy()
            bad[lo], bad[hi] = nch + 1, 255
            assert _union(ctx, bad, nch) == (lo << 8) | (nch + 1)
            bad[lo] = 0
            assert _union(ctx, bad, nch) == (hi << 8) | 255
