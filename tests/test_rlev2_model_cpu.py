"""CPU checks of tests/rlev2_model.py, before any GPU is involved: the exact
model and the oracle (oracle/orc_oracle.c, RleDecoderV2.cc restated) agree bit
for bit, in values and in error text, on the known-answer vectors, on streams
of the library's own encoder, on every shape of tests/test_gpu_rlev2_shapes.py
and on every prefix of the grammar streams; every shape holds the run it
claims at the window byte it names; the model's copy of the kernels'
constants is the sources'; and the host planner (orc_amd.Plan: host_parse_run
and the cut loop) agrees with the model on every grammar shape and every cut.

The model departs from the oracle in one place, on purpose: a DELTA header
longer than HDR_LIM bytes (test_long_delta_headers). No GPU."""
import os
import re

import numpy as np
import pytest

import orc_amd
import rlev2_model as m
from conftest import ROOT, load_golden
from oracle import oracle

KATS = load_golden("kat_rlev2.json")
OFFS = (0, 1, 15)


def oracle_decode(data, signed):
    """(values, n, error text): what the oracle hands out before it throws."""
    n = 0
    dec = oracle.RleDecoderV2(data, signed)
    out = []
    while True:
        try:
            out.append(dec.next(1)[0])
            n += 1
        except oracle.OracleError as e:
            return np.array(out, dtype=np.int64), n, str(e)


def agree(data, signed, hdr_lim=m.HDR_LIM):
    """Model == oracle: every value, then the same error at the same value.
    (One decoder per count: a failed next() leaves the oracle's run state
    behind.)"""
    vals, n, err, at = m.decode(data, signed, hdr_lim=hdr_lim)
    assert at == n
    np.testing.assert_array_equal(oracle.RleDecoderV2(data, signed).next(n), vals)
    with pytest.raises(oracle.OracleError) as e:
        oracle.RleDecoderV2(data, signed).next(n + 1)
    assert str(e.value) == err, (err, str(e.value))
    return vals, n, err


def agree_shape(s):
    vals, n, err = agree(s.data, s.signed)
    assert err == m.READ_ERROR  # whole runs to the stream's end
    table = dict(m.run_table(s.data))
    assert all(table[off] == vi for off, vi in s.segs) and m.table_error(s.data, s.segs) is None
    return vals


# ---- the decoder -----------------------------------------------------------------
@pytest.mark.parametrize("fx", KATS, ids=[f["name"] for f in KATS])
def test_model_on_known_answers(fx):
    data = bytes.fromhex(fx["data"])
    vals, n, _, _ = m.decode(data, fx["signed"])
    if fx.get("not_null") is not None:  # None: a null row, which takes no value
        exp = [e for e in fx["expected"] if e is not None]
    else:  # None: a value the vector does not state
        exp = [int(v) if e is None else e for e, v in zip(fx["expected"], vals)]
    assert n >= len(exp) == len(fx["expected"]) - (fx["expected"].count(None) if fx.get("not_null") else 0)
    assert [int(v) for v in vals[:len(exp)]] == exp
    agree(data, fx["signed"])
    if "seek" in fx:
        off, skip = fx["seek"]["position"]
        got = m.decode(data[off:], fx["signed"])[0]
        assert [int(v) for v in got[skip:skip + len(fx["seek"]["expected"])]] == fx["seek"]["expected"]


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_model_on_the_encoders_streams(signed):
    """A few hundred streams of orcg_rlev2_encode_runs (every kind, the
    encoder's choice of widths) and of orcg_rlev2_encode_direct."""
    rng = np.random.default_rng(int(signed))
    kinds = ("short_repeat", "direct", "patched_base", "delta")
    compared = 0
    for it in range(150):
        ks, ls, vs = [], [], []
        for _ in range(int(rng.integers(1, 12))):
            k = kinds[int(rng.integers(0, 4))]
            bits = int(rng.integers(1, 62))
            lo = -(1 << bits) if signed else 0
            if k == "short_repeat":
                L = int(rng.integers(3, 11))
                v = np.full(L, rng.integers(lo, 1 << bits), dtype=np.int64)
            elif k == "patched_base":
                L = int(rng.integers(20, 513))
                v = rng.integers(lo >> 8, 1 << max(bits - 8, 1), size=L, dtype=np.int64)
                v[rng.integers(0, L, size=max(L // 30, 1))] = (1 << bits) - 1
            elif k == "delta":
                L = int(rng.integers(3, 513))
                step = rng.integers(0, 1 << max(bits - 10, 1), size=L, dtype=np.int64)
                v = int(rng.integers(lo, 1 << bits)) + np.cumsum(step) * (1 if it % 2 or not signed else -1)
            else:
                L = int(rng.integers(1, 513))
                v = rng.integers(lo, 1 << bits, size=L, dtype=np.int64)
            ks.append(k)
            ls.append(L)
            vs.append(v.astype(np.int64))
        want = np.concatenate(vs)
        try:
            data, offs = orc_amd.rle.encode_runs(want, signed, ks, ls)
        except orc_amd.OrcError:
            continue  # the encoder refuses what its narrow grammar cannot say
        got, n, _ = agree(bytes(data), signed)
        np.testing.assert_array_equal(got, want)
        assert [r.off for r in m.runs(bytes(data))] == offs.tolist()
        compared += 1
    assert compared >= 120  # the encoder refuses about one stream in ten
    for it in range(60):
        L = int(rng.integers(1, 3000))
        bits = int(rng.integers(1, 63))
        want = rng.integers(-(1 << bits) if signed else 0, 1 << bits, size=L, dtype=np.int64)
        data, _ = orc_amd.rle.encode_direct(want, signed, aligned=bool(it % 2))
        got, n, _ = agree(bytes(data), signed)
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("family", sorted(m.FAMILIES))
def test_grammar_shapes(family, signed):
    s = m.grammar(family, signed)
    agree_shape(s)
    rs = m.runs(s.data, signed)
    assert len(rs) == 3 * len(s.segs)  # a SHORT_REPEAT, the run under test, a SHORT_REPEAT
    kind = {"sr": m.SR, "direct": m.DIRECT, "patched": m.PATCHED, "delta": m.DELTA}[family]
    assert all(r.kind == kind for r in rs[1::3]) and all(r.kind == m.SR for r in rs[0::3] + rs[2::3])
    assert [r.off for r in rs[0::3]] == s.marks["starts"] and max(b - a for a, b in zip(s.marks["starts"], s.marks["starts"][1:])) < 4500
    under = rs[1::3]
    if family == "direct":
        assert {(r.W, r.L) for r in under} == {(w, L) for w in m.FBS for L in m.DIRECT_L}
    if family == "delta":
        assert {(r.W, r.L) for r in under} >= {(w, L) for w in m.FBS[1:] for L in m.DELTA_L} | {(0, L) for L in (1, 2, 3, 512)}
        hdrs = {r.hdr for r in under}
        assert hdrs >= set(range(4, 23)) | {26, 64} and max(hdrs) == m.HDR_LIM
    if family == "patched":
        assert {r.W for r in under} == set(m.FBS) and {r.L for r in under} >= set(m.PATCHED_L)
        seen = {(m.FBS[s.data[r.off + 2] & 31], (s.data[r.off + 3] >> 5) + 1) for r in under}
        assert seen == {(pw, pgw) for pw in m.FBS for pgw in range(1, 9) if pw + pgw <= 64}
        assert {s.data[r.off + 3] & 31 for r in under} >= {1, 31} and {(s.data[r.off + 2] >> 5) + 1 for r in under} == set(range(1, 9))
    if family == "sr":
        assert {(r.W // 8, r.L) for r in under} == {(nb, L) for nb in range(1, 9) for L in range(3, 11)}


def test_the_issues_patched_walks():
    """The three corrupt patch lists that the reference decodes: each patches
    value 2 and stalls; and the two base bytes."""
    rng = np.random.default_rng(0)
    cases = dict(m.patched_cases(rng, True))
    for name in ("later gap 0", "position >= L", "trailing escape"):
        assert m.decode(cases["patched " + name], True)[0].tolist() == [6, 7, 264, 9, 10, 11]
    assert m.decode(cases["patched base 0x80"], True)[0].tolist() == [1, 2, 259, 4, 5, 6]
    assert m.decode(cases["patched base 0x85"], False)[0].tolist() == [-4, -3, 254, -1, 0, 1]
    d = dict(m.delta_cases(rng, False))
    assert m.decode(m.delta(0, 3, m.M64, m.zigzag(-1), 10, 1), False)[0].tolist() == [-1, -2, -3]
    assert m.decode(d["delta W=4 L=2"], False)[0].tolist() == [77, 72] and len(d["delta W=4 L=2"]) == 4
    assert len(m.delta(0, 512, 5, 6)) == 4


def test_long_delta_headers():
    """The one place where the model departs from the oracle: padded varints
    that carry a DELTA header past HDR_LIM bytes. The oracle decodes them; the
    model (the library's rule, include/orcg.h) reports a bad read at the run's
    first value. Without the limit the model is the oracle again."""
    for n in (9, 10, 11, 12, 30):
        assert m.decode(m.delta(0, 5, m.zigzag(3), m.zigzag(2), n, n), True)[0].tolist() == [3, 5, 7, 9, 11]
    seen = set()
    for name, data, signed in m.error_cases():
        if not name.startswith("delta header"):
            continue
        hdr = int(name.split()[3])
        vals, n, err, _ = m.decode(data, signed)
        free = agree(data, signed, hdr_lim=None)
        seen.add(hdr)
        if hdr <= m.HDR_LIM:
            agree(data, signed)
            assert n == free[1] == 3 + 4 + 5 + 3
        else:
            assert n == 3 + 4 and err == m.READ_ERROR and free[1] == 3 + 4 + 5 + 3
            np.testing.assert_array_equal(vals, free[0][:n])
    assert {64, 65, 66, 70} <= seen


@pytest.mark.parametrize("name,data,signed", m.error_cases(), ids=[c[0] for c in m.error_cases()])
def test_error_precedence(name, data, signed):
    if name.startswith("delta header") and int(name.split()[3]) > m.HDR_LIM:
        return  # test_long_delta_headers
    vals, n, err = agree(data, signed)
    want = m.PL0_ERROR if name in ("pl == 0", "pl == 0, cut in the base", "pw = 64 and pl == 0") else \
        m.WIDTH_ERROR if name in ("pw = 64", "pw = 64, cut in the list") else \
        m.DELTA_ERROR if name == "delta L = 1" else m.READ_ERROR
    assert err == want and n == (8 if name == "delta L = 1, fixed" else 7 + 5 + 3 if name.startswith("delta header") else 7)


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_every_prefix_of_the_grammar_streams(signed):
    """Cut at every byte: the values and the error text are the oracle's. Each
    case is cut on its own (a few KB at most); the long DIRECT cases are
    thinned to those of up to 70 bytes, every width among them."""
    errs = set()
    for family in sorted(m.FAMILIES):
        rng = np.random.default_rng(2)
        for name, b in m.FAMILIES[family](rng, signed):
            if len(b) > (70 if family == "direct" else 700):
                continue
            whole = m.decode(b, signed)[0]
            for cut in range(len(b) + 1):
                vals, n, err, _ = m.decode(b[:cut], signed)
                got, gn, gerr = oracle_decode(b[:cut], signed)
                assert (n, err) == (gn, gerr), (name, cut)
                np.testing.assert_array_equal(vals, got)
                np.testing.assert_array_equal(vals, whole[:n])
                errs.add(err)
    for name, b, sg in m.error_cases():
        if name.startswith("delta header"):
            continue
        for cut in range(len(b) + 1):
            vals, n, err, _ = m.decode(b[:cut], sg)
            assert (n, err) == oracle_decode(b[:cut], sg)[1:], (name, cut)
            errs.add(err)
    assert errs == {m.READ_ERROR, m.PL0_ERROR, m.WIDTH_ERROR, m.DELTA_ERROR}


def test_every_cut_of_the_cut_stream():
    s = m.cut_stream()
    assert 140 <= len(s.data) <= 170
    rs = m.runs(s.data, True)
    assert {r.kind for r in rs} == {m.SR, m.DIRECT, m.PATCHED, m.DELTA} and max(r.hdr for r in rs) == 13
    whole = agree_shape(s)
    where = set()
    for cut in range(len(s.data) + 1):
        vals, n, err, _ = m.decode(s.data[:cut], True)
        assert (n, err) == oracle_decode(s.data[:cut], True)[1:]
        np.testing.assert_array_equal(vals, whole[:n])
        last = m.runs(s.data[:cut], True)[-1:] or [None]
        if last[0] is not None and last[0].err:
            where.add((last[0].kind, last[0].hdr > 0))
    assert where >= {(k, inside) for k in (m.DIRECT, m.PATCHED, m.DELTA) for inside in (False, True)}  # cut in the header, in the data


@pytest.mark.parametrize("win", m.WINDOWS, ids=["%d-%d" % w for w in m.WINDOWS])
def test_cuts_of_the_long_stream(win):
    s = m.trunc_long(*win)
    whole = agree_shape(s)
    w = m.serial_windows(s.data, 0, len(s.data), 0, *win)
    assert len(w) >= 4 and len(s.marks["cuts"]) >= 25 and [x.need for x in w[:3]] == [win[0], win[1], win[1]]
    cut_runs = 0
    for cut in s.marks["cuts"]:
        vals, n, err = agree(s.data[:cut], False)
        np.testing.assert_array_equal(vals, whole[:n])
        cut_runs += m.runs(s.data[:cut])[-1].err is not None
    assert cut_runs >= 20


def test_truncate_is_a_cast():
    v = [0, -1, 1 << 31, (1 << 31) - 1, -(1 << 31) - 1, 0x12345_8000, -(1 << 63), (1 << 63) - 1]
    b = m.direct(31, len(v), v)
    for nb, t in ((4, np.int32), (2, np.int16)):
        np.testing.assert_array_equal(m.decode(b, False, nb)[0], np.array(v, dtype=np.int64).astype(t))
        np.testing.assert_array_equal(m.decode(b, False, nb)[0], m.truncate(v, nb))
        np.testing.assert_array_equal(oracle.RleDecoderV2(b, False).next(len(v), dtype=t), m.truncate(v, nb))


# ---- the geometry --------------------------------------------------------------------
def source_constants(name):
    """name -> value of every `constexpr <type> kName = <integer>;` and
    `#define ORCG_NAME <integer>` of a source file."""
    text = open(os.path.join(ROOT, "orc_amd", "csrc", name)).read()
    out = {}
    for stmt in re.findall(r"constexpr\s+\w+\s+(k\w+\s*=[^;]*);", text):  # `k = 1;` or `a = 1, b = 2;`
        for k, v in re.findall(r"(k\w+)\s*=\s*(\d+)u?\s*(?:,|$)", stmt):
            out[k] = int(v)
    for k, v in re.findall(r"^#define\s+(ORCG_\w+)\s+(\d+)\s*$", text, flags=re.M):
        out[k] = int(v)
    return out


def check_constants(table):
    for name, want in table.items():
        have = source_constants(name)
        for k, v in want.items():
            assert have.get(k) == v, "%s: %s is %s in the source, %s in the model" % (name, k, have.get(k), v)


def test_the_models_constants_are_the_sources():
    check_constants(m.CONSTANTS)
    moved = {k: dict(v) for k, v in m.CONSTANTS.items()}
    moved["rlev2_tiled_common.hh"]["kShortL"] += 1
    with pytest.raises(AssertionError, match="kShortL is 16 in the source, 17 in the model"):
        check_constants(moved)  # the check can fail
    csrc = os.path.join(ROOT, "orc_amd", "csrc")
    common, walk, dense, kernel = (open(os.path.join(csrc, "rlev2_tiled_%s.hh" % f)).read()
                                   for f in ("common", "walk", "dense", "kernel"))
    # what the model derives, or holds as a literal, as the source states it
    assert "constexpr uint32_t kBlk = kSlab / kThreads;" in common and "constexpr uint32_t kDenseRuns = kSlab / 2;" in common
    assert "constexpr uint32_t kSup = 8u * kBlk;" in dense
    assert "constexpr uint32_t kChunk = kWin - kMaxRun;" in kernel and "constexpr uint32_t kChunk = kWin - kMaxRun;" in walk
    assert "constexpr uint32_t kCap = kDense ? kDenseRuns : 512u;" in kernel and m.SERIAL_RUNS == 512
    assert "constexpr uint32_t kWin = kWinKB * 1024u + (kDense ? 512u : 0u);" in kernel
    assert "kUnion ? kWin + (uint32_t)(kWaves * kStage * 8 + kSlab / 8) : kWin;" in kernel
    assert m.LONGEST_RUN == 4 + 8 + 512 * 8 + 31 * 8 <= m.MAX_RUN
    # the header limit has one definition (host_plan.hh, pinned above); the kernels name it
    assert "constexpr uint32_t kHdrLim = kRlev2HdrLim;" in common
    assert "avail, kRlev2HdrLim, is_signed)" in open(os.path.join(csrc, "rlev2_expand.hip")).read()
    assert open(os.path.join(csrc, "rlev2_kernels.hip")).read().count("kRlev2HdrLim") >= 3
    assert not re.search(r"parse_run\([^;]*\b64u?,\s*is_signed", "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))))
    # the instances, kInstances' rows: `{id, enqueue<options, window KB, min waves, kDense, kDefer>, drain}`,
    # the ids by their names in rlev2_route.hh
    ids = source_constants("rlev2_route.hh")
    text = open(os.path.join(csrc, "rlev2_tiled.cpp")).read()
    table = text[text.index("constexpr Instance kInstances[] = {"):]
    table = table[:table.index("};")]
    inst = re.findall(r"\{(kRlev2\w+), enqueue<[^,]+, (\d+), \d+, (\d+), \d+>, (?:nullptr|enqueue<[^>]*>)\}", table)
    assert sorted(ids[v] for v, _, _ in inst) == list(range(2, 11))
    # every enqueue<...> the table names is instantiated in exactly one instance unit, and nothing else is
    units = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.startswith("rlev2_tiled_inst_"))
    made = re.findall(r"^template void enqueue<([^>]*)>\(Ctx\*, const TiledLaunch&\);$", units, flags=re.M)
    assert sorted(made) == sorted(set(re.findall(r"enqueue<([^>]*)>", table))) and len(made) >= 2
    assert units.count("enqueue<") == len(made)
    for v, kb, dense in inst:
        v, kb = ids[v], int(kb)
        win, kind, wins = m.VARIANTS[v]
        assert win == kb * 1024 + (512 if dense == "2" else 0), v
        assert (kind in ("dense", "union", "two-pass")) == (dense == "2"), v
        assert (wins is not None) == (kind in ("union", "two-pass")) and (wins is None or wins == win + 4 * 256 * 8 + 256)
    assert sorted(m.VARIANTS) == orc_amd.rlev2_variants() == list(range(m.CONSTANTS["rlev2_route.hh"]["kMaxRlev2Variant"] + 1))
    assert m.WINDOWS == [(8704, 8704), (8704, 17152), (12800, 12800), (21504, 21504), (33792, 33792)]


def test_serial_window_schedule():
    """The schedule on streams small enough to check by hand (win 8704:
    kChunk = 4096)."""
    rng = np.random.default_rng(1)
    one = m.sr(1, 3, 1)
    # runs at 0, 2, 4100 (past kChunk, ends at 8198 <= 8704: taken), 8198 (not whole: the next window)
    data = one + m.filler(rng, 3 * m.BIG) + one
    w = m.serial_windows(data, 0, len(data), 0, 8704)
    assert [x.runs for x in w] == [[0, 2, 4100], [8198, 12296]] and w[0].need == 8704 and w[1].wpos == 8192
    assert w[1].need == 12304 - 8192  # the segment's end, rounded up 16
    w = m.serial_windows(data, 0, len(data), 15, 8704)  # the stream 15 bytes into a 16-byte line
    assert w[0].wpos == -15 and w[0].byte(4100) == 4115 and w[1].wpos == 8198 - (8198 + 15) % 16
    # a run table of 512 runs: the same window goes on with a second pass
    data = b"".join(m.sr(1, 3, 1) for _ in range(600))
    assert [len(x.runs) for x in m.serial_windows(data, 0, len(data), 0, 8704)] == [600]
    # a later window of another size
    data = one + m.filler(rng, 8 * m.BIG)
    w = m.serial_windows(data, 0, len(data), 0, 8704, 17152)
    assert [len(x.runs) for x in w] == [3, 4, 2] and w[1].need == 17152


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("win", m.WINDOWS, ids=["%d-%d" % w for w in m.WINDOWS])
def test_placements(win, off):
    """Every run of the sweeps starts at the window byte it names, in the
    window it names; the sweeps cover kChunk - 80 .. kChunk + 16 and the 16
    bytes on either side of the last start at which the run is fully loaded;
    a run that is not fully loaded opens the next window."""
    s = m.placement(win[0], win[1], off, step=1 if off == 0 else 7)  # as the GPU test builds them
    agree_shape(s)
    k = s.marks["window"]
    kwin = win[1]
    chunk = kwin - m.MAX_RUN
    size = {r.off: r.size for r in m.runs(s.data)}
    want = {"delta22": 22 + 4 * 510, "longest": m.LONGEST_RUN, "direct64": m.BIG, "sr": 2, "straddle": 23}
    seen = {kind: set() for kind in m.PLACED}
    for kind, at, o, seg in s.marks["runs"]:
        start = s.segs[seg][0]
        end = s.segs[seg + 1][0] if seg + 1 < len(s.segs) else len(s.data)
        assert size[o] == want[kind]
        w = m.serial_windows(s.data, start, end, off, *win)
        j, b = m.window_of(w, o)
        if at + size[o] > kwin - 17:
            assert w[k].need == kwin  # the window is loaded whole: the segment goes on past it
        if at + size[o] <= w[k].need:
            assert (j, b) == (k, at), (kind, at, j, b)
        else:  # not fully loaded: the next window starts at it
            assert j == k + 1 and at >= chunk
            if at <= w[k].need:  # (else the run before it is cut by the window too, and opens the next)
                assert w[j].runs[0] == o and b == (off + o) % 16
        seen[kind].add(at)
    if off == 0:
        for kind in m.PLACED:
            assert seen[kind] >= set(range(chunk - 80, chunk + 17)) | set(range(kwin - want[kind] - 16, kwin - want[kind] + 17))


@pytest.mark.parametrize("off", OFFS)
def test_header_slice_shape(off):
    """A DELTA run with a 22-byte header and a PATCHED run each start at every
    offset 180..330 of a segment, behind runs of at most 62 bytes."""
    s = m.header_slice(off)
    agree_shape(s)
    rs = {r.off: r for r in m.runs(s.data)}
    assert max(len(s.data[a:b]) for a, b in zip(s.marks["starts"], s.marks["starts"][1:])) < 1024
    for (kind, at), start in zip(s.marks["at"], s.marks["starts"]):
        a = rs[start + at]
        b = rs[start + at + a.size]
        assert a.kind == kind and {a.kind, b.kind} == {m.DELTA, m.PATCHED}
        assert (a if kind == m.DELTA else b).hdr == 22 and (b if kind == m.DELTA else a).hdr == 6
        assert all(rs[o].size <= 62 for o in rs if start <= o < start + at)
    assert sorted(s.marks["at"]) == sorted((k, at) for k in (m.DELTA, m.PATCHED) for at in range(180, 331))


@pytest.mark.parametrize("win", m.WINDOWS, ids=["%d-%d" % w for w in m.WINDOWS])
def test_placement_cuts(win):
    """The placement runs cut around their window's kChunk and end and around
    their own ends: model == oracle at every cut, and the run under test is
    the one the stream's end cuts in some of them."""
    s = m.placement_cuts(*win)
    whole = agree_shape(s)
    under = {o: kind for kind, at, o, seg in s.marks["runs"]}
    assert sorted(kind for kind in under.values()) == sorted(2 * ["longest", "delta22", "straddle"])
    chunk = win[1] - m.MAX_RUN
    assert {at for _, at, _, _ in s.marks["runs"]} >= {chunk} and len(s.marks["cuts"]) >= 40
    cut_kinds = set()
    for cut in s.marks["cuts"]:
        vals, n, err = agree(s.data[:cut], False)
        np.testing.assert_array_equal(vals, whole[:n])
        last = m.runs(s.data[:cut])[-1]
        if last.err and last.off in under:
            cut_kinds.add(under[last.off])
    assert cut_kinds == {"longest", "delta22", "straddle"}


@pytest.mark.parametrize("off", (0, 15))
def test_item_and_table_shapes(off):
    s = m.items(off)
    agree_shape(s)
    rs = m.runs(s.data, True)
    by_seg = [[r for r in rs if a <= r.off < b] for a, b in zip(s.marks["starts"], s.marks["starts"][1:] + [len(s.data)])]
    short = lambda r: r.L <= m.SHORT_L and r.kind != m.PATCHED
    for n, seg in zip((63, 64, 65, 128, 129), by_seg):
        assert not short(seg[0]) and all(short(r) for r in seg[1:n + 1]) and not short(seg[n + 1])
    assert {r.L for r in by_seg[5][1:-1]} == {16} and {r.L for r in by_seg[6][1:-1]} == {17}
    assert {r.kind for r in by_seg[5][1:-1]} == {m.DIRECT, m.DELTA}
    for seg in by_seg[7:]:
        assert sum(r.kind == m.PATCHED and r.L <= m.SHORT_L for r in seg) == 3
    if off:
        return
    s = m.tables()
    agree_shape(s)
    rs = m.runs(s.data, True)
    ends = s.marks["starts"][1:] + [len(s.data)]
    counts = [sum(a <= r.off < b for r in rs) for a, b in zip(s.marks["starts"], ends)]
    assert counts == list(m.TABLE_RUNS) + [m.DENSE_RUNS, m.DENSE_RUNS + 1]
    chunk = min(w for w, kind, _ in m.VARIANTS.values() if kind == "serial" and w > 30000) - m.MAX_RUN
    assert max(b - a for a, b in zip(s.marks["starts"], ends)) + 16 <= chunk  # inside one 33 KB window
    assert ends[4] - s.marks["starts"][4] == m.SLAB  # a slab of two-byte runs


@pytest.mark.parametrize("off", (0, 1))
def test_dense_phase_shapes(off):
    """Every run size 2..12; the second header byte, a varint and the payload
    cross a block, a super-block and the slab's edge with every count of the
    run's bytes before it (edges counted from the segment's first run, where
    the first dense pass starts)."""
    s = m.dense_phases(off)
    agree_shape(s)
    rs = m.runs(s.data, True)
    assert {r.size for r in rs} == set(range(2, 14)) and max(r.L for r in rs) <= m.SHORT_L
    assert max(b - a for a, b in zip(s.marks["starts"], s.marks["starts"][1:])) < m.SLAB + 64
    cross = {(edge, what): set() for edge in (m.BLK, m.SUPER, m.SLAB) for what in ("second", "varint", "payload")}
    seg = 0
    for r in rs:
        while seg + 1 < len(s.segs) and s.segs[seg + 1][0] <= r.off:
            seg += 1
        lp = r.off - s.segs[seg][0]
        if lp >= m.SLAB:
            continue  # the next pass: its blocks start at its own first run
        for edge in (m.BLK, m.SUPER, m.SLAB):
            for e in range((lp // edge + 1) * edge, lp + r.size, edge):
                before = e - lp  # bytes of the run before the edge
                if before == 1:
                    cross[edge, "second"].add((r.size, 1))
                if r.kind == m.DELTA and before > 2:
                    cross[edge, "varint"].add((r.size, before))
                if r.kind != m.DELTA and before >= r.hdr:
                    cross[edge, "payload"].add((r.size, before))
    for edge in (m.BLK, m.SUPER, m.SLAB):
        assert {p[0] for p in cross[edge, "second"]} >= set(range(2, 13)), edge
        assert cross[edge, "varint"] >= {(sz, k) for sz in range(4, 13) for k in range(3, sz)}, edge
        assert cross[edge, "payload"] >= {(sz, k) for sz in range(3, 13) for k in range(2, sz)} | {(sz, k) for sz in range(2, 10) for k in range(1, sz)}, edge


def test_dense_mix_and_slice_shapes():
    s = m.dense_mixes()
    agree_shape(s)
    rs = m.runs(s.data, True)
    seg = lambda k: [r for r in rs if s.marks["starts"][k] <= r.off < (s.marks["starts"] + [len(s.data)])[k + 1]]
    assert {r.hdr for r in seg(0) if r.kind == m.DELTA} >= {14} and any(r.kind == m.PATCHED for r in seg(0))
    assert {(r.size, r.L) for r in seg(1)} == {(4, 512)} and len(seg(1)) * 4 > 2 * m.SLAB
    assert [max(r.L for r in seg(k)) for k in range(2, 6)] == [16, 17, 256, 257]
    sizes = sorted({r.size for k in range(6, len(s.segs)) for r in seg(k) if r.size > 14})
    t = m.CONSTANTS["rlev2_tiled_common.hh"]
    for edge in (t["kToDense"], t["kToSerial"], t["ORCG_TAB_TO_DENSE"], t["ORCG_TAB_TO_SERIAL"]):
        assert any(a < edge <= b for a, b in zip(sizes, sizes[1:])), edge
    s = m.slices()
    vals = agree_shape(s)
    assert m.two_pass_shape(vals.size, len(s.segs)) == (4, m.SLICE_MAX)  # slices of 1,024 values
    rs = m.runs(s.data, True)
    firsts = []
    for a, b, vi in zip(s.marks["starts"], s.marks["starts"][1:] + [len(s.data)], [v for _, v in s.segs]):
        inside = [r for r in rs if a <= r.off < b]
        starts = np.cumsum([0] + [r.L for r in inside])
        firsts.append((inside, starts))
        assert 0.75 * 2524 < starts[-1] < 1.25 * 2524 and len(s.data[a:b]) / len(inside) < t["kToDense"]
    for k, edge in enumerate((1023, 1024, 1025)):
        assert edge in firsts[k][1]
    for k, kind in ((3, m.DELTA), (4, m.PATCHED)):
        inside, starts = firsts[k]
        over = [(r, v) for r, v in zip(inside, starts) if v < m.SLICE_MAX < v + r.L]
        assert len(over) == 1 and over[0][0].kind == kind and over[0][0].W > 0
        if kind == m.PATCHED:
            assert over[0][1] + 50 < m.SLICE_MAX < over[0][1] + 150  # patches at values 50 and 150 of it
    for k, n in zip(range(5, 9), m.SLICE_RUNS):
        assert firsts[k][1][n] == m.SLICE_MAX  # exactly n runs in the first slice


def test_range_shape():
    s = m.ranges()
    vals = agree_shape(s)
    first = s.marks["first"]
    rs = m.runs(s.data, True)
    assert [r.kind for r in rs] == [m.SR, m.DIRECT, m.PATCHED, m.DELTA, m.DELTA, m.DIRECT, m.SR]
    for a, b in zip(first, first[1:]):
        begins = {x - a for x, c in s.marks["ranges"] if a <= x < b}
        ends = {x + c - 1 - a for x, c in s.marks["ranges"] if a <= x + c - 1 < b}
        want = {x for x in m.RANGE_AT + (b - a - 1,) if x < b - a}
        assert begins >= want and ends >= want
    assert (m.truncate(vals, 4) != vals).mean() > 0.5 and m.positions(s.data, vals.size, 100)[1:, 1].min() > 0


# ---- the host planner ------------------------------------------------------------------
def check_plan(data, label):
    """orc_amd.Plan == the model: values, the error's text and value index,
    and a table of run-aligned segments with the model's value indices."""
    rs = m.runs(data)
    good = [r for r in rs if not r.err]
    n = sum(r.L for r in good)
    p = orc_amd.Plan(data, max_segment_bytes=64, max_segment_values=100)
    assert p.values == n, label
    if len(good) == len(rs):
        assert p.error() is None, label
    else:
        rc, pat, msg = p.error()
        assert (pat, msg) == (n, rs[-1].err), (label, pat, msg)
    table = dict(zip([r.off for r in good], np.cumsum([0] + [r.L for r in good]).tolist()))
    segs = [(int(a), int(b)) for a, b in p.segments()]
    assert all(table.get(off) == vi for off, vi in segs), label
    assert (not segs and not table) or segs[0] == (0, 0), label
    assert len(segs) >= min(len(data) // 700, 1)


@pytest.mark.parametrize("family", sorted(m.FAMILIES))
def test_host_plan_on_the_grammar_shapes(family):
    s = m.grammar(family, False)
    check_plan(s.data, family)
    rng = np.random.default_rng(2)
    for name, b in m.FAMILIES[family](rng, False):
        if len(b) > (70 if family == "direct" else 700):
            check_plan(b, name)
            continue
        for cut in range(len(b) + 1):
            check_plan(b[:cut], "%s cut %d" % (name, cut))


def test_host_plan_on_errors_and_long_headers():
    """The precedence cases at every cut, and the header limit: the plan
    accepts a DELTA header of 64 bytes and reports a longer one as the device
    does."""
    for name, b, _ in m.error_cases():
        for cut in range(len(b) + 1):
            check_plan(b[:cut], "%s cut %d" % (name, cut))
    s = m.cut_stream()
    for cut in range(len(s.data) + 1):
        check_plan(s.data[:cut], "cut %d" % cut)
    ok = orc_amd.Plan(m.delta(0, 5, 6, 4, 31, 31))
    assert ok.values == 5 and ok.error() is None
    bad = orc_amd.Plan(m.sr(1, 3, 1) + m.delta(0, 5, 6, 4, 32, 32))
    assert bad.values == 3 and bad.error()[1:] == (3, m.READ_ERROR)
