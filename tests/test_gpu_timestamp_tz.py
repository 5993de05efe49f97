"""TIMESTAMP columns written in a zone other than UTC.

timestamp_tz_kernel (through orc_amd.timestamp_decode_tz_device) against the
Python restatement of TimestampColumnReader::next (tests/tz_model.py,
c++/src/ColumnReader.cc:318-347), bit-exact, on value patterns in which the
lanes of a wave agree on their zone variants, differ, or alternate; then the file
reader on the reference's example files against the reference's expected
ColumnPrinter output and pyarrow, the reader zone, the local zone, a missing
and a malformed zone. Zone rules come from tests/golden/tz (registered on the
reader), never from the machine's tzdata."""
import base64
import os
import struct

import numpy as np
import pytest

import orc_amd
import tz_model
from conftest import GOLDEN, load_golden
from file_parity import expected_json, path, printer_equal, to_printer_form
from utc_zones import utc_tzdir

pytestmark = pytest.mark.gpu

TZ = os.path.join(GOLDEN, "tz")
FIXTURE_ZONES = ["America/Los_Angeles", "America/New_York", "Asia/Shanghai", "Asia/Kolkata", "Australia/Sydney",
                 "Europe/London", "GMT"]
KAT = load_golden("kat_timezone.json")
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]


def zone_bytes(name):
    if name in KAT["zones"]:  # LA_VER1 (no rule), LA_VER2: the reference's test files
        return base64.b64decode(KAT["zones"][name])
    with open(os.path.join(TZ, name), "rb") as f:
        return f.read()


def hourly_zone(count=2000):
    """A TZif v2 file with `count` hourly transitions between two variants
    (+0:00 standard, +0:30 DST) from 2000-01-01 and no footer rule: its table
    (count * 12 bytes) does not fit the kernel's LDS budget next to another."""
    v1 = b"TZif2" + bytes(15) + struct.pack(">6l", 0, 0, 0, 0, 1, 4) + struct.pack(">lBB", 0, 0, 0) + b"UTC\0"
    times = [946684800 + 3600 * i for i in range(count)]
    v2 = b"TZif2" + bytes(15) + struct.pack(">6l", 0, 0, 0, count, 2, 8)
    v2 += struct.pack(">%dq" % count, *times) + bytes(i & 1 for i in range(count))
    v2 += struct.pack(">lBB", 0, 0, 0) + struct.pack(">lBB", 1800, 1, 4) + b"STD\0DST\0"
    return v1 + v2 + b"\n\n"


_zones = {}


def zones(name):
    """(model, C handle) of a zone, parsed once."""
    if name not in _zones:
        data = hourly_zone() if name == "hourly" else zone_bytes(name)
        _zones[name] = (tz_model.Zone(name, data), orc_amd.Timezone.parse(name, data))
    return _zones[name]


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def encode_nanos(i, small):
    """An encoded SECONDARY value: trailing-zero code i % 8; decoded nanos
    <= 999,999 when `small`, else above."""
    z = i % 8
    if small:
        base = 1 + i % 9 if z >= 5 else 1 + i % 99  # base * 10^(z + 1) <= 999,999 needs z <= 4 ... or z = 0
        if z >= 5:
            z = 0
        return (base << 3) | z
    base = (123 + i) if z else 1_000_000 + i  # z = 0 keeps the value: above 999,999 on its own
    while tz_model.decode_nanos((base << 3) | z) <= 999_999:
        base *= 10
    return (base << 3) | z


def run_kernel(ctx, w, r, times, nanos_enc):
    """times: writer-zone seconds (after the epoch); returns the kernel's and
    the model's (seconds, nanos)."""
    import torch
    wm, wc = w
    rm, rc = r
    raw = np.array([t - wm.epoch for t in times], dtype=np.int64)
    enc = np.array(nanos_enc, dtype=np.int64)
    want = [tz_model.adjust(wm, rm if rc is not wc else wm, int(a), int(b)) for a, b in zip(raw, enc)]
    ds, dn = torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(enc.copy()).cuda()
    orc_amd.timestamp_decode_tz_device(ctx, ds, dn, wc, rc)
    return ds.cpu().numpy(), dn.cpu().numpy(), want


def check(ctx, w, r, times, nanos_enc=None, where=""):
    if nanos_enc is None:
        nanos_enc = [encode_nanos(i, i % 3 == 0) for i in range(len(times))]
    gs, gn, want = run_kernel(ctx, w, r, times, nanos_enc)
    ws = np.array([x[0] for x in want], dtype=np.int64)
    wn = np.array([x[1] for x in want], dtype=np.int64)
    bad = np.nonzero((gs != ws) | (gn != wn))[0]
    assert bad.size == 0, "%s: value %d (t = %d): got (%d, %d), want (%d, %d)" % (
        where, bad[0], times[bad[0]], gs[bad[0]], gn[bad[0]], ws[bad[0]], wn[bad[0]])


PAIRS = [("America/Los_Angeles", "GMT"), ("GMT", "America/Los_Angeles"),
         ("America/Los_Angeles", "America/New_York"), ("America/Los_Angeles", "Australia/Sydney"),
         ("Asia/Kolkata", "Europe/London"), ("America/Los_Angeles", "America/Los_Angeles"),
         ("LA_VER1", "GMT"), ("LA_VER2", "GMT")]


def transitions_of(model, years=(1960, 2037)):
    """Explicit transitions, plus the rule's in the given years."""
    out = list(model.transitions)
    if model.rule.has_dst:
        for y in years:
            out += model.rule.cycle[(y - 1970) * 2 + 1:(y - 1970) * 2 + 3] if y >= 1970 else []
    return out


@pytest.mark.parametrize("wname,rname", PAIRS, ids=["%s->%s" % p for p in PAIRS])
def test_kernel_matches_model(ctx, wname, rname):
    w, r = zones(wname), zones(rname)
    wm, rm = w[0], r[0]
    calm, other = 1_700_000_000, 1_690_000_000  # November / July 2023
    for n in SIZES:
        # (a) one interval
        a = [calm + i for i in range(n)]
        check(ctx, w, r, a, where="a n=%d" % n)
        # (b) one lane elsewhere: lanes 0, 31, 63, and the last lane of the partial wave
        for lane in sorted({0, 31, 63, n - 1}):
            if lane < n:
                b = list(a)
                b[lane] = other
                check(ctx, w, r, b, where="b n=%d lane=%d" % (n, lane))
    # (c) neighbouring lanes on both sides of a transition
    edges = transitions_of(wm) or transitions_of(rm)
    for T in (edges[len(edges) // 2], edges[-1]):
        for n in (64, 257):
            check(ctx, w, r, [T - 1 + (i & 1) for i in range(n)], where="c T=%d n=%d" % (T, n))
    # (d) every transition of both zones at -1 / 0 / +1, and where the adjusted
    # time crosses a reader transition
    d = []
    for T in transitions_of(wm) + transitions_of(rm):
        d += [T - 1, T, T + 1]
    for T in transitions_of(rm):
        for probe in (T - 1, T + 1):
            wv, rv = wm.variant(probe), rm.variant(probe)
            x = T - wv.gmt_offset + rv.gmt_offset
            d += [x - 1, x, x + 1]
    check(ctx, w, r, d, where="d")
    # (e) negative times, nanos on both sides of 999,999, every trailing-zero code
    e = [-1 - 7919 * i for i in range(64)] + [-wm.epoch - 1, -wm.epoch, -wm.epoch + 1, -1, 0, 1] * 4
    for small in (False, True):
        check(ctx, w, r, e, [encode_nanos(i, small) for i in range(len(e))], where="e small=%s" % small)
    codes = {encode_nanos(i, False) & 7 for i in range(len(e))}
    assert codes == set(range(8))
    # (f) before the first transition, 1900, 2038, 2369, 2400 and later
    first = min(transitions_of(wm) + transitions_of(rm) + [0])
    f = [first - 1, first - 86400 * 365, -2208988800, -2208988800 + 15552000, 2145916800, 2145916800 + 15552000,
         12591244800, 12591244800 + 15552000, 13569465600, 13569465600 + 15552000, 13569465600 + 31536000 * 7,
         tz_model.SECONDS_PER_400_YEARS * 3 + 15552000, -tz_model.SECONDS_PER_400_YEARS - 1,
         -tz_model.SECONDS_PER_400_YEARS + 15552000]
    check(ctx, w, r, f * 5, where="f")


def test_same_rules_in_two_handles(ctx):
    """Two parses of one file are different zones to the API (no shortcut to
    the plain kernel) with equal rules: nothing is adjusted."""
    data = zone_bytes("America/Los_Angeles")
    a = (tz_model.Zone("a", data), orc_amd.Timezone.parse("a", data))
    b = (tz_model.Zone("b", data), orc_amd.Timezone.parse("b", data))
    check(ctx, a, b, [1_690_000_000 + 86400 * 30 * i for i in range(300)], where="same rules")


def test_version1_zone_keeps_its_last_variant(ctx):
    """LA_VER1 has no rule: past 2037 every time is PST; LA_VER2 follows the rule."""
    july_2100 = 4118688000
    gmt = zones("GMT")
    for name, off in (("LA_VER1", -28800), ("LA_VER2", -25200)):
        gs, _, want = run_kernel(ctx, zones(name), gmt, [july_2100], [0])
        assert int(gs[0]) == want[0][0] == july_2100 + off


@pytest.mark.parametrize("wname,rname", [("hourly", "America/Los_Angeles"), ("America/Los_Angeles", "hourly"),
                                         ("hourly", "GMT")])
def test_oversized_table_is_searched_in_global_memory(ctx, wname, rname):
    w, r = zones(wname), zones(rname)
    big = w[0] if wname == "hourly" else r[0]
    assert len(big.transitions) == 2000
    t = []
    for T in big.transitions[::7]:
        t += [T - 1, T, T + 1801]
    t += [big.transitions[0] - 5, big.transitions[-1] + 5, 1_700_000_000, -1]
    check(ctx, w, r, t, where="hourly edges")
    for n in (65, 1000):
        check(ctx, w, r, [big.transitions[500] + 3 * i for i in range(n)], where="hourly run n=%d" % n)


# ---- files -----------------------------------------------------------------

def register(r):
    for name in FIXTURE_ZONES:
        r.set_zone_rules(name, zone_bytes(name))


def ts_ids(r):
    return [i for i, t in enumerate(r.types) if t.kind == 9]


def stripe_rows(r):
    rows = []
    for s in range(r.num_stripes):
        b = r.read_stripe(s)
        for tid in ts_ids(r):
            assert tid in b.columns, "stripe %d: TIMESTAMP column %d not decoded" % (s, tid)
        rows.extend(b.to_pylist())
    return rows


def row_reader_rows(r, capacity=1000, **kw):
    rr = r.create_row_reader(**kw)
    b = rr.create_row_batch(capacity)
    rows = []
    while rr.next(b):
        for tid in ts_ids(r):
            assert tid in b.columns
        rows.extend(b.to_pylist())
    return rows


def ts_ns(r, name, tid):
    """Column `tid` over the whole file: (int64 nanoseconds, validity)."""
    vals, valid = [], []
    for s in range(r.num_stripes):
        c = r.read_stripe(s).columns[tid]
        vals.append(c.data * 1_000_000_000 + c.secondary)
        valid.append(np.ones(len(c.data), bool) if c.not_null is None else c.not_null.astype(bool))
    return np.concatenate(vals), np.concatenate(valid)


GOLDEN_FILES = ["TestOrcFile.testTimestamp.orc", "TestOrcFile.testUnionAndTimestamp.orc",
                "TestOrcFile.testDate1900.orc", "TestOrcFile.testDate2038.orc", "orc_split_elim_new.orc"]


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_golden_files_match_expected_output(ctx, monkeypatch, name):
    """US/Pacific and America/Los_Angeles writers read in GMT: every row equals
    the reference's expected ColumnPrinter output, through read_stripe and
    through a RowReader; the time column also equals pyarrow's."""
    monkeypatch.setenv("TZDIR", utc_tzdir())  # the machine's tzdata plays no part
    want = expected_json(name)
    r = orc_amd.Reader(path(name), ctx)
    register(r)
    assert ts_ids(r)
    for how, got in (("read_stripe", stripe_rows(r)), ("row reader", row_reader_rows(r))):
        assert len(got) == len(want) == r.num_rows
        for i, (w, g) in enumerate(zip(want, got)):
            assert printer_equal(w, to_printer_form(g)), "%s %s row %d: %r vs %r" % (name, how, i, w, g)
    root = r.types[0]
    if root.kind != 12:
        return
    import pyarrow as pa
    import pyarrow.orc as po
    monkeypatch.setenv("TZDIR", TZ)  # pyarrow's ORC reader: the same fixture rules
    for field, tid in zip(root.field_names, root.subtypes):
        if r.types[tid].kind != 9:
            continue
        col = po.ORCFile(path(name)).read(columns=[field]).column(field).combine_chunks()
        theirs = col.cast(pa.timestamp("ns")).cast(pa.int64())
        valid_t = np.asarray(col.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
        ours, valid_o = ts_ns(r, name, tid)
        assert np.array_equal(valid_o, valid_t)
        assert np.array_equal(ours[valid_o], theirs.fill_null(0).to_numpy()[valid_t])


@pytest.fixture(scope="module")
def gmt_file(tmp_path_factory):
    """pyarrow-written (writer zone GMT): 3,000 rows, 3 stripes, 20 % nulls,
    around both 2023 US transitions at +-2 h, one-second steps near the edges."""
    import pyarrow as pa
    import pyarrow.orc as po
    os.environ.setdefault("TZDIR", TZ)
    rng = np.random.default_rng(11)
    secs = []
    for edge in (1678615200, 1699174800):  # 2023-03-12 10:00 UTC, 2023-11-05 09:00 UTC
        secs += list(range(edge - 300, edge + 300))                     # one-second steps
        secs += list(range(edge - 7200, edge + 7200, 16))               # +-2 h
    secs += list(range(edge - 7200 + 36000, edge - 7200 + 36000 + 3000 - len(secs)))
    secs = np.array(secs[:3000], dtype=np.int64)
    # the same wall-clock instants also cross the reader zones' edges
    ns = secs * 1_000_000_000 + rng.integers(0, 1_000_000_000, size=3000)
    mask = rng.random(3000) < 0.2
    t = pa.table({"id": pa.array(np.arange(3000)), "ts": pa.array(ns, pa.timestamp("ns"), mask=mask)})
    p = str(tmp_path_factory.mktemp("tz") / "gmt_writer.orc")
    po.write_table(t, p, stripe_size=1, batch_size=1000)
    return p, ns, ~mask


@pytest.mark.parametrize("zone", ["America/Los_Angeles", "Australia/Sydney"])
def test_reader_zone(ctx, gmt_file, zone):
    p, ns, valid = gmt_file
    r = orc_amd.Reader(p, ctx)
    register(r)
    assert r.num_stripes == 3 and r.num_rows == 3000
    tid = ts_ids(r)[0]
    base, base_valid = ts_ns(r, p, tid)
    assert np.array_equal(base_valid, valid) and np.array_equal(base[valid], ns[valid])
    gmt, target = zones("GMT")[0], zones(zone)[0]
    want = np.array([tz_model.convert(gmt, target, int(v // 1_000_000_000)) * 1_000_000_000 + int(v % 1_000_000_000)
                     for v in base], dtype=np.int64)
    assert np.any(want[valid] != base[valid])

    def rr_ns(rr):
        b = rr.create_row_batch(1000)
        out = []
        while rr.next(b):
            c = b.columns[tid]
            out.append(c.data * 1_000_000_000 + c.secondary)
        return np.concatenate(out)

    plain = r.create_row_reader()            # created at GMT: keeps it
    zoned = r.create_row_reader(timezone=zone)
    r.set_timezone(zone)
    got, got_valid = ts_ns(r, p, tid)
    assert np.array_equal(got_valid, valid)
    assert np.array_equal(got[valid], want[valid])
    assert np.array_equal(rr_ns(zoned)[valid], want[valid])
    assert np.array_equal(rr_ns(plain)[valid], base[valid])
    with pytest.raises(orc_amd.InvalidArgument):
        r.set_timezone("Mars/Olympus_Mons")
    with pytest.raises(orc_amd.InvalidArgument):
        r.create_row_reader(timezone="Mars/Olympus_Mons")


def test_local_zone(ctx, monkeypatch):
    """orc_split_elim.orc names no writer zone: undecoded until the caller
    names one; then the model applied to the UTC-assumed read."""
    monkeypatch.setenv("TZDIR", utc_tzdir())
    name = "orc_split_elim.orc"
    r = orc_amd.Reader(path(name), ctx)
    register(r)
    tid = ts_ids(r)[0]
    b = r.read_stripe(0)
    assert tid not in b.columns
    assert all(i in b.columns for i in range(len(r.types)) if i != tid)
    r.set_local_timezone("GMT")
    utc, valid = ts_ns(r, name, tid)
    r.set_local_timezone("America/Los_Angeles")
    got, got_valid = ts_ns(r, name, tid)
    la, gmt = zones("America/Los_Angeles")[0], zones("GMT")[0]

    def as_la(v):
        # the stream values back from the UTC-assumed read (one second was
        # taken off a negative time with nanos above 999,999), then as Los_Angeles
        t, nanos = int(v // 1_000_000_000), int(v % 1_000_000_000)
        raw = t + (1 if t < 0 and nanos > 999_999 else 0) - tz_model.ORC_EPOCH_UTC
        s, n = tz_model.adjust(la, gmt, raw, nanos << 3)
        return s * 1_000_000_000 + n

    want = np.array([as_la(v) for v in utc], dtype=np.int64)
    assert np.array_equal(valid, got_valid)
    assert np.array_equal(got[valid], want[valid])
    # its expected output is byte-identical to orc_split_elim_new's (a
    # Los_Angeles writer): read as Los_Angeles it equals the expected output
    expect = expected_json(name)
    rows = stripe_rows(r)
    assert len(rows) == len(expect)
    for i, (w, g) in enumerate(zip(expect, rows)):
        assert printer_equal(w, to_printer_form(g)), "row %d: %r vs %r" % (i, w, g)
    r.set_local_timezone(None)
    assert tid not in r.read_stripe(0).columns


def test_missing_zone_leaves_the_column_undecoded(ctx, monkeypatch):
    monkeypatch.setenv("TZDIR", utc_tzdir())
    r = orc_amd.Reader(path("TestOrcFile.testDate1900.orc"), ctx)
    tid = ts_ids(r)[0]
    for s in range(r.num_stripes):
        b = r.read_stripe(s)
        assert tid not in b.columns
        assert all(i in b.columns for i in range(len(r.types)) if i != tid)
    rr = r.create_row_reader()
    b = rr.create_row_batch(1000)
    assert rr.next(b) and tid not in b.columns and 0 in b.columns


def test_malformed_zone_fails_the_read(ctx, monkeypatch):
    monkeypatch.setenv("TZDIR", utc_tzdir())
    r = orc_amd.Reader(path("TestOrcFile.testDate1900.orc"), ctx)
    r.set_zone_rules("US/Pacific", b"TZif" + bytes(10))
    with pytest.raises(orc_amd.ParseError, match="non-tzfile "):
        r.read_stripe(0)
    # only a read of the TIMESTAMP column needs the zone
    date_id = [i for i, t in enumerate(r.types) if t.kind == 15][0]
    r.select([date_id])
    assert date_id in r.read_stripe(0).columns
