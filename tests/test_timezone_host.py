"""Time zone rules on the host (orc_amd/csrc/timezone.cpp through the
orcg_timezone_* C ABI; no GPU): the reference's own known answers
(tests/golden/kat_timezone.json, from c++/test/TestTimezone.cc), agreement
with the Python restatement (tests/tz_model.py) and with zoneinfo on the IANA
fixture zones (tests/golden/tz), the TimezoneError texts, the lookup's path
safety, and a sanitizer build of the parser fed truncated and corrupted files."""
import base64
import datetime
import os
import shutil
import struct
import subprocess
import zoneinfo

import pytest

import orc_amd
import tz_model
from conftest import GOLDEN, ROOT, load_golden

TZ = os.path.join(GOLDEN, "tz")
ZONES = ["America/Los_Angeles", "America/New_York", "Asia/Shanghai", "Asia/Kolkata", "Australia/Sydney",
         "Europe/London", "GMT"]
KAT = load_golden("kat_timezone.json")


def zone_bytes(name):
    with open(os.path.join(TZ, name), "rb") as f:
        return f.read()


def kat_bytes(key):
    return base64.b64decode(KAT["zones"][key])


def both(name, data):
    return tz_model.Zone(name, data), orc_amd.Timezone.parse(name, data)


def rule_zone(rule):
    """A TZif v2 file with one variant, no transitions and `rule` as footer."""
    def block():
        return b"TZif2" + bytes(15) + struct.pack(">6l", 0, 0, 0, 0, 1, 4) + struct.pack(">lBB", 0, 0, 0) + b"UTC\0"
    return block() + block() + b"\n" + rule.encode() + b"\n"


def same_variant(model, c, clk):
    m, v = model.variant(clk), c.variant(clk)
    assert (m.gmt_offset, m.is_dst, m.name) == (v.gmt_offset, v.is_dst, v.name), clk
    return m


@pytest.mark.parametrize("key,version,points", KAT["parser"], ids=[p[0] for p in KAT["parser"]])
def test_parser_kat(key, version, points):
    model, c = both("America/Los_Angeles", kat_bytes(key))
    assert model.version == version and c.version == version
    for _, clk, name in points:
        assert same_variant(model, c, clk).name == name


def test_version1_has_no_rule():
    model, c = both("LA", kat_bytes("LA_VER1"))
    assert model.last_transition == tz_model.INT64_MAX
    assert c.variant(1 << 40).name == "PST"  # past 2038 a version 1 file has no rule
    assert c.epoch() == model.epoch == 1420070400 + 8 * 3600


@pytest.mark.parametrize("rule,std_name,std_off,dst_name,dst_off", KAT["rules_ok"],
                         ids=[r[0] for r in KAT["rules_ok"]])
def test_future_rule_accepted(rule, std_name, std_off, dst_name, dst_off):
    model, c = both("rule", rule_zone(rule))
    assert (model.rule.std.name, model.rule.std.gmt_offset) == (std_name, std_off)
    if dst_name is not None:
        assert (model.rule.dst.name, model.rule.dst.gmt_offset) == (dst_name, dst_off)
    # the C side exposes the rule through variant(): every variant it returns
    # over a year is one of the two asserted, and both occur when there is DST
    seen = set()
    for day in range(0, 366):
        v = same_variant(model, c, day * 86400 + 43200)
        seen.add((v.name, v.gmt_offset, v.is_dst))
    want = {(std_name, std_off, False)}
    if dst_name is not None:
        want.add((dst_name, dst_off, True))
    assert seen <= want and (std_name, std_off, False) in seen | want
    if dst_name is not None and rule != "FOO10BAR1,3,4":
        assert seen == want
    assert model.last_transition == tz_model.INT64_MIN


@pytest.mark.parametrize("rule", KAT["rules_bad"])
def test_future_rule_rejected(rule):
    with pytest.raises(tz_model.TimezoneError) as m:
        tz_model.Zone("rule", rule_zone(rule))
    with pytest.raises(orc_amd.ParseError) as c:
        orc_amd.Timezone.parse("rule", rule_zone(rule))
    assert str(c.value) == str(m.value)
    assert str(c.value).endswith(" in '%s'" % rule)


def test_empty_rule_is_undefined():
    model, c = both("rule", rule_zone(""))
    assert not model.rule.defined and model.last_transition == tz_model.INT64_MAX
    assert c.variant(0).name == "UTC"


def test_use_future_rule_kat():
    zones = {}
    for rule, _, clk, name in KAT["future"]:
        if rule not in zones:
            zones[rule] = both("rule", rule_zone(rule))
        model, c = zones[rule]
        assert same_variant(model, c, clk).name == name, (rule, clk)
    assert len(KAT["future"]) == 52


def test_convert_from_utc_kat():
    for name, clk, want in KAT["from_utc"]:
        model, c = both(name, zone_bytes(name))
        assert model.convert_from_utc(clk) == want
        assert c.convert_from_utc(clk) == want
        assert c.convert_to_utc(clk) == model.convert_to_utc(clk)


def probe_points(model):
    t = model.transitions
    pts = {-1, -tz_model.SECONDS_PER_400_YEARS - 1, -tz_model.SECONDS_PER_400_YEARS,
           -tz_model.SECONDS_PER_400_YEARS + 1, -2208988800, tz_model.ORC_EPOCH_UTC}
    for x in t:
        pts.update((x - 1, x, x + 1))
    if model.rule.defined and t:
        pts.update((model.last_transition, model.last_transition + 1))
    if model.rule.has_dst:
        cy = model.rule.cycle
        for year in (1970, 2037, 2369):
            for k in ((year - 1970) * 2 + 1, (year - 1970) * 2 + 2):
                pts.update((cy[k] - 1, cy[k], cy[k] + 1))
        for k in (1, 2):  # 2370: the cycle starts again
            b = tz_model.SECONDS_PER_400_YEARS + cy[k]
            pts.update((b - 1, b, b + 1))
        pts.update((tz_model.SECONDS_PER_400_YEARS - 1, tz_model.SECONDS_PER_400_YEARS))
    return sorted(pts)


@pytest.mark.parametrize("name", ZONES)
def test_model_c_and_zoneinfo_agree(name):
    data = zone_bytes(name)
    model, c = both(name, data)
    assert c.version == model.version == 2
    assert c.epoch() == model.epoch
    with open(os.path.join(TZ, name), "rb") as f:
        zi = zoneinfo.ZoneInfo.from_file(f, key=name)
    first = model.transitions[0] if model.transitions else tz_model.INT64_MIN
    compared = 0
    for clk in probe_points(model):
        v = same_variant(model, c, clk)
        assert c.convert_from_utc(clk) == model.convert_from_utc(clk)
        assert c.convert_to_utc(clk) == model.convert_to_utc(clk)
        if clk >= first:  # before it zoneinfo answers LMT, the reference the ancient variant
            d = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc) + datetime.timedelta(seconds=clk)
            local = d.astimezone(zi)
            assert local.utcoffset().total_seconds() == v.gmt_offset, (name, clk)
            assert local.tzname() == v.name, (name, clk)
            compared += 1
    assert compared >= 6
    if model.transitions:
        ancient = model.variant(first - 1)
        assert not ancient.is_dst and ancient == model.variants[model.ancient]


def test_zone_shapes():
    """The fixture zones cover the cases the kernel tests rely on."""
    assert tz_model.Zone("k", zone_bytes("Asia/Kolkata")).variant(1700000000).gmt_offset == 19800
    assert not tz_model.Zone("s", zone_bytes("Australia/Sydney")).rule.start_in_std
    assert tz_model.Zone("l", zone_bytes("America/Los_Angeles")).rule.start_in_std


def _v2_header(data):
    """Offset of the 64-bit block's header and its six counts."""
    n = struct.unpack(">6L", data[20:44])
    second = 44 + n[3] * 5 + n[4] * 6 + n[5] + n[2] * 8 + n[1] + n[0]
    return second + 20, struct.unpack(">6L", data[second + 20:second + 44])


def test_malformed_files():
    la = zone_bytes("America/Los_Angeles")
    hdr, (n_gmt, n_std, n_leap, n_time, n_var, n_name) = _v2_header(la)
    idx_off = hdr + 24 + 8 * n_time
    var_off = idx_off + n_time
    bad_name = bytearray(la)
    bad_name[var_off + 5] = 200
    bad_rule = bytearray(la)
    bad_rule[idx_off + 3] = 77
    cases = [
        (b"TZif" + bytes(10), "non-tzfile zone"),
        # the 64-bit block ends where the footer "\n<rule>\n" starts
        (la[:100], "tzfile too short zone needs %d and has 100" % la.rindex(b"\n", 0, len(la) - 1)),
        (bytes(bad_name), "name out of range in variant 0 - 200 >= %d" % n_name),
        (bytes(bad_rule), "tzfile rule out of range zone references rule 77 of %d" % n_var),
    ]
    for data, text in cases:
        with pytest.raises(tz_model.TimezoneError) as m:
            tz_model.Zone("zone", data)
        with pytest.raises(orc_amd.ParseError) as c:
            orc_amd.Timezone.parse("zone", data)
        assert str(m.value) == text
        assert str(c.value) == text
    with pytest.raises(orc_amd.ParseError, match="non-tzfile zone"):
        orc_amd.Timezone.parse("zone", b"")


def test_lookup_by_name(monkeypatch):
    monkeypatch.setenv("TZDIR", TZ)
    la = orc_amd.Timezone.load("America/Los_Angeles")
    assert la.variant(126698400).name == "PDT"
    # the US aliases resolve before the directory is read (no US/ files here)
    assert orc_amd.Timezone.load("US/Pacific").epoch() == la.epoch() == 1420070400 + 8 * 3600
    assert orc_amd.Timezone.load("US/Eastern").variant(0).name == "EST"
    # UTC names need no file
    monkeypatch.setenv("TZDIR", os.path.join(TZ, "no-such-directory"))
    assert orc_amd.Timezone.load("Etc/UTC").epoch() == 1420070400
    with pytest.raises(orc_amd.InvalidArgument, match="does not exist"):
        orc_amd.Timezone.load("America/Los_Angeles")


def test_lookup_never_leaves_the_directory(monkeypatch):
    monkeypatch.setenv("TZDIR", TZ)
    assert os.path.exists(os.path.join(TZ, "../tz/GMT"))
    for name in ("../tz/GMT", "America/../GMT", "..", "/" + os.path.join(TZ, "GMT").lstrip("/"), "",
                 "America/" + "x" * 260):
        with pytest.raises(orc_amd.InvalidArgument):
            orc_amd.Timezone.load(name)
    assert orc_amd.Timezone.load("America/New_York").variant(0).name == "EST"


def test_parser_under_sanitizers(tmp_path):
    """tests/cxx/tz_parse_test.cpp + timezone.cpp, -fsanitize=address,undefined:
    every prefix and every header-count overwrite of the Los_Angeles file."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "tz_parse_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cxx", "tz_parse_test.cpp"),
                    os.path.join(ROOT, "orc_amd", "csrc", "timezone.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, os.path.join(TZ, "America", "Los_Angeles")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    assert p.stdout.startswith("parsed ")
