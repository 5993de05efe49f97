#!/usr/bin/env python3
"""Generate tests/golden/kat_timezone.json from the reference's time zone
tests (c++/test/TestTimezone.cc).

Run with ORC_REFERENCE naming an apache/orc checkout:

    ORC_REFERENCE=<checkout> python tests/golden/make_tz_fixtures.py

The fixture is DATA ONLY: the base64 zone files the reference tests parse,
the rule strings they feed parseFutureRule, and the values they assert.

    zones          {"LA_VER1", "LA_VER2", "GMT"}: base64 TZif bytes, verbatim
    parser         testParser / testGMTv1: [zone, version, [[time, epoch seconds, variant name], ...]]
    rules_ok       parseFutureRule: [rule, standard name, standard gmtOffset,
                   dst name | null, dst gmtOffset | null] from the printed rule it asserts
    rules_bad      parseFutureRule: strings that must raise TimezoneError
    future         useFutureRule: [rule, time, epoch seconds, variant name]
    from_utc       testConvertFromUtc: [zone name, utc seconds, expected]
"""
import calendar
import json
import os
import re
import time

REF = os.environ.get("ORC_REFERENCE", "")
HERE = os.path.dirname(os.path.abspath(__file__))


def epoch(text):
    return calendar.timegm(time.strptime(text, "%Y-%m-%d %H:%M:%S"))


def c_string(src, ident):
    """The concatenated string literals of `ident = ( "..." "..." );`."""
    m = re.search(r"\b" + ident + r"(?:\[\])?\s*=\s*\(?((?:\s*\"[^\"]*\")+)\s*\)?;", src)
    return "".join(re.findall(r"\"([^\"]*)\"", m.group(1)))


def blocks(src):
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"TEST\(TestTimezone,\s*(\w+)\)", src)]
    return {name: src[pos:(starts[i + 1][0] if i + 1 < len(starts) else len(src))]
            for i, (pos, name) in enumerate(starts)}


def main():
    if not REF:
        raise SystemExit("set ORC_REFERENCE to an apache/orc checkout")
    with open(os.path.join(REF, "c++/test/TestTimezone.cc")) as f:
        src = f.read()
    tests = blocks(src)
    out = {"source": "c++/test/TestTimezone.cc",
           "zones": {k: c_string(src, k) for k in ("LA_VER1", "LA_VER2", "GMT")}}

    # testParser / testGMTv1
    parser = []
    body = tests["testParser"] + tests["testGMTv1"]
    cur = None
    for m in re.finditer(r"decodeBase64\((\w+)\)|EXPECT_EQ\((\d), \w+->getVersion\(\)\)|"
                         r"EXPECT_EQ\(\"(\w+)\", getVariantFromZone\(\*\w+, \"([^\"]+)\"\)\)", body):
        if m.group(1):
            cur = [m.group(1), None, []]
            parser.append(cur)
        elif m.group(2):
            cur[1] = int(m.group(2))
        else:
            cur[2].append([m.group(4), epoch(m.group(4)), m.group(3)])
    out["parser"] = parser

    # parseFutureRule
    body = tests["parseFutureRule"]
    out["rules_bad"] = re.findall(r"EXPECT_THROW\(stringifyRule\(\"([^\"]*)\"\)", body)
    ok = []
    for m in re.finditer(r"EXPECT_EQ\(\(?((?:\s*\"[^\"]*\")+)\)?,\s*stringifyRule\(\"([^\"]*)\"\)\)", body):
        printed = "".join(re.findall(r"\"([^\"]*)\"", m.group(1))).replace("\\n", "\n")
        std = re.search(r"  standard (\S+) (-?\d+)\n", printed)
        dst = re.search(r"  dst (\S+) (-?\d+) \(dst\)\n", printed)
        ok.append([m.group(2), std.group(1), int(std.group(2)), dst.group(1) if dst else None,
                   int(dst.group(2)) if dst else None])
    out["rules_ok"] = ok

    # useFutureRule
    future = []
    rule = None
    for m in re.finditer(r"parseFutureRule\(\"([^\"]*)\"\)|"
                         r"EXPECT_EQ\(\"(\w+)\", getZoneFromRule\(rule.get\(\), \"([^\"]+)\"\)\)",
                         tests["useFutureRule"]):
        if m.group(1) is not None:
            rule = m.group(1)
        else:
            future.append([rule, m.group(3), epoch(m.group(3)), m.group(2)])
    out["future"] = future

    # testConvertFromUtc
    body = tests["testConvertFromUtc"]
    names = dict(re.findall(r"const Timezone\* (\w+) = &getTimezoneByName\(\"([^\"]+)\"\)", body))
    conv = []
    for m in re.finditer(r"EXPECT_EQ\(([-+*\d ]+), (\w+)->convertFromUTC\((\d+)\)\)", body):
        conv.append([names[m.group(2)], int(m.group(3)), int(eval(m.group(1), {"__builtins__": {}}))])
    out["from_utc"] = conv

    with open(os.path.join(HERE, "kat_timezone.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print({k: len(v) for k, v in out.items() if not isinstance(v, str)})


if __name__ == "__main__":
    main()
