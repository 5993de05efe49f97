"""A Python restatement of the reference's time zone rules, used as the
checker of the C ABI and of timestamp_tz_kernel.

  Zone.parse        TimezoneImpl::parseZoneFile      c++/src/Timezone.cc:869-946
  parse_rule        FutureRuleParser / computeOffsets  :307-466, :225-252
  search_le         binarySearch                      :85-113
  Zone.variant      TimezoneImpl::getVariant          :948-963, FutureRuleImpl::getVariant :275-290
  Zone.epoch        TimezoneImpl ctor                 :664-679
  convert_*         :608-616
  adjust            TimestampColumnReader::next       c++/src/ColumnReader.cc:318-347

Python's zoneinfo is no checker before a zone's first transition: it gives
LMT there, the reference the "ancient" variant (the first non-DST variant a
transition points at)."""
import collections
import struct

Variant = collections.namedtuple("Variant", "gmt_offset is_dst name")

SECONDS_PER_DAY = 86400
SECONDS_PER_400_YEARS = SECONDS_PER_DAY * (365 * 303 + 366 * 97)
ORC_EPOCH_UTC = 1420070400  # 2015-01-01 00:00:00 UTC
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
DAYS = ((31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31), (31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31))


class TimezoneError(Exception):
    pass


def is_leap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def search_le(a, target):
    """Index of the last element <= target, or -1."""
    if not a:
        return -1
    lo, hi = 0, len(a) - 1
    mid = (lo + hi) // 2
    while a[mid] != target and lo < hi:
        if a[mid] < target:
            lo = mid + 1
        else:
            hi = 0 if mid == 0 else mid - 1
        mid = (lo + hi) // 2
    return mid - 1 if target < a[mid] else mid


def _cdiv(a, b):  # C++ division truncates toward zero
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _cmod(a, b):
    return a - _cdiv(a, b) * b


class _Day:
    def __init__(self):
        self.kind, self.day, self.week, self.month, self.time = "day", 0, 0, 0, 0

    def at(self, year):
        """Seconds past local 1 January 00:00:00 (Transition::getTime)."""
        r = self.time
        leap = is_leap(year)
        if self.kind == "julian":
            r += SECONDS_PER_DAY * self.day
            if self.day > 60 and leap:
                r += SECONDS_PER_DAY
        elif self.kind == "day":
            r += SECONDS_PER_DAY * self.day
        else:
            m = (self.month + 9) % 12 + 1
            y = year - 1 if self.month <= 2 else year
            c, yr = _cdiv(y, 100), _cmod(y, 100)
            dow = _cmod(_cdiv(26 * m - 2, 10) + 1 + yr + _cdiv(yr, 4) + _cdiv(c, 4) - 2 * c, 7)
            if dow < 0:
                dow += 7
            d = self.day - dow
            if d < 0:
                d += 7
            for _ in range(1, self.week):
                if d + 7 >= DAYS[leap][self.month - 1]:
                    break
                d += 7
            r += d * SECONDS_PER_DAY
            r += sum(DAYS[leap][:self.month - 1]) * SECONDS_PER_DAY
        return r


class Rule:
    """FutureRuleImpl: the POSIX TZ string of a TZif v2+ footer."""

    def __init__(self, text):
        self.text = text
        self.defined = bool(text)
        self.has_dst = False
        self.start_in_std = True
        self.std = self.dst = None
        self.cycle = [0]
        self._pos = 0
        if not self.defined:
            return
        name = self._name()
        self.std = Variant(-self._offset(), False, name)
        self.has_dst = self._pos < len(text)
        start, end = _Day(), _Day()
        if self.has_dst:
            name = self._name()
            off = -self._offset() if self._peek() != "," else self.std.gmt_offset + 3600
            self.dst = Variant(off, True, name)
            self._day(start)
            self._day(end)
        if self._pos != len(text):
            self._fail("Extra text")
        if self.has_dst:
            self.cycle = [0] * 801
            self.start_in_std = start.at(1970) < end.at(1970)
            base = 0
            for year in range(1970, 2370):
                to_dst = base + start.at(year) - self.std.gmt_offset
                to_std = base + end.at(year) - self.dst.gmt_offset
                k = (year - 1970) * 2
                self.cycle[k + 1], self.cycle[k + 2] = (to_dst, to_std) if self.start_in_std else (to_std, to_dst)
                base += (366 if is_leap(year) else 365) * SECONDS_PER_DAY

    def _fail(self, msg):
        raise TimezoneError("%s at %d in '%s'" % (msg, self._pos, self.text))

    def _peek(self):
        return self.text[self._pos] if self._pos < len(self.text) else "\0"

    def _name(self):
        t = self.text
        if self._pos == len(t):
            self._fail("name required")
        start = self._pos
        if t[start] == "<":
            while self._pos < len(t) and t[self._pos] != ">":
                self._pos += 1
            if self._pos == len(t):
                self._fail("missing close '>'")
            self._pos += 1
        else:
            while self._pos < len(t) and not (t[self._pos].isdigit() or t[self._pos] in "-+,"):
                self._pos += 1
        if self._pos == start:
            self._fail("empty string not allowed")
        return t[start:self._pos]

    def _number(self):
        if self._pos >= len(self.text):
            self._fail("missing number")
        v = 0
        while self._peek().isdigit():
            v = v * 10 + int(self._peek())
            self._pos += 1
        return v

    def _offset(self):
        scale, neg = 3600, False
        if self._peek() in "-+":
            neg = self._peek() == "-"
            self._pos += 1
        v = self._number() * scale
        while scale > 1 and self._peek() == ":":
            scale //= 60
            self._pos += 1
            v += self._number() * scale
        return -v if neg else v

    def _day(self, d):
        if len(self.text) - self._pos < 2 or self.text[self._pos] != ",":
            self._fail("missing transition")
        self._pos += 1
        if self._peek() == "J":
            d.kind = "julian"
            self._pos += 1
            d.day = self._number()
        elif self._peek() == "M":
            d.kind = "month"
            self._pos += 1
            d.month = self._number()
            if self._peek() != ".":
                self._fail("missing first .")
            self._pos += 1
            d.week = self._number()
            if self._peek() != ".":
                self._fail("missing second .")
            self._pos += 1
            d.day = self._number()
        else:
            d.kind = "day"
            d.day = self._number()
        if self._peek() == "/":
            self._pos += 1
            d.time = self._offset()
        else:
            d.time = 2 * 3600

    def variant(self, clk):
        if not self.has_dst:
            return self.std
        idx = search_le(self.cycle, clk % SECONDS_PER_400_YEARS)  # Python's % floors
        return self.std if self.start_in_std == (idx % 2 == 0) else self.dst


class Zone:
    def __init__(self, name, data):
        self.name = name
        self._section(bytes(data), 0, False)
        self.epoch = ORC_EPOCH_UTC - self.variant(ORC_EPOCH_UTC).gmt_offset

    def _section(self, b, section, v2):
        header = section + 20
        if len(b) < header + 24 or b[section:section + 4] != b"TZif":
            raise TimezoneError("non-tzfile " + self.name)
        n_gmt, n_std, n_leap, n_time, n_var, n_name = struct.unpack(">6L", b[header:header + 24])
        tsize = 8 if v2 else 4
        time_off = header + 24
        idx_off = time_off + tsize * n_time
        var_off = idx_off + n_time
        name_off = var_off + 6 * n_var
        end = name_off + n_name + (tsize + 4) * n_leap + n_gmt + n_std
        if end > len(b):
            raise TimezoneError("tzfile too short %s needs %d and has %d" % (self.name, end, len(b)))
        if section == 0 and b[4] != 0:
            return self._section(b, end, True)
        self.version = 2 if v2 else 1
        self.variants = []
        for v in range(n_var):
            off, dst, at = struct.unpack(">lBB", b[var_off + 6 * v:var_off + 6 * v + 6])
            if at >= n_name:
                raise TimezoneError("name out of range in variant %d - %d >= %d" % (v, at, n_name))
            names = b[name_off + at:name_off + n_name]
            self.variants.append(Variant(off, dst != 0, names.split(b"\0")[0].decode()))
        self.transitions = list(struct.unpack(">%d%s" % (n_time, "q" if v2 else "l"), b[time_off:idx_off]))
        self.current = list(b[idx_off:var_off])
        self.ancient = 0
        found = False
        for c in self.current:
            if c >= n_var:
                raise TimezoneError("tzfile rule out of range %s references rule %d of %d" % (self.name, c, n_var))
            if not found and not self.variants[c].is_dst:
                found, self.ancient = True, c
        text = b[end + 1:len(b) - 1].decode() if v2 and len(b) - end >= 2 else ""
        self.rule = Rule(text)
        if self.rule.defined:
            self.last_transition = self.transitions[-1] if self.transitions else INT64_MIN
        else:
            self.last_transition = INT64_MAX

    def variant(self, clk):
        if clk > self.last_transition:
            return self.rule.variant(clk)
        i = search_le(self.transitions, clk)
        return self.variants[self.ancient if i < 0 else self.current[i]]

    def convert_to_utc(self, clk):
        return clk + self.variant(clk).gmt_offset

    def convert_from_utc(self, clk):
        return clk - self.variant(clk - self.variant(clk).gmt_offset).gmt_offset


def decode_nanos(enc):
    """The trailing-zero code of the SECONDARY stream (ColumnReader.cc:320-326)."""
    zeros, v = enc & 7, enc >> 3
    return v * 10 ** (zeros + 1) if zeros else v


def convert(writer, reader, t):
    """A writer-zone time in the reader zone (ColumnReader.cc:333-345)."""
    if writer is reader:
        return t
    wv, rv = writer.variant(t), reader.variant(t)
    if wv.gmt_offset == rv.gmt_offset and wv.is_dst == rv.is_dst:
        return t
    adjusted = t + wv.gmt_offset - rv.gmt_offset
    return t + wv.gmt_offset - reader.variant(adjusted).gmt_offset


def adjust(writer, reader, raw_secs, enc_nanos):
    """(seconds, nanos) of one value from the DATA / SECONDARY stream values."""
    nanos = decode_nanos(enc_nanos)
    t = raw_secs + writer.epoch
    if t < 0 and nanos > 999999:
        t -= 1
    return convert(writer, reader, t), nanos
