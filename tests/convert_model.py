"""Exact model of the reference's schema-evolution value conversions, for the
numeric and decimal kinds: Python integers for the 128-bit work, numpy.float32
/ numpy.float64 for the floating steps. Each function names the lines of the
reference it restates (c++/src/ConvertColumnReader.cc = CCR, c++/src/Int128.cc
= I128). Nothing here is shared with the code under test.

Types are written as ORC type strings ("tinyint", "decimal(10,2)"). A value
is an int (boolean 0/1, the integers, a decimal's unscaled value), a
numpy.float32 (float) or a numpy.float64 (double); a conversion returns the
converted value, or None where the reference calls handleOverflow (CCR:66-76:
the row becomes NULL, or the read raises under throwOnSchemaEvolutionOverflow).

Two definitions where the reference's behaviour is undefined, both the result
of the x86 conversion instruction (INT64_MIN): static_cast<int64_t> of a NaN
or of a value outside int64 in number -> boolean (so the result is 1), and of
the rounded fraction in convertDecimal<T> for scales above 18. One deliberate
deviation: the factor of decimal -> float / double for file scales above 18 is
the correctly rounded 10^scale (the reference's int64 product overflows).
"""
import math
import re

import numpy as np

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INT128_MIN, INT128_MAX = -(1 << 127), (1 << 127) - 1
INT_WIDTH = {"tinyint": 1, "smallint": 2, "int": 4, "bigint": 8}
INTEGERS = ("boolean", "tinyint", "smallint", "int", "bigint")
NUMERIC = INTEGERS + ("float", "double")


def parse(t):
    """type string -> (kind, precision, scale)"""
    m = re.fullmatch(r"decimal\((\d+),(\d+)\)", t)
    if m:
        return "decimal", int(m.group(1)), int(m.group(2))
    assert t in NUMERIC, t
    return t, 0, 0


def wrap(x, bits):
    """two's complement wrap to a signed integer of `bits` bits"""
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def trunc_div(a, b):
    """C++ integer division (Int128::divide keeps its sign rules, I128:288-)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def fits_in_long(v):
    return INT64_MIN <= v <= INT64_MAX


# ---- Int128.cc ---------------------------------------------------------------

def scale_up_int128(value, power):
    """scaleUpInt128ByPowerOfTen, I128:502-522 -> (value, overflow)"""
    while power > 0:
        step = min(power, 18)
        if value > 0 and trunc_div(INT128_MAX, 10 ** step) < value:
            return INT128_MAX, True
        if value < 0 and trunc_div(INT128_MIN, 10 ** step) > value:
            return INT128_MIN, True
        value *= 10 ** step
        power -= step
    return value, False


def scale_down_int128(value, power):
    """scaleDownInt128ByPowerOfTen, I128:524-532: truncating division in steps"""
    while power > 0:
        step = min(power, 18)
        value = trunc_div(value, 10 ** step)
        power -= step
    return value


def convert_decimal_int128(value, from_scale, to_precision, to_scale):
    """convertDecimal(Int128, fromScale, toPrecision, toScale, round = true),
    I128:534-579 -> (overflow, result). Works on the magnitude; every bound
    check is strictly greater (:562, :569), so a magnitude of exactly 10^p
    passes; the bound drops to 10^p - 1 only when rounding up (:557-560)."""
    assert 1 <= to_precision <= 38 and 0 <= to_scale <= to_precision and from_scale >= 0
    assert INT128_MIN < value <= INT128_MAX
    negative = value < 0
    mag = abs(value)
    upper, overflow = scale_up_int128(1, to_precision)  # :549
    round_offset = 0
    delta = from_scale - to_scale
    if delta > 0:
        scale, overflow = scale_up_int128(1, delta)  # :554
        mag, rem = divmod(mag, scale)  # :555
        rem = wrap(rem * 2, 128)  # :556, a signed Int128 product: wraps past 2^127
        if rem >= scale:  # :557
            upper -= 1
            round_offset = 1
    elif delta < 0:
        if mag > upper:  # :562
            return True, mag
        mag, overflow = scale_up_int128(mag, -delta)  # :566
    if mag > upper:  # :569
        return True, mag
    mag += round_offset
    return overflow, (-mag if negative else mag)


def round_half_away(x):
    """std::round of a finite non-negative float, as an int"""
    f = float(x)
    fl = math.floor(f)
    return int(fl) + (1 if f - fl >= 0.5 else 0)


def convert_decimal_fp(value, precision, scale, T):
    """convertDecimal<T>(T value, precision, scale), I128:581-624, computed in
    T (numpy.float32 or numpy.float64) -> (overflow, result)."""
    value = T(value)
    upper = T(2.0 ** 127)  # :584
    if np.isnan(value) or value <= -upper or value >= upper:  # :593
        return True, 0
    negative = bool(value < 0)
    value = np.abs(value)
    if value >= T(2.0 ** 64):  # :601-604
        hi = int(np.ldexp(value, -64))
        lo = int(value - np.ldexp(T(hi), 64))
        i128 = (hi << 64) | lo
    else:
        i128 = int(value)  # :606 (uint64_t)value
    value = value - np.floor(value)  # :608
    assert type(value) is T
    i128, overflow = scale_up_int128(i128, scale)  # :611
    if overflow or i128 >= scale_up_int128(1, precision)[0]:  # :612
        return True, 0
    value = value * T(math.pow(10, scale))  # :617, (T)pow(10, scale) from libm
    assert type(value) is T
    r = round_half_away(value)  # :618, then static_cast<int64_t>: no second bound check
    r = r if fits_in_long(r) else INT64_MIN
    i128 = wrap(i128 + r, 128)
    return False, (wrap(-i128, 128) if negative else i128)


def int128_to_double(v):
    """Int128::toDouble, I128:473-478: two roundings when the value needs both words"""
    if fits_in_long(v):
        return np.float64(np.int64(v))
    lo, hi = v & ((1 << 64) - 1), v >> 64
    return np.float64(np.uint64(lo)) + np.ldexp(np.float64(np.int64(hi)), 64)


def pow10_as(T, scale):
    """(T)factor_ of DecimalToNumericColumnReader, CCR:498-501, :536: the int64
    product cast to T; above scale 18 the correctly rounded 10^scale."""
    if scale <= 18:
        return T(np.int64(10 ** scale))
    exact = 10 ** scale
    if T is np.float64:
        return np.float64(float(exact))  # int -> float is correctly rounded
    c = np.float32(float(exact))
    cands = [np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(np.inf))]
    return min(cands, key=lambda x: abs(int(x) - exact))


# ---- ConvertColumnReader.cc --------------------------------------------------

def can_fit_in_long(v):
    """canFitInLong, CCR:59-63, in double; NaN fails"""
    v = np.float64(v)
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(np.float64(-2.0 ** 63) - v < 1.0) and bool(v < np.float64(2.0 ** 63))


def down_cast(v, width):
    """downCastToInteger, CCR:96-106: cast to the read width and compare back"""
    t = wrap(v, 8 * width)
    return t if t == v else None


def cast_int64(v):
    """static_cast<int64_t> of a float or double: truncation; outside int64 or
    NaN the x86 conversion's INT64_MIN (a definition, see the module text)"""
    v = float(v)
    if math.isnan(v) or math.isinf(v):
        return INT64_MIN
    t = int(v)
    return t if fits_in_long(t) else INT64_MIN


def convert(value, src, dst):
    """One value of file type `src` read as `dst`; None = overflow."""
    sk, sp, ss = parse(src)
    dk, dp, ds = parse(dst)
    src_fp = sk in ("float", "double")
    if src_fp:
        value = (np.float32 if sk == "float" else np.float64)(value)
    if dk == "boolean":
        if sk == "decimal":
            return int(value != 0)  # CCR:559: the unscaled value
        return int(cast_int64(value) != 0) if src_fp else int(value != 0)  # CCR:198, :203
    if dk in INT_WIDTH:
        if sk == "decimal":  # CCR:521-531
            value = scale_down_int128(value, ss)
            if not fits_in_long(value):
                return None
        elif src_fp:  # CCR:134-137
            if not can_fit_in_long(value):
                return None
            value = int(value)  # truncates toward zero
        return down_cast(value, INT_WIDTH[dk])  # CCR:146
    if dk in ("float", "double"):
        T = np.float32 if dk == "float" else np.float64
        with np.errstate(over="ignore", invalid="ignore"):
            if sk == "decimal":  # CCR:533-537
                return T(int128_to_double(value)) / pow10_as(T, ss)
            if src_fp:
                return T(value)  # CCR:132: a plain cast; overflow gives +-inf
            return T(np.int64(value))  # CCR:141: a plain cast (the NaN check cannot fire)
    assert dk == "decimal"
    if sk == "decimal":
        overflow, r = convert_decimal_int128(value, ss, dp, ds)  # CCR:592-611
    elif src_fp:
        overflow, r = convert_decimal_fp(value, dp, ds, np.float32 if sk == "float" else np.float64)  # CCR:373-390
    else:
        overflow, r = convert_decimal_int128(value, 0, dp, ds)  # CCR:393-409
    if overflow or (dp <= 18 and not fits_in_long(r)):
        return None
    return r


# ---- columns in the reader's batch layout -------------------------------------

def pack(values, t):
    """values of type `t` as the reader lays a column out: int64 for boolean /
    integers / decimal with precision <= 18, float64 for float (holding the
    float value) / double, int64 [n, 2] = [hi, lo] for decimal above 18.
    None (a NULL) packs as 0."""
    k, p, _ = parse(t)
    if k in ("float", "double"):
        return np.array([0.0 if v is None else float(v) for v in values], dtype=np.float64)
    if k == "decimal" and p > 18:
        out = np.zeros((len(values), 2), dtype=np.int64)
        for i, v in enumerate(values):
            v = 0 if v is None else v
            out[i, 0] = v >> 64
            out[i, 1] = wrap(v & ((1 << 64) - 1), 64)
        return out
    return np.array([0 if v is None else int(v) for v in values], dtype=np.int64)


def convert_column(values, not_null, src, dst):
    """-> (values read as dst with None for NULL, mask bytes, rows nulled by
    the conversion). not_null None = every row set."""
    out, mask, nulled = [], [], 0
    for i, v in enumerate(values):
        if not_null is not None and not not_null[i]:
            out.append(None)
            mask.append(0)
            continue
        r = convert(v, src, dst)
        nulled += r is None
        out.append(r)
        mask.append(int(r is not None))
    return out, np.array(mask, dtype=np.uint8), nulled
