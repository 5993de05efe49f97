"""tests/convert_model.py, the exact model of the reference's schema-evolution
conversions, pinned by the reference's own tests (c++/test/
TestConvertColumnReader.cc: their inputs regenerated from the formulas there,
tests/convert_cases.py, and the values and null flags they assert), plus the
quirks a reader of the rules would get wrong. No GPU."""
import math

import numpy as np
import pytest

import convert_model as M
from convert_cases import reference_tests

TESTS = reference_tests()


@pytest.mark.parametrize("name", sorted(TESTS))
def test_reference_test(name):
    for col in TESTS[name]:
        for i, v in enumerate(col.values):
            got = M.convert(v, col.src, col.dst)
            assert col.check(i, got), "%s %s -> %s row %d: %r -> %r" % (name, col.src, col.dst, i, v, got)


def test_magnitude_of_exactly_ten_to_the_precision_passes():
    # Int128.cc:562, :569: result > upperBound, strictly
    assert M.convert(1000, "decimal(10,0)", "decimal(3,0)") == 1000
    assert M.convert(-1000, "decimal(10,0)", "decimal(3,0)") == -1000
    assert M.convert(1001, "decimal(10,0)", "decimal(3,0)") is None
    assert M.convert(1000, "bigint", "decimal(3,0)") == 1000
    # scaling up checks the unscaled magnitude first, then the scaled one
    assert M.convert(10, "bigint", "decimal(3,2)") == 1000
    assert M.convert(11, "bigint", "decimal(3,2)") is None
    # rounding up lowers the bound to 10^p - 1, and the bound is tested before
    # the round-up is added: 999.5 -> 1000 and 1000.4 -> 1000 pass, 1000.5 does not
    assert M.convert(9995, "decimal(10,1)", "decimal(3,0)") == 1000
    assert M.convert(10004, "decimal(10,1)", "decimal(3,0)") == 1000
    assert M.convert(10005, "decimal(10,1)", "decimal(3,0)") is None
    assert M.convert(9994, "decimal(10,1)", "decimal(3,0)") == 999
    # across the 64 / 128 boundary: 10^18 as decimal(18,0) passes the bound and fits int64
    assert M.convert(10 ** 18, "decimal(38,0)", "decimal(18,0)") == 10 ** 18
    assert M.convert(10 ** 19, "decimal(38,0)", "decimal(19,0)") == 10 ** 19


def test_rounding_half_away_from_zero_on_the_magnitude():
    assert M.convert(25, "decimal(5,1)", "decimal(5,0)") == 3
    assert M.convert(-25, "decimal(5,1)", "decimal(5,0)") == -3
    assert M.convert(24, "decimal(5,1)", "decimal(5,0)") == 2
    assert M.convert(-15, "decimal(5,1)", "decimal(5,0)") == -2
    # remainder * 2 is a signed 128-bit product (Int128.cc:556): at a scale
    # difference of 38 it wraps negative and the round-up is lost
    assert M.convert(9 * 10 ** 37, "decimal(38,38)", "decimal(5,0)") == 0
    assert M.convert(6 * 10 ** 37, "decimal(38,38)", "decimal(5,0)") == 1


def test_fraction_is_added_without_a_second_bound_check():
    # Int128.cc:617-618: 9.9999 as decimal(3,2) is 9.00 + round(99.999) = 1000
    assert M.convert(np.float64(9.9999), "double", "decimal(3,2)") == 1000
    assert M.convert(np.float64(-9.9999), "double", "decimal(3,2)") == -1000
    assert M.convert(np.float64(10.0), "double", "decimal(3,2)") is None
    assert M.convert(np.float64("nan"), "double", "decimal(38,0)") is None
    assert M.convert(np.float64(2.0 ** 127), "double", "decimal(38,0)") is None
    # the hi / lo split at 2^64
    assert M.convert(np.float64(2.0 ** 100), "double", "decimal(38,0)") == 2 ** 100
    assert M.convert(np.float32(-2.0 ** 70), "float", "decimal(38,2)") == -(2 ** 70) * 100


def test_number_to_boolean_truncates_first():
    # ConvertColumnReader.cc:198: (int64)v == 0 ? 0 : 1
    assert M.convert(np.float64(0.5), "double", "boolean") == 0
    assert M.convert(np.float64(-0.9), "double", "boolean") == 0
    assert M.convert(np.float32(0.5), "float", "boolean") == 0
    assert M.convert(np.float64(1.0), "double", "boolean") == 1
    assert M.convert(np.float64(-0.0), "double", "boolean") == 0
    # the definition for NaN and values outside int64
    for v in (float("nan"), float("inf"), -float("inf"), 1e35, 2.0 ** 63):
        assert M.convert(np.float64(v), "double", "boolean") == 1
    # a decimal is compared unscaled (:559): 0.001 is true
    assert M.convert(1, "decimal(10,3)", "boolean") == 1
    assert M.convert(0, "decimal(10,3)", "boolean") == 0


def test_float_source_is_worked_in_float():
    # convertDecimal<float> computes in float (Int128.cc:581-624): the same
    # value worked in double gives other digits
    v = np.float32(0.7)
    as_float = M.convert(v, "float", "decimal(10,8)")
    as_double = M.convert(np.float64(v), "double", "decimal(10,8)")
    # (float)0.7 = 0.699999988079071...; times 1e8 a float keeps multiples of 8
    # there (70000000), a double keeps 69999998.8...
    assert as_float == 70000000 and as_double == 69999999
    # and a value where they agree
    assert M.convert(np.float32(0.5), "float", "decimal(10,8)") == M.convert(np.float64(0.5), "double", "decimal(10,8)")


def test_number_to_integer():
    # canFitInLong, then truncation, then the cast compared back
    assert M.convert(np.float64(-1.9), "double", "tinyint") == -1
    assert M.convert(np.float64(127.9), "double", "tinyint") == 127
    assert M.convert(np.float64(128.0), "double", "tinyint") is None
    assert M.convert(np.float64(-128.9), "double", "tinyint") == -128
    assert M.convert(np.float64(-2.0 ** 63), "double", "bigint") == -(1 << 63)
    assert M.convert(np.float64(2.0 ** 63), "double", "bigint") is None
    assert M.convert(np.nextafter(np.float64(2.0 ** 63), 0), "double", "bigint") == (1 << 63) - 1024
    assert M.convert(np.nextafter(np.float64(-2.0 ** 63), -np.inf), "double", "bigint") is None
    assert M.convert(np.float64("nan"), "double", "bigint") is None
    assert M.convert(1 << 31, "bigint", "int") is None
    assert M.convert(-(1 << 31), "bigint", "int") == -(1 << 31)
    assert M.convert(1 << 15, "int", "smallint") is None


def test_integer_to_floating_point_rounds_to_nearest_even():
    # 2^24 + 1 and 2^53 + 1 are ties; the reference's (1 << 62) + 112312
    assert M.convert((1 << 24) + 1, "bigint", "float") == np.float32(2.0 ** 24)
    assert M.convert((1 << 24) + 3, "bigint", "float") == np.float32(2.0 ** 24 + 4)
    assert M.convert((1 << 53) + 1, "bigint", "double") == np.float64(2.0 ** 53)
    assert M.convert((1 << 53) + 3, "bigint", "double") == np.float64(2.0 ** 53 + 4)
    assert M.convert((1 << 62) + 112312, "bigint", "float") == np.float32(2.0 ** 62)
    # one rounding, not two: 2^53 + 2^29 + 1 is above the float tie, its double is the tie
    assert M.convert((1 << 53) + (1 << 29) + 1, "bigint", "float") == np.float32(2.0 ** 53 + 2.0 ** 30)
    # double -> float overflows to infinity, not NULL
    assert M.convert(np.float64(1e39), "double", "float") == np.float32("inf")


def test_decimal_to_floating_point():
    # Int128::toDouble rounds twice when both words are needed (Int128.cc:477)
    v = (1 << 64) + (1 << 11) + 1  # low word rounds to even first, then the sum
    assert M.int128_to_double(v) == np.float64(np.uint64((1 << 11) + 1)) + np.float64(2.0 ** 64)
    assert M.convert(12345, "decimal(10,2)", "double") == np.float64(12345) / np.float64(100)
    # float: the double cast to float, divided in float by (float)factor
    assert M.convert(1, "decimal(10,1)", "float") == np.float32(1) / np.float32(10)
    # scales above 18: the correctly rounded power of ten (the one deviation)
    assert M.pow10_as(np.float64, 23) == np.float64(1e23)
    assert float(M.pow10_as(np.float32, 25)) == float(np.float32(1e25))
    assert M.convert(10 ** 25, "decimal(38,25)", "double") == np.float64(1.0)


def test_decimal_to_integer():
    assert M.convert(-19, "decimal(5,1)", "int") == -1  # truncating division
    assert M.convert((1 << 63) * 10, "decimal(38,1)", "bigint") is None
    assert M.convert(((1 << 63) - 1) * 10 + 9, "decimal(38,1)", "bigint") == (1 << 63) - 1
    assert M.convert(-(1 << 63) * 10 - 9, "decimal(38,1)", "bigint") == -(1 << 63)
    assert M.convert(1280, "decimal(5,1)", "tinyint") is None


def test_pack_layout():
    a = M.pack([-1, (1 << 64) + 5, None], "decimal(20,0)")
    assert a.tolist() == [[-1, -1], [1, 5], [0, 0]]
    assert M.pack([np.float32(0.1)], "float")[0] == float(np.float32(0.1))
    assert math.isnan(M.pack([np.float64("nan")], "double")[0])
