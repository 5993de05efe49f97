"""Inputs and expectations of the reference's own schema-evolution tests
(c++/test/TestConvertColumnReader.cc), regenerated from the formulas there:
only numbers and formulas are restated. Shared by the model's CPU test and
the GPU tests.

reference_tests() -> {test name: [Column]}; Column.check(i, got) says whether
row i (got = the value read, None for a NULL) satisfies what the reference's
test asserts for it."""
import collections

import numpy as np

Column = collections.namedtuple("Column", "src dst values check")

N = 1024  # TEST_CASES


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def _ulps(a, b):
    """distance in representable doubles (EXPECT_DOUBLE_EQ allows 4)"""
    ia, ib = (int(np.float64(v).view(np.int64)) for v in (a, b))
    ia, ib = (v if v >= 0 else -(1 << 63) - v for v in (ia, ib))
    return abs(ia - ib)


def _between_numeric_without_overflows():
    # TestConvertColumnReader.cc:43-95
    h = N // 2
    c0 = [1 if (i % 2 or i % 3) else 0 for i in range(N)]
    c1 = [_i32((h - i) * N) for i in range(N)]
    c2 = [np.float64(N - i) / np.float64(h) for i in range(N)]
    c3 = [np.float32(N - i) / np.float32(h) for i in range(N)]
    return [
        Column("boolean", "int", c0, lambda i, g: g == (1 if (i % 2 or i % 3) else 0)),
        Column("int", "boolean", c1, lambda i, g: g is not None and (g == 1 or i == h)),
        Column("double", "bigint", c2, lambda i, g: g == (0 if i > h else (N - i) // h)),
        Column("float", "boolean", c3, lambda i, g: g is not None and (g == 1 or i > h)),
    ]


def _between_numeric_overflows():
    # :103-146: notNull flags only
    want = [[False, True], [False, True], [True, True]]

    def chk(col):
        return lambda i, g: (g is not None) == want[col][i]

    return [
        Column("double", "int", [np.float64(1e35), np.float64(1e9 + 7)], chk(0)),
        Column("bigint", "int", [1 << 31, (1 << 31) - 1], chk(1)),
        Column("bigint", "float", [(1 << 62) + 112312, (1 << 20) + 77553], chk(2)),
    ]


def _numeric_to_decimal():
    # :364-445
    h = N // 2
    c1 = [i * 12 if i < h else 12345678910 * i for i in range(N)]
    c3 = [i * 16 if i < h else 12345678910 * i for i in range(N)]

    def low(i):
        return np.float64(-1 if i % 2 else 1) * (np.float64(i * 1000) + np.float64(0.111111) * np.float64(i % 9))

    c2 = [low(i) if i < h else np.float64(12345678910.1234) * np.float64(i) for i in range(N)]
    c4 = [low(i) if i < h else
          (np.float64(123456.0) * np.float64(i) + np.float64(0.1111) * np.float64(i % 9)) * np.float64(-1 if i % 2 else 1)
          for i in range(N)]
    sgn = lambda i: -1 if i % 2 else 1  # noqa: E731
    return [
        Column("bigint", "decimal(10,2)", c1, lambda i, g: g == (i * 1200 if i < h else None)),
        Column("double", "decimal(10,4)", c2,
               lambda i, g: g == ((i * 10000000 + (1111 * (i % 9) + (i % 9 > 4))) * sgn(i) if i < h else None)),
        Column("bigint", "decimal(20,3)", c3, lambda i, g: g == (i * 16000 if i < h else 12345678910000 * i)),
        Column("double", "decimal(20,3)", c4,
               lambda i, g: g == ((i * 1000000 if i < h else 123456000 * i) + (111 * (i % 9) + (i % 9 > 4))) * sgn(i)),
    ]


def _decimal_to_numeric():
    # :527-600
    h = N // 2
    flag = lambda i: 1 if i % 2 else -1  # noqa: E731
    c1 = [flag(i) * (i * 123 if i % 2 else 0) if i < h else 0 for i in range(N)]
    c2 = [flag(i) * (i * 10000 + i) if i < h else (32767 + i) * 10000 + i for i in range(N)]
    c3 = [flag(i) * (i * 10000 + i) if i < h else (2147483647 + i) * 10000 + i for i in range(N)]
    c4 = [flag(i) * (i * 10000 + i) if i < h else 0 for i in range(N)]
    return [
        Column("decimal(10,2)", "boolean", c1, lambda i, g: g is not None and (i >= h or g == (1 if i % 2 else 0))),
        Column("decimal(10,4)", "smallint", c2, lambda i, g: g == (flag(i) * i if i < h else None)),
        Column("decimal(20,4)", "int", c3, lambda i, g: g == (flag(i) * i if i < h else None)),
        Column("decimal(20,4)", "double", c4,
               lambda i, g: g is not None and (i >= h or _ulps(g, np.float64(1.0001) * flag(i) * i) <= 4)),
    ]


def _decimal_to_decimal():
    # :602-679
    h = N // 2
    flag = lambda i: 1 if i % 2 else -1  # noqa: E731
    low = [flag(i) * (i * 10000 + i) for i in range(h)]
    c1 = low + [100000000 + i for i in range(h, N)]
    c3 = low + [100000000000 + i for i in range(h, N)]
    c4 = low + [100000000000000000000 + i for i in range(h, N)]
    up = lambda i, g: g == flag(i) * (i * 100000 + i * 10)  # noqa: E731
    down = lambda i, g: g == flag(i) * (i * 1000 + (i + 5) // 10)  # noqa: E731
    return [
        Column("decimal(10,4)", "decimal(9,5)", c1, lambda i, g: up(i, g) if i < h else g is None),
        Column("decimal(10,4)", "decimal(20,5)", c1, lambda i, g: up(i, g) if i < h else g is not None),
        Column("decimal(20,4)", "decimal(10,3)", c3, lambda i, g: down(i, g) if i < h else g is None),
        Column("decimal(20,4)", "decimal(19,3)", c4, lambda i, g: down(i, g) if i < h else g is None),
    ]


def reference_tests():
    return {
        "betweenNumericWithoutOverflows": _between_numeric_without_overflows(),
        "betweenNumricOverflows": _between_numeric_overflows(),
        "TestConvertNumericToDecimal": _numeric_to_decimal(),
        "TestConvertDecimalToNumeric": _decimal_to_numeric(),
        "TestConvertDecimalToDecimal": _decimal_to_decimal(),
    }
