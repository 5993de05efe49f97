"""Search arguments (include/orcg_filter.h).

`SearchArgumentBuilder` has the reference's method names
(c++/include/orc/sargs/SearchArgument.hh: startAnd / startOr / startNot / end,
equals, lessThan, lessThanEquals, in, between, isNull, build); the built
`SearchArgument` is what `Reader.filter_stripe` and
`Reader.read_stripe(filter=...)` take. Columns are type ids or top-level field
names (resolved against the reader the filter is used with); literals are
plain Python values: int (LONG), float (FLOAT), str / bytes (STRING),
datetime.date (DATE), decimal.Decimal (DECIMAL), bool (BOOLEAN).
"""
import ctypes
import datetime
import decimal

from . import _lib
from ._lib import check

EQUALS, NULL_SAFE_EQUALS, LESS_THAN, LESS_THAN_EQUALS, IN, BETWEEN, IS_NULL = range(7)
LONG, FLOAT, STRING, DATE, DECIMAL, TIMESTAMP, BOOLEAN = range(7)
EXPR_LEAF, EXPR_AND, EXPR_OR, EXPR_NOT, EXPR_CONSTANT = range(5)
_EPOCH = datetime.date(1970, 1, 1)


def literal_type(v):
    """PredicateDataType of a Python literal."""
    if isinstance(v, bool):
        return BOOLEAN
    if isinstance(v, int):
        return LONG
    if isinstance(v, float):
        return FLOAT
    if isinstance(v, (str, bytes, bytearray)):
        return STRING
    if isinstance(v, datetime.datetime):
        return TIMESTAMP
    if isinstance(v, datetime.date):
        return DATE
    if isinstance(v, decimal.Decimal):
        return DECIMAL
    raise TypeError("not a search argument literal: %r" % (v,))


def decimal_parts(v):
    """(unscaled int, scale >= 0) of a finite decimal.Decimal."""
    sign, digits, exp = v.as_tuple()
    if not isinstance(exp, int):
        raise ValueError("not a finite decimal: %r" % (v,))
    u = int("".join(map(str, digits)) or "0")
    if exp > 0:
        u, exp = u * 10 ** exp, 0
    return (-u if sign else u), -exp


class SearchArgument:
    """A built search argument: leaves (op, column, literal type, literals)
    and a postfix program of (op, arg) over them. One argument may serve
    several readers, also on several threads: the C filter it creates (one
    per resolution of its column names) runs one filter at a time."""

    def __init__(self, leaves, program):
        self.leaves = leaves
        self.program = program
        self._handles = {}

    def handle(self, lib, resolve):
        """The orcg_filter of this argument with its column names resolved by
        `resolve` (created once per resolution)."""
        cols = tuple(resolve(c) for _, c, _, _ in self.leaves)
        h = self._handles.get(cols)
        if h is None:
            h = self._handles[cols] = _Handle(lib, self, cols)
        return h.h


class _Handle:
    def __init__(self, lib, sarg, cols):
        self._L = lib
        self.h = None
        keep = []
        leaves = (_lib.FilterLeaf * max(len(sarg.leaves), 1))()
        for i, ((op, _, typ, lits), col) in enumerate(zip(sarg.leaves, cols)):
            arr = (_lib.FilterLiteral * max(len(lits), 1))()
            for k, v in enumerate(lits):
                if typ == FLOAT:
                    arr[k].d = float(v)
                elif typ == STRING:
                    b = v.encode() if isinstance(v, str) else bytes(v)
                    buf = ctypes.create_string_buffer(b, max(len(b), 1))
                    keep.append(buf)
                    arr[k].bytes = ctypes.cast(buf, ctypes.c_void_p)
                    arr[k].len = len(b)
                elif typ == DATE:
                    arr[k].lo = (v - _EPOCH).days
                elif typ == DECIMAL:
                    u, scale = decimal_parts(v)
                    if not -(1 << 127) <= u < (1 << 127):
                        raise _lib.InvalidArgument("decimal literal does not fit 128 bits")
                    arr[k].lo = ((u & ((1 << 64) - 1)) ^ (1 << 63)) - (1 << 63)
                    arr[k].hi = u >> 64
                    arr[k].scale = scale
                elif typ == TIMESTAMP:
                    pass  # refused by orcg_filter_create
                else:
                    arr[k].lo = int(v)
            keep.append(arr)
            leaves[i].op, leaves[i].column, leaves[i].literal_type = op, col, typ
            leaves[i].nliterals = len(lits)
            leaves[i].literals = arr
        prog = (_lib.FilterOp * max(len(sarg.program), 1))()
        for i, (op, arg) in enumerate(sarg.program):
            prog[i].op, prog[i].arg = op, arg
        h = ctypes.c_void_p()
        check(lib.orcg_filter_create(leaves, len(sarg.leaves), prog, len(sarg.program), ctypes.byref(h)),
              lambda: lib.orcg_filter_last_error(None))
        self.h = h

    def __del__(self):
        if self.h:
            self._L.orcg_filter_destroy(self.h)
            self.h = None


class SearchArgumentBuilder:
    """SearchArgumentBuilder (sargs/SearchArgument.hh:120-260)."""

    def __init__(self):
        self._leaves = []
        self._program = []
        self._open = []  # [op, operands so far] of the open start_*()

    def _start(self, op):
        self._open.append([op, 0])
        return self

    def start_and(self):
        return self._start(EXPR_AND)

    def start_or(self):
        return self._start(EXPR_OR)

    def start_not(self):
        return self._start(EXPR_NOT)

    def _operand(self):
        if self._open:
            self._open[-1][1] += 1

    def end(self):
        if not self._open:
            raise ValueError("end() without a start")
        op, n = self._open.pop()
        if n == 0 or (op == EXPR_NOT and n != 1):
            raise ValueError("%s of %d operands" % (("AND", "OR", "NOT")[op - 1], n))
        self._program.append((op, n if op != EXPR_NOT else 0))
        self._operand()
        return self

    def _leaf(self, op, column, lits, typ=None):
        if typ is None:
            kinds = {literal_type(v) for v in lits}
            if len(kinds) != 1:
                raise TypeError("literals of one leaf have one type")
            typ = kinds.pop()
        # (leaves are not shared: 0.0 == -0.0 and True == 1 in Python, not in a filter)
        self._leaves.append((op, column, typ, list(lits)))
        self._program.append((EXPR_LEAF, len(self._leaves) - 1))
        self._operand()
        return self

    def equals(self, column, literal):
        return self._leaf(EQUALS, column, [literal])

    def null_safe_equals(self, column, literal):
        return self._leaf(NULL_SAFE_EQUALS, column, [literal])

    def less_than(self, column, literal):
        return self._leaf(LESS_THAN, column, [literal])

    def less_than_equals(self, column, literal):
        return self._leaf(LESS_THAN_EQUALS, column, [literal])

    def is_in(self, column, literals):
        return self._leaf(IN, column, list(literals))

    def between(self, column, lower, upper):
        return self._leaf(BETWEEN, column, [lower, upper])

    def is_null(self, column):
        return self._leaf(IS_NULL, column, [], typ=LONG)

    def build(self):
        if self._open:
            raise ValueError("%d start(s) without end()" % len(self._open))
        return SearchArgument(list(self._leaves), list(self._program))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def filter_columns_device(ctx, sarg, columns, n):
    """orcg_filter_columns_device: `sarg` over device tensors. columns: dicts
    with id, kind (reader.LONG ...), optional precision / scale, and torch
    tensors by view field: not_null (uint8), data, length, blob (uint8), index,
    dict_offsets (has_nulls: the view's flag, by default whether not_null is given). Returns (device pointer of the selected int64 rows, count);
    the pointer lives in the context's scratch until its next call."""
    L = _lib.load()
    h = sarg.handle(L, int)
    views = (_lib.ColumnView * max(len(columns), 1))()
    types = (_lib.TypeInfo * max(len(columns), 1))()
    for v, t, c in zip(views, types, columns):
        v.type_id, v.kind, v.decoded, v.num_elements = c["id"], c["kind"], 1, n
        t.kind, t.precision, t.scale = c["kind"], c.get("precision", 0), c.get("scale", 0)
        nn = c.get("not_null")
        v.has_nulls = int(c.get("has_nulls", nn is not None))
        v.not_null = _p(nn)
        for name in ("data", "length", "blob", "index", "dict_offsets"):
            setattr(v, name, _p(c.get(name)))
        if c.get("blob") is not None:
            v.blob_len = c["blob"].numel()
        if c.get("dict_offsets") is not None:
            v.dict_size = c["dict_offsets"].numel() - 1
    p, cnt = ctypes.c_void_p(), ctypes.c_uint64()
    check(L.orcg_filter_columns_device(ctx.handle, h, views, types, len(columns), n, ctypes.byref(p),
                                       ctypes.byref(cnt)), lambda: L.orcg_filter_last_error(h))
    return p.value, cnt.value


def gather_device(ctx, sel, count, n_src, src8=(), src16=None, not_null=None):
    """orcg_filter_gather_device: rows sel[0 .. count) (a device pointer or an
    int64 tensor) of up to three 8-byte tensors, one 16-byte-per-row tensor
    and the mask. Returns (list of gathered 8-byte tensors, gathered 16-byte
    tensor or None, gathered mask or None, nulls among them)."""
    import torch

    L = _lib.load()
    sel_p = ctypes.c_void_p(sel.data_ptr() if hasattr(sel, "data_ptr") else sel)
    dev = (src8[0] if src8 else src16 if src16 is not None else not_null).device
    # (whole buffers are passed: an empty slice has no data pointer)
    out8 = [torch.empty(max(count, 1), dtype=s.dtype, device=dev) for s in src8]
    a_src, a_dst = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
    for k, (s, d) in enumerate(zip(src8, out8)):
        a_src[k], a_dst[k] = s.data_ptr(), d.data_ptr()
    out16 = None if src16 is None else torch.empty(2 * max(count, 1), dtype=src16.dtype, device=dev)
    out_nn = None if not_null is None else torch.empty(max(count, 1), dtype=torch.uint8, device=dev)
    nulls = ctypes.c_uint64()
    check(L.orcg_filter_gather_device(ctx.handle, sel_p, count, n_src, a_src, a_dst, _p(src16), _p(out16),
                                      _p(not_null), _p(out_nn), ctypes.byref(nulls)), ctx.last_error)
    return ([o[:count] for o in out8], None if out16 is None else out16[:2 * count],
            None if out_nn is None else out_nn[:count], nulls.value)


__all__ = ["SearchArgument", "SearchArgumentBuilder", "filter_columns_device", "gather_device"]
