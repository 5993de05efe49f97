"""The truth rules of the row-level filter (include/orcg_filter.h), restated
with Python ints, struct-level doubles and bytes; shares nothing with the
kernels or with orc_amd/csrc/filter_plan.cpp.

A column is a list of Python values, None for a null row: int (integers,
boolean 0 / 1, date days, a decimal's unscaled value at the column's scale),
float, or bytes. A leaf is (op, column, literals); a program is a postfix list
of (op, arg): (LEAF, leaf index), (AND, operand count), (OR, operand count),
(NOT, 0).

Java's row-level filter (LeafFilter.java:41-84, leaf/*.java) selects the same
rows: a leaf, negated or not, never selects a null row; AND intersects and OR
unites selections."""
import struct

EQUALS, NULL_SAFE_EQUALS, LESS_THAN, LESS_THAN_EQUALS, IN, BETWEEN, IS_NULL = range(7)
LEAF, AND, OR, NOT = range(4)
YES, NO, NULL = "YES", "NO", "NULL"


def double_bits(x):
    """Double.doubleToLongBits as a signed int: every NaN is the canonical one."""
    if x != x:
        return 0x7FF8000000000000
    return struct.unpack("<q", struct.pack("<d", x))[0]


def double_compare(a, b):
    """Double.compare: -0.0 < 0.0, NaN equal to itself and above +inf."""
    if a < b:
        return -1
    if a > b:
        return 1
    x, y = double_bits(a), double_bits(b)
    return (x > y) - (x < y)


def leaf_truth(op, v, lits):
    """YES / NO / NULL of one leaf on one value."""
    if v is None:
        return YES if op == IS_NULL else NULL
    if op == IS_NULL:
        return NO
    if op == EQUALS:
        r = v == lits[0]          # floats: IEEE (NaN never equal, -0.0 == 0.0)
    elif op == LESS_THAN:
        r = v < lits[0]           # bytes: unsigned, a proper prefix is smaller
    elif op == LESS_THAN_EQUALS:
        r = v <= lits[0]
    elif op == BETWEEN:
        r = lits[0] <= v and v <= lits[1]
    elif op == IN:
        if isinstance(v, float):  # Arrays.binarySearch over Double.compare
            r = any(double_compare(v, x) == 0 for x in lits)
        else:
            r = any(v == x for x in lits)
    else:
        raise ValueError("operator %r is not built" % op)
    return YES if r else NO


def not3(t):
    return {YES: NO, NO: YES, NULL: NULL}[t]


def and3(ts):
    return NO if NO in ts else (NULL if NULL in ts else YES)


def or3(ts):
    return YES if YES in ts else (NULL if NULL in ts else NO)


def eval_program(program, truths):
    """The postfix program over the leaves' truths of one row."""
    st = []
    for op, arg in program:
        if op == LEAF:
            st.append(truths[arg])
        elif op == NOT:
            st.append(not3(st.pop()))
        else:
            ts = [st.pop() for _ in range(arg)]
            st.append(and3(ts) if op == AND else or3(ts))
    assert len(st) == 1
    return st[0]


def push_down_not(program):
    """The program with NOT pushed to the leaves (De Morgan): a postfix list
    of ("leaf", index, negated) / ("and", n) / ("or", n)."""
    st = []
    for op, arg in program:
        if op == LEAF:
            st.append(("leaf", arg))
        elif op == NOT:
            st.append(("not", st.pop()))
        else:
            kids = [st.pop() for _ in range(arg)][::-1]
            st.append(("and" if op == AND else "or", kids))
    out = []

    def emit(node, neg):
        if node[0] == "leaf":
            out.append(("leaf", node[1], neg))
        elif node[0] == "not":
            emit(node[1], not neg)
        else:
            for k in node[1]:
                emit(k, neg)
            kind = node[0] if not neg else ("or" if node[0] == "and" else "and")
            out.append((kind, len(node[1])))

    emit(st[0], False)
    return out


def eval_pushed(pushed, truths):
    st = []
    for item in pushed:
        if item[0] == "leaf":
            t = truths[item[1]]
            st.append(not3(t) if item[2] else t)
        else:
            ts = [st.pop() for _ in range(item[1])]
            st.append(and3(ts) if item[0] == "and" else or3(ts))
    assert len(st) == 1
    return st[0]


def select(leaves, program, columns, n):
    """Row indices the filter selects: the expression is YES."""
    out = []
    for i in range(n):
        truths = [leaf_truth(op, columns[col][i], lits) for op, col, lits in leaves]
        if eval_program(program, truths) == YES:
            out.append(i)
    return out


def rescale(unscaled, scale, column_scale):
    """A decimal literal at the column's scale; ValueError where the filter
    refuses it (a larger scale, or a value past 128 bits)."""
    if scale > column_scale:
        raise ValueError("decimal literal scale %d exceeds the column's scale %d" % (scale, column_scale))
    u = unscaled * 10 ** (column_scale - scale)
    if not -(1 << 127) <= u < (1 << 127):
        raise ValueError("decimal literal does not fit 128 bits")
    return u
