"""An exact model of the column kernels (orc_amd/csrc/column_kernels.hip) in
plain Python / numpy: the null scatter, the exclusive scan with its
StringDirect checks, one job of the batched dictionary launch, the row-group
prefix / segment table and the UNION tag kernels. Every result is an integer
array; 64-bit sums wrap mod 2^64 as the kernels' (and the reference's int64)
sums do. No import of orc_amd: tests/test_column_model_cpu.py checks the model
against independent arithmetic, the GPU tests check the kernels against it."""
import numpy as np

M64 = (1 << 64) - 1


def _i64(a):
    return np.asarray(a, dtype=np.uint64).view(np.int64)


def scatter(dense, nn, out_before, fill=None):
    """Rows with nn != 0 take the dense values in order; the others keep
    out_before, or take `fill`. 16-byte elements are [hi, lo] int64 pairs
    (arrays of shape (n, 2)): their fill is [-1 if fill < 0 else 0, fill]."""
    nn = np.asarray(nn)
    out = np.array(out_before, copy=True)
    set_rows = nn != 0
    k = int(set_rows.sum())
    assert len(dense) >= k
    if fill is not None:
        if out.ndim == 2:
            out[~set_rows] = np.array([-1 if fill < 0 else 0, fill], dtype=out.dtype)
        else:
            out[~set_rows] = np.array(fill).astype(out.dtype)
    out[set_rows] = np.asarray(dense)[:k]
    return out


def scan(x):
    """(offsets[n + 1] int64, neg, wrap, total): the exclusive scan of int64
    values, sums mod 2^64; neg = a value below 0; wrap = some start + value
    (mod 2^64) below its start, compared unsigned; total = offsets[n] as an
    unsigned integer."""
    x = np.ascontiguousarray(x, dtype=np.int64)
    u = x.view(np.uint64)
    with np.errstate(over="ignore"):
        inc = np.cumsum(u, dtype=np.uint64)
    off = np.concatenate([np.zeros(1, dtype=np.uint64), inc])
    neg = int(bool((x < 0).any()))
    wrap = int(bool((off[1:] < off[:-1]).any()))
    return _i64(off), neg, wrap, int(off[-1])


def dict_job(lengths, idx, nn, n, start_before=None, len_before=None):
    """One job of the batched dictionary launch: (offsets[D + 1],
    summary[2] = [sum of the lengths mod 2^64, a length is negative],
    start[n], len[n], err). err = the lowest row that is not null and whose
    index, as uint64, is >= D (None without one). Null rows are (0, 0); rows in
    error keep start_before / len_before (zeros by default)."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    D = lengths.size
    off, neg, _, total = scan(lengths)
    start = np.zeros(n, dtype=np.int64) if start_before is None else np.array(start_before[:n], dtype=np.int64)
    ln = np.zeros(n, dtype=np.int64) if len_before is None else np.array(len_before[:n], dtype=np.int64)
    idx = np.ascontiguousarray(idx, dtype=np.int64)[:n]
    present = np.ones(n, dtype=bool) if nn is None else np.asarray(nn)[:n] != 0
    bad = present & (idx.view(np.uint64) >= np.uint64(D))
    good = present & ~bad
    start[~present] = 0
    ln[~present] = 0
    e = idx[good]
    start[good] = off[e]
    with np.errstate(over="ignore"):
        ln[good] = off[e + 1] - off[e]
    rows = np.flatnonzero(bad)
    err = int(rows[0]) if rows.size else None
    return off, np.array([total, neg], dtype=np.uint64), start, ln, err


def rg_segments(mask, n, rows, trip, boolean):
    """(prefix[G + 1], seg[G][2]) of a masked row-index stream. Row group g
    covers rows [rows[g], rows[g + 1]) (row n ends the last), both ends clamped
    to n; prefix[g] = the non-zero mask bytes of the row groups before g.
    trip[g] = {byte offset, values (bytes for a boolean stream) to skip, bits
    to skip}; seg[g] = {byte offset, first value index} with the value index
    prefix - skip, or trunc_toward_zero((prefix - bits) / 8) - skip for a
    boolean stream, clamped at 0."""
    mask = np.asarray(mask)
    rows = np.asarray(rows, dtype=np.int64)
    trip = np.asarray(trip, dtype=np.int64).reshape(-1, 3)
    G = rows.size
    bounds = np.minimum(np.concatenate([rows, [n]]).astype(np.uint64), np.uint64(n)).astype(np.int64)
    nz = np.concatenate([[0], np.cumsum(mask[:n] != 0)]).astype(np.int64)
    a, b = bounds[:-1], bounds[1:]
    counts = np.where(b > a, nz[b] - nz[a], 0)
    prefix = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    seg = np.zeros((G, 2), dtype=np.uint64)
    for g in range(G):
        off, skip, bits = (int(t) for t in trip[g])
        p = int(prefix[g])
        if boolean:
            d = p - bits
            q = abs(d) // 8
            v = (q if d >= 0 else -q) - skip
        else:
            v = p - skip
        seg[g, 0] = off & M64
        seg[g, 1] = max(v, 0)
    return prefix, seg


def union(tags, nchildren, offsets_before=None):
    """(offsets[n], counts[nchildren], first_bad) of a union's tags: a row's
    offset is its rank among the rows with its tag (rows whose tag is >=
    nchildren keep offsets_before, zeros by default); counts[k] = the rows
    with tag k; first_bad = (lowest index << 8) | tag of the first tag >=
    nchildren, or None."""
    tags = np.asarray(tags, dtype=np.uint8)
    n = tags.size
    offsets = np.zeros(n, dtype=np.int64) if offsets_before is None else np.array(offsets_before, dtype=np.int64)
    counts = np.zeros(nchildren, dtype=np.int64)
    for k in range(nchildren):
        sel = tags == k
        counts[k] = int(sel.sum())
        offsets[sel] = np.arange(counts[k], dtype=np.int64)
    bad = np.flatnonzero(tags >= nchildren) if nchildren < 256 else np.zeros(0, dtype=np.int64)
    first_bad = (int(bad[0]) << 8 | int(tags[bad[0]])) if bad.size else None
    return offsets, counts, first_bad


# ---- nested values ---------------------------------------------------------------
class Node:
    """One type of a type tree. kind: "struct" (children + names), "list"
    (one child), "map" (key, value), "union" (children), or a leaf "long",
    "boolean", "byte", "string" (dictionary: dictionary-encoded, its entries
    in first-use order; else direct). nullable: the column has a PRESENT
    stream. Python values: a dict for a struct, a list for a list, a list of
    (key, value) for a map, (tag, value) for a union, int / bool / str for a
    leaf, None for a null."""

    def __init__(self, kind, children=(), names=(), nullable=False, dictionary=False):
        self.kind, self.children, self.names = kind, list(children), list(names)
        self.nullable, self.dictionary = nullable, dictionary

    def walk(self):
        yield self
        for c in self.children:
            yield from c.walk()


class Column:
    """One column's ground truth, as the reference lays its batch out.
    n: the rows of its own row space. incoming (uint8[n], or None = all): the
    rows its parent struct is not null at: PRESENT holds one bit per such row
    (`present`, None without a PRESENT stream). not_null (uint8[n]): the
    batch's mask, the parent struct's included. dense: the values of the
    non-null rows (leaves; bytes for a string). lengths (dense) and
    offsets[n + 1] for a list / map; tags (dense), offsets (dense: the row's
    rank among the rows with its tag) and counts[child] for a union. For a
    dictionary string: entries (bytes each) and dense = the entry indices."""

    def __init__(self, cid, node, n):
        self.id, self.node, self.n = cid, node, n
        self.incoming = self.present = self.not_null = self.dense = None
        self.lengths = self.offsets = self.tags = self.counts = self.entries = None
        self.children = []

    @property
    def nonnull(self):
        return int(self.not_null.sum())


def flatten(tree, rows):
    """The columns of `rows` (values of the root type) in type-id order."""
    out = []

    def fl(node, vals, incoming):
        col = Column(len(out), node, len(vals))
        out.append(col)
        nn = np.array([v is not None for v in vals], dtype=np.uint8)
        inc = np.ones(len(vals), dtype=bool) if incoming is None else incoming != 0
        assert not (nn[~inc]).any()
        if node.nullable:
            col.present = nn[inc]
        else:
            assert nn[inc].all(), "a null in column %d, which has no PRESENT stream" % col.id
        col.incoming, col.not_null = incoming, nn
        dense = [v for v in vals if v is not None]
        k = node.kind
        if k == "struct":
            for name, c in zip(node.names, node.children):
                col.children.append(fl(c, [None if v is None else v[name] for v in vals], nn))
        elif k in ("list", "map"):
            col.lengths = np.array([len(v) for v in dense], dtype=np.int64)
            per_row = np.zeros(len(vals), dtype=np.int64)
            per_row[nn != 0] = col.lengths
            col.offsets = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int64)
            elems = [e for v in dense for e in v]
            if k == "list":
                col.children.append(fl(node.children[0], elems, None))
            else:
                col.children.append(fl(node.children[0], [e[0] for e in elems], None))
                col.children.append(fl(node.children[1], [e[1] for e in elems], None))
        elif k == "union":
            col.tags = np.array([v[0] for v in dense], dtype=np.uint8)
            col.offsets, col.counts, bad = union(col.tags, len(node.children))
            assert bad is None
            for t, c in enumerate(node.children):
                col.children.append(fl(c, [v[1] for v in dense if v[0] == t], None))
        elif k == "string":
            raw = [v.encode() for v in dense]
            if node.dictionary:
                where = {}
                col.dense = np.array([where.setdefault(b, len(where)) for b in raw], dtype=np.int64)
                col.entries = list(where)
            else:
                col.dense = raw
        else:
            col.dense = np.array([int(v) for v in dense], dtype=np.int64)
        return col

    fl(tree, list(rows), None)
    return out


def rebuild(cols):
    """The Python rows back from flatten()'s columns, by the logic of
    orc_amd.reader.Batch.value (masks, offsets, tags and dense values only)."""
    rank = {c.id: np.cumsum(c.not_null, dtype=np.int64) - 1 for c in cols}  # a non-null row's index among the dense values

    def value(c, i):
        if not c.not_null[i]:
            return None
        k, j = c.node.kind, int(rank[c.id][i])
        if k == "struct":
            return {name: value(ch, i) for name, ch in zip(c.node.names, c.children)}
        if k == "list":
            return [value(c.children[0], e) for e in range(int(c.offsets[i]), int(c.offsets[i + 1]))]
        if k == "map":
            return [(value(c.children[0], e), value(c.children[1], e))
                    for e in range(int(c.offsets[i]), int(c.offsets[i + 1]))]
        if k == "union":
            tag = int(c.tags[j])
            return (tag, value(c.children[tag], int(c.offsets[j])))
        if k == "string":
            return (c.entries[int(c.dense[j])] if c.node.dictionary else c.dense[j]).decode()
        return bool(c.dense[j]) if k == "boolean" else int(c.dense[j])

    return [value(cols[0], i) for i in range(cols[0].n)]
