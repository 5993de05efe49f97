"""Crafted ORC files with nested and nullable columns for the reader's column
kernels (orc_amd/csrc/column_kernels.hip) and its parent-mask -> child-count
-> child-row-group chain: uncompressed files of an arbitrary type tree, their
streams built from column_model.flatten()'s ground truth with the encoders the
other crafted files use (RLEv2 runs from orc_amd.encode_runs, byte / boolean
RLE from byterle_files.encode), wrapped by orc_craft.tree_file with a row
index. A child's positions are its streams' positions at every value, taken
at the child's value count at the parent row group's first row.

  N1  struct<a:array<bigint>>, stride 16, 2,101 rows (132 row groups, the
      last of 5 rows): PRESENT on the struct, the list and the elements;
      lengths 0-5; null structs, null lists and empty lists over whole row
      groups.
  N2  struct<m:map<string,bigint>>, stride 1000, 4,097 rows: dictionary keys
      (16, 4096 or 4097 entries, each used), null maps and values.
  N3  struct<u:uniontype<bigint,string,boolean>>, stride 100, 5,001 rows:
      PRESENT on the union and each child, tags in long runs (the string child
      absent from row groups 10-17), the string child direct-encoded.
  N4  struct<l:array<uniontype<bigint,array<tinyint>>>>, stride 64, 1,500
      rows, nulls at every level below the root.
  N5  N1's schema without nulls or PRESENT streams.  N6  N1 without an index.
  N7  struct<s:string>, dictionary, 70,000 rows, 65,536 or 65,537 one-byte
      entries; bad: the last entry's length is 2^63 + 1 as the unsigned LENGTH
      value (negative as int64).
  N8  struct<s:string>, direct, 8,193 rows (three 4,096-value scan tiles);
      bad: the last length negative, the last two 2^63 - 1 (the running
      total wraps at the last), the blob one byte short.
  N9  struct<a:array<bigint>, s:string, m:map<string,bigint>,
      u:uniontype<bigint,boolean>, x:bigint, t:string, b:array<tinyint>>,
      stride 64, 2,101 rows, no PRESENT on the root: seven top-level subtrees
      (the struct's fork over the side lanes, two subtrees to a lane), three
      lists / maps waiting for the fork's next level (the map's 64-entry
      dictionary keys and its values on two lanes), nulls in a, its elements,
      s, m, its values, u, its children and x; t (direct) and b have none (a
      batched length scan and batched LENGTH streams beside the keys'
      pre-loaded dictionary). Column ids 0..13: the keys are 5, u is 7, t 11.
      Bad: the key index = the dictionary's size at keys 5 and 1,500; tag 3
      at the union's non-null rows 7 and 1,000; t's blob one byte short.
  Bad N3: tag 3 at non-null rows 1,234 and 4,000, tag 255 at the last.
  Bad N2 (16 and 4097 entries): entry index = the dictionary's size at key
  2,047 (the last of the first 2,048-row tile) and at key 3,000.

The Python rows a file is built from are its expected values;
tests/test_column_model_cpu.py checks them against pyarrow's ORC reader."""
import functools

import numpy as np

import byterle_files as bf
import byterle_model as bm
import column_model as cm
import orc_amd
import orc_craft as oc
from column_model import Node

KIND = {"struct": oc.T_STRUCT, "list": oc.T_LIST, "map": oc.T_MAP, "union": oc.T_UNION, "long": oc.T_LONG,
        "boolean": oc.T_BOOLEAN, "byte": oc.T_BYTE, "string": oc.T_STRING}


class IntStream:
    """An RLEv2 stream of SHORT_REPEAT runs (3 to 10 equal values) and DIRECT
    runs of random lengths up to 300 between them."""

    def __init__(self, values, signed, rng):
        v = np.ascontiguousarray(values, dtype=np.int64)
        kinds, lens, i = [], [], 0
        while i < v.size:
            e = i + 1
            while e < v.size and e - i < 10 and v[e] == v[i]:
                e += 1
            repeat = e - i >= 3
            if not repeat:
                limit, e = i + int(rng.integers(1, 301)), i + 1
                while e < v.size and e < limit and not (e + 2 < v.size and v[e] == v[e + 1] == v[e + 2]):
                    e += 1
            kinds.append("short_repeat" if repeat else "direct")
            lens.append(e - i)
            i = e
        self.values, self.signed = v, signed
        self.data, offs = (orc_amd.encode_runs(v, signed, kinds, lens) if kinds else (np.zeros(0, np.uint8), []))
        self.data = self.data.tobytes()
        self.offs = [int(o) for o in offs]
        self.first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

    def at(self, v):
        """The row-index position of value v: the byte offset of its run and
        the values to skip in it (the end of the stream: all of the last run)."""
        if not self.offs:
            return [0, 0]
        k = min(int(np.searchsorted(self.first, v, side="right")) - 1, len(self.offs) - 1)
        return [self.offs[k], int(v - self.first[k])]


class ByteStream(bf.ByteStream):
    def __init__(self, decoded, rng, boolean):
        super().__init__(decoded, rng, boolean)
        by = np.frombuffer(bytes(decoded), dtype=np.uint8)
        self.values = np.unpackbits(by) if boolean else by  # what the stream decodes to (padding bits included)

    def at(self, v):
        """Byte mode: (group start, bytes to skip); boolean: of row v's byte,
        and the bits consumed of it."""
        if not self.groups:
            return [0, 0, 0] if self.boolean else [0, 0]
        first = bm.firsts(self.groups)
        byte = v // 8 if self.boolean else v
        k = min(int(np.searchsorted(first, byte, side="right")) - 1, len(self.groups) - 1)
        return [self.groups[k][0], int(byte - first[k])] + ([v % 8] if self.boolean else [])


def craft_column(col, rg_rows, rng):
    """The CraftColumn of one column; rg_rows: the first row of every row
    group in the column's own row space (None: no index)."""
    node, kind = col.node, col.node.kind
    inc = np.ones(col.n, dtype=np.int64) if col.incoming is None else (col.incoming != 0)
    inc_before = np.concatenate([[0], np.cumsum(inc, dtype=np.int64)])
    nn_before = np.concatenate([[0], np.cumsum(col.not_null, dtype=np.int64)])
    streams, parts = [], []  # parts: (stream, "rows" | "values" | "bytes")
    encoding, dict_size = (oc.ENC_DIRECT if kind == "struct" else oc.ENC_DIRECT_V2), None
    if col.present is not None:
        ps = ByteStream(bf.pack(col.present), rng, True)
        streams.append((oc.PRESENT, ps.data))
        parts.append((ps, "rows"))
    if kind == "long":
        s = IntStream(col.dense, True, rng)
        streams.append((oc.DATA, s.data))
        parts.append((s, "values"))
    elif kind in ("byte", "boolean", "union"):
        by = bf.pack(col.dense) if kind == "boolean" else \
            (col.tags if kind == "union" else col.dense.astype(np.int8).view(np.uint8)).tobytes()
        s = ByteStream(by, rng, kind == "boolean")
        streams.append((oc.DATA, s.data))
        parts.append((s, "values"))
        encoding = oc.ENC_DIRECT_V2 if kind == "union" else oc.ENC_DIRECT
    elif kind in ("list", "map"):
        s = IntStream(col.lengths, False, rng)
        streams.append((oc.LENGTH, s.data))
        parts.append((s, "values"))
    elif kind == "string" and node.dictionary:
        lens = getattr(col, "entry_lengths", None)
        lens = np.array([len(e) for e in col.entries], dtype=np.int64) if lens is None else lens
        s = IntStream(col.dense, False, rng)
        streams += [(oc.DATA, s.data), (oc.LENGTH, IntStream(lens, False, rng).data),
                    (oc.DICTIONARY_DATA, b"".join(col.entries))]
        parts.append((s, "values"))
        encoding, dict_size = oc.ENC_DICTIONARY_V2, len(col.entries)
    elif kind == "string":
        lens = getattr(col, "value_lengths", None)
        true_lens = np.array([len(b) for b in col.dense], dtype=np.int64)
        s = IntStream(true_lens if lens is None else lens, False, rng)
        blob = b"".join(col.dense)
        streams += [(oc.DATA, blob[:len(blob) - getattr(col, "blob_cut", 0)]), (oc.LENGTH, s.data)]
        parts += [(np.concatenate([[0], np.cumsum(true_lens)]), "bytes"), (s, "values")]
    pos = None
    col.seeks = []  # per positioned RLE stream: (stream, its value index at every row group's first row)
    if rg_rows is not None and parts:
        pos = [[] for _ in rg_rows]
        for s, what in parts:
            at = [int((inc_before if what == "rows" else nn_before)[r]) for r in rg_rows]
            for e, v in zip(pos, at):
                if what == "bytes":
                    e.append(int(s[v]))
                else:
                    e += s.at(v)
            if what != "bytes":
                col.seeks.append((s, at))
    return oc.CraftColumn(streams, pos, encoding, dict_size)


def child_rows(col, k, rg_rows):
    """Child k's row-group starts from its parent's."""
    kind = col.node.kind
    if kind == "struct":
        return list(rg_rows)
    if kind in ("list", "map"):
        return [int(col.offsets[r]) for r in rg_rows]
    nn_before = np.concatenate([[0], np.cumsum(col.not_null, dtype=np.int64)])
    tag_before = np.concatenate([[0], np.cumsum(col.tags == k, dtype=np.int64)])
    return [int(tag_before[nn_before[r]]) for r in rg_rows]


def type_messages(tree):
    nodes = list(tree.walk())
    ids = {id(n): i for i, n in enumerate(nodes)}
    return [oc.type_msg(KIND[n.kind], [ids[id(c)] for c in n.children], n.names) for n in nodes]


class NestedFile:
    """tree, rows (Python values of the root struct; None = a null root row),
    cols (column_model.flatten's ground truth, after `tweak`), data (the
    file's bytes)."""

    def __init__(self, tree, rows, stride, seed, tweak=None):
        self.tree, self.rows, self.stride = tree, rows, stride
        self.cols = cm.flatten(tree, rows)
        if tweak:
            tweak(self.cols)
        rng = np.random.default_rng(seed)
        n = len(rows)
        crafted = [None] * len(self.cols)

        def go(col, rg_rows):
            crafted[col.id] = craft_column(col, rg_rows, rng)
            for k, ch in enumerate(col.children):
                go(ch, None if rg_rows is None else child_rows(col, k, rg_rows))

        go(self.cols[0], list(range(0, n, stride)) if stride else None)
        self.crafted = crafted
        self.data = oc.tree_file(type_messages(tree), [(n, crafted)], stride)

    def pylist(self):
        """The rows as Batch.to_pylist and pyarrow give them (a null root
        row: every field None; a union value: as given)."""
        names = self.tree.names
        return [dict.fromkeys(names) if r is None else r for r in self.rows]


def mask_runs(rng, n, p_null, runs):
    """True = keep: nulls at rate p_null, and the given (first, count) runs of nulls."""
    keep = rng.random(n) >= p_null
    for a, k in runs:
        keep[a:a + k] = False
    return keep


# ---- N1 / N5 / N6 -------------------------------------------------------------------
N1_ROWS, N1_STRIDE = 2101, 16


def n1_rows(nulls):
    rng = np.random.default_rng(1)
    n = N1_ROWS
    root = mask_runs(rng, n, 0.1 if nulls else 0, [(160, 48)] if nulls else [])
    lists = mask_runs(rng, n, 0.15 if nulls else 0, [(320, 80), (1000, 7)] if nulls else [])
    lens = rng.integers(0, 6, size=n)
    lens[480:560] = 0  # empty lists over five row groups
    lens[2090:] = 5
    rows = []
    for i in range(n):
        if not root[i]:
            rows.append(None)
        elif not lists[i]:
            rows.append({"a": None})
        else:
            keep = rng.random(lens[i]) >= (0.2 if nulls else 0)
            vals = rng.integers(-(1 << 40), 1 << 40, size=lens[i])
            if i % 50 < 8:
                vals[:] = 7 * (i // 50)  # equal values: SHORT_REPEAT runs
            rows.append({"a": [int(v) if k else None for v, k in zip(vals, keep)]})
    return rows


def n1_tree(nulls):
    return Node("struct", [Node("list", [Node("long", nullable=nulls)], nullable=nulls)], ["a"], nullable=nulls)


@functools.lru_cache(maxsize=None)
def n1():
    return NestedFile(n1_tree(True), n1_rows(True), N1_STRIDE, 11)


@functools.lru_cache(maxsize=None)
def n5():
    return NestedFile(n1_tree(False), n1_rows(False), N1_STRIDE, 15)


@functools.lru_cache(maxsize=None)
def n6():
    return NestedFile(n1_tree(True), n1_rows(True), 0, 16)


# ---- N2 -----------------------------------------------------------------------------
N2_ROWS, N2_STRIDE, N2_BAD_KEYS = 4097, 1000, (2047, 3000)


def _n2_bad(cols):
    for k in N2_BAD_KEYS:
        cols[2].dense[k] = len(cols[2].entries)


@functools.lru_cache(maxsize=None)
def n2(D, bad=False):
    rng = np.random.default_rng(2)
    n = N2_ROWS
    maps = mask_runs(rng, n, 0.1, [(1990, 30)])
    lens = rng.integers(0, 5, size=n)
    total = int(lens[maps].sum())
    assert total >= D + 1000
    keys = np.concatenate([rng.permutation(D), rng.integers(0, D, size=total - D)])
    rows, at = [], 0
    for i in range(n):
        if not maps[i]:
            rows.append({"m": None})
            continue
        m = []
        for _ in range(lens[i]):
            m.append(("k%05d" % keys[at], None if rng.random() < 0.2 else int(rng.integers(-1000, 1000))))
            at += 1
        rows.append({"m": m})
    tree = Node("struct", [Node("map", [Node("string", dictionary=True), Node("long", nullable=True)], nullable=True)],
                ["m"])
    f = NestedFile(tree, rows, N2_STRIDE, 20 + D % 7, tweak=_n2_bad if bad else None)
    assert len(f.cols[2].entries) == D and f.cols[2].n > N2_BAD_KEYS[1]
    return f


# ---- N3 -----------------------------------------------------------------------------
N3_ROWS, N3_STRIDE, N3_BAD = 5001, 100, (1234, 4000)


def _n3_bad(cols):
    u = cols[1]
    assert u.tags.size > N3_BAD[1]
    u.tags[N3_BAD[0]] = u.tags[N3_BAD[1]] = 3
    u.tags[-1] = 255


@functools.lru_cache(maxsize=None)
def n3(bad=False):
    rng = np.random.default_rng(3)
    n = N3_ROWS
    keep = mask_runs(rng, n, 0.1, [(2500, 130)])
    tags = np.repeat(rng.integers(0, 3, size=n // 40 + 1), 40)[:n]
    tags[1000:1800] = np.where(tags[1000:1800] == 1, 2, tags[1000:1800])  # no string in row groups 10-17
    tags[3000:3050] = rng.integers(0, 3, size=50)
    rows = []
    for i in range(n):
        if not keep[i]:
            rows.append({"u": None})
            continue
        t = int(tags[i])
        if rng.random() < 0.15:
            v = None
        elif t == 0:
            v = int(rng.integers(-(1 << 50), 1 << 50))
        elif t == 1:
            v = "s%d" % i * int(rng.integers(0, 4))
        else:
            v = bool(rng.integers(0, 2))
        rows.append({"u": (t, v)})
    tree = Node("struct", [Node("union", [Node("long", nullable=True), Node("string", nullable=True),
                                          Node("boolean", nullable=True)], nullable=True)], ["u"])
    return NestedFile(tree, rows, N3_STRIDE, 30, tweak=_n3_bad if bad else None)


# ---- N4 -----------------------------------------------------------------------------
N4_ROWS, N4_STRIDE = 1500, 64


@functools.lru_cache(maxsize=None)
def n4():
    rng = np.random.default_rng(4)
    n = N4_ROWS
    keep = mask_runs(rng, n, 0.1, [(256, 70)])
    rows = []
    for i in range(n):
        if not keep[i]:
            rows.append({"l": None})
            continue
        elems = []
        for _ in range(int(rng.integers(0, 4)) if not 640 <= i < 720 else 0):
            p = rng.random()
            if p < 0.15:
                elems.append(None)
            elif (i // 100) % 2 == 0 or p < 0.3:
                elems.append((0, None if rng.random() < 0.2 else int(rng.integers(-(1 << 30), 1 << 30))))
            elif rng.random() < 0.15:
                elems.append((1, None))
            else:
                elems.append((1, [None if rng.random() < 0.2 else int(x)
                                  for x in rng.integers(-128, 128, size=int(rng.integers(0, 4)))]))
        rows.append({"l": elems})
    inner = Node("list", [Node("byte", nullable=True)], nullable=True)
    tree = Node("struct", [Node("list", [Node("union", [Node("long", nullable=True), inner], nullable=True)],
                                nullable=True)], ["l"])
    return NestedFile(tree, rows, N4_STRIDE, 40)


# ---- N7 -----------------------------------------------------------------------------
N7_ROWS = 70_000
NEG_LENGTH = -(1 << 63) + 1  # 2^63 + 1 as the unsigned LENGTH value


@functools.lru_cache(maxsize=None)
def n7(D, bad=False):
    rng = np.random.default_rng(7)
    entries = [bytes([33 + e % 90]) for e in range(D)]  # one byte an entry, not distinct
    idx = np.concatenate([rng.permutation(D), rng.integers(0, D, size=N7_ROWS - D)]).astype(np.int64)
    rows = [{"s": entries[e].decode()} for e in idx]

    def tweak(cols):
        cols[1].entries, cols[1].dense = entries, idx
        if bad:
            cols[1].entry_lengths = np.array([1] * (D - 1) + [NEG_LENGTH], dtype=np.int64)

    tree = Node("struct", [Node("string", dictionary=True)], ["s"])
    return NestedFile(tree, rows, 10_000, 70, tweak=tweak)


# ---- N8 -----------------------------------------------------------------------------
N8_ROWS = 8193
BIG = (1 << 63) - 1


@functools.lru_cache(maxsize=None)
def n8(bad=None):
    """bad: None, "negative", "wrap" or "short"."""
    rng = np.random.default_rng(8)
    rows = [{"s": "v%d" % i * int(rng.integers(0, 3))} for i in range(N8_ROWS)]
    rows[-1] = {"s": "last"}

    def tweak(cols):
        lens = np.array([len(b) for b in cols[1].dense], dtype=np.int64)
        if bad == "negative":
            lens[-1] = NEG_LENGTH
        elif bad == "wrap":
            lens[-2:] = BIG  # the total passes 2^64 at the last value: the only one of the third tile
        if bad in ("negative", "wrap"):
            cols[1].value_lengths = lens
        if bad == "short":
            cols[1].blob_cut = 1

    tree = Node("struct", [Node("string")], ["s"])
    return NestedFile(tree, rows, 1000, 80, tweak=tweak)


# ---- N9 -----------------------------------------------------------------------------
N9_ROWS, N9_STRIDE, N9_DICT, N9_BAD_KEYS, N9_BAD_TAGS = 2101, 64, 64, (5, 1500), (7, 1000)
N9_KEYS, N9_UNION, N9_T = 5, 7, 11  # column ids


@functools.lru_cache(maxsize=None)
def n9(bad=()):
    """bad: any of "index" (the keys), "tag" (the union), "short" (t's blob)."""
    rng = np.random.default_rng(9)
    n, D = N9_ROWS, N9_DICT

    def maybe(p, v):
        return None if rng.random() < p else v

    keys = iter(np.concatenate([rng.permutation(D), rng.integers(0, D, size=5 * n)]).tolist())
    rows = []
    for i in range(n):
        tag = int(rng.integers(0, 2))
        rows.append({
            "a": maybe(0.15, [maybe(0.2, int(v)) for v in rng.integers(-(1 << 40), 1 << 40, size=rng.integers(0, 5))]),
            "s": maybe(0.1, "s%d" % i * int(rng.integers(0, 3))),
            "m": maybe(0.15, [("k%02d" % next(keys), maybe(0.2, int(rng.integers(-1000, 1000))))
                              for _ in range(int(rng.integers(0, 5)))]),
            "u": maybe(0.1, (tag, maybe(0.15, bool(rng.integers(0, 2)) if tag else int(rng.integers(-(1 << 50), 1 << 50))))),
            "x": maybe(0.2, int(rng.integers(-(1 << 30), 1 << 30))),
            "t": "t%d" % i * int(rng.integers(0, 3)),
            "b": [int(v) for v in rng.integers(-128, 128, size=rng.integers(0, 4))],
        })
    tree = Node("struct", [Node("list", [Node("long", nullable=True)], nullable=True), Node("string", nullable=True),
                           Node("map", [Node("string", dictionary=True), Node("long", nullable=True)], nullable=True),
                           Node("union", [Node("long", nullable=True), Node("boolean", nullable=True)], nullable=True),
                           Node("long", nullable=True), Node("string"), Node("list", [Node("byte")])],
                ["a", "s", "m", "u", "x", "t", "b"])

    def tweak(cols):
        assert [c.node.kind for c in cols] == ["struct", "list", "long", "string", "map", "string", "long", "union",
                                               "long", "boolean", "long", "string", "list", "byte"]
        assert len(cols[N9_KEYS].entries) == D and cols[N9_KEYS].n > N9_BAD_KEYS[1]
        assert cols[N9_UNION].tags.size > N9_BAD_TAGS[1]
        if "index" in bad:
            for k in N9_BAD_KEYS:
                cols[N9_KEYS].dense[k] = D
        if "tag" in bad:
            for k in N9_BAD_TAGS:
                cols[N9_UNION].tags[k] = 3
        if "short" in bad:
            cols[N9_T].blob_cut = 1

    return NestedFile(tree, rows, N9_STRIDE, 9, tweak=tweak)


GOOD = {"N1": n1, "N2-16": lambda: n2(16), "N2-4096": lambda: n2(4096), "N2-4097": lambda: n2(4097), "N3": n3,
        "N4": n4, "N5": n5, "N6": n6, "N7-65536": lambda: n7(65536), "N7-65537": lambda: n7(65537), "N8": n8, "N9": n9}

UNION_TAG = "Invalid union tag 3 for union with 3 children"
DICT_INDEX = "Entry index out of range in StringDictionaryColumn"
DICT_NEGATIVE = "Negative dictionary entry length for column 1"
STR_NEGATIVE = "Negative string length in StringDirectColumnReader for column 1"
STR_OVERFLOW = "String length overflow in StringDirectColumnReader for column 1"
STR_SHORT = "failed to read in StringDirectColumnReader.next"
UNION_TAG_2 = "Invalid union tag 3 for union with 2 children"
BAD = {"N3-tags": (lambda: n3(bad=True), UNION_TAG),
       "N2-16-index": (lambda: n2(16, bad=True), DICT_INDEX),
       "N2-4097-index": (lambda: n2(4097, bad=True), DICT_INDEX),
       "N7-65536-negative": (lambda: n7(65536, bad=True), DICT_NEGATIVE),
       "N7-65537-negative": (lambda: n7(65537, bad=True), DICT_NEGATIVE),
       "N8-negative": (lambda: n8("negative"), STR_NEGATIVE),
       "N8-wrap": (lambda: n8("wrap"), STR_OVERFLOW),
       "N8-short": (lambda: n8("short"), STR_SHORT),
       # the earliest column's error, across the fork's lanes and levels: the keys (column 5, a device record of
       # fork level 1) before t's blob (column 11, a deferred check of level 0) and before the union's tags (column
       # 7, an inline failure of level 0: StructColumnReader::next reads m before u); the tags before t's blob
       "N9-index": (lambda: n9(("index", "short")), DICT_INDEX),
       "N9-tag": (lambda: n9(("index", "tag")), DICT_INDEX),
       "N9-tag-short": (lambda: n9(("tag", "short")), UNION_TAG_2)}
