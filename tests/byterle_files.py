"""Crafted ORC files for the reader's byte / boolean RLE paths (BOOLEAN and
TINYINT columns and a nullable BIGINT whose PRESENT stream mixes runs and
literals, which orc_craft.bool_rle never writes): uncompressed structs whose
byte-RLE streams are built group by group, wrapped by tests/orc_craft.py with
a row index whose positions come from byterle_model.positions().

  A  stride 1000, 3001 rows (4 row groups, the last of 1 row): every byte-RLE
     stream stays under 2 KB a row group, so the reader keeps the row index.
  B  stride 100 (no multiple of 8: the boolean positions carry bits), 5001
     rows of long runs: several row groups start in one group.
  C  stride 10,000, 30,001 rows: the TINYINT stream passes 2 KB a row group
     and gets 4 KB host plans.
  A0 A without an index section.
  AS three stripes of A's schema, 1001 rows each.
  P  tests/golden/files/byterle_struct_nulls.orc, written by pyarrow: a
     nullable struct with nullable bigint, boolean and tinyint children (the
     reader's device-count path: the children's positions count the parent's
     non-null rows). pyarrow_rows() regenerates the rows it was written from.

A's cut variants shorten the PRESENT stream inside its last literal, whose
last PAD bytes no row needs: "padding" drops them (every row is still there:
the file reads like the whole one), "short" drops one byte more (the
reference's error).

The generated values are the expected values; tests/test_byterle_model_cpu.py
checks on the CPU that the oracle and pyarrow decode the same bytes to them."""
import functools
import os

import numpy as np

import byterle_model as m
import orc_craft as oc
from rlev1_files import V1Stream, literals

A_ROWS, A_STRIDE = 3001, 1000
B_ROWS, B_STRIDE = 5001, 100
C_ROWS, C_STRIDE = 30_001, 10_000
S_ROWS, S_SEEDS = 1001, (31, 32, 33)
PAD = 6  # bytes past the last row's in the PRESENT stream's last literal
P_ROWS, P_STRIDE = 5000, 1000
P_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "files", "byterle_struct_nulls.orc")
NAMES = ["flag", "tiny", "nullable"]
KINDS = [oc.T_BOOLEAN, oc.T_BYTE, oc.T_LONG]


def encode(by, rng, longest=128):
    """Byte RLE of `by`: a run wherever 3 to 130 equal bytes stand, literals
    of random lengths up to `longest` between them."""
    by, out, i = bytes(by), bytearray(), 0
    while i < len(by):
        j = i
        while j < len(by) and j - i < 130 and by[j] == by[i]:
            j += 1
        if j - i >= 3:
            out += m.run(j - i, by[i])
            i = j
            continue
        k, e = int(rng.integers(1, longest + 1)), i + 1
        while e < len(by) and e - i < k and not (e + 2 < len(by) and by[e] == by[e + 1] == by[e + 2]):
            e += 1
        out += m.lit(by[i:e])
        i = e
    return bytes(out)


class ByteStream:
    """One byte / boolean RLE stream: its decoded bytes, stream bytes and groups."""

    def __init__(self, decoded, rng, boolean, tail=b""):
        self.boolean = boolean
        self.data = encode(decoded, rng) + tail
        self.full = self.data
        self.groups = m.walk(self.data)
        assert m.decode_bytes(self.data)[:len(decoded)] == bytes(decoded)

    def positions(self, rows, stride):
        return [list(p) for p in m.positions(self.groups, rows, stride, self.boolean)]


def pack(bits):
    return np.packbits(np.asarray(bits, dtype=np.uint8)).tobytes()


class Column:
    """name, Type.Kind, the expected values (bool, int or None a row) and the
    column's streams: data (a ByteStream or, for the nullable BIGINT, a
    V1Stream) and present (a ByteStream, or None)."""

    def __init__(self, name, kind, values, data, present=None, bits=None):
        self.name, self.kind, self.values, self.data, self.present, self.bits = name, kind, values, data, present, bits

    def craft(self, stride):
        n = len(self.values)
        if self.present is None:
            pos = self.data.positions(n, stride) if stride else None
            return oc.CraftColumn([(oc.DATA, self.data.data)], pos, oc.ENC_DIRECT)
        pos = None
        if stride:
            before = np.concatenate([[0], np.cumsum(self.bits)])
            every = self.data.positions(1).tolist()  # DATA's pair of every non-null value
            pos = [p + [int(x) for x in every[int(before[g])]]
                   for g, p in zip(range(0, n, stride), self.present.positions(n, stride))]
        return oc.CraftColumn([(oc.PRESENT, self.present.data), (oc.DATA, self.data.data)], pos, oc.ENC_DIRECT)


def runs_and_noise(rng, n, values, run_len):
    """n bytes: stretches of one value (run_len() bytes) and stretches of
    random bytes from `values` in turn."""
    out = bytearray()
    while len(out) < n:
        out += bytes([int(rng.choice(values))]) * run_len()
        out += bytes(int(x) for x in rng.choice(values, size=int(rng.integers(1, 60))))
    return bytes(out[:n])


def columns(seed, n, run_len=None, tiny_run=None):
    """The three columns of n rows. run_len: the length of the PRESENT and
    BOOLEAN streams' equal-byte stretches; tiny_run: of the TINYINT's (None:
    random values, no runs to speak of)."""
    rng = np.random.default_rng(seed)
    run_len = run_len or (lambda: int(rng.integers(3, 40)))
    nb = (n + 7) // 8
    flags = np.unpackbits(np.frombuffer(runs_and_noise(rng, nb, np.arange(256), run_len), dtype=np.uint8))[:n]
    cols = [Column("flag", oc.T_BOOLEAN, [bool(x) for x in flags], ByteStream(pack(flags), rng, True))]
    both = np.array([-128, -127, -2, -1, 0, 1, 126, 127] + list(range(-60, 60, 7)))  # both sides of 0x80
    if tiny_run is None:
        tiny = rng.integers(-128, 128, size=n).astype(np.int8)
        for a in range(50, n - 150, 700):  # a run now and then
            tiny[a:a + int(rng.integers(3, 140))] = both[a % both.size]
    else:
        tiny = np.frombuffer(runs_and_noise(rng, n, both.astype(np.int8).view(np.uint8), tiny_run), dtype=np.int8)
    cols.append(Column("tiny", oc.T_BYTE, [int(x) for x in tiny], ByteStream(tiny.tobytes(), rng, False)))
    # PRESENT: bytes of 0xFF (no nulls), 0x00 and mixed bytes; its last literal
    # holds PAD bytes no row needs
    pbytes = bytearray(runs_and_noise(rng, nb, np.array([0xFF, 0xFF, 0xFF, 0x00, 0xFE, 0x7F, 0xA5, 0x5A, 0xEF]), run_len))
    pbytes[-3:] = bytes([0xB7, 0x6D, 0xDB])  # no run at the end: the last group is a literal
    bits = np.unpackbits(np.frombuffer(bytes(pbytes), dtype=np.uint8))[:n].copy()
    bits[[0, n - 1]] = 1
    body = pack(bits)
    k = int(rng.integers(4, 9))  # the last literal: k bytes of rows, then the padding
    pad = bytes([0x91, 0x23, 0x45, 0x67, 0x89, 0xAB][:PAD])
    present = ByteStream(body[:-k], rng, True, tail=m.lit(body[-k:] + pad))
    data = V1Stream("DATA", literals(rng.integers(-(1 << 40), 1 << 40, size=int(bits.sum()))), True)
    it = iter(data.values.tolist())
    cols.append(Column("nullable", oc.T_LONG, [next(it) if p else None for p in bits], data, present, bits))
    return cols


class ByteFile:
    def __init__(self, stride, stripes):
        self.names, self.kinds, self.stride, self.stripes = NAMES, KINDS, stride, stripes
        self.data = oc.struct_file(NAMES, KINDS, [(n, [c.craft(stride) for c in cols]) for n, cols in stripes], stride)

    def rows(self, stripe=0):
        """The stripe's rows as dicts (Batch.to_pylist's shape)."""
        return [dict(zip(self.names, row)) for row in zip(*[c.values for c in self.stripes[stripe][1]])]

    def byte_streams(self, stripe=0):
        """(column, ByteStream) of every byte / boolean RLE stream."""
        out = []
        for c in self.stripes[stripe][1]:
            out += [(c, s) for s in (c.present, c.data) if isinstance(s, ByteStream)]
        return out


@functools.lru_cache(maxsize=None)
def file_a(stride=A_STRIDE, cut=None):
    """File A; stride 0: A0; cut "padding" / "short": the PRESENT stream
    without its last literal's padding / without one byte more (positions
    unchanged)."""
    cols = columns(1, A_ROWS)
    if cut is not None:
        p = cols[2].present
        p.data = p.full[:len(p.full) - PAD - (cut == "short")]
    return ByteFile(stride, [(A_ROWS, cols)])


@functools.lru_cache(maxsize=None)
def file_b():
    rng = np.random.default_rng(102)
    long_runs = lambda: int(rng.integers(100, 400))
    return ByteFile(B_STRIDE, [(B_ROWS, columns(2, B_ROWS, run_len=long_runs, tiny_run=long_runs))])


@functools.lru_cache(maxsize=None)
def file_c():
    return ByteFile(C_STRIDE, [(C_ROWS, columns(3, C_ROWS))])


@functools.lru_cache(maxsize=None)
def file_as():
    return ByteFile(A_STRIDE, [(S_ROWS, columns(seed, S_ROWS)) for seed in S_SEEDS])


def pyarrow_rows():
    """The rows tests/golden/files/byterle_struct_nulls.orc was written from:
    {"s": None} or {"s": {"big": ..., "flag": ..., "tiny": ...}}, each child
    None at its own rate, in stretches and at random."""
    rng = np.random.default_rng(41)

    def mask(p_null):
        keep = rng.random(P_ROWS) >= p_null
        for _ in range(6):  # stretches without and of nulls: runs in the PRESENT stream
            a = int(rng.integers(0, P_ROWS - 400))
            keep[a:a + int(rng.integers(100, 400))] = bool(rng.integers(0, 2))
        return keep

    s, big, flag, tiny = mask(0.2), mask(0.1), mask(0.3), mask(0.05)
    vb = rng.integers(-(1 << 50), 1 << 50, size=P_ROWS)
    vf = np.repeat(rng.random(P_ROWS // 25) < 0.5, 25) ^ (rng.random(P_ROWS) < 0.1)
    vt = rng.integers(-128, 128, size=P_ROWS)
    rows = []
    for i in range(P_ROWS):
        rows.append({"s": None if not s[i] else {"big": int(vb[i]) if big[i] else None,
                                                 "flag": bool(vf[i]) if flag[i] else None,
                                                 "tiny": int(vt[i]) if tiny[i] else None}})
    return rows


def pyarrow_table():
    import pyarrow as pa

    t = pa.struct([("big", pa.int64()), ("flag", pa.bool_()), ("tiny", pa.int8())])
    return pa.table({"s": pa.array([r["s"] for r in pyarrow_rows()], type=t)})


def file_p():
    with open(P_PATH, "rb") as f:
        return f.read()
