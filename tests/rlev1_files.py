"""Crafted ORC files for the reader's RLEv1 paths (DIRECT / DICTIONARY column
encodings: collect -> queue_stream's V1SegDesc tables -> plan_rlev1_multi, the
kMulti instances of rlev1_kernel, and segments() -> rg_segtab for a column
under a PRESENT stream): uncompressed structs whose streams are built group
by group with tests/rlev1_writer.py, wrapped by tests/orc_craft.py with a row
index whose positions skip into runs.

  V  stride 1000, 3001 rows (4 row groups, the last of 1 row), eight columns.
     Its streams are under 64 KB (kV1SmallStream, reader_prepare.cpp), as
     those of the flagship workload are: the reader cuts them with 1 KB host
     plans and keeps the row index for the PRESENT stream alone.
  W  stride 100, 140,001 rows of 130-value runs: several row groups start in
     one run (empty segments, equal value indices). The runs' bases are
     padded varints, so the streams pass 64 KB and keep the row index; its
     segments are under 2 KB (kCB = 4).
  R  stride 1000, 9001 rows of streams past 64 KB whose row groups run to
     about 10 KB (kCB = 16): 10-byte literals, short runs with padded bases,
     and 10-byte literals under a PRESENT stream.
  V0 V without an index section.
  VS three stripes of V's schema, 1001 rows each.

The generated values are the expected values; tests/test_rlev1_model_cpu.py
checks on the CPU that the oracle and pyarrow decode the same bytes to them
and that the positions skip as they mean to."""
import functools

import numpy as np

import orc_craft as oc
import rlev1_model as m
from multi_stream_files import DICTIONARY, CraftedFile
from rlev1_writer import encode, random_groups

V_ROWS, V_STRIDE = 3001, 1000
W_ROWS, W_STRIDE = 140_001, 100
R_ROWS, R_STRIDE = 9001, 1000
SMALL_STREAM = 64 << 10  # kV1SmallStream: an RLEv1 stream up to this long gets a host plan
S_ROWS, S_SEEDS = 1001, (21, 22, 23)


class V1Stream:
    """One RLEv1 stream: its values, bytes and whole groups (rlev1_model.walk)."""

    def __init__(self, slot, groups, signed, indexed=True):
        self.slot, self.signed, self.indexed = slot, signed, indexed
        self.data, self.values = encode(groups, signed)
        self.full = self.data
        self.groups = m.walk(self.data)

    def positions(self, stride):
        return m.positions(self.groups, self.values.size, stride)

    def cut_in_last_group(self):
        """Cut the stream inside its last group (the groups before stay whole)."""
        off, _, _, size = self.groups[-1]
        assert size >= 2
        self.data = self.full[:off + max(1, size // 2)]


class Column:
    """name, Type.Kind, expected values (ints, str or None per row), the RLEv1
    streams in the order the reader queues them, and what else the column
    kind holds: dictionary / blob bytes, or the PRESENT bits."""

    def __init__(self, name, kind, values, rle, dictionary=None, blob=None, present=None):
        self.name, self.kind, self.values, self.rle = name, kind, values, rle
        self.dictionary, self.blob, self.present = dictionary, blob, present

    def craft(self, stride):
        s = {x.slot: x for x in self.rle}
        n = len(self.values)
        pos = [list(p) for p in s["DATA" if self.blob is None else "LENGTH"].positions(stride)] if stride else None
        if self.dictionary is not None:
            return oc.CraftColumn([(oc.DATA, s["DATA"].data), (oc.LENGTH, s["LENGTH"].data),
                                   (oc.DICTIONARY_DATA, self.dictionary)], pos, oc.ENC_DICTIONARY,
                                  dictionary_size=s["LENGTH"].values.size)
        if self.blob is not None:
            if stride:
                starts = np.concatenate([[0], np.cumsum(s["LENGTH"].values)])
                pos = [[int(starts[g])] + p for g, p in zip(range(0, n, stride), pos)]
            return oc.CraftColumn([(oc.DATA, self.blob), (oc.LENGTH, s["LENGTH"].data)], pos, oc.ENC_DIRECT)
        if self.present is not None:
            if stride:
                # a row group starts on a byte of the PRESENT stream (stride % 8
                # == 0): the 129-byte literal group holding it, bytes to skip, no
                # bits; then DATA's pair, counted in non-null values
                assert stride % 8 == 0
                before = np.concatenate([[0], np.cumsum(self.present)])
                data_pos = m.positions(s["DATA"].groups, s["DATA"].values.size, 1)  # of every value
                pos = []
                for g in range(0, n, stride):
                    k = int(before[g])
                    d = list(data_pos[k]) if k < s["DATA"].values.size else [len(s["DATA"].full), 0]
                    pos.append([129 * (g // 8 // 128), g // 8 % 128, 0] + d)
            return oc.CraftColumn([(oc.PRESENT, oc.bool_rle(self.present)), (oc.DATA, s["DATA"].data)], pos, oc.ENC_DIRECT)
        return oc.CraftColumn([(oc.DATA, s["DATA"].data)], pos, oc.ENC_DIRECT)


def exact(rng, n, signed, max_bits):
    """random_groups trimmed to exactly n values."""
    gs, left = [], n
    for g in random_groups(rng, n, signed, max_bits):
        k = g[3] if g[0] == "run" else len(g[1])
        if k > left:
            g = ("lit", [int(rng.integers(0, 100)) for _ in range(left)])
            k = left
        if k:
            gs.append(g)
        left -= k
    assert left == 0
    return gs


def literals(values):
    return [("lit", [int(x) for x in values[i:i + 128]]) for i in range(0, len(values), 128)]


def runs_only(rng, n, length=130, pad=None):
    """Runs of `length` values (a callable: drawn per run) back to back, the
    last one shorter (a literal if it is under 3 values); pad: the bases as
    padded varints of that many bytes."""
    gs, at = [], 0
    while at < n:
        k = min(length() if callable(length) else length, n - at)
        base, delta = int(rng.integers(-(1 << 40), 1 << 40)), int(rng.integers(-128, 128))
        if k < 3:
            gs.append(("lit", [base + i * delta for i in range(k)]))
        else:
            gs.append(("run", base, delta, k) + (() if pad is None else (pad,)))
        at += k
    return gs


def wide_literals(rng, n):
    """Literals of 10-byte varints."""
    return literals([int(x) | (1 << 62) for x in rng.integers(0, 1 << 62, size=n)])


def nullable(rng, n, groups_of):
    present = (rng.random(n) < 0.85).astype(np.uint8)
    present[[0, n - 1]] = 1
    s = V1Stream("DATA", groups_of(int(present.sum())), True)
    it = iter(s.values.tolist())
    return Column("nullable", oc.T_LONG, [next(it) if p else None for p in present], [s], present=present)


NAMES = ["mix", "tiny", "wide", "small", "runs", "dict", "str", "nullable"]
KINDS = [oc.T_LONG, oc.T_INT, oc.T_LONG, oc.T_SHORT, oc.T_LONG, oc.T_STRING, oc.T_STRING, oc.T_LONG]


def _ints(name, kind, groups):
    s = V1Stream("DATA", groups, True)
    return Column(name, kind, s.values, [s])


def columns(seed, n):
    rng = np.random.default_rng(seed)
    cols = [_ints("mix", oc.T_LONG, exact(rng, n, True, 64)),
            # 1-byte varints: a row group of 1000 values stays under 2 KB (kCB = 4)
            _ints("tiny", oc.T_INT, literals(rng.integers(-64, 64, size=n))),
            # 10-byte varints: a row group runs to about 10 KB (kCB = 16)
            _ints("wide", oc.T_LONG, wide_literals(rng, n)),
            _ints("small", oc.T_SHORT, exact(rng, n, True, 13)),  # |base| < 2^13, 129 steps of at most 128: within int16
            _ints("runs", oc.T_LONG, runs_only(rng, n))]
    idx = rng.integers(0, 3, size=n)
    length = V1Stream("LENGTH", [("lit", [len(e) for e in DICTIONARY])], False, indexed=False)
    data = V1Stream("DATA", _index_groups(rng, idx), False)
    cols.append(Column("dict", oc.T_STRING, [DICTIONARY[i] for i in data.values], [length, data],
                       dictionary="".join(DICTIONARY).encode()))
    ln = V1Stream("LENGTH", _length_groups(rng, n), False)
    blob = rng.integers(97, 122, size=int(ln.values.sum()), dtype=np.uint8, endpoint=True).tobytes()
    ends, text = np.cumsum(ln.values), blob.decode()
    cols.append(Column("str", oc.T_STRING, [text[e - k:e] for e, k in zip(ends.tolist(), ln.values.tolist())], [ln],
                       blob=blob))
    cols.append(nullable(rng, n, lambda k: exact(rng, k, True, 40)))
    return cols


def _length_groups(rng, n):
    """String lengths 0..139: literals of 0..40 and runs stepping by 0 or 1."""
    gs, left = [], n
    while left:
        if rng.random() < 0.4 and left >= 3:
            k = min(int(rng.integers(3, 131)), left)
            gs.append(("run", int(rng.integers(0, 11)), int(rng.integers(0, 2)), k))
        else:
            k = min(int(rng.integers(1, 129)), left)
            gs.append(("lit", [int(x) for x in rng.integers(0, 41, size=k)]))
        left -= k
    return gs


def _index_groups(rng, idx):
    """Dictionary indices 0..2: literals, and a run wherever 3 to 130 equal
    or stepping indices can be made."""
    gs, at, n = [], 0, len(idx)
    while at < n:
        if rng.random() < 0.3 and n - at >= 3:
            k = min(int(rng.integers(3, 131)), n - at)
            gs.append(("run", int(idx[at]), 0, k))
        else:
            k = min(int(rng.integers(1, 129)), n - at)
            gs.append(("lit", [int(x) for x in idx[at:at + k]]))
        at += k
    return gs


class V1File(CraftedFile):
    def rows(self, stripe=0):
        """The stripe's rows as dicts (Batch.to_pylist's shape)."""
        n, cols = self.stripes[stripe]
        lists = [c.values if isinstance(c.values, list) else c.values.tolist() for c in cols]
        return [dict(zip(self.names, row)) for row in zip(*lists)]


@functools.lru_cache(maxsize=None)
def file_v(stride=V_STRIDE, cut=()):
    """File V; stride 0: V0; cut: column ids whose DATA stream is cut inside
    its last group (positions unchanged)."""
    cols = columns(1, V_ROWS)
    for cid in cut:
        [s for s in cols[cid - 1].rle if s.slot == "DATA"][0].cut_in_last_group()
    return V1File(NAMES, KINDS, stride, [(V_ROWS, cols)])


@functools.lru_cache(maxsize=None)
def file_w():
    rng = np.random.default_rng(2)
    names, kinds = ["runs", "shifted", "tiny"], [oc.T_LONG, oc.T_LONG, oc.T_INT]
    cols = [_ints("runs", oc.T_LONG, runs_only(rng, W_ROWS, pad=62)),
            _ints("shifted", oc.T_LONG, [("lit", [7, -9, 11])] + runs_only(rng, W_ROWS - 3, pad=62)),
            _ints("tiny", oc.T_INT, literals(rng.integers(-64, 64, size=W_ROWS)))]
    return V1File(names, kinds, W_STRIDE, [(W_ROWS, cols)])


@functools.lru_cache(maxsize=None)
def file_r():
    rng = np.random.default_rng(3)
    names, kinds = ["wide", "runs", "nullable"], [oc.T_LONG, oc.T_LONG, oc.T_LONG]
    cols = [_ints("wide", oc.T_LONG, wide_literals(rng, R_ROWS)),
            _ints("runs", oc.T_LONG, runs_only(rng, R_ROWS, length=lambda: int(rng.integers(3, 6)), pad=40)),
            nullable(rng, R_ROWS, lambda k: wide_literals(rng, k))]
    return V1File(names, kinds, R_STRIDE, [(R_ROWS, cols)])


@functools.lru_cache(maxsize=None)
def file_vs():
    return V1File(NAMES, KINDS, V_STRIDE, [(S_ROWS, columns(seed, S_ROWS)) for seed in S_SEEDS])
