"""Crafted ORC files for the multi-stream RLEv2 launches (the reader's
collect -> queue_stream -> plan_rlev2_multi -> run_multi path, whose kernel
instantiations only a file can reach): uncompressed structs of non-nullable
columns whose streams are built run by run with orc_amd.encode_runs, wrapped
by tests/orc_craft.py with a row index.

  M "mixed":   stride 10,000, 30,001 rows (4 row groups, the last of 1 row),
               ten columns, one per run make-up the instances treat apart.
  F "flat":    stride 40,000, 80,001 rows: two columns of 512-value W=64 /
               W=56 DIRECT runs and one SHORT_REPEAT column.
  S "stripes": three stripes of M's schema, 10,001 rows each.

The generated values are the expected values; tests/test_multi_stream_files.py
checks on the CPU that the oracle and pyarrow decode the same bytes to them
and that every stream holds the runs it means to hold."""
import functools

import numpy as np

import orc_craft as oc
from rle_streams import DELTA, DIRECT, PATCHED, SR, direct_values, positions, walk

M_ROWS, M_STRIDE = 30_001, 10_000
F_ROWS, F_STRIDE = 80_001, 40_000
S_ROWS, S_STRIDE, S_SEEDS = 10_001, 10_000, (11, 12, 13)
DICTIONARY = ["abc", "defgh", "i"]


class RleStream:
    """One RLEv2 stream: its values, bytes and runs (rle_streams.walk).
    indexed: the row index holds positions for it."""

    def __init__(self, slot, values, signed, kinds, lengths, indexed=True):
        import orc_amd

        self.slot, self.signed, self.indexed = slot, signed, indexed
        self.values = np.ascontiguousarray(values, dtype=np.int64)
        assert int(np.sum(lengths)) == self.values.size
        data, _ = orc_amd.encode_runs(self.values, signed, kinds, lengths)
        self.data = data
        self.full = data  # the uncut bytes
        self.runs = walk(data)
        assert [(r[1], r[3]) for r in self.runs] == [(int(k), int(ln)) for k, ln in zip(kinds, lengths)]

    def positions(self, stride):
        return positions(self.runs, self.values.size, stride)

    def cut_in_last_run(self):
        """Cut the stream inside its last run (the runs before it stay whole)."""
        off, _, _, _, size = self.runs[-1]
        assert size >= 2
        self.data = self.full[:off + max(1, size // 2)]


class Column:
    """name, Type.Kind, expected values (int64 array, or a list of str), the
    RLEv2 streams in the order the reader queues them, the file's CraftColumn."""

    def __init__(self, name, kind, values, rle):
        self.name, self.kind, self.values, self.rle = name, kind, values, rle
        self.blob = self.dictionary = None

    def craft(self, stride):
        s = {x.slot: x for x in self.rle}
        n = len(self.values)
        groups = range(0, n, stride) if stride else ()
        if self.dictionary is not None:
            pos = [list(p) for p in s["DATA"].positions(stride)] if stride else None
            return oc.CraftColumn([(oc.DATA, s["DATA"].data), (oc.LENGTH, s["LENGTH"].data),
                                   (oc.DICTIONARY_DATA, self.dictionary)], pos, oc.ENC_DICTIONARY_V2,
                                  dictionary_size=s["LENGTH"].values.size)
        if self.blob is not None:
            pos = None
            if stride:
                starts = np.concatenate([[0], np.cumsum(s["LENGTH"].values)])
                pos = [[int(starts[g])] + list(p) for g, p in zip(groups, s["LENGTH"].positions(stride))]
            return oc.CraftColumn([(oc.DATA, self.blob), (oc.LENGTH, s["LENGTH"].data)], pos)
        pos = [list(p) for p in s["DATA"].positions(stride)] if stride else None
        return oc.CraftColumn([(oc.DATA, s["DATA"].data)], pos)


class CraftedFile:
    def __init__(self, names, kinds, stride, stripes):
        self.names, self.kinds, self.stride, self.stripes = names, kinds, stride, stripes
        self.data = oc.struct_file(names, kinds, [(n, [c.craft(stride) for c in cols]) for n, cols in stripes], stride)

    def rle_streams(self, stripe=0):
        """(column id, RleStream) in the order the reader queues them."""
        return [(cid, s) for cid, c in enumerate(self.stripes[stripe][1], start=1) for s in c.rle]


def split(rng, n, lo, hi):
    """Random lengths in [lo, hi] that sum to n (n >= lo)."""
    out, rem = [], n
    while rem > 0:
        if rem <= hi:
            ln = rem
        else:
            ln = int(rng.integers(lo, min(hi, rem - lo), endpoint=True))
        out.append(ln)
        rem -= ln
    assert sum(out) == n and min(out) >= lo and max(out) <= hi
    return out


def full_runs(n):
    return [512] * (n // 512) + ([n % 512] if n % 512 else [])


def _direct(rng, spec, signed=True, slot="DATA"):
    v = np.concatenate([direct_values(rng, W, L, signed) for W, L in spec])
    s = RleStream(slot, v, signed, [DIRECT] * len(spec), [L for _, L in spec])
    assert [(r[2], r[3]) for r in s.runs] == list(spec)
    return s


def wide_periodic(rng, n, W):
    return _direct(rng, [(W, L) for L in full_runs(n)])


def chain_stops(rng, n):
    """W=48 x5, a 511-value run, W=56 x3, W=40, a 300-value run, W=64 to the end."""
    spec = [(48, 512)] * 5 + [(48, 511)] + [(56, 512)] * 3 + [(40, 512), (40, 300)]
    spec += [(64, L) for L in full_runs(n - sum(L for _, L in spec))]
    return _direct(rng, spec)


def short_direct(rng, n, W, L):
    return _direct(rng, [(W, L)] * (n // L) + ([(W, n % L)] if n % L else []))


def short_repeat_bytes(rng, n):
    """SHORT_REPEAT runs of 1-byte values, lengths 3-10: 2 bytes a run."""
    lens = split(rng, n, 3, 10)
    v = np.repeat(rng.integers(-64, 63, size=len(lens), endpoint=True), lens)
    return RleStream("DATA", v, True, [SR] * len(lens), lens)


def _delta_values(rng, L, fixed, bits, lim):
    base = int(rng.integers(-lim, lim))
    if L == 1:
        return np.array([base], dtype=np.int64)
    if fixed or L == 2:
        return base + int(rng.integers(-(1 << bits), 1 << bits)) * np.arange(L, dtype=np.int64)
    steps = rng.integers(0, 1 << bits, size=L - 1, dtype=np.int64)
    steps[0] = max(int(steps[0]), 1)
    steps[1] = (steps[0] + 1) % (1 << bits)  # not a fixed step
    if steps[1] == steps[0]:
        steps[1] = 0
    if rng.integers(0, 2):
        steps = -steps
    return base + np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)


def delta_runs(rng, n):
    """DELTA runs, fixed-step and variable-width in turn: stretches of runs of
    3-16 values with a 512-value run after each."""
    lens, rem = [], n
    while rem > 800:
        k = split(rng, int(rng.integers(30, 200)), 3, 16) + [512]
        lens += k
        rem -= sum(k)
    lens += split(rng, rem, 3, 16)
    parts = [_delta_values(rng, L, i % 2 == 0, 4 if L == 512 else int(rng.integers(2, 10)), 1 << 20)
             for i, L in enumerate(lens)]
    return RleStream("DATA", np.concatenate(parts), True, [DELTA] * len(lens), lens)


PATCH_AT = ([100], [7, 50, 51, 300, 511], [10, 400])  # one patch, several, a gap of 390 (> 255: an escape entry)
PATCH_LIST = (1, 5, 3)                                 # their patch-list lengths


def _patched_values(rng, L, at, base, bits, high):
    v = base + rng.integers(0, 1 << bits, size=L, dtype=np.int64)
    v[1] = base
    v[2] = base + (1 << bits) - 1
    for i in at:
        v[i] = base + (1 << high) + int(rng.integers(0, 1 << bits))
    return v


def patched_runs(rng, n):
    """512-value PATCHED_BASE runs (PATCH_AT in turn) between short DIRECT runs."""
    parts, kinds, rem, k = [], [], n, 0
    while rem > 600:
        for L in split(rng, int(rng.integers(6, 80)), 3, 20):
            parts.append(direct_values(rng, int(rng.integers(2, 20)), L, True))
            kinds.append(DIRECT)
        parts.append(_patched_values(rng, 512, PATCH_AT[k % 3], int(rng.integers(-(1 << 24), 1 << 24)), 10, 30))
        kinds.append(PATCHED)
        k += 1
        rem = n - sum(p.size for p in parts)
    for L in split(rng, rem, 3, 20):
        parts.append(direct_values(rng, int(rng.integers(2, 20)), L, True))
        kinds.append(DIRECT)
    return RleStream("DATA", np.concatenate(parts), True, kinds, [p.size for p in parts])


def all_kinds_int16(rng, n):
    """SHORT_REPEAT, DIRECT, PATCHED_BASE and DELTA runs of random lengths and
    widths, every value within int16."""
    parts, kinds, rem = [], [], n
    while rem > 600:
        kind = int(rng.integers(0, 4))
        if kind == SR:
            v = np.full(int(rng.integers(3, 10, endpoint=True)), int(rng.integers(-(1 << 15), 1 << 15)), dtype=np.int64)
        elif kind == DIRECT:
            L = 512 if rng.integers(0, 8) == 0 else int(rng.integers(1, 60))
            v = direct_values(rng, int(rng.integers(1, 16, endpoint=True)), L, True)
        elif kind == DELTA:
            L = 512 if rng.integers(0, 8) == 0 else int(rng.integers(3, 40))
            v = _delta_values(rng, L, bool(rng.integers(0, 2)), int(rng.integers(2, 5)), 1000)
        else:
            L = int(rng.integers(100, 512, endpoint=True))
            at = sorted({int(x) for x in rng.integers(3, L, size=int(rng.integers(1, 4)))})
            v = _patched_values(rng, L, at, int(rng.integers(-2000, 2000)), 6, 12)
        parts.append(v)
        kinds.append(kind)
        rem -= v.size
    for L in split(rng, rem, 3, 20):
        parts.append(direct_values(rng, int(rng.integers(1, 16, endpoint=True)), L, True))
        kinds.append(DIRECT)
    v = np.concatenate(parts)
    assert v.min() >= -(1 << 15) and v.max() < (1 << 15)
    return RleStream("DATA", v, True, kinds, [p.size for p in parts])


def dictionary_column(rng, name, n):
    """DICTIONARY_V2 with 3 entries: DATA W=2 DIRECT indices in 512-value
    runs, LENGTH one run of 3 values (no row-index positions: a host plan)."""
    idx = rng.integers(0, 3, size=n, dtype=np.int64)
    idx[::512] = 2  # every run is 2 bits wide
    lens = full_runs(n)
    data = RleStream("DATA", idx, False, [DIRECT] * len(lens), lens)
    assert all(r[2] == 2 for r in data.runs)
    length = RleStream("LENGTH", [len(e) for e in DICTIONARY], False, [DIRECT], [3], indexed=False)
    c = Column(name, oc.T_STRING, [DICTIONARY[i] for i in idx], [length, data])
    c.dictionary = "".join(DICTIONARY).encode()
    return c


def direct_string_column(rng, name, n):
    """DIRECT_V2: LENGTH unsigned runs of 3-20 values (DIRECT, and
    SHORT_REPEAT where a run of at most 10 is made constant), lengths 0-40."""
    ln = rng.integers(0, 40, size=n, dtype=np.int64, endpoint=True)
    lens, kinds, at = split(rng, n, 3, 20), [], 0
    for i, L in enumerate(lens):
        if i % 4 == 3 and L <= 10:
            ln[at:at + L] = ln[at]
            kinds.append(SR)
        else:
            kinds.append(DIRECT)
        at += L
    length = RleStream("LENGTH", ln, False, kinds, lens)
    blob = rng.integers(97, 122, size=int(ln.sum()), dtype=np.uint8, endpoint=True).tobytes()
    ends = np.cumsum(ln)
    text = blob.decode()
    c = Column(name, oc.T_STRING, [text[e - k:e] for e, k in zip(ends.tolist(), ln.tolist())], [length])
    c.blob = blob
    return c


M_NAMES = ["wide", "chain", "w24", "w16x5", "sr", "delta", "patched", "small", "dict", "str"]
M_KINDS = [oc.T_LONG, oc.T_LONG, oc.T_LONG, oc.T_LONG, oc.T_INT, oc.T_LONG, oc.T_LONG, oc.T_SHORT, oc.T_STRING,
           oc.T_STRING]


def m_columns(seed, n):
    rng = np.random.default_rng(seed)
    ints = [wide_periodic(rng, n, 64), chain_stops(rng, n), wide_periodic(rng, n, 24), short_direct(rng, n, 16, 5),
            short_repeat_bytes(rng, n), delta_runs(rng, n), patched_runs(rng, n), all_kinds_int16(rng, n)]
    cols = [Column(nm, k, s.values, [s]) for nm, k, s in zip(M_NAMES, M_KINDS, ints)]
    return cols + [dictionary_column(rng, "dict", n), direct_string_column(rng, "str", n)]


@functools.lru_cache(maxsize=None)
def file_m(stride=M_STRIDE, cut=()):
    """File M; stride 0: no index section; cut: column ids whose DATA stream
    is cut inside its last run (positions unchanged)."""
    cols = m_columns(1, M_ROWS)
    for cid in cut:
        cols[cid - 1].rle[0].cut_in_last_run()
    return CraftedFile(M_NAMES, M_KINDS, stride, [(M_ROWS, cols)])


@functools.lru_cache(maxsize=None)
def file_f():
    rng = np.random.default_rng(2)
    ss = [wide_periodic(rng, F_ROWS, 64), wide_periodic(rng, F_ROWS, 56), short_repeat_bytes(rng, F_ROWS)]
    names, kinds = ["w64", "w56", "sr"], [oc.T_LONG, oc.T_LONG, oc.T_LONG]
    cols = [Column(nm, k, s.values, [s]) for nm, k, s in zip(names, kinds, ss)]
    return CraftedFile(names, kinds, F_STRIDE, [(F_ROWS, cols)])


@functools.lru_cache(maxsize=None)
def file_s():
    return CraftedFile(M_NAMES, M_KINDS, S_STRIDE, [(S_ROWS, m_columns(seed, S_ROWS)) for seed in S_SEEDS])


# ---- the launch planner's rules, restated (rlev2_route.hh; checked against
# it by tests/test_cxx_rlev2_route.py) ------------------------------------------
def density_class(src_len, values):
    """route_rlev2 for a job of a multi-stream launch: the instance a stream
    of src_len bytes and `values` values gets (6: the union instance)."""
    return 2 if src_len >= 5 * values else (3 if 4 * src_len >= 5 * values else 6)


def seg_value_bound(values, nsegs):
    avg = (values + nsegs - 1) // max(nsegs, 1)
    return avg + avg // 8 + 512


def segment_values(stream, stride):
    """Values each row-index segment decodes: from the first value of the run
    its position names to the next group's first row."""
    n = stream.values.size
    pos = stream.positions(stride).astype(np.int64)
    rows = np.arange(0, n, stride)
    first = rows - pos[:, 1]
    return np.concatenate([rows[1:], [n]]) - first
