"""RLEv2 stream helpers shared by the stream-level and the crafted-file
tests: the run walker (a stream's runs from its bytes alone, so a test can
check that a stream holds the runs it means to hold), the row-index positions
of a stream, and DIRECT runs of an exact width."""
import numpy as np

FBS = list(range(1, 25)) + [26, 28, 30, 32, 40, 48, 56, 64]  # FBSToBitWidthMap
SR, DIRECT, PATCHED, DELTA = 0, 1, 2, 3


def _closest(n):
    for w in FBS:
        if n <= w:
            return w
    return 64


def walk(buf):
    """The stream's runs from its bytes: (offset, kind, W, L, bytes) each."""
    b = bytes(buf)
    runs, p = [], 0
    while p < len(b):
        fb = b[p]
        kind = fb >> 6
        if kind == SR:
            nb = ((fb >> 3) & 7) + 1
            W, L, size = 8 * nb, (fb & 7) + 3, 1 + nb
        else:
            L = (((fb & 1) << 8) | b[p + 1]) + 1
            code = (fb >> 1) & 0x1F
            if kind == DIRECT:
                W = FBS[code]
                size = 2 + (W * L + 7) // 8
            elif kind == PATCHED:
                W = FBS[code]
                third, fourth = b[p + 2], b[p + 3]
                bw, pbs = (third >> 5) + 1, FBS[third & 0x1F]
                pgw, pl = (fourth >> 5) + 1, fourth & 0x1F
                size = 4 + bw + (W * L + 7) // 8 + (_closest(pbs + pgw) * pl + 7) // 8
            else:
                W = FBS[code] if code else 0
                q = p + 2
                for _ in range(2):
                    while b[q] >= 0x80:
                        q += 1
                    q += 1
                size = q - p + ((W * (L - 2) + 7) // 8 if W else 0)
        runs.append((p, kind, W, L, size))
        p += size
    assert p == len(b)
    return runs


def positions(runs, n, stride):
    """Row-index positions every `stride` values: the byte offset of the run
    holding the group's first value and the values to skip in it."""
    if stride >= n:
        return np.array([[0, 0]], dtype=np.uint64)
    starts = np.concatenate([[0], np.cumsum([r[3] for r in runs])[:-1]]).astype(np.int64)
    offs = np.array([r[0] for r in runs], dtype=np.int64)
    g = np.arange(0, n, stride)
    ri = np.searchsorted(starts, g, side="right") - 1
    return np.stack([offs[ri], g - starts[ri]], axis=1).astype(np.uint64)


def direct_values(rng, W, L, signed):
    """L values whose DIRECT run is exactly W bits wide."""
    if signed:
        v = rng.integers(-(1 << (W - 1)), (1 << (W - 1)) - 1, size=L, dtype=np.int64, endpoint=True)
        v[0] = -(1 << (W - 1))  # zigzag: W one bits
    elif W == 64:
        v = rng.integers(-(1 << 63), (1 << 63) - 1, size=L, dtype=np.int64, endpoint=True)
        v[0] = -1
    else:
        v = rng.integers(0, (1 << W) - 1, size=L, dtype=np.int64, endpoint=True)
        v[0] = (1 << W) - 1
    return v
