"""LZ4 chunks inflated on the device (include/orcg.h "LZ4 chunks"): the
host plan of a run of ORC-framed chunks and the one-launch device inflate."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check

# a table row: src_offset, src_bytes, dst_offset, dst_bytes, flags (orcg_lz4_chunk)
CHUNK_FIELDS = 5
LZ4_STORED = 1


def lz4_device_info():
    """(bytes of history a chunk keeps on chip, threads per chunk)."""
    out = (ctypes.c_uint32 * 2)()
    _lib.load().orcg_lz4_device_info(out)
    return int(out[0]), int(out[1])


def lz4_plan(data, block_size):
    """The chunk table (uint64 [n, 5]) and the decompressed size of `data`,
    chunks framed by ORC's 3-byte headers. Raises ParseError with the host
    decoder's text."""
    L = _lib.load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n, total, err = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_char_p()
    src = ctypes.c_void_p(buf.ctypes.data) if buf.size else None
    # a chunk takes at least its 3-byte header
    table = np.zeros((buf.size // 3 + 1, CHUNK_FIELDS), dtype=np.uint64)
    check(L.orcg_lz4_plan(src, buf.size, int(block_size), ctypes.c_void_p(table.ctypes.data), table.shape[0],
                             ctypes.byref(n), ctypes.byref(total), ctypes.byref(err)), lambda: err.value)
    return table[:n.value].copy(), int(total.value)


def lz4_decompress_device(ctx, src, table, dst):
    """Inflates the chunks of `table` (uint64 [n, 5], host) from the uint8
    device tensor `src` into the uint8 device tensor `dst`. Synchronous; a
    corrupt chunk raises ParseError (ctx.last_error_value() = its index)."""
    L = _lib.load()
    table = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, CHUNK_FIELDS)
    ctx.after_torch()
    check(L.orcg_lz4_decompress_device(ctx.handle, ctypes.c_void_p(src.data_ptr()), src.numel(),
                                          ctypes.c_void_p(table.ctypes.data), table.shape[0],
                                          ctypes.c_void_p(dst.data_ptr()), dst.numel()), ctx.last_error)
    return dst
