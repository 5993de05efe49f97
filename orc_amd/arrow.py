"""Column-level entries of the Arrow export (include/orcg_arrow.h) on torch
tensors: each runs one kernel family of arrow_kernels.hip on device arrays, so
the kernels can be driven without a file. Every result is a uint8 tensor of
the buffer with its 64-byte zero padding (a missing kernel is an error; there
is no host fallback). The file-level export is Reader.read_stripe_arrow."""
import ctypes

from . import _lib
from ._lib import check
from .rle import _tensor_ptr

INT8, INT16, INT32, BOOL, FLOAT32, DEC64, DEC128, TIMESTAMP_NS = range(8)
_WIDTH = {INT8: 1, INT16: 2, INT32: 4, FLOAT32: 4, DEC64: 16, DEC128: 16, TIMESTAMP_NS: 8}


def padded(nbytes):
    """ORCG_ARROW_PADDED: a buffer's size with its 64-byte padding."""
    return (int(nbytes) + 63) & ~63


def fixed_bytes(form, n):
    return (n + 7) // 8 if form == BOOL else _WIDTH[form] * n


def _out(nbytes, like, fill=0xAA):
    """An output buffer, pre-filled so that padding the kernel forgot shows."""
    import torch

    return torch.full((max(nbytes, 1),), fill, dtype=torch.uint8, device=like.device)[:nbytes]


def validity_device(ctx, not_null):
    """not_null (uint8 [n], or None) -> (bitmap buffer or None, null count)."""
    if not_null is None:
        nulls = ctypes.c_uint64(1)
        check(_lib.load().orcg_arrow_validity_device(ctx.handle, None, 0, None, 0, ctypes.byref(nulls)), ctx.last_error)
        return None, int(nulls.value)
    n = not_null.numel()
    out = _out(padded((n + 7) // 8), not_null)
    nulls = ctypes.c_uint64(0)
    ctx.after_torch()
    check(_lib.load().orcg_arrow_validity_device(ctx.handle, _tensor_ptr(not_null), n, _tensor_ptr(out), out.numel(),
                                                 ctypes.byref(nulls)), ctx.last_error)
    return out, int(nulls.value)


def fixed_device(ctx, form, src, src2=None, n=None):
    """One fixed-width form over src (int64 / float64 [n]; DEC128: int64
    [n, 2] = [hi, lo]; TIMESTAMP_NS: seconds, with src2 = nanoseconds)."""
    n = src.shape[0] if n is None else n
    out = _out(padded(fixed_bytes(form, n)), src)
    ctx.after_torch()
    check(_lib.load().orcg_arrow_fixed_device(ctx.handle, int(form), _tensor_ptr(src),
                                              None if src2 is None else _tensor_ptr(src2), n, _tensor_ptr(out),
                                              out.numel()), ctx.last_error)
    return out


def offsets_device(ctx, n, offsets64=None, lengths=None, not_null=None):
    """int32 offsets [n + 1] from int64 offsets [n + 1], or from lengths [n]
    masked by not_null."""
    like = offsets64 if offsets64 is not None else lengths
    out = _out(padded(4 * (n + 1)), like)
    ctx.after_torch()
    check(_lib.load().orcg_arrow_offsets_device(ctx.handle, None if offsets64 is None else _tensor_ptr(offsets64),
                                                None if lengths is None else _tensor_ptr(lengths),
                                                None if not_null is None else _tensor_ptr(not_null), n,
                                                _tensor_ptr(out), out.numel()), ctx.last_error)
    return out


def dict_strings_device(ctx, index, not_null, dict_offsets, blob, dictionary=False):
    """A dictionary-encoded string column. dictionary=False: (int32 offsets
    buffer [n + 1], gathered bytes buffer, bytes gathered); dictionary=True:
    (int32 indices buffer [n], the dictionary's int32 offsets buffer, its
    size in bytes)."""
    L = _lib.load()
    n, dict_size = index.numel(), dict_offsets.numel() - 1
    nn = None if not_null is None else _tensor_ptr(not_null)
    nbytes = ctypes.c_uint64(0)
    ctx.after_torch()

    def call(out, data):
        check(L.orcg_arrow_dict_strings_device(ctx.handle, int(bool(dictionary)), _tensor_ptr(index), nn, n,
                                               _tensor_ptr(dict_offsets), dict_size, _tensor_ptr(blob), blob.numel(),
                                               _tensor_ptr(out), out.numel(),
                                               None if data is None else _tensor_ptr(data),
                                               0 if data is None else data.numel(), ctypes.byref(nbytes)),
              ctx.last_error)

    if dictionary:
        out, data = _out(padded(4 * n), index), _out(padded(4 * (dict_size + 1)), index)
        call(out, data)
        return out, data, int(nbytes.value)
    out = _out(padded(4 * (n + 1)), index)
    call(out, None)  # the size
    data = _out(padded(nbytes.value), index)
    if data.numel():
        call(out, data)
    return out, data, int(nbytes.value)
