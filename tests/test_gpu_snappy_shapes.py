"""snappy_inflate_kernel (orc_amd/csrc/inflate_kernels.hip) against the exact
model (tests/snappy_model.py), byte for byte and between sentinel bytes, on
the built streams of tests/snappy_cases.py: every literal length form, copies
by offset and length (overlap, pattern repeat), dependent chains, the edges of
the on-chip history (R from orcg_snappy_device_info) and the read-back path
behind it, small and unaligned outputs, stored chunks, many chunks a launch,
and one crafted chunk per error text."""
import numpy as np
import pytest

import orc_amd
import snappy_cases as C
import snappy_model as M

pytestmark = pytest.mark.gpu

R, _ = orc_amd.snappy_device_info()
GUARD = 256
SENTINEL = 0xA5
GOOD = C.good_cases(R)
BAD = C.bad_cases()


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def inflate(ctx, chunks, src_pad=0, dst_pad=0):
    """Runs one launch over `chunks`, source and destination `*_pad` bytes past
    a 256-byte boundary. Returns (the destination bytes, its leading and
    trailing guard bytes, the plan)."""
    import torch

    framed = b"".join(M.frame(b, st) for b, st in chunks)
    table, total = orc_amd.snappy_plan(framed, C.BLOCK)
    src = torch.zeros(src_pad + len(framed) + 16, dtype=torch.uint8, device="cuda")
    src[src_pad:src_pad + len(framed)] = torch.frombuffer(bytearray(framed), dtype=torch.uint8).cuda()
    buf = torch.full((GUARD + dst_pad + total + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    lo = GUARD + dst_pad
    dst = buf[lo:lo + total]
    try:
        orc_amd.snappy_decompress_device(ctx, src[src_pad:src_pad + len(framed)], table, dst)
        err = None
    except orc_amd.ParseError as e:
        err = (ctx.last_error_value(), str(e))
    host = buf.cpu().numpy()
    return host[lo:lo + total].tobytes(), np.concatenate([host[:lo], host[lo + total:]]), table, err


def expected(chunks):
    out = []
    for body, stored in chunks:
        d = bytes(body) if stored else M.decode(body, C.BLOCK)
        out.append(d)
    return out


@pytest.mark.parametrize("name", sorted(GOOD))
def test_matches_model(ctx, name):
    chunks = GOOD[name]
    want = b"".join(expected(chunks))
    got, guard, table, err = inflate(ctx, chunks)
    assert err is None
    assert len(got) == len(want) == int(table[:, 3].sum())
    assert got == want
    assert (guard == SENTINEL).all()


@pytest.mark.parametrize("name", ["sizes", "stored_mixed", "copy_len_63"])
def test_every_alignment(ctx, name):
    chunks = GOOD[name]
    want = b"".join(expected(chunks))
    for a in range(16):
        got, guard, _, err = inflate(ctx, chunks, src_pad=a, dst_pad=(a * 7 + 3) % 16)
        assert err is None and got == want, a
        assert (guard == SENTINEL).all(), a
        got, guard, _, err = inflate(ctx, chunks, src_pad=5, dst_pad=a)
        assert err is None and got == want, a
        assert (guard == SENTINEL).all(), a


@pytest.mark.parametrize("name", sorted(BAD))
def test_crafted_errors(ctx, name):
    chunks, index, text = BAD[name]
    # the model first: exactly this check fires, in this chunk
    _, merr = M.decode_framed(b"".join(M.frame(b, st) for b, st in chunks), C.BLOCK)
    assert merr == (index, text)
    got, guard, table, err = inflate(ctx, chunks, src_pad=3, dst_pad=9)
    assert err == (index, text)
    assert (guard == SENTINEL).all()
    # the sound chunks of the launch are whole: a failing chunk writes inside its own range only
    for row, (body, stored) in zip(table, chunks):
        d = bytes(body) if stored else M.decode(body, C.BLOCK)
        if isinstance(d, bytes):
            assert got[int(row[2]):int(row[2] + row[3])] == d
    # the context is usable afterwards
    got, guard, _, err = inflate(ctx, GOOD["chunks_2"])
    assert err is None and got == b"".join(expected(GOOD["chunks_2"]))


def test_table_outside_the_buffers_is_refused(ctx):
    import torch

    framed = M.frame(M.Stream(1).literal(40).block())
    table, total = orc_amd.snappy_plan(framed, C.BLOCK)
    src = torch.frombuffer(bytearray(framed), dtype=torch.uint8).cuda()
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    for col, delta in ((0, 1), (1, 1), (2, 1), (3, 1)):
        t = table.copy()
        t[0, col] += delta
        with pytest.raises(orc_amd.InvalidArgument):
            orc_amd.snappy_decompress_device(ctx, src, t, dst)
    assert (dst.cpu().numpy() == SENTINEL).all()
    # a destination length that disagrees with the preamble: nothing is written past it
    t = table.copy()
    t[0, 3] -= 1
    with pytest.raises(orc_amd.ParseError) as e:
        orc_amd.snappy_decompress_device(ctx, src, t, dst)
    assert str(e.value) == M.LENGTH_MISMATCH
    assert dst.cpu().numpy()[-1] == SENTINEL
