"""lz4_inflate_kernel (orc_amd/csrc/inflate_kernels.hip) against the exact
model (tests/lz4_model.py), byte for byte and between sentinel bytes, on the
built streams of tests/lz4_cases.py: every literal length form (extension runs
longer than a source slice), matches by offset and length (overlap, pattern
repeat, the phase across steps), dependent chains, the farthest offset at the
edges of the on-chip history (R from orcg_lz4_device_info), matches longer
than the history, small and unaligned outputs, stored chunks, many chunks a
launch, and one crafted chunk per rule of the walk. A corrupt block has no
plan, so the crafted launches carry tables written by hand."""
import numpy as np
import pytest

import orc_amd
import lz4_cases as C
import lz4_model as M

pytestmark = pytest.mark.gpu

R, _ = orc_amd.lz4_device_info()
GUARD = 256
SENTINEL = 0xA5
GOOD = C.good_cases(R)
BAD = C.bad_cases()


@pytest.fixture(scope="module")
def ctx():
    return orc_amd.Context(0)


def inflate(ctx, chunks, src_pad=0, dst_pad=0, table=None):
    """Runs one launch over `chunks` ((body, stored) and more), source and
    destination `*_pad` bytes past a 256-byte boundary; the table is the
    library's plan unless given. Returns (the destination bytes, its leading
    and trailing guard bytes, the table, the error)."""
    import torch

    framed = b"".join(M.frame(c[0], c[1]) for c in chunks)
    if table is None:
        table, total = orc_amd.lz4_plan(framed, C.BLOCK)
    else:
        total = int(table[:, 3].sum())
    src = torch.zeros(src_pad + len(framed) + 16, dtype=torch.uint8, device="cuda")
    src[src_pad:src_pad + len(framed)] = torch.frombuffer(bytearray(framed), dtype=torch.uint8).cuda()
    buf = torch.full((GUARD + dst_pad + total + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    lo = GUARD + dst_pad
    dst = buf[lo:lo + total]
    try:
        orc_amd.lz4_decompress_device(ctx, src[src_pad:src_pad + len(framed)], table, dst)
        err = None
    except orc_amd.ParseError as e:
        err = (ctx.last_error_value(), str(e))
    host = buf.cpu().numpy()
    return host[lo:lo + total].tobytes(), np.concatenate([host[:lo], host[lo + total:]]), table, err


def hand_table(chunks):
    """The table of (body, stored, dst_bytes) chunks framed one after another."""
    rows, src, dst = [], 0, 0
    for body, stored, dst_bytes in chunks:
        rows.append((src + 3, len(body), dst, dst_bytes, M.STORED if stored else 0))
        src += 3 + len(body)
        dst += dst_bytes
    return np.array(rows, dtype=np.uint64).reshape(-1, 5)


@pytest.fixture(scope="module")
def expected():
    """name -> the model's bytes of every good case, computed once."""
    return {name: b"".join(bytes(b) if st else M.decode(b, C.BLOCK) for b, st in chunks)
            for name, chunks in GOOD.items()}


@pytest.mark.parametrize("name", sorted(GOOD))
def test_matches_model(ctx, expected, name):
    want = expected[name]
    got, guard, table, err = inflate(ctx, GOOD[name])
    assert err is None
    assert len(got) == len(want) == int(table[:, 3].sum())
    assert got == want
    assert (guard == SENTINEL).all()


@pytest.mark.parametrize("name", ["sizes", "stored_mixed", "offsets_len_65"])
def test_every_alignment(ctx, expected, name):
    chunks, want = GOOD[name], expected[name]
    if name.startswith("offsets"):
        chunks = chunks[:16]  # the offsets below 4,095: the overlap shapes
        want = b"".join(M.decode(b, C.BLOCK) for b, _ in chunks)
    for a in range(16):
        got, guard, _, err = inflate(ctx, chunks, src_pad=a, dst_pad=(a * 7 + 3) % 16)
        assert err is None and got == want, a
        assert (guard == SENTINEL).all(), a
        got, guard, _, err = inflate(ctx, chunks, src_pad=5, dst_pad=a)
        assert err is None and got == want, a
        assert (guard == SENTINEL).all(), a


@pytest.mark.parametrize("name", sorted(BAD))
def test_crafted_errors(ctx, expected, name):
    chunks, index = BAD[name]
    # the model first: this chunk is the first that fails
    results = [bytes(b) if st else M.decode_exact(b, dst) for b, st, dst in chunks]
    assert [i for i, d in enumerate(results) if d == M.CORRUPT][0] == index
    table = hand_table(chunks)
    got, guard, _, err = inflate(ctx, chunks, src_pad=3, dst_pad=9, table=table)
    assert err == (index, M.CORRUPT)
    assert (guard == SENTINEL).all()
    # the sound chunks of the launch are whole: a failing chunk writes inside its own range only
    for row, d in zip(table, results):
        if d != M.CORRUPT:
            assert got[int(row[2]):int(row[2] + row[3])] == d
    # the context is usable afterwards
    got, guard, _, err = inflate(ctx, GOOD["chunks_2"])
    assert err is None and got == expected["chunks_2"]


def test_table_outside_the_buffers_is_refused(ctx):
    import torch

    framed = M.frame(M.Stream(1).literal(40).match(8, 3).literal(C.END).block())
    table, total = orc_amd.lz4_plan(framed, C.BLOCK)
    assert total == 60
    src = torch.frombuffer(bytearray(framed), dtype=torch.uint8).cuda()
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    for col, delta in ((0, 1), (1, 1), (2, 1), (3, 1), (1, 1 << 31), (3, 1 << 31)):
        t = table.copy()
        t[0, col] += np.uint64(delta)
        with pytest.raises(orc_amd.InvalidArgument):
            orc_amd.lz4_decompress_device(ctx, src, t, dst)
    assert (dst.cpu().numpy() == SENTINEL).all()
    # a destination length below the block's: nothing is written past it
    t = table.copy()
    t[0, 3] -= np.uint64(1)
    with pytest.raises(orc_amd.ParseError) as e:
        orc_amd.lz4_decompress_device(ctx, src, t, dst)
    assert str(e.value) == M.CORRUPT
    assert dst.cpu().numpy()[-1] == SENTINEL
