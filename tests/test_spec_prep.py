"""The inputs of a verify step (csrc/ext_decode.hip `mrs_spec_verify_prep`, `spec_prep_kernel`) against a plain numpy restatement, for EQUALITY: the anchor id, the rows'
positions, context lengths and slots, and the verify-only copy of the sequence's block-table row -- at sequences other than 0, at tables longer than one trip of the copy
loop (256 entries), across a block edge and past the end of the table; and `mrs_spec_advance` held to the same slot arithmetic: the slot it leaves after n accepted drafts
is the slot the prep computed for row n + 1 of that round.
Every body takes a backend of tests/abi_backends.py: the host emulation in the CPU suite, the MI355X under `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

VP, I = C.c_void_p, C.c_int
NSEQ = 5
KEEP = -77            # what the signed outputs hold before a launch (-1 is an answer of the kernel: not a sentinel)
KEEP_U = 0x0BADF00D   # ... and the unsigned ones; no block-table entry below has this value
ENTRY0 = 1 << 27      # block ids start here: entry * block_size passes 2^31 (block 16) and 2^32 (block 32), so a slot computed in 32 bits shows


def _state(max_blocks, block_size, seq, p):
    """a 5-sequence decode state whose input_ids / positions entries all differ and whose block-table entries are all distinct and not ascending"""
    rng = np.random.default_rng(1000 * max_blocks + block_size)
    bt = (ENTRY0 + rng.permutation(NSEQ * max_blocks)).astype(np.uint32).reshape(NSEQ, max_blocks)
    assert np.unique(bt).size == bt.size and not np.any(bt == KEEP_U) and (max_blocks == 1 or np.any(np.diff(bt.astype(np.int64), axis=1) < 0))
    ids = (300 + 11 * np.arange(NSEQ)).astype(np.int32)
    pos = (1000 + 17 * np.arange(NSEQ)).astype(np.int32)
    pos[seq] = p
    assert np.unique(pos).size == NSEQ
    return ids, pos, bt


def _slot(bt_row, pos, block_size):
    blk = pos // block_size
    return int(bt_row[blk]) * block_size + pos % block_size if blk < bt_row.size else -1


def run_prep(be, ids, pos, bt, seq, n_rows, max_blocks, block_size):
    """one launch over sentinel-filled outputs: (rc, inputs after the launch, outputs)"""
    ib, pb, tb = be.buf(ids), be.buf(pos), be.buf(bt)
    o_ids, o_pos, o_ctx = be.buf(np.full(9, KEEP, np.int32)), be.buf(np.full(8, KEEP, np.int32)), be.buf(np.full(8, KEEP_U, np.uint32))
    o_slots, o_tab = be.buf(np.full(8, KEEP, np.int64)), be.buf(np.full((8, bt.shape[1]), KEEP_U, np.uint32))
    rc = be.sym("mrs_spec_verify_prep", [VP, VP, VP, I, I, I, I, VP, VP, VP, VP, VP, VP], I)(
        ib.ptr, pb.ptr, tb.ptr, seq, n_rows, max_blocks, block_size, o_ids.ptr, o_pos.ptr, o_ctx.ptr, o_slots.ptr, o_tab.ptr, be.stream or None)
    u32 = lambda b: b.numpy().view(np.uint32)
    return rc, (ib.numpy(), pb.numpy(), u32(tb)), dict(ids=o_ids.numpy(), pos=o_pos.numpy(), ctx=u32(o_ctx), slots=o_slots.numpy(), tables=u32(o_tab))


# (seq, n_rows, anchor position, max_blocks, block_size)
CASES = [
    (0, 1, 0, 1, 32),                  # the smallest launch
    (4, 2, 31, 1, 32),                 # a one-entry table: the second row is past it
    (2, 4, 29, 6, 32),                 # rows 29 .. 32 straddle the block edge
    (4, 8, 29, 6, 32),                 # the last sequence, all eight rows, the same edge
    (2, 4, 13, 6, 16),                 # ... and the edge of a 16-token block
    (0, 2, 0, 6, 16),
    (4, 8, 6 * 32 - 3, 6, 32),         # rows 0 .. 2 in the last block, rows 3 .. 7 past the table
    (1, 4, 6 * 16, 6, 16),             # the anchor is the first position past the table
    (3, 2, 6 * 32 + 40, 6, 32),        # ... and one a block further out
    (4, 8, 0, 256, 32),                # exactly one trip of the copy loop
    (2, 8, 256 * 16 - 2, 256, 16),
    (4, 8, 257 * 32 - 5, 257, 32),     # a second trip of one entry; rows 0 .. 4 read that entry (block 256)
    (2, 1, 256 * 16 + 3, 257, 16),
    (2, 4, 599 * 16 + 13, 600, 16),    # a third, partial trip (600 = 256 + 256 + 88); rows 0 .. 2 read the last entry
    (0, 2, 300 * 32 + 31, 600, 32),    # an entry of the second trip on both sides of a block edge
]


def check_prep(be, seq, n_rows, p, max_blocks, block_size):
    ids, pos, bt = _state(max_blocks, block_size, seq, p)
    rc, (ids2, pos2, bt2), out = run_prep(be, ids, pos, bt, seq, n_rows, max_blocks, block_size)
    assert rc == 0
    assert np.array_equal(ids2, ids) and np.array_equal(pos2, pos) and np.array_equal(bt2, bt), "the prep wrote to its inputs"
    assert out["ids"].tolist() == [int(ids[seq])] + [KEEP] * 8, out["ids"]
    rows = np.arange(n_rows)
    assert out["pos"].tolist() == (p + rows).tolist() + [KEEP] * (8 - n_rows), out["pos"]
    assert out["ctx"].tolist() == (p + rows + 1).tolist() + [KEEP_U] * (8 - n_rows), out["ctx"]
    want = [_slot(bt[seq], p + r, block_size) for r in range(n_rows)]
    assert out["slots"].tolist() == want + [KEEP] * (8 - n_rows), (out["slots"], want)
    for r in range(8):
        bad = np.nonzero(out["tables"][r] != (bt[seq] if r < n_rows else KEEP_U))[0]
        assert bad.size == 0, f"verify table row {r}: {bad.size} entries differ, the first at column {bad[0]}"
    return want


def check_prep_cases_are_what_they_claim():
    """the case list itself: every value of the issue's axes occurs, in range and past the table"""
    assert {c[0] for c in CASES} >= {0, 2, 4} and {c[1] for c in CASES} == {1, 2, 4, 8}
    assert {c[3] for c in CASES} == {1, 6, 256, 257, 600} and {c[4] for c in CASES} == {16, 32}
    past = [(p + n - 1) // bs >= mb for _, n, p, mb, bs in CASES]
    anchor_past = [p // bs >= mb for _, n, p, mb, bs in CASES]
    assert any(a for a in anchor_past) and any(l and not a for l, a in zip(past, anchor_past)) and not all(past)
    assert {c[0] for c, l in zip(CASES, past) if l} >= {1, 3, 4}  # past the table: middle sequences and the last one (the row after theirs is another sequence's, or none)


def check_prep_refusals(be):
    ids, pos, bt = _state(6, 32, 2, 29)
    for seq, n_rows, max_blocks, block_size in ((-1, 4, 6, 32), (2, 0, 6, 32), (2, 9, 6, 32), (2, 4, 0, 32), (2, 4, 6, 0), (2, 4, -1, 32), (2, 4, 6, -32)):
        rc, (ids2, pos2, bt2), out = run_prep(be, ids, pos, bt, seq, n_rows, max_blocks, block_size)
        assert rc == -1, (seq, n_rows, max_blocks, block_size)
        assert np.array_equal(ids2, ids) and np.array_equal(pos2, pos) and np.array_equal(bt2, bt)
        assert np.all(out["ids"] == KEEP) and np.all(out["pos"] == KEEP) and np.all(out["slots"] == KEEP) and np.all(out["ctx"] == KEEP_U) and np.all(out["tables"] == KEEP_U)


# (seq, anchor position, max_blocks, block_size): eight rows each -- across a block edge, running off the table, wholly past it
ADVANCE_CASES = [(2, 29, 6, 32), (4, 13, 6, 16), (3, 6 * 32 - 3, 6, 32), (1, 257 * 16 - 5, 257, 16), (0, 6 * 32 + 1, 6, 32)]


def check_prep_feeds_advance(be, seq, p, max_blocks, block_size):
    """after a round with n accepted drafts the sequence sits at row n + 1 of that round: `mrs_spec_advance` must leave the position, context length and slot that the
    prep computed for that row, for every n in 0..6 -- the two kernels restate the slot arithmetic separately"""
    ids, pos, bt = _state(max_blocks, block_size, seq, p)
    rc, _, prep = run_prep(be, ids, pos, bt, seq, 8, max_blocks, block_size)
    assert rc == 0 and prep["slots"].tolist() == [_slot(bt[seq], p + r, block_size) for r in range(8)]
    toks = (40 + np.arange(8)).astype(np.int32)
    ctx0, slots0 = (pos + 1).astype(np.uint32), (7000 + np.arange(NSEQ)).astype(np.int64)
    adv = be.sym("mrs_spec_advance", [VP, VP, I, VP, VP, I, VP, VP, VP, VP, VP, I, I, VP], I)
    for n in range(7):
        ib, tout, step = be.buf(ids), be.buf(np.full((NSEQ, 16), KEEP, np.int32)), be.buf(np.array([3], np.int32))
        pb, cb, sb, tb = be.buf(pos), be.buf(ctx0), be.buf(slots0), be.buf(bt)
        nb, kb = be.buf(np.array([n], np.int32)), be.buf(toks)
        assert adv(nb.ptr, kb.ptr, seq, ib.ptr, tout.ptr, 16, step.ptr, pb.ptr, cb.ptr, sb.ptr, tb.ptr, max_blocks, block_size, be.stream or None) == 0
        got_pos, got_ctx, got_slots = pb.numpy(), cb.numpy().view(np.uint32), sb.numpy()
        assert got_slots[seq] == prep["slots"][n + 1], (n, got_slots[seq], prep["slots"][n + 1])
        assert got_pos[seq] == prep["pos"][n + 1] and got_ctx[seq] == prep["ctx"][n + 1]
        others = np.arange(NSEQ) != seq
        assert np.array_equal(got_pos[others], pos[others]) and np.array_equal(got_ctx[others], ctx0[others]) and np.array_equal(got_slots[others], slots0[others])
        want_ids = ids.copy()
        want_ids[seq] = toks[n]
        assert np.array_equal(ib.numpy(), want_ids) and int(step.numpy()[0]) == 3 + n + 1
        t = tout.numpy().reshape(NSEQ, 16)
        assert t[seq, 3:4 + n].tolist() == toks[:n + 1].tolist() and np.all(t[seq, 4 + n:] == KEEP) and np.all(t[seq, :3] == KEEP) and np.all(t[others] == KEEP)
        assert np.array_equal(tb.numpy().view(np.uint32), bt)


# ---------------------------------------------------------------- the two backends
@pytest.fixture(scope="module")
def host():
    from tests.abi_backends import HostBackend
    return HostBackend()


@pytest.fixture(scope="module")
def gpu(dev):
    from tests.abi_backends import GpuBackend
    return GpuBackend(dev)


_ids = lambda cases: ["-".join(str(v) for v in c) for c in cases]


def test_prep_case_list():
    check_prep_cases_are_what_they_claim()


@pytest.mark.parametrize("seq,n_rows,p,max_blocks,block_size", CASES, ids=_ids(CASES))
def test_prep_host_emulation(host, seq, n_rows, p, max_blocks, block_size):
    check_prep(host, seq, n_rows, p, max_blocks, block_size)


def test_prep_refusals_host_emulation(host):
    check_prep_refusals(host)


@pytest.mark.parametrize("seq,p,max_blocks,block_size", ADVANCE_CASES, ids=_ids(ADVANCE_CASES))
def test_prep_feeds_advance_host_emulation(host, seq, p, max_blocks, block_size):
    check_prep_feeds_advance(host, seq, p, max_blocks, block_size)


@pytest.mark.gpu
@pytest.mark.parametrize("seq,n_rows,p,max_blocks,block_size", CASES, ids=_ids(CASES))
def test_prep_gpu(gpu, seq, n_rows, p, max_blocks, block_size):
    check_prep(gpu, seq, n_rows, p, max_blocks, block_size)


@pytest.mark.gpu
def test_prep_refusals_gpu(gpu):
    check_prep_refusals(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("seq,p,max_blocks,block_size", ADVANCE_CASES, ids=_ids(ADVANCE_CASES))
def test_prep_feeds_advance_gpu(gpu, seq, p, max_blocks, block_size):
    check_prep_feeds_advance(gpu, seq, p, max_blocks, block_size)
