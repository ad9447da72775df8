"""CPU-only: the decode of ONE LZ4 frame is the decode of a batch of one (both run the same round kernels, sizes step, pack layout,
checksum verdicts and item record: lz4net_amd/csrc/lz4hip_lz4f.hpp), compared emulator against emulator; and every scratch query of
the paths that share the round loop of lz4hip_framing.hpp returns a recorded value."""
import itertools

import pytest

import lz4f_batch_cases as batch
import lz4f_cases as one
import lz4f_ref as ref
from emu_lib import E_ARGUMENT, GRIDS, I32, I64

SLOT, MAX_BLOCKS = 65536, 8


def decode_one(oracle, frame, round_blocks, verify, grid):
    """the one-frame emulator call -> (record, the whole output buffer)"""
    want, _, _, rows = ref.read_frame(oracle, frame, SLOT, MAX_BLOCKS, verify)
    rec, dst, _ = one.run_frame(one.PLAIN, frame, rows, b"", 0, SLOT, MAX_BLOCKS, round_blocks, verify, want["decoded_bytes"], grid)
    return rec, dst.tobytes()


def decode_batch_of_one(oracle, frame, round_blocks, verify, grid):
    """the batch emulator call with n = 1 -> (the item's record, the whole output buffer)"""
    want, _, _, rows = ref.read_frame(oracle, frame, SLOT, MAX_BLOCKS, verify)
    _, recs, _, dst, _, _ = one.run_batch(one.PLAIN, [frame], rows, b"", 0, SLOT, MAX_BLOCKS, round_blocks, verify, want["decoded_bytes"], grid)
    return recs[0], dst.tobytes()


# ---- 1. one frame = a batch of one ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("verify", [0, 3])
@pytest.mark.parametrize("round_blocks", [0, 1, 3])        # 1 and 3: rounds end inside the frame
def test_one_frame_is_the_batch_of_one(oracle, round_blocks, verify, grid):
    good, _, faults = batch.outcome_items(oracle)
    for name, frame in [("good", good)] + [(name, bad) for name, bad, _ in faults]:
        rec1, out1 = decode_one(oracle, frame, round_blocks, verify, grid)
        recn, outn = decode_batch_of_one(oracle, frame, round_blocks, verify, grid)
        assert rec1 == recn, (name, {f: (rec1[f], recn[f]) for f in one.INFO_FIELDS if rec1[f] != recn[f]})
        assert out1 == outn, (name, "the output bytes differ")
        if name == "good":
            assert rec1["error"] == ref.OK and rec1["decoded_bytes"] == len(out1) > 4 * 65536


# ---- 2. the scratch queries return what they returned before the round loop had one owner ----------------------------------------------
# Recorded from the library's size entry points under the emulator at the commit before the loop was unified (512c820); pieces are
# 256-aligned sums, so the carving order may change and these totals may not.
NS, MAXES, ROUNDS, SLOTS = (0, 1, 5), (1, 7, 300), (0, 1, 4), (65536, 4194304)


def _table(args, values):
    """the recorded values, in the order itertools.product yields the arguments"""
    args = list(args)
    assert len(args) == len(values)
    return dict(zip(args, values))


# (slot_bytes, max_blocks, round_blocks)
LZ4F = _table(itertools.product(SLOTS, MAXES, ROUNDS), (
    69632, 69632, 69632, 462848, 69632, 266240, 19681280, 82944, 279552, 4198400, 4198400, 4198400, 29364224, 4198400, 16781312, 1258311680,
    4211712, 16794624))
# (n, slot_bytes, max_blocks, round_blocks)
LZ4F_BATCH = _table(itertools.product(NS, SLOTS, MAXES, ROUNDS), (
    69888, 69888, 69888, 463104, 69888, 266496, 19682560, 84224, 280832, 4198656, 4198656, 4198656, 29364480, 4198656, 16781568, 1258312960,
    4212992, 16795904, 71936, 71936, 71936, 465152, 71936, 268544, 19684608, 86272, 282880, 4200704, 4200704, 4200704, 29366528, 4200704,
    16783616, 1258315008, 4215040, 16797952, 72192, 72192, 72192, 465408, 72192, 268800, 19684864, 86528, 283136, 4200960, 4200960, 4200960,
    29366784, 4200960, 16783872, 1258315264, 4215296, 16798208))
# (n_blocks, slot_bytes, round_blocks): the packed encode's and the compact decode's alike
PACKED = _table(itertools.product(NS + MAXES[1:], SLOTS, ROUNDS), (
    0, 0, 0, 0, 0, 0, 66816, 66816, 66816, 4195584, 4195584, 4195584, 328960, 66816, 263424, 20972800, 4195584, 16778496, 460032, 66816,
    263424, 29361408, 4195584, 16778496, 19665152, 66816, 263424, 1258295552, 4195584, 16778496))
# (chunk_size, max_chunks, round_chunks)
FRAME_COMPACT = _table(itertools.product(SLOTS, (0,) + MAXES, ROUNDS), (
    768, 768, 768, 68864, 68864, 68864, 462080, 68864, 265472, 19677184, 78848, 275456, 768, 768, 768, 4197632, 4197632, 4197632, 29363456,
    4197632, 16780544, 1258307584, 4207616, 16790528))


def _framing():
    L = one.emu()
    for f, args in (("emu_packed_scratch_bytes", [I64, I32, I64]), ("emu_compact_scratch_bytes", [I64, I32, I64]), ("emu_frame_compact_scratch_bytes", [I32, I64, I64])):
        getattr(L, f).argtypes, getattr(L, f).restype = args, I64
    return L


def test_lz4f_decode_scratch_bytes_are_the_recorded_ones():
    L = _framing()
    for (slot, m, r), want in LZ4F.items():
        assert L.emu_lz4f_decode_scratch_bytes(slot, m, r) == want, (slot, m, r)
    assert L.emu_lz4f_decode_scratch_bytes(SLOT, 0, 0) == E_ARGUMENT


def test_lz4f_batch_decode_scratch_bytes_are_the_recorded_ones():
    L = one.emu()
    for (n, slot, m, r), want in LZ4F_BATCH.items():
        assert L.emu_lz4f_batch_decode_scratch_bytes(n, slot, m, r) == want, (n, slot, m, r)
    assert L.emu_lz4f_batch_decode_scratch_bytes(-1, SLOT, 1, 0) == E_ARGUMENT


def test_packed_and_compact_scratch_bytes_are_the_recorded_ones():
    L = _framing()
    for (n, slot, r), want in PACKED.items():
        assert L.emu_packed_scratch_bytes(n, slot, r) == want, (n, slot, r)
        assert L.emu_compact_scratch_bytes(n, slot, r) == want, (n, slot, r)
    for (chunk, m, r), want in FRAME_COMPACT.items():
        assert L.emu_frame_compact_scratch_bytes(chunk, m, r) == want, (chunk, m, r)
