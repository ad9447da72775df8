"""CPU-only: batches of LZ4 frames (lz4net_amd/csrc/lz4hip_lz4f_batch.hpp and its host code in lz4hip_framing.hpp) under the SIMT
emulator (tests/simt/emu_lz4f_batch.inc): the real kernels, the library's fronts, launch sequences and host-pointer calls, with the
block codec replaced by results and bytes computed here with the oracle.  The reference is the one-frame path: the frame the one-frame
emulator path writes for every item alone, and the from-the-spec twin reader (tests/lz4f_ref.py) on every item alone."""
import ctypes as C

import numpy as np
import pytest

import lz4f_lib
import lz4f_ref as ref
from emu_lib import E_ARGUMENT, GRIDS, Guarded, u8
from lz4f_batch_cases import emu_encode_batch, frames_alone, golden_batch, outcome_items, sources, tiny_items
from lz4f_cases import PLAIN, BatchRun as EmuRun, check_batch, emu, expect, offsets_of, sample, standin
from lz4net_amd._lib import Lz4fBatchInfo, Lz4fInfo


def with_a_bad_item(items, at):
    """the batch's bytes and offsets with one more item at index `at` whose offsets decrease: the item behind it starts 5 bytes early"""
    src = b"".join(items)
    off = list(offsets_of(items))
    off.insert(at + 1, off[at] - 5)
    return src, np.array(off, np.int64)


# ---- 1. encode identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("hc", [False, True])
@pytest.mark.parametrize("block_id", [4, 5])
@pytest.mark.parametrize("flags", range(8))
def test_encode_is_the_frame_of_every_item_alone(oracle, flags, block_id, hc, grid):
    items = sources(oracle)
    emu_encode_batch(oracle, b"".join(items), offsets_of(items), block_id, hc, flags, grid, want=frames_alone(oracle, items, block_id, hc, flags))


@pytest.mark.parametrize("grid", GRIDS)
def test_encode_an_item_with_decreasing_offsets_takes_no_bytes(oracle, grid):
    items = sources(oracle)
    src, off = with_a_bad_item(items, 4)
    got, got_off = emu_encode_batch(oracle, src, off, 4, False, 7, grid)
    assert got_off[4] == got_off[5], "the bad item"
    assert got[:got_off[4]] == b"".join(frames_alone(oracle, items[:4], 4, False, 7)), "the items before it are the fault-free batch's"


# ---- 2. decode identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("flags", [0, 7])
def test_decode_is_the_decode_of_every_item_alone(oracle, flags, grid):
    items = sources(oracle)
    frames = frames_alone(oracle, items, 4, False, flags)
    for verify in (3, 0):
        recs, outs, info = check_batch(PLAIN, oracle, frames, slot=65536, verify=verify, grid=grid)
        assert outs == items and info["error"] == ref.OK and all(r["frame_bytes"] == len(f) for r, f in zip(recs, frames))


# ---- 3. every outcome once, all in one batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_every_outcome_in_one_batch(oracle, grid):
    good, src, faults = outcome_items(oracle)
    items = [good]
    for _, bad, _ in faults:
        items += [bad, good]
    items += frames_alone(oracle, sources(oracle)[2:4], 4, False, 7)
    recs, outs, info = check_batch(PLAIN, oracle, items, slot=65536, round_blocks=3, grid=grid)
    assert [r["error"] for r in recs] == [ref.OK] + [c for _, _, code in faults for c in (code, ref.OK)] + [ref.OK, ref.OK]
    assert info["first_error"] == 1 and info["error"] == ref.BAD_MAGIC, "the lowest failing item, as a sequential loop raises it"
    # the neighbours are byte-identical to the fault-free batch's
    assert all(outs[k] == src for k in range(0, 2 * len(faults) + 1, 2))
    # precedence with two faults in one item: the lowest bad block over the content checksum and over the walk's error
    by_name = {name: recs[2 * k + 1] for k, (name, _, _) in enumerate(faults)}
    assert by_name["sum_and_content"]["error"] == ref.BLOCK_CHECKSUM and by_name["sum_and_cut"]["error"] == ref.BLOCK_CHECKSUM
    assert by_name["sum_and_cut"]["error_offset"] == by_name["block_sum"]["error_offset"]
    # unverified, the flipped byte is the decoder's to find
    recs, _, _ = check_batch(PLAIN, oracle, items, slot=65536, verify=2, grid=grid)
    assert recs[2 * [name for name, _, _ in faults].index("block_sum") + 1]["error"] == ref.CORRUPT_BLOCK


@pytest.mark.parametrize("grid", GRIDS)
def test_decode_an_item_with_bad_offsets(oracle, grid):
    frames = frames_alone(oracle, sources(oracle)[1:4], 4, False, 7)
    blob, off = with_a_bad_item(frames, 1)
    recs, outs, info = check_batch(PLAIN, oracle, blob, off=off, slot=65536, grid=grid)
    assert recs[1]["error"] == E_ARGUMENT and outs[1] == b"" and recs[0]["error"] == ref.OK and info["first_error"] == 1
    off = offsets_of(frames)
    off[3] += 1                                                         # the last item leaves the buffer
    recs, outs, info = check_batch(PLAIN, oracle, b"".join(frames), off=off, slot=65536, grid=grid)
    assert [r["error"] for r in recs] == [ref.OK, ref.OK, E_ARGUMENT] and info["first_error"] == 2 and info["error"] == E_ARGUMENT


# ---- 4. table, rounds, slots and clipping -------------------------------------------------------------------------------------------------
def mixed_batch(oracle):
    items = sources(oracle)
    return frames_alone(oracle, items, 4, False, 7) + frames_alone(oracle, items[3:], 5, True, 3), items + items[3:]


@pytest.mark.parametrize("grid", GRIDS)
def test_table_exact_and_one_row_short(oracle, grid):
    frames, items = mixed_batch(oracle)
    blob, off = b"".join(frames), offsets_of(frames)
    rows = len(expect(oracle, frames, 262144, 3)[2])
    assert rows == 1 + 1 + 1 + 1 + 2 + 4 + 1 + 1 + 1 + 1
    _, outs, info = check_batch(PLAIN, oracle, blob, off=off, slot=262144, max_blocks=rows, grid=grid)
    assert outs == items and info["blocks"] == rows and info["error"] == ref.OK
    _, _, info = check_batch(PLAIN, oracle, blob, off=off, slot=262144, max_blocks=rows - 1, grid=grid)
    assert info["error"] == ref.TABLE_FULL and info["blocks"] == rows, "the count needed"


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("round_blocks", [1, 2])
def test_rounds_that_start_inside_an_item(oracle, round_blocks, grid):
    frames, items = mixed_batch(oracle)
    _, outs, info = check_batch(PLAIN, oracle, frames, slot=262144, max_blocks=17, round_blocks=round_blocks, grid=grid)
    assert outs == items and info["error"] == ref.OK


@pytest.mark.parametrize("grid", GRIDS)
def test_block_ids_together_and_a_slot_too_small_for_one_item(oracle, grid):
    frames, items = mixed_batch(oracle)
    big = frames_alone(oracle, [items[5]], 6, False, 7)
    frames, items = frames[:3] + big + frames[3:], items[:3] + [b""] + items[3:]
    recs, outs, info = check_batch(PLAIN, oracle, frames, slot=262144, grid=grid)
    assert [r["error"] for r in recs] == [ref.OK] * 3 + [ref.SLOT_TOO_SMALL] + [ref.OK] * (len(recs) - 4)
    assert outs == items and info["first_error"] == 3 and recs[3]["block_max"] == 1 << 20
    assert {r["block_max"] for r in recs} == {65536, 262144, 1 << 20}


@pytest.mark.parametrize("grid", GRIDS)
def test_clipping_by_position(oracle, grid):
    frames, items = mixed_batch(oracle)
    blob, off = b"".join(frames), offsets_of(frames)
    ends = offsets_of(items)
    for cap in (0, int(ends[5]), int(ends[5]) - 1, int(ends[6]) + 70000):
        recs, _, info = check_batch(PLAIN, oracle, blob, off=off, slot=262144, round_blocks=2, dst_cap=cap, grid=grid)
        assert info["decoded_bytes"] == ends[-1] and info["error"] == ref.OK
        for i, r in enumerate(recs):
            assert (r["checks"] >> 2) == (ref.VERIFIED if ends[i + 1] <= cap else ref.SKIPPED), (cap, i)


# ---- 5. boundaries of the shared steps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 64, 65])
def test_item_counts_around_the_checksum_kernel_s_rows(oracle, n):
    """sixteen content rows per wavefront, 64 per workgroup"""
    rng = np.random.default_rng(n)
    items = [sample(oracle, 2, int(k)) for k in rng.integers(0, 300, n)]
    src, off = b"".join(items), offsets_of(items)
    for grid in GRIDS:
        got, got_off = emu_encode_batch(oracle, src, off, 4, False, 7, grid)
        recs, outs, _ = check_batch(PLAIN, oracle, got, off=got_off, slot=65536, grid=grid)
        assert outs == items and all((r["checks"] >> 2) == ref.VERIFIED for r in recs)


def test_4100_tiny_items_cross_a_scan_tile(oracle):
    """items, rows and segments each cross a scan tile of 4 096"""
    items = tiny_items()
    assert emu().emu_lz4f_batch_sizeof(100) == 4096 < len(items)
    src, off = b"".join(items), offsets_of(items)
    got, got_off = emu_encode_batch(oracle, src, off, 4, False, 7)
    recs, outs, info = check_batch(PLAIN, oracle, got, off=got_off, slot=65536, round_blocks=4099)
    assert outs == items and info["blocks"] == len(items) and info["error"] == ref.OK
    bad = bytearray(got)
    bad[got_off[4097] + 15 + 4] ^= 0xFF                                 # the first data byte of item 4097's only block
    recs, outs, info = check_batch(PLAIN, oracle, bytes(bad), off=got_off, slot=65536)
    assert info["first_error"] == 4097 and info["error"] == ref.BLOCK_CHECKSUM and [i for i, r in enumerate(recs) if r["error"]] == [4097]


# ---- 6. other formats of item ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_skippable_trailing_bytes_empty_item_and_no_item(oracle, grid):
    src = sample(oracle, 3, 70000)
    frame = frames_alone(oracle, [src], 4, False, 7)[0]
    items = [frame, ref.skippable(b"user data", 3), frame + frame[:40], b"", frame]
    recs, outs, info = check_batch(PLAIN, oracle, items, slot=65536, grid=grid)
    assert [r["error"] for r in recs] == [ref.OK, ref.OK, ref.OK, ref.BAD_MAGIC, ref.OK] and info["first_error"] == 3
    assert recs[1]["kind"] == 1 and recs[1]["frame_bytes"] == 17 and outs[1] == b""
    assert recs[2]["frame_bytes"] == len(frame) and outs[2] == src, "what lies behind the frame is left alone"
    _, _, info = check_batch(PLAIN, oracle, b"", off=np.zeros(1, np.int64), slot=65536, grid=grid)
    assert info == dict(items=0, blocks=0, decoded_bytes=0, first_error=-1, error_offset=-1, error=0, reserved=0)
    got, got_off = emu_encode_batch(oracle, b"", np.zeros(1, np.int64), grid=grid)
    assert got == b"" and list(got_off) == [0]
    # a batch of empty items alone: n frames of a descriptor and an EndMark
    emu_encode_batch(oracle, b"", np.zeros(4, np.int64), 4, False, 7, grid, want=frames_alone(oracle, [b""] * 3, 4, False, 7))


# ---- 7. liblz4's frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_golden_frames_as_one_batch(oracle, grid):
    names, recs_json, frames, srcs = golden_batch(oracle)
    recs, outs, info = check_batch(PLAIN, oracle, frames, slot=0, round_blocks=5, grid=grid)
    for name, j, r, out, src in zip(names, recs_json, recs, outs, srcs):
        if j["linked"]:
            assert r["error"] == ref.UNSUPPORTED_LINKED and out == b"", name
        elif j["skippable_bytes"]:
            assert r["kind"] == 1 and r["error"] == ref.OK and out == b"", name
        else:
            assert r["error"] == ref.OK and out == src, name
    assert info["first_error"] == names.index("linked") and info["error"] == ref.UNSUPPORTED_LINKED


@pytest.mark.skipif(lz4f_lib.load() is None, reason="liblz4 >= 1.8.0 is not installed")
def test_liblz4_reads_every_frame_of_an_encoded_batch(oracle):
    items = sources(oracle)
    for flags, hc in ((0, False), (7, True)):
        got, off = emu_encode_batch(oracle, b"".join(items), offsets_of(items), 4, hc, flags)
        for i, src in enumerate(items):
            frame = got[off[i]:off[i + 1]]
            out, used, err = lz4f_lib.decompress(frame, len(src))
            assert err is None and out == src and used == len(frame), (i, err)


# ---- 8. the host-pointer calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_host_pointer_calls(oracle, grid):
    L = emu()
    items = sources(oracle)
    src, off = b"".join(items), offsets_of(items)
    device, device_off = emu_encode_batch(oracle, src, off, 4, False, 7, grid)
    staged, staged_off = emu_encode_batch(oracle, src, off, 4, False, 7, grid, host=True)
    assert staged == device and list(staged_off) == list(device_off), "the same bytes as the device front"
    recs, outs, rows, ends, _ = expect(oracle, [staged[a:b] for a, b in zip(staged_off[:-1], staged_off[1:])], 65536, 3)
    n = len(items)
    table = len(staged) // 4096 + n + 16
    arrs = standin(rows, table)
    run = EmuRun(dec_results=arrs[0].ctypes.data, dec_len=arrs[1].ctypes.data, dec_at=arrs[2].ctypes.data, dec_bytes=arrs[3].ctypes.data, dec_rows=table, grid=grid)
    a = u8(staged)
    dst_off, item_info, info = np.full(n + 1, -1, np.int64), (Lz4fInfo * n)(), Lz4fBatchInfo()
    # a size query, then the decode into exactly that size
    assert L.emu_lz4f_batch_decode_host(a.ctypes.data, a.size, staged_off.ctypes.data, n, 3, None, 0, dst_off.ctypes.data, item_info, C.byref(info),
                                        C.byref(run)) == E_ARGUMENT
    assert info.decoded_bytes == len(src) and list(dst_off) == list(ends) and run.intact == 1
    out = Guarded(len(src))
    assert L.emu_lz4f_batch_decode_host(a.ctypes.data, a.size, staged_off.ctypes.data, n, 3, out.ptr, len(src), dst_off.ctypes.data, item_info, C.byref(info),
                                        C.byref(run)) == 0, run.error
    assert out.a.tobytes() == src and out.intact() and run.shape_errors == 0 and list(dst_off) == list(ends)
    assert run.intact == 1 and run.reserves == 1 and run.moves == 1 and run.passes == 1, "one staged image, one pass"
    for g, w in zip(item_info, recs):
        assert {f: int(getattr(g, f)) for f in w} == w
    assert (info.items, info.blocks, info.first_error, info.error) == (n, len(rows), -1, 0)
    # the first failing item's code is the call's
    bad = bytearray(staged)
    bad[staged_off[3] - 1] ^= 1                                         # item 2's content checksum
    b = u8(bad)
    assert L.emu_lz4f_batch_decode_host(b.ctypes.data, b.size, staged_off.ctypes.data, n, 3, out.ptr, len(src), dst_off.ctypes.data, item_info, C.byref(info),
                                        C.byref(run)) == ref.CONTENT_CHECKSUM
    assert info.first_error == 2 and item_info[2].error == ref.CONTENT_CHECKSUM and out.a.tobytes() == src
    # offsets in host memory are checked, not decoded as empty items
    wrong = staged_off.copy()
    wrong[2] = wrong[3] + 1
    assert L.emu_lz4f_batch_decode_host(a.ctypes.data, a.size, wrong.ctypes.data, n, 3, out.ptr, len(src), dst_off.ctypes.data, item_info, C.byref(info),
                                        C.byref(run)) == E_ARGUMENT


def test_front_arguments():
    L = emu()
    assert L.emu_lz4f_batch_bound(2, 10, 3, 0) == E_ARGUMENT and L.emu_lz4f_batch_bound(2, 10, 4, 8) == E_ARGUMENT
    assert L.emu_lz4f_batch_bound(2, 10, 0, 7) == 2 * (15 + 4 + 4) + 10 + 2 * 8
    assert L.emu_lz4f_batch_decode_scratch_bytes(2, 65535, 4, 0) == E_ARGUMENT and L.emu_lz4f_batch_decode_scratch_bytes(2, 65536, 0, 0) == E_ARGUMENT
    a, off, dst, doff, scratch, run = np.zeros(64, np.uint8), np.array([0, 10, 20], np.int64), np.zeros(512, np.uint8), np.zeros(3, np.int64), np.zeros(1 << 20, np.uint8), EmuRun()
    ok = [a.ctypes.data, 20, off.ctypes.data, 2, 4, 0, 0, dst.ctypes.data, 512, doff.ctypes.data, scratch.ctypes.data, scratch.size]
    for at, bad in ((0, None), (1, -1), (2, None), (3, -1), (4, 3), (5, 2), (6, 8), (7, None), (8, 10), (9, None), (10, None), (11, 16)):
        args = list(ok)
        args[at] = bad
        assert L.emu_lz4f_batch_encode(*args, C.byref(run)) == E_ARGUMENT, at
    recs, info, written = (Lz4fInfo * 2)(), Lz4fBatchInfo(), np.zeros(1, np.int64)
    ok = [a.ctypes.data, 20, off.ctypes.data, 2, 65536, 4, 0, 3, scratch.ctypes.data, scratch.size, dst.ctypes.data, 64, doff.ctypes.data, recs, C.byref(info),
          written.ctypes.data]
    for at, bad in ((0, None), (1, -1), (2, None), (3, -1), (4, 1000), (5, 0), (6, -1), (7, 4), (8, None), (9, 100), (10, None), (11, -1), (12, None), (13, None),
                    (14, None), (15, None)):
        args = list(ok)
        args[at] = bad
        assert L.emu_lz4f_batch_decode(*args, C.byref(run)) == E_ARGUMENT, at
