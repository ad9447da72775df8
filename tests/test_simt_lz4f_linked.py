"""CPU-only: the decode of LZ4 frames with linked blocks (LZ4HIP_LZ4F_ACCEPT_LINKED: lz4net_amd/csrc/lz4hip_lz4f_linked.hpp inside the
sequences of lz4hip_framing.hpp) under the SIMT emulator, against the twin tests/lz4f_ref.py field by field, in guarded
buffers.  The size walk, the plan, the rounds and the ordered decode are the library's own kernels and launch sequences; the linked
rows run the real wavefront decoder, the independent rows the stand-in codec (the LINKED path of tests/lz4f_cases.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import lz4f_built as built
import lz4f_cases as cases
import lz4f_ref as ref
from emu_lib import E_ARGUMENT, GRIDS, Guarded, u8
from lz4f_cases import ACCEPT, LINKED, BatchRun as EmuRun, check_image, emu, offsets_of, records_of, standin
from lz4f_linked_cases import golden, hand_built, mixed_batch
from lz4net_amd._lib import Lz4fBatchInfo, Lz4fInfo

check_frame = functools.partial(cases.check_frame, LINKED, accept=True)   # the calls with the flag, on the emulator's linked entry points
check_batch = functools.partial(cases.check_batch, LINKED, accept=True)
expect = functools.partial(cases.expect, accept=True)


@pytest.mark.parametrize("name", sorted(hand_built()))
def test_hand_built_frames_alone_and_behind_another_item(oracle, name):
    frame, content, bad = hand_built()[name]
    rec, out = check_frame(oracle, frame)
    assert (rec["error"] == ref.OK) == (content is not None) and (content is None or out == content)
    check_batch(oracle, [frame])
    recs, _, _ = check_batch(oracle, [built.front_item(), frame])
    assert recs[0]["error"] == ref.OK and recs[1] == rec
    if content is None:                                                # the item in front and the one behind are intact, whatever dst held
        recs, _, got = check_batch(oracle, [built.front_item(), frame, built.front_item()], round_blocks=2)
        assert got["first_error"] == 1 and recs[2]["error"] == ref.OK


def test_a_match_may_not_start_in_another_item_s_bytes(oracle):
    """(a'): the byte in front of the frame's first byte is the last byte of the item before it, and it is not history"""
    frame = hand_built()["a_before_the_frame"][0]
    recs, _, _ = check_batch(oracle, [built.front_item(), frame])
    assert recs[1]["error"] == ref.CORRUPT_BLOCK and recs[1]["good_bytes"] == 1000 and recs[1]["decoded_bytes"] == 1032


def test_a_bad_checksum_ends_the_item_and_the_next_packs_behind(oracle):
    frame = hand_built()["f_bad_checksum"][0]
    recs, _, got = check_batch(oracle, [frame, built.front_item()])
    assert recs[0]["error"] == ref.BLOCK_CHECKSUM and recs[0]["good_bytes"] == recs[0]["decoded_bytes"] == 120 and got["decoded_bytes"] == 120 + len(built.FRONT)
    recs, _, _ = check_batch(oracle, [frame, built.front_item()], verify=0)
    assert recs[0]["error"] == ref.OK and recs[0]["decoded_bytes"] == 234, "unverified, the flipped literal decodes"


@pytest.mark.parametrize("round_blocks", [0, 2])
def test_golden_frames(oracle, round_blocks):
    names, golden_recs, frames, srcs = golden(oracle)
    for rec, frame, src in zip(golden_recs, frames, srcs):
        got, out = check_frame(oracle, frame, slot=ref.block_bytes(rec["block_id"]), round_blocks=round_blocks)
        assert got["error"] == ref.OK and out == src
    recs, _, got = check_batch(oracle, frames, slot=262144, round_blocks=round_blocks)
    assert got["error"] == ref.OK and got["decoded_bytes"] == sum(len(s) for s in srcs)


@pytest.mark.parametrize("verify", [0, 1, 2, 3])
@pytest.mark.parametrize("round_blocks", [0, 2])
def test_mixed_batch(oracle, round_blocks, verify):
    frames, _ = mixed_batch(oracle)
    recs, _, got = check_batch(oracle, frames, round_blocks=round_blocks, verify=verify)
    assert [r["error"] for r in recs] == [0, 0, 0, 0, 0, 0, ref.UNSUPPORTED_DICT] and got["first_error"] == 6
    assert recs[2]["kind"] == 1 and recs[5]["decoded_bytes"] == 0


@pytest.mark.parametrize("grid", GRIDS)
def test_mixed_batch_at_forced_grids(oracle, grid):
    check_batch(oracle, mixed_batch(oracle)[0], round_blocks=2, grid=grid)


def test_mixed_batch_clipped(oracle):
    frames, two = mixed_batch(oracle)
    _, _, _, ends, total = expect(oracle, list(frames), 65536, 3)
    inside_second_block = int(ends[two]) + 50 + 500                    # block 1 of that item has 50 bytes, block 2 has 1 012
    for cap in (0, inside_second_block, total):
        recs, _, _ = check_batch(oracle, frames, dst_cap=cap)
        check_batch(oracle, frames, dst_cap=cap, round_blocks=2)
    assert recs[two]["error"] == ref.OK


def test_a_table_one_row_short_writes_nothing(oracle):
    frames, _ = mixed_batch(oracle)
    rows = expect(oracle, list(frames), 65536, 3)[2]
    _, _, got = check_batch(oracle, frames, max_blocks=len(rows) - 1)
    assert got["error"] == ref.TABLE_FULL and got["blocks"] == len(rows)


def test_the_host_calls(oracle):
    """the staged calls pass the flag through: the batch, a size query, and one frame"""
    L = emu()
    frames, _ = mixed_batch(oracle)
    frames = list(frames)
    recs, outs, rows, ends, total = expect(oracle, frames, 65536, 3)
    src, off = b"".join(frames), offsets_of(frames)
    max_rows = len(src) // 4096 + len(frames) + 16                     # the staged call's own guess of the table
    for cap in (total, 0):
        arrs = standin(rows, max_rows)
        run = EmuRun(dec_results=arrs[0].ctypes.data, dec_len=arrs[1].ctypes.data, dec_at=arrs[2].ctypes.data, dec_bytes=arrs[3].ctypes.data, dec_rows=max_rows)
        a = Guarded(len(src))
        a.a[:] = u8(src)
        dst, dst_off, items = Guarded(cap), Guarded(8 * (len(frames) + 1)), Guarded(C.sizeof(Lz4fInfo) * len(frames))
        info = Lz4fBatchInfo()
        rc = L.emu_lz4f_linked_batch_decode_host(a.ptr, len(src), off.ctypes.data, len(frames), 3 | ACCEPT, dst.ptr, cap, dst_off.ptr, items.ptr, C.byref(info),
                                                 C.byref(run))
        assert rc == (ref.UNSUPPORTED_DICT if cap else E_ARGUMENT), run.error
        assert run.intact == 1 and dst.intact() and dst_off.intact() and items.intact() and a.intact()
        assert list(dst_off.a.view(np.int64)) == list(ends) and info.decoded_bytes == total and info.first_error == 6
        if cap:
            got = records_of(items.a.tobytes(), len(frames))
            assert got == recs, [(g, w) for g, w in zip(got, recs) if g != w]
            check_image(dst.a, outs, ends, cap, 0x5A)
    frame, content, _ = hand_built()["c_across_a_raw_block"]
    want, _, _, rows = ref.read_frame(oracle, frame, 65536, accept_linked=True)
    arrs = standin(rows, 64)
    run = EmuRun(dec_results=arrs[0].ctypes.data, dec_len=arrs[1].ctypes.data, dec_at=arrs[2].ctypes.data, dec_bytes=arrs[3].ctypes.data, dec_rows=64)
    dst, info = Guarded(len(content)), Lz4fInfo()
    assert L.emu_lz4f_linked_decode_host(frame, len(frame), 3 | ACCEPT, dst.ptr, len(content), C.byref(info), C.byref(run)) == 0, run.error
    assert dst.a.tobytes() == content and dst.intact() and info.decoded_bytes == len(content)
    assert L.emu_lz4f_linked_decode_host(frame, len(frame), 3, dst.ptr, len(content), C.byref(info), C.byref(run)) == ref.UNSUPPORTED_LINKED


def test_an_unknown_flag_is_still_refused(oracle):
    L = emu()
    frame = hand_built()["d_run_fill"][0]
    run, info, dst = EmuRun(), Lz4fInfo(), Guarded(2000)
    assert L.emu_lz4f_linked_decode_host(frame, len(frame), 16, dst.ptr, 2000, C.byref(info), C.byref(run)) == E_ARGUMENT
    assert b"unknown flag" in run.error
