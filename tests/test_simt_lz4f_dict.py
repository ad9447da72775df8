"""CPU-only: the decode of LZ4 frames with a dictionary (lz4hip_lz4f_decode_dict_* and lz4hip_lz4f_batch_decode_dict_*: the dictionary
forms of the sequences of lz4hip_framing.hpp) under the SIMT emulator, against the twin tests/lz4f_ref.py field by field, in
guarded buffers.  The walk, the plan, the rounds and the ordered decode are the library's own kernels and launch sequences, and every
block runs the real wavefront decoder: decode_dict_kernel in the rounds, the dictionary form of lz4f_linked_decode_kernel behind them
(the DICT path of tests/lz4f_cases.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import lz4f_built as built
import lz4f_cases as cases
import lz4f_ref as ref
from emu_lib import E_ARGUMENT, GRIDS, GUARD, Guarded, u8
from lz4f_cases import ACCEPT, DICT, DICT_PLAIN, DictRun as EmuRun, PlacedDict, check_image, check_records, emu, offsets_of, records_of, run_batch
from lz4f_dict_cases import GOLDEN_DICT_ID, dictionary, golden, golden_dictionary, hand_built, hand_built_params, mixed_batch
from lz4net_amd._lib import Lz4fBatchInfo, Lz4fInfo

check_frame = functools.partial(cases.check_frame, DICT, None, accept=True)   # the dictionary calls: no codec, every block is the twin's own to decode
check_batch = functools.partial(cases.check_batch, DICT, None, accept=True)
expect = functools.partial(cases.expect, None, slot_bytes=65536, verify=3, accept=True)


@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("n,name", hand_built_params())
def test_hand_built_frames_alone_and_behind_another_item(n, name, odd):
    frame, content, bad = hand_built(n)[name]
    d = dictionary(n)
    rec, out = check_frame(frame, d, odd=odd)
    assert (rec["error"] == ref.OK) == (content is not None) and (content is None or out == content)
    if content is None:
        assert rec["error"] == ref.CORRUPT_BLOCK and rec["blocks"] == 2 and rec["good_bytes"] == (1000 if name.startswith("l") else 100)
    recs, _, _ = check_batch([built.front_item(), frame], d, odd=odd, round_blocks=2 * odd)
    assert recs[0]["error"] == ref.OK and recs[1] == rec
    if content is None:                                                # the item in front and the one behind are intact, whatever dst held
        recs, _, got = check_batch([built.front_item(), frame, built.front_item()], d, round_blocks=2, odd=odd)
        assert got["first_error"] == 1 and recs[2]["error"] == ref.OK


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("round_blocks", [0, 2])
def test_every_hand_built_frame_of_one_dictionary_as_one_batch(grid, round_blocks):
    cases = hand_built(4097)
    frames = [cases[k][0] for k in sorted(cases)]
    recs, _, got = check_batch(frames, dictionary(4097), grid=grid, round_blocks=round_blocks)
    assert [r["error"] == ref.OK for r in recs] == [cases[k][1] is not None for k in sorted(cases)]


def test_a_refused_linked_block_keeps_its_place():
    frame = hand_built(13)["l_before_the_dictionary"][0]
    recs, _, _ = check_batch([built.front_item(), frame], dictionary(13))
    assert recs[1]["error"] == ref.CORRUPT_BLOCK and recs[1]["good_bytes"] == 1000 and recs[1]["decoded_bytes"] == 1032
    assert recs[1]["error_offset"] == 7 + 4 + 1000


@pytest.mark.parametrize("dict_id,frame_id,error", [(7, 7, ref.OK), (7, 8, ref.DICT_ID_MISMATCH), (0, 8, ref.OK), (7, None, ref.OK)])
def test_the_dictionary_id(dict_id, frame_id, error):
    d = dictionary(13)
    for name in ("i_into_the_block", "l_run_fill"):
        frame, content, _ = hand_built(13, frame_id)[name]
        rec, out = check_frame(frame, d, dict_id)
        assert rec["error"] == error and (out == content if error == ref.OK else (rec["error_offset"] == 6 and rec["blocks"] == 0 and out == b""))
        check_batch([built.front_item(), frame], d, dict_id)
    sized = built.frame_of([(b"0123456789", True)], linked=False, flags=ref.F_CONTENT_SIZE, content=b"0123456789", dict_id=frame_id)
    rec, _ = check_frame(sized, d, dict_id)
    assert rec["error"] == error and (error == ref.OK or rec["error_offset"] == 14)


def test_the_mismatch_comes_before_the_linked_check_and_the_slot_check():
    d = dictionary(13)
    frame = hand_built(13, 8)["l_run_fill"][0]
    recs, _, _ = check_batch([frame], d, 7, accept=False)
    assert recs[0]["error"] == ref.DICT_ID_MISMATCH
    recs, _, _ = check_batch([hand_built(13, 7)["l_run_fill"][0]], d, 7, accept=False)
    assert recs[0]["error"] == ref.UNSUPPORTED_LINKED
    big = built.frame_of([(b"0123456789", True)], linked=False, block_id=6, dict_id=8)
    assert check_batch([big], d, 7)[0][0]["error"] == ref.DICT_ID_MISMATCH
    assert check_batch([big], d, 8)[0][0]["error"] == ref.SLOT_TOO_SMALL


@pytest.mark.parametrize("round_blocks", [0, 2])
def test_golden_frames(round_blocks):
    names, golden_recs, frames, srcs = golden()
    d = golden_dictionary()
    for rec, frame, src in zip(golden_recs, frames, srcs):
        got, out = check_frame(frame, d, GOLDEN_DICT_ID, round_blocks=round_blocks, odd=round_blocks & 1)
        assert got["error"] == ref.OK and out == src, rec
    recs, _, got = check_batch(frames, d, GOLDEN_DICT_ID, round_blocks=round_blocks)
    assert got["error"] == ref.OK and got["decoded_bytes"] == sum(len(s) for s in srcs)
    recs, _, got = check_batch([built.front_item()] + frames[:4], d, 0, round_blocks=round_blocks, odd=1)
    assert got["error"] == ref.OK


@pytest.mark.parametrize("verify", [0, 3])
@pytest.mark.parametrize("round_blocks", [0, 2])
def test_mixed_batch(round_blocks, verify):
    frames, d, dict_id, _ = mixed_batch()
    recs, _, got = check_batch(frames, d, dict_id, round_blocks=round_blocks, verify=verify)
    assert [r["error"] for r in recs] == [0, 0, 0, 0, ref.DICT_ID_MISMATCH] and got["first_error"] == 4 and recs[3]["kind"] == 1


@pytest.mark.parametrize("grid", GRIDS)
def test_mixed_batch_at_forced_grids(grid):
    frames, d, dict_id, _ = mixed_batch()
    check_batch(frames, d, dict_id, round_blocks=2, grid=grid, odd=1)


def test_mixed_batch_clipped_at_every_block_boundary_of_the_linked_item():
    frames, d, dict_id, linked = mixed_batch()
    _, _, _, ends, total = expect(list(frames), dictionary=d, dict_id=dict_id)
    begin = int(ends[linked])
    for cap in (0, begin, begin + 5, begin + 10, begin + 11, begin + 10 + 54, begin + 10 + 55, int(ends[linked + 1]) - 1, int(ends[linked + 1]), total):
        recs, _, _ = check_batch(frames, d, dict_id, dst_cap=cap)
        check_batch(frames, d, dict_id, dst_cap=cap, round_blocks=2)
        assert recs[linked]["error"] == ref.OK


def test_a_table_one_row_short_writes_nothing():
    frames, d, dict_id, _ = mixed_batch()
    recs, _, _, ends, total = expect(list(frames), dictionary=d, dict_id=dict_id)
    rows = sum(r["blocks"] for r in recs)
    got, got_recs, off, dst, written, _ = run_batch(DICT, list(frames), (), d, dict_id, 65536, rows - 1, 0, 3 | ACCEPT, total)
    assert got["error"] == ref.TABLE_FULL and got["blocks"] == rows and (dst == GUARD).all() and written == 0 and (off == 0).all()


def test_without_a_dictionary_the_call_is_the_plain_call():
    """dict_len = 0, dict NULL, any dict_id: record for record and byte for byte, UNSUPPORTED_DICT for a frame with an ID included"""
    frames, d, _, _ = mixed_batch()
    frames = [built.front_item()] + list(frames)
    for flags in (3, 3 | ACCEPT):
        plain = run_batch(DICT_PLAIN, frames, (), b"", 0, 65536, 16, 2, flags, 4096)
        with_none = run_batch(DICT, frames, (), b"", 99, 65536, 16, 2, flags, 4096)
        assert plain[:2] == with_none[:2] and list(plain[2]) == list(with_none[2]) and (plain[3] == with_none[3]).all() and plain[4] == with_none[4]
        assert [r["error"] for r in plain[1]][1] == ref.UNSUPPORTED_DICT and with_none[5].plain_calls == 8 and with_none[5].dict_calls == 0
    L = emu()
    frame = frames[1]
    for entry, args in ((L.emu_lz4f_dict_plain_decode, ()), (L.emu_lz4f_dict_decode, (None, 0, 5))):
        run, dst, info = EmuRun(), Guarded(64), Guarded(C.sizeof(Lz4fInfo))
        scratch = Guarded(L.emu_lz4f_dict_decode_scratch_bytes(65536, 4, 0))
        a = Guarded(len(frame))
        a.a[:] = u8(frame)
        assert entry(a.ptr, len(frame), *args, 65536, 4, 0, 3, scratch.ptr, scratch.n, dst.ptr, 64, info.ptr, C.byref(run)) == 0
        rec = records_of(info.a.tobytes(), 1)[0]
        assert rec["error"] == ref.UNSUPPORTED_DICT and rec["error_offset"] == 4 and (dst.a == GUARD).all() and run.dict_calls == 0


@pytest.mark.parametrize("n", [13, 65535, 70000])
def test_the_host_calls_upload_the_reachable_tail_once(n):
    """the batch (whole, then as a size query, whose image grows for the second pass) and one frame: ONE upload of min(n, 65 535) bytes, the
    dictionary's last, before anything else goes up, into staging of its own between intact guard bytes"""
    L = emu()
    d = dictionary(n)
    cases = hand_built(n, 7)
    frames = [cases[k][0] for k in sorted(cases) if cases[k][1] is not None] + [built.front_item()]
    recs, outs, _, ends, total = expect(frames, dictionary=d, dict_id=7)
    src, off = b"".join(frames), offsets_of(frames)
    for cap in (total, 0):
        run, pd = EmuRun(), PlacedDict(d, 1)
        a = Guarded(len(src))
        a.a[:] = u8(src)
        dst, dst_off, items = Guarded(cap), Guarded(8 * (len(frames) + 1)), Guarded(C.sizeof(Lz4fInfo) * len(frames))
        info = Lz4fBatchInfo()
        rc = L.emu_lz4f_dict_batch_decode_host(a.ptr, len(src), off.ctypes.data, len(frames), pd.ptr, n, 7, 3 | ACCEPT, dst.ptr, cap, dst_off.ptr, items.ptr,
                                               C.byref(info), C.byref(run))
        assert rc == (0 if cap else E_ARGUMENT), run.error
        assert (run.dict_uploads, run.dict_bytes, run.dict_first_byte, run.uploads_before_dict) == (1, min(n, 65535), n - min(n, 65535), 0)
        assert run.dict_intact == 1 and run.intact == 1 and dst.intact() and dst_off.intact() and items.intact() and a.intact() and pd.g.intact()
        assert list(dst_off.a.view(np.int64)) == list(ends) and info.decoded_bytes == total and info.first_error == -1
        if cap:
            check_records(records_of(items.a.tobytes(), len(frames)), recs)
            check_image(dst.a, outs, ends, cap, 0x5A)
    # an item that decodes to more than four times its bytes: the image grows for a second pass and MOVES; the dictionary stays
    for frame, content, _ in (cases["l_run_fill"],):
        run, pd, dst, dst_off, items, info = EmuRun(), PlacedDict(d, 1), Guarded(len(content)), Guarded(16), Guarded(C.sizeof(Lz4fInfo)), Lz4fBatchInfo()
        off = offsets_of([frame])
        assert L.emu_lz4f_dict_batch_decode_host(frame, len(frame), off.ctypes.data, 1, pd.ptr, n, 7, 3 | ACCEPT, dst.ptr, len(content), dst_off.ptr, items.ptr,
                                                 C.byref(info), C.byref(run)) == 0, run.error
        assert run.moves == 2 and run.dict_uploads == 1 and run.dict_intact == 1 and run.intact == 1 and dst.a.tobytes() == content and dst.intact()
        run, dst, one = EmuRun(), Guarded(len(content)), Lz4fInfo()
        assert L.emu_lz4f_dict_decode_host(frame, len(frame), pd.ptr, n, 7, 3 | ACCEPT, dst.ptr, len(content), C.byref(one), C.byref(run)) == 0, run.error
        assert run.moves == 2 and run.dict_uploads == 1 and run.dict_intact == 1 and run.intact == 1 and dst.a.tobytes() == content and dst.intact()
    frame, content, _ = cases["l_across_a_raw_block"]
    run, pd, dst, info = EmuRun(), PlacedDict(d), Guarded(len(content)), Lz4fInfo()
    assert L.emu_lz4f_dict_decode_host(frame, len(frame), pd.ptr, n, 7, 3 | ACCEPT, dst.ptr, len(content), C.byref(info), C.byref(run)) == 0, run.error
    assert dst.a.tobytes() == content and dst.intact() and info.decoded_bytes == len(content) and run.dict_uploads == 1 and run.dict_bytes == min(n, 65535)
    assert L.emu_lz4f_dict_decode_host(frame, len(frame), pd.ptr, n, 8, 3 | ACCEPT, dst.ptr, len(content), C.byref(info), C.byref(run)) == ref.DICT_ID_MISMATCH
    assert L.emu_lz4f_dict_decode_host(frame, len(frame), pd.ptr, n, 7, 3, dst.ptr, len(content), C.byref(info), C.byref(run)) == ref.UNSUPPORTED_LINKED


def test_the_front_checks():
    """dict_len < 0 and a NULL dictionary of some length are refused before anything else is looked at, and nothing is uploaded; the
    plain calls' checks follow"""
    L = emu()
    frame = hand_built(13)["l_run_fill"][0]
    d = PlacedDict(dictionary(13))
    dst, info, binfo = Guarded(2000), Lz4fInfo(), Lz4fBatchInfo()
    off = offsets_of([frame])
    dst_off, items, written = Guarded(16), Guarded(C.sizeof(Lz4fInfo)), Guarded(8)
    scratch = Guarded(L.emu_lz4f_dict_batch_decode_scratch_bytes(1, 65536, 4, 0))
    for ptr, n, text in ((d.ptr, -1, b"dict_len < 0"), (None, 5, b"dict is NULL")):
        run = EmuRun()
        assert L.emu_lz4f_dict_decode_host(frame, len(frame), ptr, n, 0, 3, dst.ptr, 2000, C.byref(info), C.byref(run)) == E_ARGUMENT
        assert text in run.error and run.dict_uploads == 0 and run.reserves == 0
        assert L.emu_lz4f_dict_batch_decode_host(frame, len(frame), off.ctypes.data, 1, ptr, n, 0, 3, dst.ptr, 2000, dst_off.ptr, items.ptr, C.byref(binfo),
                                                 C.byref(run)) == E_ARGUMENT
        assert text in run.error and run.dict_uploads == 0 and run.reserves == 0
        assert L.emu_lz4f_dict_decode(frame, len(frame), ptr, n, 0, 65536, 4, 0, 3, scratch.ptr, scratch.n, dst.ptr, 2000, items.ptr, C.byref(run)) == E_ARGUMENT
        assert text in run.error
        assert L.emu_lz4f_dict_batch_decode(frame, len(frame), off.ctypes.data, 1, ptr, n, 0, 65536, 4, 0, 3, scratch.ptr, scratch.n, dst.ptr, 2000, dst_off.ptr,
                                            items.ptr, C.byref(binfo), written.ptr, C.byref(run)) == E_ARGUMENT
        assert text in run.error and (dst.a == GUARD).all()
    run = EmuRun()
    assert L.emu_lz4f_dict_decode_host(frame, len(frame), d.ptr, 13, 0, 16, dst.ptr, 2000, C.byref(info), C.byref(run)) == E_ARGUMENT
    assert b"unknown flag" in run.error and run.dict_uploads == 0
    assert L.emu_lz4f_dict_decode_host(frame, len(frame), d.ptr, 13, 0, 0x100 | 3, dst.ptr, 2000, C.byref(info), C.byref(run)) == E_ARGUMENT
    assert b"unknown flag" in run.error, "the walk's internal bit is no public flag"
    assert L.emu_lz4f_dict_batch_decode_host(frame, len(frame), off.ctypes.data, 1, d.ptr, 13, 0, 0x100, dst.ptr, 2000, dst_off.ptr, items.ptr, C.byref(binfo),
                                             C.byref(run)) == E_ARGUMENT
    assert b"unknown flag" in run.error and run.dict_uploads == 0
    assert L.emu_lz4f_dict_batch_decode(frame, len(frame), off.ctypes.data, 1, d.ptr, 13, 0, 65536, 4, 0, 0x100, scratch.ptr, scratch.n, dst.ptr, 2000,
                                        dst_off.ptr, items.ptr, C.byref(binfo), written.ptr, C.byref(run)) == E_ARGUMENT
    assert b"unknown flag" in run.error
