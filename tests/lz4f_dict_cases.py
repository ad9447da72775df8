"""TEST INFRASTRUCTURE for the tests of LZ4 frames with a dictionary -- tests/test_simt_lz4f_dict.py and tests/test_gpu_lz4f_dict.py:
the dictionary entry points of the framing emulator library (tests/simt/emu_lz4f_dict.inc, a part of libsimt_framing.so), the frames
and batches the tests are made of, what the twin (tests/lz4f_dict_ref.py) expects of a batch, and the emulator path checked against it
field by field.  Every block runs the real wavefront decoder under the emulator: the rounds' rows decode_dict_kernel, the linked rows the
dictionary form of the ordered decode."""
import base64
import ctypes as C
import functools
import json
import os

import numpy as np

import emu_lib
import lz4f_dict_ref as dr
import lz4f_ref as ref
from emu_lib import GUARD, Guarded, I32 as _I32, I64 as _I64, P as _P, U32 as _U32, u8
from lz4f_batch_cases import BATCH_FIELDS, INFO_FIELDS, expect_batch, offsets_of
from lz4f_linked_cases import check_image, check_records, records_of
from lz4net_amd._lib import Lz4fBatchInfo, Lz4fInfo

ACCEPT = 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_dict_frames.json")
GOLDEN_DICT_SEED, GOLDEN_DICT_BYTES, GOLDEN_DICT_ID = 4242, 20000, 0x0D1C7105


class EmuRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("grid", _I32), ("pad", _I32), ("plain_calls", _I64), ("dict_calls", _I64), ("dict_uploads", _I64), ("dict_bytes", _I64),
                ("dict_first_byte", _I64), ("dict_intact", _I64), ("uploads_before_dict", _I64), ("counters", emu_lib.EmuCounters)]


@functools.lru_cache(maxsize=None)
def emu():
    L = emu_lib.framing()
    L.emu_lz4f_dict_sizeof.restype = _I64
    assert L.emu_lz4f_dict_sizeof(0) == C.sizeof(Lz4fInfo) and L.emu_lz4f_dict_sizeof(1) == C.sizeof(EmuRun)
    assert L.emu_lz4f_dict_sizeof(2) == C.sizeof(Lz4fBatchInfo) and L.emu_lz4f_dict_sizeof(3) == C.sizeof(emu_lib.EmuCounters)
    L.emu_lz4f_dict_decode_scratch_bytes.argtypes, L.emu_lz4f_dict_decode_scratch_bytes.restype = [_I32, _I64, _I64], _I64
    L.emu_lz4f_dict_batch_decode_scratch_bytes.argtypes, L.emu_lz4f_dict_batch_decode_scratch_bytes.restype = [_I64, _I32, _I64, _I64], _I64
    L.emu_lz4f_dict_decode.argtypes = [_P, _I64, _P, _I64, _U32, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P]
    L.emu_lz4f_dict_batch_decode.argtypes = [_P, _I64, _P, _I64, _P, _I64, _U32, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]
    L.emu_lz4f_dict_plain_decode.argtypes = [_P, _I64, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P]
    L.emu_lz4f_dict_plain_batch_decode.argtypes = [_P, _I64, _P, _I64, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]
    L.emu_lz4f_dict_decode_host.argtypes = [_P, _I64, _P, _I64, _U32, C.c_uint, _P, _I64, _P, _P]
    L.emu_lz4f_dict_batch_decode_host.argtypes = [_P, _I64, _P, _I64, _P, _I64, _U32, C.c_uint, _P, _I64, _P, _P, _P, _P]
    return L


# ---- dictionaries, frames and batches ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dictionary(n):
    return dr.dictionary(n)


@functools.lru_cache(maxsize=None)
def hand_built(n, dict_id=None):
    return dr.hand_built(dictionary(n), dict_id)


def hand_built_params():
    """(dictionary length, case name) for every case that length allows"""
    return [(n, name) for n in dr.DICT_LENGTHS for name in sorted(hand_built(n))]


@functools.lru_cache(maxsize=None)
def golden_dictionary():
    return dr.dictionary(GOLDEN_DICT_BYTES, GOLDEN_DICT_SEED)


def golden_source(n):
    """what the golden frames hold: pieces of the dictionary, a little noise, and repeats of the source's own bytes up to 60 000 back (a 32-bit
    LCG picks them: the same bytes wherever this runs)"""
    d = golden_dictionary()
    out, state = bytearray(), [(n * 2654435761 + 12345) & 0xFFFFFFFF]

    def pick():
        state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
        return state[0] >> 8

    while len(out) < n:
        kind, k = pick() % 12, 16 + pick() % 240
        if kind:
            at = pick() % (len(d) - 256)
            out += d[at:at + k]
        else:
            out += dr.lk.noise(8 + k % 17, pick() & 0xFFFF)
        if len(out) > 200 and pick() % 4 == 0:
            back = 1 + pick() % min(len(out) - 1, 60000)
            out += out[-back:][:k]
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def golden():
    """the frames liblz4 wrote with LZ4F_compressFrame_usingCDict (tests/golden/lz4f_dict_frames.json), in name order
    -> (names, records, frames, sources)"""
    with open(GOLDEN) as f:
        recs = json.load(f)["frames"]
    names = sorted(recs)
    return names, [recs[k] for k in names], [base64.b64decode(recs[k]["frame"]) for k in names], [golden_source(recs[k]["bytes"]) for k in names]


MIXED_DICT = 4097


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """dictionary independent, dictionary linked (three blocks, the middle one raw), plain independent, skippable, a frame with another
    dictionary ID -> (frames, dictionary, the call's dict_id, index of the linked item)"""
    with_id, no_id = hand_built(MIXED_DICT, 7), hand_built(MIXED_DICT)
    other = dr.lk.frame_of([(b"0123456789", True)], linked=False, dict_id=8)
    frames = (with_id["i_into_the_block"][0], with_id["l_across_a_raw_block"][0], no_id["i_first_byte"][0], ref.skippable(b"between the frames", 3), other)
    return frames, dictionary(MIXED_DICT), 7, 1


def expect(frames, d, dict_id, slot=65536, verify=3, dst_cap=None, accept=True):
    """what the twin says of every item of a batch decoded with the dictionary -> (records, [(written and specified bytes, the item's
    bytes behind them unspecified)], prefix sums of the decoded sizes, the cap)"""
    sizes = [dr.read_frame_dict(f, d, dict_id, slot, 1 << 30, verify, accept)[0]["decoded_bytes"] for f in frames]
    ends = np.cumsum([0] + sizes).astype(np.int64)
    cap = int(ends[-1]) if dst_cap is None else dst_cap
    recs, outs = [], []
    for i, f in enumerate(frames):
        info, out, unspecified = dr.read_frame_dict(f, d, dict_id, slot, 1 << 30, verify, accept, cap - int(ends[i]))
        recs.append(info)
        outs.append((out, unspecified))
    return recs, outs, ends, cap


class PlacedDict:
    """the dictionary between guard bytes, at an even (odd = 0) or odd address"""
    def __init__(self, d, odd=0):
        self.g = Guarded(len(d) + odd)
        self.g.a[odd:] = u8(d)
        self.ptr, self.n = self.g.ptr + odd, len(d)


# ---- the emulator path against the twin --------------------------------------------------------------------------------------------------
def run_batch(frames, d, dict_id, slot, max_blocks, round_blocks, flags, cap, grid=0, odd=0, plain=False):
    """the emulator's batch decode in guarded buffers -> (batch record, item records, dst_off, dst bytes, written_items, run)"""
    L, n = emu(), len(frames)
    src, off = b"".join(frames), offsets_of(frames)
    run = EmuRun(grid=grid)
    a = Guarded(len(src))
    a.a[:] = u8(src)
    pd = PlacedDict(d, odd)
    scratch = Guarded(L.emu_lz4f_dict_batch_decode_scratch_bytes(n, slot, max_blocks, round_blocks))
    dst, dst_off, item_info, written = Guarded(cap), Guarded(8 * (n + 1)), Guarded(C.sizeof(Lz4fInfo) * n), Guarded(8)
    info = Lz4fBatchInfo()
    if plain:
        rc = L.emu_lz4f_dict_plain_batch_decode(a.ptr, len(src), off.ctypes.data, n, slot, max_blocks, round_blocks, flags, scratch.ptr, scratch.n, dst.ptr, cap,
                                                dst_off.ptr, item_info.ptr, C.byref(info), written.ptr, C.byref(run))
    else:
        rc = L.emu_lz4f_dict_batch_decode(a.ptr, len(src), off.ctypes.data, n, pd.ptr if pd.n else None, pd.n, dict_id, slot, max_blocks, round_blocks, flags,
                                          scratch.ptr, scratch.n, dst.ptr, cap, dst_off.ptr, item_info.ptr, C.byref(info), written.ptr, C.byref(run))
    assert rc == 0, run.error
    rounds = (max_blocks + (round_blocks or max_blocks) - 1) // (round_blocks or max_blocks)
    assert (run.plain_calls, run.dict_calls) == ((rounds, 0) if plain or not pd.n else (0, rounds)), "every round went to the dictionary decode, once"
    assert scratch.intact() and dst.intact() and a.intact() and dst_off.intact() and item_info.intact() and written.intact() and pd.g.intact()
    return ({f: int(getattr(info, f)) for f in BATCH_FIELDS}, records_of(item_info.a.tobytes(), n), dst_off.a.view(np.int64).copy(), dst.a.copy(),
            int(written.a.view(np.int64)[0]), run)


def check_batch(frames, d, dict_id=0, slot=65536, max_blocks=None, round_blocks=0, verify=3, dst_cap=None, grid=0, odd=0, accept=True):
    """the emulator path against the twin: every record field by field, the batch's record, dst_off, written_items, the image of dst
    -> (records, batch record)"""
    frames = list(frames)
    recs, outs, ends, cap = expect(frames, d, dict_id, slot, verify, dst_cap, accept)
    if max_blocks is None:
        max_blocks = max(sum(r["blocks"] for r in recs), 1)
    want = expect_batch(recs, ends)
    got, got_recs, got_off, dst, written, _ = run_batch(frames, d, dict_id, slot, max_blocks, round_blocks, verify | (ACCEPT if accept else 0), cap, grid, odd)
    assert got == want, {f: (got[f], want[f]) for f in BATCH_FIELDS if got[f] != want[f]}
    assert list(got_off) == list(ends)
    check_records(got_recs, recs)
    check_image(dst, outs, ends, cap, GUARD)
    assert written == sum(1 for e in ends[1:] if e <= cap), "written_items: the prefix of items wholly inside dst_cap"
    return recs, got


def check_frame(frame, d, dict_id=0, slot=65536, max_blocks=None, round_blocks=0, verify=3, dst_cap=None, grid=0, odd=0):
    """the emulator's one-frame call against the twin -> (record, written bytes)"""
    L = emu()
    whole = dr.read_frame_dict(frame, d, dict_id, slot, 1 << 30, verify)[0]
    if max_blocks is None:
        max_blocks = max(whole["blocks"], 1)
    cap = whole["decoded_bytes"] if dst_cap is None else dst_cap
    want, out, unspecified = dr.read_frame_dict(frame, d, dict_id, slot, max_blocks, verify, True, cap)
    run = EmuRun(grid=grid)
    a = Guarded(len(frame))
    a.a[:] = u8(frame)
    pd = PlacedDict(d, odd)
    scratch = Guarded(L.emu_lz4f_dict_decode_scratch_bytes(slot, max_blocks, round_blocks))
    dst, info = Guarded(cap), Guarded(C.sizeof(Lz4fInfo))
    rc = L.emu_lz4f_dict_decode(a.ptr, len(frame), pd.ptr, pd.n, dict_id, slot, max_blocks, round_blocks, verify | ACCEPT, scratch.ptr, scratch.n, dst.ptr, cap,
                                info.ptr, C.byref(run))
    assert rc == 0, run.error
    assert scratch.intact() and dst.intact() and a.intact() and info.intact() and pd.g.intact() and run.plain_calls == 0
    got = records_of(info.a.tobytes(), 1)[0]
    assert got == want, {f: (got[f], want[f]) for f in INFO_FIELDS if got[f] != want[f]}
    check_image(dst.a, [(out, unspecified)], [0, want["decoded_bytes"]], cap, GUARD)
    return got, out
