"""TEST INFRASTRUCTURE for the tests of LZ4 frames with linked blocks -- tests/test_simt_lz4f_linked.py and
tests/test_gpu_lz4f_linked.py: the linked entry points of the framing emulator library (tests/simt/emu_lz4f_batch.inc, a part of
libsimt_framing.so), the frames and batches the tests are made of, what the twin (tests/lz4f_linked_ref.py) expects of a batch, and
the emulator path checked against it field by field.  The linked rows run the real wavefront decoder under the emulator; the
independent rows keep the stand-in codec of tests/lz4f_batch_cases.py, keyed by global table row."""
import base64
import ctypes as C
import functools
import json
import os

import numpy as np

import emu_lib
import lz4f_linked_ref as lk
import lz4f_ref as ref
from emu_lib import GUARD, Guarded, I32 as _I32, I64 as _I64, P as _P, u8
from lz4f_batch_cases import BATCH_FIELDS, INFO_FIELDS, EmuRun, expect_batch, offsets_of, standin
from lz4net_amd._lib import Lz4fBatchInfo, Lz4fInfo

ACCEPT = lk.ACCEPT_LINKED
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_linked_frames.json")


@functools.lru_cache(maxsize=None)
def emu():
    L = emu_lib.framing()
    L.emu_lz4f_batch_sizeof.restype = _I64
    assert L.emu_lz4f_batch_sizeof(0) == C.sizeof(Lz4fInfo) and L.emu_lz4f_batch_sizeof(1) == C.sizeof(EmuRun)
    assert L.emu_lz4f_batch_sizeof(2) == C.sizeof(Lz4fBatchInfo)
    L.emu_lz4f_batch_decode_scratch_bytes.argtypes, L.emu_lz4f_batch_decode_scratch_bytes.restype = [_I64, _I32, _I64, _I64], _I64
    L.emu_lz4f_linked_decode_scratch_bytes.argtypes, L.emu_lz4f_linked_decode_scratch_bytes.restype = [_I32, _I64, _I64], _I64
    L.emu_lz4f_linked_decode.argtypes = [_P, _I64, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P]
    L.emu_lz4f_linked_decode_host.argtypes = [_P, _I64, C.c_uint, _P, _I64, _P, _P]
    L.emu_lz4f_linked_batch_decode.argtypes = [_P, _I64, _P, _I64, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]
    L.emu_lz4f_linked_batch_decode_host.argtypes = [_P, _I64, _P, _I64, C.c_uint, _P, _I64, _P, _P, _P, _P]
    return L


# ---- frames and batches ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden(oracle):
    """the linked frames liblz4 wrote (tests/golden/lz4f_linked_frames.json), in name order -> (names, records, frames, sources)"""
    with open(GOLDEN) as f:
        recs = json.load(f)["frames"]
    names = sorted(recs)
    frames = [base64.b64decode(recs[k]["frame"]) for k in names]
    srcs = [ref.golden_source(oracle, recs[k]["source"], recs[k]["bytes"]) for k in names]
    return names, [recs[k] for k in names], frames, srcs


@functools.lru_cache(maxsize=None)
def hand_built():
    return lk.hand_built()


@functools.lru_cache(maxsize=None)
def mixed_batch(oracle):
    """independent one-block, linked two-block, skippable, linked three-block with a raw middle block, independent two-block, empty
    frame, a linked frame with a dictionary ID -> (frames, index of the linked two-block item)"""
    cases = hand_built()
    d3 = ref.golden_source(oracle, "d3", 70000)
    dict_frame = lk.frame_of([(b"0123456789", True)], linked=True, dict_id=7)
    frames = [ref.write_frame(oracle, d3[:3000], 4, False, 7)[0], cases["d_run_fill"][0], ref.skippable(b"between the frames", 3),
              cases["c_across_a_raw_block"][0], ref.write_frame(oracle, d3, 4, True, 3)[0], ref.write_frame(oracle, b"", 4, False, 0)[0], dict_frame]
    return tuple(frames), 1


def expect(oracle, frames, slot_bytes, verify, dst_cap=None, max_blocks=1 << 30):
    """what the twin says of every item of a batch decoded with the flag -> (records, [(written and specified bytes, the item's bytes
    behind them unspecified)], rows of all items for the stand-in codec, prefix sums of the decoded sizes, the cap)"""
    sizes = [lk.read_frame_linked(oracle, f, slot_bytes, max_blocks, verify)[0]["decoded_bytes"] for f in frames]
    ends = np.cumsum([0] + sizes).astype(np.int64)
    cap = int(ends[-1]) if dst_cap is None else dst_cap
    recs, outs, rows = [], [], []
    for i, f in enumerate(frames):
        info, out, unspecified, r = lk.read_frame_linked(oracle, f, slot_bytes, max_blocks, verify, cap - int(ends[i]))
        recs.append(info)
        outs.append((out, unspecified))
        rows += r
    return recs, outs, rows, ends, cap


def check_image(dst, outs, ends, cap, fill):
    """dst (at least cap bytes, `fill` before the call): every item's specified bytes; behind them, up to the item's end or the cap,
    untouched fill unless the decoder refused a block there; nothing at or past the cap or the total"""
    dst = np.asarray(dst)
    for i, (out, unspecified) in enumerate(outs):
        begin = int(ends[i])
        assert dst[begin:begin + len(out)].tobytes() == out, (i, "the item's bytes")
        if not unspecified:
            stop = min(int(ends[i + 1]), cap)
            assert (dst[begin + len(out):max(stop, begin + len(out))] == fill).all(), (i, "bytes of a block that was not to be written")
    assert (dst[min(cap, int(ends[-1])):] == fill).all(), "bytes at or past dst_cap, or past the last item, were written"


def records_of(item_info, n):
    got = (Lz4fInfo * n).from_buffer_copy(bytes(item_info)) if n else []
    return [{f: int(getattr(g, f)) for f in INFO_FIELDS} for g in got]


def check_records(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, {f: (g[f], w[f]) for f in INFO_FIELDS if g[f] != w[f]})


# ---- the emulator path against the twin --------------------------------------------------------------------------------------------------
def run_batch(frames, rows, slot, max_blocks, round_blocks, flags, cap, grid=0):
    """the emulator's batch decode in guarded buffers -> (batch record, item records, dst_off, dst bytes, written_items)"""
    L, n = emu(), len(frames)
    src, off = b"".join(frames), offsets_of(frames)
    arrs = standin(rows, max_blocks)
    run = EmuRun(dec_results=arrs[0].ctypes.data, dec_len=arrs[1].ctypes.data, dec_at=arrs[2].ctypes.data, dec_bytes=arrs[3].ctypes.data,
                 dec_rows=max_blocks, grid=grid)
    a = Guarded(len(src))
    a.a[:] = u8(src)
    scratch = Guarded(L.emu_lz4f_batch_decode_scratch_bytes(n, slot, max_blocks, round_blocks))
    dst, dst_off, item_info, written = Guarded(cap), Guarded(8 * (n + 1)), Guarded(C.sizeof(Lz4fInfo) * n), Guarded(8)
    info = Lz4fBatchInfo()
    rc = L.emu_lz4f_linked_batch_decode(a.ptr, len(src), off.ctypes.data, n, slot, max_blocks, round_blocks, flags, scratch.ptr, scratch.n, dst.ptr, cap,
                                        dst_off.ptr, item_info.ptr, C.byref(info), written.ptr, C.byref(run))
    assert rc == 0, run.error
    rounds = (max_blocks + (round_blocks or max_blocks) - 1) // (round_blocks or max_blocks)
    assert run.shape_errors == 0 and run.calls == rounds, "the ring decoder was handed every round once, linked rows as empty rows"
    assert scratch.intact() and dst.intact() and a.intact() and dst_off.intact() and item_info.intact() and written.intact()
    return ({f: int(getattr(info, f)) for f in BATCH_FIELDS}, records_of(item_info.a.tobytes(), n), dst_off.a.view(np.int64).copy(), dst.a.copy(),
            int(written.a.view(np.int64)[0]))


def check_batch(oracle, frames, slot=65536, max_blocks=None, round_blocks=0, verify=3, dst_cap=None, grid=0):
    """the emulator path with the flag against the twin: every record field by field, the batch's record, dst_off, written_items, the
    image of dst; then the same items without the flag: every item that is not linked has the same record and the same bytes
    -> (records, batch record)"""
    frames = list(frames)
    recs, outs, rows, ends, cap = expect(oracle, frames, slot, verify, dst_cap)
    if max_blocks is None:
        max_blocks = max(len(rows), 1)
    want = expect_batch(recs, ends)
    got, got_recs, got_off, dst, written = run_batch(frames, rows, slot, max_blocks, round_blocks, verify | ACCEPT, cap, grid)
    if len(rows) > max_blocks:
        assert got == dict(want, first_error=-1, error_offset=-1, error=ref.TABLE_FULL, decoded_bytes=0), got
        assert (dst == GUARD).all() and (got_off == 0).all() and written == 0
        assert all(r["error"] == ref.TABLE_FULL for r in got_recs)
        return recs, got
    assert got == want, {f: (got[f], want[f]) for f in BATCH_FIELDS if got[f] != want[f]}
    assert list(got_off) == list(ends)
    check_records(got_recs, recs)
    check_image(dst, outs, ends, cap, GUARD)
    assert written == sum(1 for e in ends[1:] if e <= cap), "written_items: the prefix of items wholly inside dst_cap"
    # without the flag: the linked items are refused and take no bytes; every other item is what it is with the flag
    plain = [ref.read_frame(oracle, f, slot, 1 << 30, verify) for f in frames]
    plain_rows = [r for p in plain for r in p[2]]
    plain_ends = offsets_of([p[1] for p in plain])
    _, plain_recs, plain_off, plain_dst, _ = run_batch(frames, plain_rows, slot, max(len(plain_rows), 1), round_blocks, verify, int(plain_ends[-1]), grid)
    for i, f in enumerate(frames):
        if lk.is_linked(f):
            assert plain_recs[i]["error"] == ref.UNSUPPORTED_LINKED and plain_off[i + 1] == plain_off[i]
        elif ends[i + 1] <= cap:
            assert plain_recs[i] == got_recs[i], (i, "an independent item's record changed with the flag")
            assert plain_dst[plain_off[i]:plain_off[i + 1]].tobytes() == dst[ends[i]:ends[i + 1]].tobytes(), (i, "an independent item's bytes changed with the flag")
    return recs, got


def check_frame(oracle, frame, slot=65536, max_blocks=None, round_blocks=0, verify=3, dst_cap=None, grid=0):
    """the emulator's one-frame call with the flag against the twin -> (record, written bytes)"""
    L = emu()
    info_w, _, _, rows = lk.read_frame_linked(oracle, frame, slot, 1 << 30, verify)
    if max_blocks is None:
        max_blocks = max(len(rows), 1)
    cap = info_w["decoded_bytes"] if dst_cap is None else dst_cap
    want, out, unspecified, rows = lk.read_frame_linked(oracle, frame, slot, max_blocks, verify, cap)
    arrs = standin(rows, max_blocks)
    run = EmuRun(dec_results=arrs[0].ctypes.data, dec_len=arrs[1].ctypes.data, dec_at=arrs[2].ctypes.data, dec_bytes=arrs[3].ctypes.data,
                 dec_rows=max_blocks, grid=grid)
    a = Guarded(len(frame))
    a.a[:] = u8(frame)
    scratch = Guarded(L.emu_lz4f_linked_decode_scratch_bytes(slot, max_blocks, round_blocks))
    dst, info = Guarded(cap), Guarded(C.sizeof(Lz4fInfo))
    rc = L.emu_lz4f_linked_decode(a.ptr, len(frame), slot, max_blocks, round_blocks, verify | ACCEPT, scratch.ptr, scratch.n, dst.ptr, cap, info.ptr, C.byref(run))
    assert rc == 0, run.error
    assert run.shape_errors == 0 and scratch.intact() and dst.intact() and a.intact() and info.intact()
    got = records_of(info.a.tobytes(), 1)[0]
    assert got == want, {f: (got[f], want[f]) for f in INFO_FIELDS if got[f] != want[f]}
    check_image(dst.a, [(out, unspecified)], [0, want["decoded_bytes"]], cap, GUARD)
    return got, out
