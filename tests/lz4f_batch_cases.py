"""TEST INFRASTRUCTURE for the tests of batches of LZ4 frames -- tests/test_simt_lz4f_batch.py and tests/test_gpu_lz4f_batch.py: the
batch path's entry points in the framing emulator library (tests/simt/emu_lz4f_batch.inc, a part of libsimt_framing.so), the
batches the tests are made of, and the emulator path checked against the one-frame path: encode against lz4f_cases.emu_encode of every
item alone, decode against the from-the-spec twin tests/lz4f_ref.py on every item alone, with the twin's per-block results and bytes
as the stand-in codec keyed by global table row."""
import ctypes as C
import functools
import os

import numpy as np

import emu_lib
import lz4f_ref as ref
from emu_lib import E_ARGUMENT, GUARD, Guarded, I32 as _I32, I64 as _I64, P as _P, u8
from lz4f_cases import emu_encode, flip, mixed, sample
from lz4net_amd._lib import Lz4fBatchInfo, Lz4fInfo

INFO_FIELDS = [f for f, _ in Lz4fInfo._fields_]
BATCH_FIELDS = [f for f, _ in Lz4fBatchInfo._fields_]
ITEM_LENGTHS = (0, 1, 13, 65535, 65536, 65537, 3 * 65536 + 5)
BAD_ITEM = dict(blocks=0, decoded_bytes=0, good_bytes=0, error_offset=-1, content_size=-1, frame_bytes=0, error=E_ARGUMENT, kind=0, block_max=0,
                flg=0, bd=0, checks=0)


class EmuRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("enc_results", _P), ("enc_bytes", _P), ("enc_at", _P), ("enc_len", _P), ("enc_src", _P), ("enc_rows", _I64),
                ("dec_results", _P), ("dec_len", _P), ("dec_at", _P), ("dec_bytes", _P), ("dec_rows", _I64),
                ("grid", _I32), ("pad", _I32), ("calls", _I64), ("shape_errors", _I64), ("counters", emu_lib.EmuCounters)]


@functools.lru_cache(maxsize=None)
def emu():
    L = emu_lib.framing()
    L.emu_lz4f_batch_sizeof.restype = _I64
    assert L.emu_lz4f_batch_sizeof(0) == C.sizeof(Lz4fInfo) and L.emu_lz4f_batch_sizeof(1) == C.sizeof(EmuRun)
    assert L.emu_lz4f_batch_sizeof(2) == C.sizeof(Lz4fBatchInfo) and L.emu_lz4f_batch_sizeof(3) == C.sizeof(emu_lib.EmuCounters)
    L.emu_lz4f_batch_bound.argtypes, L.emu_lz4f_batch_bound.restype = [_I64, _I64, C.c_int, C.c_uint], _I64
    L.emu_lz4f_batch_encode_scratch_bytes.argtypes, L.emu_lz4f_batch_encode_scratch_bytes.restype = [_I64, _I64, C.c_int], _I64
    L.emu_lz4f_batch_decode_scratch_bytes.argtypes, L.emu_lz4f_batch_decode_scratch_bytes.restype = [_I64, _I32, _I64, _I64], _I64
    L.emu_lz4f_batch_encode.argtypes = [_P, _I64, _P, _I64, C.c_int, C.c_int, C.c_uint, _P, _I64, _P, _P, _I64, _P]
    L.emu_lz4f_batch_decode.argtypes = [_P, _I64, _P, _I64, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]
    L.emu_lz4f_batch_encode_host.argtypes = [_P, _I64, _P, _I64, C.c_int, C.c_int, C.c_uint, _P, _I64, _P, _P]
    L.emu_lz4f_batch_decode_host.argtypes = [_P, _I64, _P, _I64, C.c_uint, _P, _I64, _P, _P, _P, _P]
    return L


# ---- batches -------------------------------------------------------------------------------------------------------------------------
def offsets_of(items):
    return np.cumsum([0] + [len(b) for b in items]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _sources(oracle):
    return tuple(sample(oracle, 2 + (k & 1), n) for k, n in enumerate(ITEM_LENGTHS))


def sources(oracle):
    """items of 0, 1, 13, 65535, 65536, 65537 and 3 * 65536 + 5 bytes, D2 and D3 in turn"""
    return list(_sources(oracle))


def spans(src, off):
    """item i of the batch, or None for offsets that decrease or leave the buffer"""
    out = []
    for a, b in zip(off[:-1], off[1:]):
        out.append(bytes(src[a:b]) if 0 <= a <= b <= len(src) else None)
    return out


@functools.lru_cache(maxsize=None)
def _frame_alone(oracle, item, block_id, hc, flags):
    return emu_encode(oracle, item, block_id, hc, flags)


def frames_alone(oracle, items, block_id=4, hc=False, flags=0):
    """what the one-frame emulator path writes for every item alone (checked there against the twin writer); b"" for a bad item"""
    return [b"" if it is None else _frame_alone(oracle, it, block_id, hc, flags) for it in items]


def golden_batch(oracle):
    """the frames liblz4 wrote (tests/golden/lz4f_frames.json), in name order -> (names, records, frames, sources)"""
    import base64
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_frames.json")) as f:
        recs = json.load(f)["frames"]
    names = sorted(recs)
    frames = [base64.b64decode(recs[k]["frame"]) for k in names]
    srcs = [ref.golden_source(oracle, recs[k]["source"], recs[k]["bytes"]) for k in names]
    return names, [recs[k] for k in names], frames, srcs


def tiny_items(count=4100):
    """one-block items of 1 .. 40 bytes"""
    rng = np.random.default_rng(count)
    return [bytes(rng.integers(0, 4, int(n), dtype=np.uint8)) for n in rng.integers(1, 41, count)]


# ---- the emulator path against the one-frame path -----------------------------------------------------------------------------------
def emu_encode_batch(oracle, src, off, block_id=4, hc=False, flags=0, grid=0, host=False, want=None):
    """the emulator path's batch of frames for the items src[off[i], off[i + 1]) -> (bytes, dst_off); asserts that it is `want`
    (default: the concatenation of the twin writer's frames) with the prefix sums as offsets, and that nothing else was written"""
    src, off = bytes(src), np.ascontiguousarray(off, np.int64)
    L, n, bid = emu(), len(off) - 1, block_id or 4
    items = spans(src, off)
    written = [(None, [], []) if it is None else ref.write_frame(oracle, it, bid, hc, flags) for it in items]
    if want is None:
        want = [w[0] or b"" for w in written]
    rets, blob, at, lens, where = [], b"", [], [], []
    for i, (it, (_, r, d)) in enumerate(zip(items, written)):
        for j, (ret, data) in enumerate(zip(r, d)):
            rets.append(ret)
            at.append(len(blob))
            blob += data
            lens.append(min(len(it) - j * ref.block_bytes(bid), ref.block_bytes(bid)))
            where.append(int(off[i]) + j * ref.block_bytes(bid))
    arrs = [np.array(rets + [0], np.int32), u8(blob + b"\0"), np.array(at + [0], np.int64), np.array(lens + [0], np.int32), np.array(where + [0], np.int64)]
    run = EmuRun(enc_results=arrs[0].ctypes.data, enc_bytes=arrs[1].ctypes.data, enc_at=arrs[2].ctypes.data, enc_len=arrs[3].ctypes.data,
                 enc_src=arrs[4].ctypes.data, enc_rows=len(rets), grid=grid)
    bound = L.emu_lz4f_batch_bound(n, len(src), block_id, flags)
    assert bound >= sum(len(w) for w in want)
    a = Guarded(len(src))
    a.a[:] = u8(src)
    dst, dst_off = Guarded(bound), Guarded(8 * (n + 1))
    if host:
        rc = L.emu_lz4f_batch_encode_host(a.ptr, len(src), off.ctypes.data, n, block_id, int(hc), flags, dst.ptr, bound, dst_off.ptr, C.byref(run))
        assert run.intact == 1 and (n == 0 or (run.reserves == 1 and run.moves == 1 and run.syncs >= 1)), "one staged image"
    else:
        scratch = Guarded(L.emu_lz4f_batch_encode_scratch_bytes(n, len(src), block_id))
        rc = L.emu_lz4f_batch_encode(a.ptr, len(src), off.ctypes.data, n, block_id, int(hc), flags, dst.ptr, bound, dst_off.ptr, scratch.ptr, scratch.n,
                                     C.byref(run))
        assert scratch.intact()
    assert rc == 0, run.error
    assert dst.intact() and dst_off.intact() and a.intact()
    assert run.shape_errors == 0, "the block encoder was not handed every block once, at its source position, with its length - 1 of room"
    got_off = dst_off.a.view(np.int64)
    assert list(got_off) == list(offsets_of(want)), "dst_off are the prefix sums of the frames' lengths"
    total = int(got_off[n])
    got = dst.a[:total].tobytes()
    assert (dst.a[total:] == GUARD).all(), "bytes past the last frame's end were written"
    for i, w in enumerate(want):
        assert got[got_off[i]:got_off[i + 1]] == w, (i, "not the frame of the item alone")
    return got, got_off.copy()


def expect_items(oracle, items, slot_bytes, verify, dst_cap=None):
    """what the one-frame decode gives for every item alone -> (records, contents, rows of all items, prefix sums of the contents)"""
    recs, outs, rows = [], [], []
    for it in items:
        if it is None:
            recs.append(dict(BAD_ITEM))
            outs.append(b"")
            continue
        info, out, r = ref.read_frame(oracle, it, slot_bytes, 1 << 30, verify)
        recs.append(info)
        outs.append(out)
        rows += r
    ends = offsets_of(outs)
    if dst_cap is not None:                                            # an item not wholly written: its content checksum is not looked at
        for i, it in enumerate(items):
            if it is not None and ends[i + 1] > dst_cap:
                recs[i] = ref.read_frame(oracle, it, slot_bytes, 1 << 30, verify, -1)[0]
    return recs, outs, rows, ends


def expect_batch(recs, ends):
    bad = [i for i, r in enumerate(recs) if r["error"] != ref.OK]
    want = dict(items=len(recs), blocks=sum(r["blocks"] for r in recs), decoded_bytes=int(ends[-1]), first_error=-1, error_offset=-1, error=0, reserved=0)
    if bad:
        want.update(first_error=bad[0], error_offset=recs[bad[0]]["error_offset"], error=recs[bad[0]]["error"])
    return want


def standin(rows, count):
    """the stand-in decoder's arrays for `count` table rows"""
    dec_results, dec_len, dec_at, blob = np.zeros(count + 1, np.int32), np.zeros(count + 1, np.int32), np.zeros(count + 1, np.int64), []
    at = 0
    for k, (_, size, raw, badsum, res, data) in enumerate(rows[:count]):
        dec_results[k], dec_len[k], dec_at[k] = res, 0 if raw or badsum else size, at
        blob.append(data)
        at += len(data)
    return dec_results, dec_len, dec_at, u8(b"".join(blob) + b"\0")


def check_decode_batch(oracle, src, off, slot=0, max_blocks=None, round_blocks=0, verify=3, dst_cap=None, grid=0):
    """the emulator path on the batch against the twin reader on every item alone: every record field by field, the batch's record,
    dst_off, written_items, the output bytes, nothing written outside them -> (records, contents, batch record)"""
    src, off = bytes(src), np.ascontiguousarray(off, np.int64)
    L, n = emu(), len(off) - 1
    slot_bytes = slot or (4 << 20)
    items = spans(src, off)
    recs, outs, rows, ends = expect_items(oracle, items, slot_bytes, verify, dst_cap)
    want = expect_batch(recs, ends)
    if max_blocks is None:
        max_blocks = max(len(rows), 1)
    full = len(rows) > max_blocks
    cap = int(ends[-1]) if dst_cap is None else dst_cap
    arrs = standin(rows, max_blocks)
    run = EmuRun(dec_results=arrs[0].ctypes.data, dec_len=arrs[1].ctypes.data, dec_at=arrs[2].ctypes.data, dec_bytes=arrs[3].ctypes.data,
                 dec_rows=max_blocks, grid=grid)
    a = Guarded(len(src))
    a.a[:] = u8(src)
    scratch = Guarded(L.emu_lz4f_batch_decode_scratch_bytes(n, slot, max_blocks, round_blocks))
    dst, dst_off, item_info, written = Guarded(cap), Guarded(8 * (n + 1)), Guarded(C.sizeof(Lz4fInfo) * n), Guarded(8)
    info = Lz4fBatchInfo()
    rc = L.emu_lz4f_batch_decode(a.ptr, len(src), off.ctypes.data, n, slot, max_blocks, round_blocks, verify, scratch.ptr, scratch.n, dst.ptr, cap,
                                 dst_off.ptr, item_info.ptr, C.byref(info), written.ptr, C.byref(run))
    assert rc == 0, run.error
    rounds = (max_blocks + (round_blocks or max_blocks) - 1) // (round_blocks or max_blocks)
    assert run.shape_errors == 0 and run.calls == (rounds if n else 0)
    assert scratch.intact() and dst.intact() and a.intact() and dst_off.intact() and item_info.intact() and written.intact()
    got = {f: int(getattr(info, f)) for f in BATCH_FIELDS}
    got_off = dst_off.a.view(np.int64)
    if full:
        assert got == dict(want, first_error=-1, error_offset=-1, error=ref.TABLE_FULL, decoded_bytes=0), got
        assert (dst.a == GUARD).all() and (got_off == 0).all() and int(written.a.view(np.int64)[0]) == 0
        got_recs = (Lz4fInfo * n).from_buffer_copy(item_info.a.tobytes())
        assert all(r.error == ref.TABLE_FULL for r in got_recs)
        return recs, outs, got
    assert got == want, {f: (got[f], want[f]) for f in BATCH_FIELDS if got[f] != want[f]}
    assert list(got_off) == list(ends)
    got_recs = (Lz4fInfo * n).from_buffer_copy(item_info.a.tobytes()) if n else []
    for i, (g, w) in enumerate(zip(got_recs, recs)):
        g = {f: int(getattr(g, f)) for f in INFO_FIELDS}
        assert g == w, (i, {f: (g[f], w[f]) for f in INFO_FIELDS if g[f] != w[f]})
    content = b"".join(outs)[:cap]
    assert dst.a[:len(content)].tobytes() == content
    assert (dst.a[len(content):] == GUARD).all(), "bytes past the decoded ones were written"
    assert int(written.a.view(np.int64)[0]) == sum(1 for e in ends[1:] if e <= cap), "written_items: the prefix of items wholly inside dst_cap"
    return recs, outs, got


# ---- every fault of test_gpu_lz4f.test_every_outcome_once, as items ------------------------------------------------------------------
def outcome_items(oracle):
    """-> (good frame, its source, [(name, broken frame, expected error at slot 65536)]); the last two hold two faults each"""
    src = mixed(oracle)
    frame, rets, _ = ref.write_frame(oracle, src, 4, False, 7)
    at1 = 15 + 4 + 65536 + 4                                           # block 1's size field (block 0 is stored raw)
    assert rets[0] == 0 and rets[1] > 0
    wrong_size = bytearray(flip(frame, 6))
    wrong_size[14] = (ref.xxh32(bytes(wrong_size[4:14])) >> 8) & 0xFF
    faults = [
        ("short", b"abc", ref.BAD_MAGIC), ("magic", flip(frame, 1), ref.BAD_MAGIC), ("version", flip(frame, 4, 0x80), ref.BAD_HEADER),
        ("hc", flip(frame, 14), ref.HEADER_CHECKSUM), ("linked", ref.descriptor(4, 3, len(src), linked=True) + frame[15:], ref.UNSUPPORTED_LINKED),
        ("dict", ref.descriptor(4, 7, len(src), dict_id=5) + frame[15:], ref.UNSUPPORTED_DICT),
        ("slot", ref.write_frame(oracle, src[:70000], 6, False, 0)[0], ref.SLOT_TOO_SMALL),
        ("cut_field", frame[:at1 + 2], ref.TRUNCATED), ("cut_data", frame[:at1 + 100], ref.TRUNCATED), ("cut_end", frame[:-2], ref.TRUNCATED),
        ("block_size", frame[:at1] + ref.le32(65537) + frame[at1 + 4:], ref.BAD_BLOCK_SIZE),
        ("block_sum", flip(frame, at1 + 13, 0xFF), ref.BLOCK_CHECKSUM), ("content_size", bytes(wrong_size), ref.CONTENT_SIZE),
        ("content_sum", flip(frame, len(frame) - 1), ref.CONTENT_CHECKSUM),
        ("sum_and_content", flip(flip(frame, at1 + 13, 0xFF), len(frame) - 1), ref.BLOCK_CHECKSUM),
        ("sum_and_cut", flip(frame, at1 + 13, 0xFF)[:-2], ref.BLOCK_CHECKSUM),
    ]
    return frame, src, faults
