"""TEST INFRASTRUCTURE for the LZ4 frame tests (tests/test_simt_lz4f*.py, tests/test_lz4f*_interop.py, tests/test_gpu_lz4f*.py): the
sources the frames are made of, the lz4f entry points of tests/simt/libsimt_framing.so, and ONE harness that drives a decode call and
checks it against the from-the-spec twin tests/lz4f_ref.py: what the twin expects of a frame or a batch (expect), the comparisons
(check_records, check_image), and the emulator's one-frame and batch calls between guard bytes (check_frame, check_batch), whichever
emulator path they drive (PLAIN, LINKED, DICT, DICT_PLAIN below)."""
import collections
import ctypes as C
import functools

import numpy as np

import emu_lib
import lz4f_ref as ref
from emu_lib import E_ARGUMENT, GUARD, Guarded, I32 as _I32, I64 as _I64, P as _P, U32 as _U32, u8
from lz4net_amd._lib import Lz4fBatchInfo, Lz4fInfo

LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025)
INFO_FIELDS = [f for f, _ in Lz4fInfo._fields_]
BATCH_FIELDS = [f for f, _ in Lz4fBatchInfo._fields_]
BAD_ITEM = dict(blocks=0, decoded_bytes=0, good_bytes=0, error_offset=-1, content_size=-1, frame_bytes=0, error=E_ARGUMENT, kind=0, block_max=0,
                flg=0, bd=0, checks=0)
ACCEPT = ref.ACCEPT_LINKED


# ---- the run records of tests/simt/emu_lz4f.inc, emu_lz4f_batch.inc and emu_lz4f_dict.inc --------------------------------------------------
class FrameRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("enc_results", _P), ("enc_bytes", _P), ("enc_len", _P), ("dec_results", _P), ("dec_len", _P), ("dec_at", _P), ("dec_bytes", _P), ("dec_rows", _I64),
                ("grid", _I32), ("pad", _I32), ("calls", _I64), ("shape_errors", _I64), ("counters", emu_lib.EmuCounters)]


class BatchRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("enc_results", _P), ("enc_bytes", _P), ("enc_at", _P), ("enc_len", _P), ("enc_src", _P), ("enc_rows", _I64),
                ("dec_results", _P), ("dec_len", _P), ("dec_at", _P), ("dec_bytes", _P), ("dec_rows", _I64),
                ("grid", _I32), ("pad", _I32), ("calls", _I64), ("shape_errors", _I64), ("counters", emu_lib.EmuCounters)]


class DictRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("grid", _I32), ("pad", _I32), ("plain_calls", _I64), ("dict_calls", _I64), ("dict_uploads", _I64), ("dict_bytes", _I64),
                ("dict_first_byte", _I64), ("dict_intact", _I64), ("uploads_before_dict", _I64), ("counters", emu_lib.EmuCounters)]


@functools.lru_cache(maxsize=None)
def emu():
    L = emu_lib.framing()
    frame_args = [_P, _I64, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P]
    batch_args = [_P, _I64, _P, _I64, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]
    for sizeof in (L.emu_lz4f_sizeof, L.emu_lz4f_batch_sizeof, L.emu_lz4f_dict_sizeof):
        sizeof.restype = _I64
    assert L.emu_lz4f_sizeof(0) == C.sizeof(Lz4fInfo) == L.emu_lz4f_sizeof(2) and L.emu_lz4f_sizeof(1) == C.sizeof(FrameRun)
    L.emu_xxh32_serial.argtypes, L.emu_xxh32_serial.restype = [_P, _I64, _U32], _U32
    L.emu_xxh32_rows.argtypes = [_P, _P, _I64, _P, _I64, _U32, _P, _I64, C.c_int]
    L.emu_lz4f_bound.argtypes, L.emu_lz4f_bound.restype = [_I64, C.c_int, C.c_uint], _I64
    L.emu_lz4f_encode_scratch_bytes.argtypes, L.emu_lz4f_encode_scratch_bytes.restype = [_I64, C.c_int], _I64
    L.emu_lz4f_decode_scratch_bytes.argtypes, L.emu_lz4f_decode_scratch_bytes.restype = [_I32, _I64, _I64], _I64
    L.emu_lz4f_encode.argtypes = [_P, _I64, C.c_int, C.c_int, C.c_uint, _P, _I64, _P, _P, _I64, _P]
    L.emu_lz4f_decode.argtypes = frame_args
    L.emu_lz4f_encode_host.argtypes = [_P, _I64, C.c_int, C.c_int, C.c_uint, _P, _I64, _P, _P]
    L.emu_lz4f_decode_host.argtypes = [_P, _I64, C.c_uint, _P, _I64, _P, _P]
    # batches, and frames with linked blocks
    assert L.emu_lz4f_batch_sizeof(0) == C.sizeof(Lz4fInfo) and L.emu_lz4f_batch_sizeof(1) == C.sizeof(BatchRun)
    assert L.emu_lz4f_batch_sizeof(2) == C.sizeof(Lz4fBatchInfo) and L.emu_lz4f_batch_sizeof(3) == C.sizeof(emu_lib.EmuCounters)
    L.emu_lz4f_batch_bound.argtypes, L.emu_lz4f_batch_bound.restype = [_I64, _I64, C.c_int, C.c_uint], _I64
    L.emu_lz4f_batch_encode_scratch_bytes.argtypes, L.emu_lz4f_batch_encode_scratch_bytes.restype = [_I64, _I64, C.c_int], _I64
    L.emu_lz4f_batch_decode_scratch_bytes.argtypes, L.emu_lz4f_batch_decode_scratch_bytes.restype = [_I64, _I32, _I64, _I64], _I64
    L.emu_lz4f_batch_encode.argtypes = [_P, _I64, _P, _I64, C.c_int, C.c_int, C.c_uint, _P, _I64, _P, _P, _I64, _P]
    L.emu_lz4f_batch_decode.argtypes = batch_args
    L.emu_lz4f_batch_encode_host.argtypes = [_P, _I64, _P, _I64, C.c_int, C.c_int, C.c_uint, _P, _I64, _P, _P]
    L.emu_lz4f_batch_decode_host.argtypes = [_P, _I64, _P, _I64, C.c_uint, _P, _I64, _P, _P, _P, _P]
    L.emu_lz4f_linked_decode_scratch_bytes.argtypes, L.emu_lz4f_linked_decode_scratch_bytes.restype = [_I32, _I64, _I64], _I64
    L.emu_lz4f_linked_decode.argtypes = frame_args
    L.emu_lz4f_linked_decode_host.argtypes = [_P, _I64, C.c_uint, _P, _I64, _P, _P]
    L.emu_lz4f_linked_batch_decode.argtypes = batch_args
    L.emu_lz4f_linked_batch_decode_host.argtypes = [_P, _I64, _P, _I64, C.c_uint, _P, _I64, _P, _P, _P, _P]
    # frames with a dictionary
    assert L.emu_lz4f_dict_sizeof(0) == C.sizeof(Lz4fInfo) and L.emu_lz4f_dict_sizeof(1) == C.sizeof(DictRun)
    assert L.emu_lz4f_dict_sizeof(2) == C.sizeof(Lz4fBatchInfo) and L.emu_lz4f_dict_sizeof(3) == C.sizeof(emu_lib.EmuCounters)
    L.emu_lz4f_dict_decode_scratch_bytes.argtypes, L.emu_lz4f_dict_decode_scratch_bytes.restype = [_I32, _I64, _I64], _I64
    L.emu_lz4f_dict_batch_decode_scratch_bytes.argtypes, L.emu_lz4f_dict_batch_decode_scratch_bytes.restype = [_I64, _I32, _I64, _I64], _I64
    L.emu_lz4f_dict_decode.argtypes = frame_args[:2] + [_P, _I64, _U32] + frame_args[2:]
    L.emu_lz4f_dict_batch_decode.argtypes = batch_args[:4] + [_P, _I64, _U32] + batch_args[4:]
    L.emu_lz4f_dict_plain_decode.argtypes = frame_args
    L.emu_lz4f_dict_plain_batch_decode.argtypes = batch_args
    L.emu_lz4f_dict_decode_host.argtypes = [_P, _I64, _P, _I64, _U32, C.c_uint, _P, _I64, _P, _P]
    L.emu_lz4f_dict_batch_decode_host.argtypes = [_P, _I64, _P, _I64, _P, _I64, _U32, C.c_uint, _P, _I64, _P, _P, _P, _P]
    return L


# ---- sources ---------------------------------------------------------------------------------------------------------------------
def sample(oracle, dist, n):
    """n bytes: 0 zeros, 1 random, 2 / 3 the oracle's D2 / D3 generators"""
    if dist == 0:
        return bytes(n)
    if dist == 1:
        return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    return oracle.gen(dist, 5, 0, (n + 65535) // 65536 or 1).reshape(-1)[:n].tobytes()


def mixed(oracle, block=65536):
    """raw and compressed blocks inside one frame: random, D2, zeros, D3, and a ragged random end"""
    return sample(oracle, 1, block) + sample(oracle, 2, block) + sample(oracle, 0, block) + sample(oracle, 3, block) + sample(oracle, 1, 5)


def flip(frame, at, x=0x01):
    b = bytearray(frame)
    b[at] ^= x
    return bytes(b)


def offsets_of(items):
    return np.cumsum([0] + [len(b) for b in items]).astype(np.int64)


def spans(src, off):
    """item i of the batch, or None for offsets that decrease or leave the buffer"""
    out = []
    for a, b in zip(off[:-1], off[1:]):
        out.append(bytes(src[a:b]) if 0 <= a <= b <= len(src) else None)
    return out


# ---- the one-frame encode path against the twin ----------------------------------------------------------------------------------
def emu_encode(oracle, src, block_id=4, hc=False, flags=0, grid=0, host=False):
    """the emulator path's frame, with the twin writer's per-block encoder results and bytes as the stand-in codec"""
    src = bytes(src)
    L = emu()
    bid = block_id or 4
    want, rets, datas = ref.write_frame(oracle, src, bid, hc, flags)
    stride = min(len(src), ref.block_bytes(bid))
    enc_results = np.array(rets + [0], np.int32)
    enc_bytes = np.zeros(len(rets) * stride + 1, np.uint8)
    for j, d in enumerate(datas):
        enc_bytes[j * stride:j * stride + len(d)] = u8(d)
    enc_len = np.array([len(b) for b in ref.cut(src, bid)] + [0], np.int32)
    run = FrameRun(enc_results=enc_results.ctypes.data, enc_bytes=enc_bytes.ctypes.data, enc_len=enc_len.ctypes.data, grid=grid)
    bound = L.emu_lz4f_bound(len(src), block_id, flags)
    assert bound >= len(want)
    a = u8(src + b"\0")
    dst = Guarded(bound)
    out_len = np.full(1, -1, np.int64)
    if host:
        rc = L.emu_lz4f_encode_host(a.ctypes.data, len(src), block_id, int(hc), flags, dst.ptr, bound, out_len.ctypes.data, C.byref(run))
        assert run.intact == 1 and run.syncs >= 1
    else:
        scratch = Guarded(L.emu_lz4f_encode_scratch_bytes(len(src), block_id))
        rc = L.emu_lz4f_encode(a.ctypes.data, len(src), block_id, int(hc), flags, dst.ptr, bound, out_len.ctypes.data, scratch.ptr, scratch.n, C.byref(run))
        assert scratch.intact()
    assert rc == 0, run.error
    assert dst.intact() and run.shape_errors == 0, "the block encoder was not handed the blocks' lengths and lengths - 1 of room"
    got = dst.a[:int(out_len[0])].tobytes()
    assert (dst.a[int(out_len[0]):] == GUARD).all(), "bytes past the frame's end were written"
    assert got == want, (len(got), len(want))
    return got


# ---- what the twin expects of a decode call ------------------------------------------------------------------------------------------
def expect(codec, frames, slot_bytes, verify, dst_cap=None, max_blocks=1 << 30, accept=False, dictionary=b"", dict_id=0):
    """what the twin says of every item of a batch (None: an item with bad offsets) -> (records, [(written and specified bytes, the
    item's bytes behind them unspecified)], rows of all items for the stand-in codec, prefix sums of the decoded sizes, the cap)"""
    def read(f, room):
        if f is None:
            return dict(BAD_ITEM), b"", False, []
        return ref.read_frame(codec, f, slot_bytes, max_blocks, verify, room, accept, dictionary, dict_id)

    ends = np.cumsum([0] + [read(f, None)[0]["decoded_bytes"] for f in frames]).astype(np.int64)
    cap = int(ends[-1]) if dst_cap is None else dst_cap
    recs, outs, rows = [], [], []
    for i, f in enumerate(frames):
        info, out, unspecified, r = read(f, cap - int(ends[i]))
        recs.append(info)
        outs.append((out, unspecified))
        rows += r
    return recs, outs, rows, ends, cap


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


def records_of(item_info, n):
    got = (Lz4fInfo * n).from_buffer_copy(bytes(item_info)) if n else []
    return [{f: int(getattr(g, f)) for f in INFO_FIELDS} for g in got]


def check_records(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, {f: (g[f], w[f]) for f in INFO_FIELDS if g[f] != w[f]})


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


def check_call(got, want, fill, table_full=False):
    """one decode call's (batch record, item records, dst_off, dst, written_items) against expect()'s answer: the batch record, dst_off
    against the prefix sums, every record field by field, the image of dst, written_items; a table that is too small takes nothing"""
    (batch, got_recs, got_off, dst, written), (recs, outs, _, ends, cap) = got, want
    want_batch = expect_batch(recs, ends)
    if table_full:
        assert batch == dict(want_batch, first_error=-1, error_offset=-1, error=ref.TABLE_FULL, decoded_bytes=0), batch
        assert (np.asarray(dst) == fill).all() and (got_off == 0).all() and written == 0
        assert len(got_recs) == len(recs) and all(r["error"] == ref.TABLE_FULL for r in got_recs)
        return
    assert batch == want_batch, {f: (batch[f], want_batch[f]) for f in BATCH_FIELDS if batch[f] != want_batch[f]}
    assert list(got_off) == list(ends), "dst_off are the prefix sums of the decoded sizes"
    check_records(got_recs, recs)
    check_image(dst, outs, ends, cap, fill)
    assert written == sum(1 for e in ends[1:] if e <= cap), "written_items: the prefix of items wholly inside dst_cap"


# ---- the emulator paths against the twin -------------------------------------------------------------------------------------------------
# PLAIN and LINKED hand every round to the stand-in codec of emu_lz4f.inc / emu_lz4f_batch.inc, keyed by global table row (LINKED: the
# linked rows run the real wavefront decoder, and are empty rows to the stand-in); DICT and DICT_PLAIN run the real kernels of
# emu_lz4f_dict.inc on every row, through the dictionary calls and through the plain calls of the same build.
Path = collections.namedtuple("Path", "frame frame_scratch frame_run batch batch_scratch batch_run standin dictionary")
PLAIN = Path("emu_lz4f_decode", "emu_lz4f_decode_scratch_bytes", FrameRun, "emu_lz4f_batch_decode", "emu_lz4f_batch_decode_scratch_bytes", BatchRun, True, False)
LINKED = Path("emu_lz4f_linked_decode", "emu_lz4f_linked_decode_scratch_bytes", BatchRun, "emu_lz4f_linked_batch_decode", "emu_lz4f_batch_decode_scratch_bytes",
              BatchRun, True, False)
DICT = Path("emu_lz4f_dict_decode", "emu_lz4f_dict_decode_scratch_bytes", DictRun, "emu_lz4f_dict_batch_decode", "emu_lz4f_dict_batch_decode_scratch_bytes",
            DictRun, False, True)
DICT_PLAIN = Path("emu_lz4f_dict_plain_decode", "emu_lz4f_dict_decode_scratch_bytes", DictRun, "emu_lz4f_dict_plain_batch_decode",
                  "emu_lz4f_dict_batch_decode_scratch_bytes", DictRun, False, False)


class PlacedDict:
    """the dictionary between guard bytes, at an even (odd = 0) or odd address"""
    def __init__(self, d, odd=0):
        self.g = Guarded(len(d) + odd)
        self.g.a[odd:] = u8(d)
        self.ptr, self.n = self.g.ptr + odd, len(d)


def _record(path, run_type, rows, max_blocks, grid):
    """the path's run record: the twin's rows as the stand-in codec where the path has one -> (record, what keeps its arrays alive)"""
    if not path.standin:
        return run_type(grid=grid), None
    arrs = standin(rows, max_blocks)
    return run_type(dec_results=arrs[0].ctypes.data, dec_len=arrs[1].ctypes.data, dec_at=arrs[2].ctypes.data, dec_bytes=arrs[3].ctypes.data,
                    dec_rows=max_blocks, grid=grid), arrs


def _dict_args(path, pd, dict_id):
    return [pd.ptr if pd.n else None, pd.n, dict_id] if path.dictionary else []


def _check_ran(path, run, rc, pd, max_blocks, round_blocks, items):
    """the call succeeded, and every round went once to the path's decoder: the stand-in (linked rows as empty rows), or the kernels
    with the dictionary where there is one and the plain ones where there is none"""
    assert rc == 0, run.error
    rounds = (max_blocks + (round_blocks or max_blocks) - 1) // (round_blocks or max_blocks) if items else 0
    if path.standin:
        assert run.shape_errors == 0 and run.calls == rounds
    else:
        assert (run.plain_calls, run.dict_calls) == ((0, rounds) if path.dictionary and pd.n else (rounds, 0))


def run_frame(path, frame, rows=(), d=b"", dict_id=0, slot=65536, max_blocks=1, round_blocks=0, flags=3, cap=0, grid=0, odd=0):
    """the emulator's one-frame decode in guarded buffers -> (record, dst bytes, run)"""
    L = emu()
    run, keep = _record(path, path.frame_run, rows, max_blocks, grid)
    a, pd = Guarded(len(frame)), PlacedDict(d, odd)
    a.a[:] = u8(frame)
    scratch = Guarded(getattr(L, path.frame_scratch)(slot, max_blocks, round_blocks))
    dst, info = Guarded(cap), Guarded(C.sizeof(Lz4fInfo))
    rc = getattr(L, path.frame)(a.ptr, len(frame), *_dict_args(path, pd, dict_id), slot, max_blocks, round_blocks, flags, scratch.ptr, scratch.n, dst.ptr, cap,
                                info.ptr, C.byref(run))
    _check_ran(path, run, rc, pd, max_blocks, round_blocks, 1)
    assert scratch.intact() and dst.intact() and a.intact() and info.intact() and pd.g.intact()
    return records_of(info.a.tobytes(), 1)[0], dst.a.copy(), run


def items_of(frames, off):
    """the items `frames`, or with off the items [off[i], off[i + 1]) of the buffer `frames` -> (buffer, offsets, items)"""
    if off is None:
        frames = list(frames)
        return b"".join(frames), offsets_of(frames), frames
    return bytes(frames), np.ascontiguousarray(off, np.int64), spans(frames, off)


def run_batch(path, frames, rows=(), d=b"", dict_id=0, slot=65536, max_blocks=1, round_blocks=0, flags=3, cap=0, grid=0, odd=0, off=None):
    """the emulator's batch decode in guarded buffers -> (batch record, item records, dst_off, dst bytes, written_items, run)"""
    L = emu()
    src, off, _ = items_of(frames, off)
    n = len(off) - 1
    run, keep = _record(path, path.batch_run, rows, max_blocks, grid)
    a, pd = Guarded(len(src)), PlacedDict(d, odd)
    a.a[:] = u8(src)
    scratch = Guarded(getattr(L, path.batch_scratch)(n, slot, max_blocks, round_blocks))
    dst, dst_off, item_info, written = Guarded(cap), Guarded(8 * (n + 1)), Guarded(C.sizeof(Lz4fInfo) * n), Guarded(8)
    info = Lz4fBatchInfo()
    rc = getattr(L, path.batch)(a.ptr, len(src), off.ctypes.data, n, *_dict_args(path, pd, dict_id), slot, max_blocks, round_blocks, flags, scratch.ptr, scratch.n,
                                dst.ptr, cap, dst_off.ptr, item_info.ptr, C.byref(info), written.ptr, C.byref(run))
    _check_ran(path, run, rc, pd, max_blocks, round_blocks, n)
    assert scratch.intact() and dst.intact() and a.intact() and dst_off.intact() and item_info.intact() and written.intact() and pd.g.intact()
    return ({f: int(getattr(info, f)) for f in BATCH_FIELDS}, records_of(item_info.a.tobytes(), n), dst_off.a.view(np.int64).copy(), dst.a.copy(),
            int(written.a.view(np.int64)[0]), run)


def check_frame(path, codec, frame, d=b"", dict_id=0, slot=65536, max_blocks=None, round_blocks=0, verify=3, dst_cap=None, grid=0, odd=0, accept=False):
    """the emulator's one-frame call against the twin: the record field by field, the image of dst, all guards, what ran
    -> (record, written bytes)"""
    frame, slot_bytes = bytes(frame), slot or (4 << 20)
    if max_blocks is None:
        max_blocks = max(len(ref.read_frame(codec, frame, slot_bytes, 1 << 30, verify, None, accept, d, dict_id)[3]), 1)
    if dst_cap is None:
        dst_cap = ref.read_frame(codec, frame, slot_bytes, max_blocks, verify, None, accept, d, dict_id)[0]["decoded_bytes"]
    want, out, unspecified, rows = ref.read_frame(codec, frame, slot_bytes, max_blocks, verify, dst_cap, accept, d, dict_id)
    got, dst, _ = run_frame(path, frame, rows, d, dict_id, slot, max_blocks, round_blocks, verify | (ACCEPT if accept else 0), dst_cap, grid, odd)
    check_records([got], [want])
    check_image(dst, [(out, unspecified)], [0, want["decoded_bytes"]], dst_cap, GUARD)
    return got, out


def check_batch(path, codec, frames, d=b"", dict_id=0, slot=65536, max_blocks=None, round_blocks=0, verify=3, dst_cap=None, grid=0, odd=0, accept=False,
                off=None):
    """the emulator's batch call on the items `frames` (with off: on the items [off[i], off[i + 1]) of the buffer `frames`) against the
    twin on every item alone: the batch's record, dst_off, every record field by field, the image of dst, written_items, all guards,
    what ran.  With the flag, the same items once more without it: the linked ones are refused and take no bytes, every other item has
    the same record and the same bytes -> (records, every item's written and specified bytes, batch record)"""
    src, off, frames = items_of(frames, off)
    slot_bytes = slot or (4 << 20)
    want = expect(codec, frames, slot_bytes, verify, dst_cap, 1 << 30, accept, d, dict_id)
    recs, outs, rows, ends, cap = want
    if max_blocks is None:
        max_blocks = max(len(rows), 1)
    got = run_batch(path, src, rows, d, dict_id, slot, max_blocks, round_blocks, verify | (ACCEPT if accept else 0), cap, grid, odd, off)
    check_call(got[:5], want, GUARD, len(rows) > max_blocks)
    if accept and len(rows) <= max_blocks:
        twin_recs, _, plain_rows, _, plain_cap = expect(codec, frames, slot_bytes, verify, None, 1 << 30, False, d, dict_id)
        _, plain_recs, plain_off, plain_dst, _, _ = run_batch(path, src, plain_rows, d, dict_id, slot, max(len(plain_rows), 1), round_blocks, verify, plain_cap,
                                                              grid, odd, off)
        for i, f in enumerate(frames):
            if f is not None and (ref.is_linked(f) or twin_recs[i]["error"] == ref.UNSUPPORTED_LINKED):
                assert plain_recs[i]["error"] == ref.UNSUPPORTED_LINKED and plain_off[i + 1] == plain_off[i]
            elif ends[i + 1] <= cap:
                assert plain_recs[i] == got[1][i], (i, "an independent item's record changed with the flag")
                assert plain_dst[plain_off[i]:plain_off[i + 1]].tobytes() == got[3][ends[i]:ends[i + 1]].tobytes(), (i, "the item's bytes changed with the flag")
    return recs, [out for out, _ in outs], got[0]
