"""TEST INFRASTRUCTURE for the LZ4 frame tests -- tests/test_simt_lz4f.py, tests/test_lz4f_interop.py and tests/test_gpu_lz4f.py: the
sources the frames are made of, and the emulator path (the lz4f entry points of tests/simt/libsimt_framing.so) checked against the
from-the-spec twin tests/lz4f_ref.py with the twin's per-block results and bytes as the stand-in codec."""
import ctypes as C
import functools

import numpy as np

import emu_lib
import lz4f_ref as ref
from emu_lib import GUARD, Guarded, I32 as _I32, I64 as _I64, P as _P, U32 as _U32, u8
from lz4net_amd._lib import Lz4fInfo

LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025)
INFO_FIELDS = [f for f, _ in Lz4fInfo._fields_]


class EmuRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("enc_results", _P), ("enc_bytes", _P), ("enc_len", _P), ("dec_results", _P), ("dec_len", _P), ("dec_at", _P), ("dec_bytes", _P), ("dec_rows", _I64),
                ("grid", _I32), ("pad", _I32), ("calls", _I64), ("shape_errors", _I64), ("counters", emu_lib.EmuCounters)]


@functools.lru_cache(maxsize=None)
def emu():
    L = emu_lib.framing()
    L.emu_lz4f_sizeof.restype = _I64
    assert L.emu_lz4f_sizeof(0) == C.sizeof(Lz4fInfo) == L.emu_lz4f_sizeof(2) and L.emu_lz4f_sizeof(1) == C.sizeof(EmuRun)
    L.emu_xxh32_serial.argtypes, L.emu_xxh32_serial.restype = [_P, _I64, _U32], _U32
    L.emu_xxh32_rows.argtypes = [_P, _P, _I64, _P, _I64, _U32, _P, _I64, C.c_int]
    L.emu_lz4f_bound.argtypes, L.emu_lz4f_bound.restype = [_I64, C.c_int, C.c_uint], _I64
    L.emu_lz4f_encode_scratch_bytes.argtypes, L.emu_lz4f_encode_scratch_bytes.restype = [_I64, C.c_int], _I64
    L.emu_lz4f_decode_scratch_bytes.argtypes, L.emu_lz4f_decode_scratch_bytes.restype = [_I32, _I64, _I64], _I64
    L.emu_lz4f_encode.argtypes = [_P, _I64, C.c_int, C.c_int, C.c_uint, _P, _I64, _P, _P, _I64, _P]
    L.emu_lz4f_decode.argtypes = [_P, _I64, _I32, _I64, _I64, C.c_uint, _P, _I64, _P, _I64, _P, _P]
    L.emu_lz4f_encode_host.argtypes = [_P, _I64, C.c_int, C.c_int, C.c_uint, _P, _I64, _P, _P]
    L.emu_lz4f_decode_host.argtypes = [_P, _I64, C.c_uint, _P, _I64, _P, _P]
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


# ---- the emulator path against the twin -----------------------------------------------------------------------------------------
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
    run = EmuRun(enc_results=enc_results.ctypes.data, enc_bytes=enc_bytes.ctypes.data, enc_len=enc_len.ctypes.data, grid=grid)
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


def check_decode(oracle, frame, slot=0, max_blocks=8, round_blocks=0, verify=3, dst_cap=None, grid=0):
    """the emulator path on `frame` against the twin reader: the record field by field, the output bytes, nothing written past them"""
    frame = bytes(frame)
    L = emu()
    slot_bytes = slot or (4 << 20)
    want, out, rows = ref.read_frame(oracle, frame, slot_bytes, max_blocks, verify, dst_cap)
    cap = want["decoded_bytes"] if dst_cap is None else dst_cap
    dec_results = np.zeros(max_blocks, np.int32)
    dec_len = np.zeros(max_blocks, np.int32)
    dec_at = np.zeros(max_blocks, np.int64)
    blob = b""
    for k, (at, size, raw, badsum, res, data) in enumerate(rows):
        dec_results[k], dec_len[k], dec_at[k] = res, 0 if raw or badsum else size, len(blob)
        blob += data
    dec_bytes = u8(blob + b"\0")
    run = EmuRun(dec_results=dec_results.ctypes.data, dec_len=dec_len.ctypes.data, dec_at=dec_at.ctypes.data, dec_bytes=dec_bytes.ctypes.data,
                 dec_rows=max_blocks, grid=grid)
    a = Guarded(len(frame))
    a.a[:] = u8(frame)
    scratch = Guarded(L.emu_lz4f_decode_scratch_bytes(slot, max_blocks, round_blocks))
    dst = Guarded(cap)
    info = Lz4fInfo()
    rc = L.emu_lz4f_decode(a.ptr, len(frame), slot, max_blocks, round_blocks, verify, scratch.ptr, scratch.n, dst.ptr, cap, C.byref(info), C.byref(run))
    assert rc == 0, run.error
    assert run.shape_errors == 0 and run.calls == (max_blocks + (round_blocks or max_blocks) - 1) // (round_blocks or max_blocks)
    assert scratch.intact() and dst.intact() and a.intact()
    got = {f: int(getattr(info, f)) for f in INFO_FIELDS}
    assert got == want, {f: (got[f], want[f]) for f in INFO_FIELDS if got[f] != want[f]}
    assert dst.a[:len(out)].tobytes() == out
    assert (dst.a[len(out):] == GUARD).all(), "bytes past the decoded ones were written"
    return want, out
