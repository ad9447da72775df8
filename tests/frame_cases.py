"""TEST INFRASTRUCTURE for the legacy frame under the SIMT emulator, shared by tests/test_simt_frame.py and tests/test_simt_compact.py:
the frame entry points of tests/simt/libsimt_framing.so, the reference reader (`walk` is parse_frame's header walk, `reader` adds
LZ4_uncompress_unknownOutputSize(in, out, size, chunk_size) per chunk), the corpora, and the index call with its table."""
import ctypes as C
import functools

import numpy as np

import emu_lib
import ref_records as rr
from emu_lib import Guarded, I32 as _I32, I64 as _I64, P as _P, u8
from lz4net_amd import legacy_frame as lf
from lz4net_amd._lib import FrameInfo

OK, BAD_MAGIC, TRUNCATED, BAD_SIZE, CORRUPT_BLOCK, TABLE_FULL = range(6)
MAGIC = lf.MAGIC.to_bytes(4, "little")


class FrameTables(C.Structure):
    _fields_ = [("max_chunks", _I64), ("src_off", _P), ("hdr_off", _P), ("dst_off", _P), ("src_len", _P), ("dst_cap", _P), ("result", _P),
                ("min_bad", _P), ("walk", _P), ("partial", _P)]


@functools.lru_cache(maxsize=None)
def emu():
    L = emu_lib.framing()
    L.emu_frame_sizeof.restype = _I64
    assert L.emu_frame_sizeof(0) == C.sizeof(FrameTables) and L.emu_frame_sizeof(1) == C.sizeof(FrameInfo)
    assert L.emu_frame_sizeof(2) == C.sizeof(emu_lib.EmuHostRun)
    for name, args in {"emu_frame_bound": [_I64, _I32], "emu_frame_encode_scratch_bytes": [_I64, _I32], "emu_frame_decode_scratch_bytes": [_I64]}.items():
        getattr(L, name).argtypes, getattr(L, name).restype = args, _I64
    L.emu_frame_tables.argtypes, L.emu_frame_tables.restype = [_P, _I64, _P], None
    L.emu_frame_encode.argtypes = [_P, _I64, _I32, C.c_int, _P, _I64, _P, _P, _I64, _P, _P, C.c_int, C.c_char_p, C.c_int]
    L.emu_frame_index.argtypes = [_P, _I64, _I32, _I64, _P, _I64, _P, C.c_int, C.c_char_p, C.c_int]
    L.emu_frame_decode.argtypes = [_P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, C.c_int, C.c_char_p, C.c_int]
    L.emu_frame_index_run.argtypes = [_P, _I64, _I32, _P, _P, C.c_int]
    L.emu_frame_decode_run.argtypes = [_P, _P, _P, _P, _P, _P, _P, C.c_int]
    L.emu_host_frame_encode.argtypes = [_P, _I64, _I32, C.c_int, _P, _I64, _P, _P]
    L.emu_host_frame_decode.argtypes = [_P, _I64, _I32, _P, _I64, _P, _P]
    return L


def bound(n):
    return n + n // 255 + 16


# ---- the reference ------------------------------------------------------------------------------------------------------------
def walk(frame, chunk):
    """decode_file's header walk -> (chunks as parse_frame gives them, header error, its offset)"""
    frame = bytes(frame)
    if len(frame) < 4 or frame[:4] != MAGIC:
        return [], BAD_MAGIC, 0
    pos, chunks = 4, []
    while pos < len(frame):
        if pos + 4 > len(frame):
            return chunks, TRUNCATED, pos
        size = int.from_bytes(frame[pos:pos + 4], "little")
        if size == lf.MAGIC:
            pos += 4
            continue
        if size > bound(chunk):
            return chunks, BAD_SIZE, pos
        if pos + 4 + size > len(frame):
            return chunks, TRUNCATED, pos
        chunks.append((pos + 4, size))
        pos += 4 + size
    return chunks, OK, -1


def reader(oracle, frame, chunk):
    """What the frame is to the reference's reader: per chunk what LZ4_uncompress_unknownOutputSize(in, out, size, chunk) returns and
    wrote, and the FrameInfo that follows from it (bad chunks take no bytes)."""
    chunks, err, err_off = walk(frame, chunk)
    a = u8(frame)
    rets, outs = [], []
    for at, size in chunks:
        r, out = oracle.uncompress_unknown_raw(a[at:at + size], size, chunk)
        rets.append(r)
        outs.append(bytes(out[:r]) if r >= 0 else b"")
    offs = np.concatenate(([0], np.cumsum([len(o) for o in outs], dtype=np.int64))).astype(np.int64)
    bad = [k for k, r in enumerate(rets) if r < 0]
    if bad:
        want = (len(chunks), int(offs[-1]), int(offs[bad[0]]), chunks[bad[0]][0] - 4, CORRUPT_BLOCK)
    else:
        want = (len(chunks), int(offs[-1]), int(offs[-1]), err_off, err)
    return chunks, rets, outs, offs, want


def info_tuple(i):
    assert i.reserved == 0
    return (i.chunks, i.decoded_bytes, i.good_bytes, i.error_offset, i.error)


# ---- corpora --------------------------------------------------------------------------------------------------------------------
def sample(oracle, n, dist=2):
    return rr.frame_sample(oracle, n, dist) if n else b""


def make_frame(oracle, data, chunk, hc=False):
    a = u8(data)
    return MAGIC + b"".join(len(c).to_bytes(4, "little") + bytes(c) for c in (oracle.compress(a[i:i + chunk], hc=hc) for i in range(0, a.size, chunk)))


# ---- the index call and its table -------------------------------------------------------------------------------------------------
class Index:
    def __init__(self, frame, chunk, max_chunks, grid=0, chunk_arg=None):
        self.frame, self.chunk, self.max_chunks, self.grid = u8(frame), chunk, max_chunks, grid
        self.src = np.concatenate([self.frame, np.full(64, 0xEE, np.uint8)])      # (the kernels may not look at these: see `walk`)
        self.scratch = Guarded(emu().emu_frame_decode_scratch_bytes(max_chunks))
        self.info = FrameInfo(-7, -7, -7, -7, -7, -7)
        text = C.create_string_buffer(200)
        self.rc = emu().emu_frame_index(self.src.ctypes.data if self.frame.size else None, self.frame.size, chunk if chunk_arg is None else chunk_arg,
                                        max_chunks, self.scratch.ptr, self.scratch.n, C.addressof(self.info), grid, text, 200)
        self.text = text.value.decode()
        assert self.scratch.intact()
        t = FrameTables()
        emu().emu_frame_tables(self.scratch.ptr, max_chunks, C.addressof(t))
        col = lambda p, ty, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(ty)), shape=(max(n, 1),))[:n]    # noqa: E731
        self.src_off, self.hdr_off = col(t.src_off, C.c_int64, max_chunks), col(t.hdr_off, C.c_int64, max_chunks)
        self.dst_off = col(t.dst_off, C.c_int64, max_chunks + 1)
        self.src_len, self.dst_cap, self.result = (col(p, C.c_int32, max_chunks) for p in (t.src_len, t.dst_cap, t.result))

    def rows(self):
        n = min(self.info.chunks, self.max_chunks)
        return [(int(self.src_off[k]), int(self.src_len[k])) for k in range(n)]

    def decode(self, oracle, grid=None, guard=0xA7):
        """frame_decode with the oracle as the block decoder at the capacities the index found -> (rc, info, output with guards)"""
        n = min(self.info.chunks, self.max_chunks)
        total = int(self.info.decoded_bytes)
        results = np.zeros(n + 1, np.int32)
        decoded = np.full(total + 1, 0x33, np.uint8)
        for k in range(n):
            at, size, cap = int(self.src_off[k]), int(self.src_len[k]), int(self.dst_cap[k])
            r, out = oracle.uncompress_unknown_raw(self.frame[at:at + size], size, cap)
            results[k] = r
            decoded[self.dst_off[k]:self.dst_off[k] + cap] = out[:cap]
        dst = Guarded(total, fill=guard)
        info = FrameInfo(-7, -7, -7, -7, -7, -7)
        host = FrameInfo.from_buffer_copy(bytes(self.info))
        text = C.create_string_buffer(200)
        rc = emu().emu_frame_decode(self.src.ctypes.data, C.addressof(host), self.max_chunks, self.scratch.ptr, self.scratch.n, dst.ptr, total,
                                    C.addressof(info), results.ctypes.data, decoded.ctypes.data, self.grid if grid is None else grid, text, 200)
        assert dst.intact() and self.scratch.intact()
        return rc, info, dst
