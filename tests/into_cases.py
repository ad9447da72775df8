"""TEST INFRASTRUCTURE for the one-call decodes under the SIMT emulator (tests/test_simt_into.py and, for their span forms,
tests/test_simt_spans.py): the entry points of tests/simt/emu_into.inc, the record its stand-in decoder is fed and reports in, and a
buffer between guard bytes of its own fill."""
import ctypes as C
import functools

import numpy as np

import emu_lib
from emu_helpers import addr
from emu_lib import I32 as _I32, I64 as _I64, P as _P
from lz4net_amd._lib import StreamInfo, StreamsInfo, UnwrapInfo

GUARD, FILL = 64, 0xA5


class IntoEmuRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("results", _P), ("bytes", _P), ("src_off", _P), ("dst_off", _P), ("len", _P), ("cap", _P), ("rows", _I64), ("count", _I64),
                ("grid_items", _I32), ("grid_copy", _I32), ("grid_walk", _I32), ("pad", _I32), ("calls", _I64), ("shape_errors", _I64),
                ("decoded_rows", _I64), ("counters", emu_lib.EmuCounters)]


@functools.lru_cache(maxsize=None)
def lib():
    L = emu_lib.framing()
    L.emu_into_sizeof.restype = _I64
    assert [L.emu_into_sizeof(i) for i in range(4)] == [C.sizeof(s) for s in (IntoEmuRun, StreamInfo, StreamsInfo, UnwrapInfo)]
    L.emu_into_scratch_bytes.argtypes, L.emu_into_scratch_bytes.restype = [C.c_int, _I64, _I64], _I64
    L.emu_stream_decode_into.argtypes = [_P, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _P]
    L.emu_streams_decode_into.argtypes = [_P, _I64, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P]
    L.emu_unwrap_into.argtypes = [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]
    return L


class Buf:
    """`size` bytes of `fill` between guard bytes of the same value"""

    def __init__(self, size, fill=FILL):
        self.whole = np.full(size + 2 * GUARD, fill, np.uint8)
        self.a, self.ptr, self.size, self.fill = self.whole[GUARD:GUARD + size], addr(self.whole, GUARD), size, fill

    def guards_intact(self):
        return bool((self.whole[:GUARD] == self.fill).all() and (self.whole[GUARD + self.size:] == self.fill).all())


def run_record(results, truth, src_off, dst_off, lens, caps, rows, count, grid):
    keep = (np.array(list(results) + [0], np.int32), np.ascontiguousarray(np.concatenate([truth, np.zeros(8, np.uint8)])),
            np.array(list(src_off) + [0], np.int64), np.array(list(dst_off) + [0], np.int64), np.array(list(lens) + [0], np.int32),
            np.array(list(caps) + [0], np.int32))
    r = IntoEmuRun(rows=rows, count=count, grid_items=grid, grid_copy=grid, grid_walk=grid)
    r.results, r.bytes, r.src_off, r.dst_off, r.len, r.cap = (addr(a) for a in keep)
    return r, keep


def info_bytes(info):
    return bytes(memoryview(info))
