"""TEST INFRASTRUCTURE: the two emulator libraries of tests/simt/build_emu.py, each built and loaded once for every test file, the
ctypes aliases the tests type their entry points with, and the twins of the records every framing run record shares
(tests/simt/emu_framing.hpp: EmuCounters, EmuHostRun)."""
import ctypes as C
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "simt"))
from build_emu import build, build_framing  # noqa: E402

P, I64, I32, U32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32


class EmuCounters(C.Structure):
    """what the emulated device counted during a call, the state of its guard bytes after it and the recorded failure text; a run
    record embeds it as its anonymous last field `counters`, so the fields read as the record's own"""
    _fields_ = [("intact", I64), ("reserves", I64), ("moves", I64), ("uploads", I64), ("downloads", I64), ("syncs", I64), ("passes", I64),
                ("last_download", I64), ("image_bytes", I64), ("error", C.c_char * 160)]


class EmuHostRun(C.Structure):
    """the emulated device of an emu_host_* call: the block codec's stand-in and the grids in, the counters out"""
    _anonymous_ = ("counters",)
    _fields_ = [("results", P), ("bytes", P), ("grid_items", I32), ("grid_copy", I32), ("grid_walk", I32), ("pad", I32), ("counters", EmuCounters)]


@functools.lru_cache(maxsize=None)
def kernels(starved=False):
    """libsimt_kernels.so (or its 'starved' build): the block codec kernels and the host-pointer block batch calls"""
    L = C.CDLL(build(starved=starved))
    L.emu_compare.restype = C.c_ulonglong
    L.emu_steps.restype = C.c_ulonglong
    return L


@functools.lru_cache(maxsize=None)
def framing():
    """libsimt_framing.so: every framing path; checks once that the twins above have the C side's sizes"""
    L = C.CDLL(build_framing())
    L.emu_framing_sizeof.restype = I64
    assert L.emu_framing_sizeof(11) == C.sizeof(EmuHostRun) and L.emu_framing_sizeof(12) == C.sizeof(EmuCounters)
    return L
