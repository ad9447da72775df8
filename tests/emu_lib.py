"""TEST INFRASTRUCTURE: the emulator libraries of tests/simt/build_emu.py -- three builds of the kernels' source (libsimt_kernels.so,
its 'starved' variant, and libsimt_dict.so with the dictionary mode's counters) and the one of the framing source
(libsimt_framing.so) -- each built and loaded once for every test file, the ctypes aliases the tests type their entry points with, the twins of the records every framing run record shares
(tests/simt/emu_framing.hpp: EmuCounters, EmuHostRun), and what every emulator test file shares: the argument error, the forced grids
and the guarded buffer."""
import ctypes as C
import functools
import os
import sys

import numpy as np

from lz4net_amd._lib import E_ARGUMENT  # noqa: F401  (the tests take it from here)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "simt"))
from build_emu import build, build_dict, build_framing  # noqa: E402

P, I64, I32, U32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32
GRIDS = (0, 1, 3)                               # the library's own grids, and grids forced to 1 and 3 workgroups
GUARD = 0x5A


def u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


class Guarded:
    """`nbytes` bytes at a multiple of 256 between guard bytes"""

    def __init__(self, nbytes, fill=GUARD):
        self.n = max(int(nbytes), 0)
        self.store = np.full(self.n + 768, GUARD, np.uint8)
        self.lead = (-self.store.ctypes.data) % 256 + 256
        self.a = self.store[self.lead:self.lead + self.n]
        self.a[:] = fill
        self.ptr = self.store.ctypes.data + self.lead

    def intact(self):
        return bool((self.store[:self.lead] == GUARD).all() and (self.store[self.lead + self.n:] == GUARD).all())


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
def dict_kernels():
    """libsimt_dict.so (tests/simt/emu_dict.cpp): the decode of block batches against a shared dictionary"""
    L = C.CDLL(build_dict())
    L.emu_dict_sizeof.restype = I64
    L.emu_dict_sizes_scratch_bytes.argtypes, L.emu_dict_sizes_scratch_bytes.restype = [I64], I64
    return L


@functools.lru_cache(maxsize=None)
def framing():
    """libsimt_framing.so: every framing path; checks once that the twins above have the C side's sizes"""
    L = C.CDLL(build_framing())
    L.emu_framing_sizeof.restype = I64
    assert L.emu_framing_sizeof(11) == C.sizeof(EmuHostRun) and L.emu_framing_sizeof(12) == C.sizeof(EmuCounters)
    return L
