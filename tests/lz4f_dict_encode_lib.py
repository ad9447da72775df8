"""TEST INFRASTRUCTURE: libsimt_lz4f_dict_encode.so (tests/simt/emu_lz4f_dict_encode.cpp) -- the encode of LZ4 frames with a dictionary
under the SIMT emulator, every block through the real encoders -- built with build_emu's recipe over the framing library's dependency
list, loaded once, its entry points typed, the twin of its run record, and the one-frame and batch calls between guard bytes."""
import ctypes as C
import functools
import os

import numpy as np

import emu_lib
import build_emu
from emu_lib import I32, I64, P, U32, Guarded, u8
from lz4f_cases import PlacedDict

SO = os.path.join(build_emu.HERE, "libsimt_lz4f_dict_encode.so")


class EncRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("grid", I32), ("waves_per_group", I32), ("plain_calls", I64), ("dict_calls", I64), ("primes", I64), ("primes_before_dict", I64),
                ("dict_uploads", I64), ("dict_bytes", I64), ("dict_first_byte", I64), ("dict_intact", I64), ("uploads_before_dict", I64),
                ("counters", emu_lib.EmuCounters)]


def build():
    deps = build_emu._files(os.path.join(build_emu.CSRC, "*.hpp"), os.path.join(build_emu.CSRC, "*.inc"), os.path.join(build_emu.HERE, "*.hpp"),
                            os.path.join(build_emu.HERE, "*.inc"))
    return build_emu._build(SO, "emu_lz4f_dict_encode.cpp", deps, ["-pthread"])


@functools.lru_cache(maxsize=None)
def emu():
    L = C.CDLL(build())
    U = C.c_uint
    L.emu_lz4f_dict_encode_sizeof.restype = I64
    assert L.emu_lz4f_dict_encode_sizeof(0) == C.sizeof(EncRun) and L.emu_lz4f_dict_encode_sizeof(1) == C.sizeof(emu_lib.EmuCounters)
    for name, args in (("emu_lz4f_dict_bound", [I64, C.c_int, U, I64, U32]), ("emu_lz4f_batch_dict_bound", [I64, I64, C.c_int, U, I64, U32]),
                       ("emu_lz4f_encode_dict_scratch_bytes", [I64, C.c_int, I64]), ("emu_lz4f_batch_encode_dict_scratch_bytes", [I64, I64, C.c_int, I64]),
                       ("emu_lz4f_plain_bound", [I64, C.c_int, U]), ("emu_lz4f_plain_batch_bound", [I64, I64, C.c_int, U]),
                       ("emu_lz4f_plain_encode_scratch_bytes", [I64, C.c_int]), ("emu_lz4f_plain_batch_encode_scratch_bytes", [I64, I64, C.c_int])):
        getattr(L, name).argtypes, getattr(L, name).restype = args, I64
    L.emu_lz4f_encode_dict.argtypes = [P, I64, P, I64, U32, C.c_int, U, P, I64, P, P, I64, P]
    L.emu_lz4f_batch_encode_dict.argtypes = [P, I64, P, I64, P, I64, U32, C.c_int, U, P, I64, P, P, I64, P]
    L.emu_lz4f_plain_encode.argtypes = [P, I64, C.c_int, U, P, I64, P, P, I64, P]
    L.emu_lz4f_plain_batch_encode.argtypes = [P, I64, P, I64, C.c_int, U, P, I64, P, P, I64, P]
    L.emu_lz4f_encode_dict_host.argtypes = [P, I64, P, I64, U32, C.c_int, U, P, I64, P, P]
    L.emu_lz4f_batch_encode_dict_host.argtypes = [P, I64, P, I64, P, I64, U32, C.c_int, U, P, I64, P, P]
    return L


FILL = 0xA7


def placed(b):
    g = Guarded(len(b))
    g.a[:] = u8(b)
    return g


def encode_one(src, d, dict_id=0, block_id=4, flags=0, odd=0, host=False, wpg=1, grid=0, plain=False):
    """one frame through the emulator, every buffer between guard bytes and the scratch of exactly the queried size -> (frame, run)"""
    L = emu()
    run, a, pd = EncRun(grid=grid, waves_per_group=wpg), placed(src), PlacedDict(d, odd)
    bound = L.emu_lz4f_plain_bound(len(src), block_id, flags) if plain else L.emu_lz4f_dict_bound(len(src), block_id, flags, len(d), dict_id)
    dst, out_len = Guarded(bound, FILL), Guarded(8)
    dict_args = (pd.ptr if d else None, len(d), dict_id)
    if host:
        rc = L.emu_lz4f_encode_dict_host(a.ptr, len(src), *dict_args, block_id, flags, dst.ptr, bound, out_len.ptr, C.byref(run))
        assert run.intact == 1 and run.dict_intact == 1
    elif plain:
        scratch = Guarded(L.emu_lz4f_plain_encode_scratch_bytes(len(src), block_id))
        rc = L.emu_lz4f_plain_encode(a.ptr, len(src), block_id, flags, dst.ptr, bound, out_len.ptr, scratch.ptr, scratch.n, C.byref(run))
        assert scratch.intact()
    else:
        scratch = Guarded(L.emu_lz4f_encode_dict_scratch_bytes(len(src), block_id, len(d)))
        rc = L.emu_lz4f_encode_dict(a.ptr, len(src), *dict_args, block_id, flags, dst.ptr, bound, out_len.ptr, scratch.ptr, scratch.n, C.byref(run))
        assert scratch.intact()
    assert rc == 0, run.error
    assert dst.intact() and a.intact() and pd.g.intact() and out_len.intact()
    n = int(out_len.a.view(np.int64)[0])
    assert 0 < n <= bound and (dst.a[n:] == FILL).all(), "bytes at or past the reported length were written"
    return dst.a[:n].tobytes(), run


def encode_batch(src, off, d, dict_id=0, block_id=4, flags=0, odd=0, host=False, wpg=1, grid=0, plain=False):
    """a batch through the emulator -> (dst_off, the bytes [0, dst_off[n]), run)"""
    L = emu()
    off = np.ascontiguousarray(off, np.int64)
    n = len(off) - 1
    run, a, pd = EncRun(grid=grid, waves_per_group=wpg), placed(src), PlacedDict(d, odd)
    bound = L.emu_lz4f_plain_batch_bound(n, len(src), block_id, flags) if plain else L.emu_lz4f_batch_dict_bound(n, len(src), block_id, flags, len(d), dict_id)
    dst, dst_off = Guarded(bound, FILL), Guarded(8 * (n + 1))
    dict_args = (pd.ptr if d else None, len(d), dict_id)
    if host:
        rc = L.emu_lz4f_batch_encode_dict_host(a.ptr, len(src), off.ctypes.data, n, *dict_args, block_id, flags, dst.ptr, bound, dst_off.ptr, C.byref(run))
        assert run.intact == 1 and run.dict_intact == 1
    elif plain:
        scratch = Guarded(L.emu_lz4f_plain_batch_encode_scratch_bytes(n, len(src), block_id))
        rc = L.emu_lz4f_plain_batch_encode(a.ptr, len(src), off.ctypes.data, n, block_id, flags, dst.ptr, bound, dst_off.ptr, scratch.ptr, scratch.n, C.byref(run))
        assert scratch.intact()
    else:
        scratch = Guarded(L.emu_lz4f_batch_encode_dict_scratch_bytes(n, len(src), block_id, len(d)))
        rc = L.emu_lz4f_batch_encode_dict(a.ptr, len(src), off.ctypes.data, n, *dict_args, block_id, flags, dst.ptr, bound, dst_off.ptr, scratch.ptr, scratch.n,
                                          C.byref(run))
        assert scratch.intact()
    assert rc == 0, run.error
    assert dst.intact() and a.intact() and pd.g.intact() and dst_off.intact()
    ends = dst_off.a.view(np.int64).copy()
    assert 0 <= ends[-1] <= bound and (dst.a[int(ends[-1]):] == FILL).all(), "bytes at or past the reported length were written"
    return ends, dst.a[:int(ends[-1])].tobytes(), run
