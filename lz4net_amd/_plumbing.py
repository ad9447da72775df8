"""What every front-end module does around a library call, written once: argument checks, the per-call device context, reading a
record back, "call, read, grow, call again", and the host size query.  stream.py, wrap.py, legacy_frame.py, lz4_frame.py, batch.py and
codec.py are written over it.  Importable without torch: the functions that touch tensors import it when they are called.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .codec import ArgumentException

BAD_OFFSETS = "offsets are invalid for the given buffer"


def mode(high_compression) -> int:
    return _lib.MODE_HC if high_compression else _lib.MODE_FAST


def compress_bound(n: int) -> int:
    return n + n // 255 + 16                                       # LZ4_compressBound, original/lz4.h:85-86


# ---- host memory ---------------------------------------------------------------------------------------------------------------------

def host_bytes(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def host_blocks(src, src_off, src_len, dst, dst_off, dst_cap, result):
    """lz4hip_batch_t over numpy arrays: block i is src[src_off[i]:][:src_len[i]] -> dst[dst_off[i]:][:dst_cap[i]]"""
    n = len(src_len)
    return _lib.Batch(src=src.ctypes.data, src_off=src_off.ctypes.data, src_stride=0, src_len=src_len.ctypes.data,
                      dst=dst.ctypes.data, dst_off=dst_off.ctypes.data, dst_stride=0, dst_cap=dst_cap.ctypes.data,
                      dst_cap_all=0, src_len_all=0, result=result.ctypes.data, n_blocks=n)


def check_host_batch(buf, offsets):
    """a batch in host memory: a 1-D uint8 array and its int64 offsets[n + 1]; bytes-like buffers are taken as uint8 arrays"""
    if isinstance(buf, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(buf, dtype=np.uint8)
    if not isinstance(buf, np.ndarray) or buf.dtype != np.uint8 or buf.ndim != 1:
        raise ArgumentException("the buffer must be a 1-D uint8 array")
    if not isinstance(offsets, np.ndarray) or offsets.dtype != np.int64 or offsets.ndim != 1:
        raise ArgumentException("offsets must be a 1-D int64 array")
    if offsets.size < 1:
        raise ArgumentException("offsets must hold n + 1 entries")
    return np.ascontiguousarray(buf), np.ascontiguousarray(offsets)


def sized_decode_host(call, info, after_e_argument_only: bool = False):
    """A host decode into exactly the bytes it produces: call(dst, dst_cap) -> rc fills `info`; a size query first (dst_cap = 0:
    LZ4HIP_E_ARGUMENT with info.decoded_bytes filled in), then the call that decodes.  Returns the decoded bytes as a uint8 array;
    the outcome is info.error.

    The two guards of the second call are the ones the fronts had, and they differ: any of these calls can fill in a decoded_bytes > 0
    and still answer the query with LZ4HIP_E_DEVICE (a header walk that did not settle, a copy that failed).  The frame fronts do not
    call again then (after_e_argument_only); the batch fronts do, on decoded_bytes > 0 alone."""
    rc = call(None, 0)
    out = np.empty(max(int(info.decoded_bytes), 1), np.uint8)
    if info.decoded_bytes > 0 and (rc == _lib.E_ARGUMENT or not after_e_argument_only):
        rc = call(out.ctypes.data, int(info.decoded_bytes))
    if rc != info.error:                                              # (the outcome itself is info.error)
        _lib.check(rc)
    return out[:int(info.decoded_bytes)]


# ---- device memory: torch CUDA tensors -----------------------------------------------------------------------------------------------

def is_device_vector(t, dtype: str) -> bool:
    import torch
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, dtype) and t.dim() == 1


def check_device_bytes(t, name):
    if not is_device_vector(t, "uint8"):
        raise ArgumentException(f"{name} must be a 1-D uint8 CUDA tensor")
    return t.contiguous()


def check_device_batch(buf, offsets):
    """a batch on the device: a 1-D uint8 CUDA tensor and its int64 offsets[n + 1]"""
    if not is_device_vector(buf, "uint8"):
        raise ArgumentException("the buffer must be a 1-D uint8 CUDA tensor")
    if not is_device_vector(offsets, "int64"):
        raise ArgumentException("offsets must be a 1-D int64 CUDA tensor")
    if offsets.numel() < 1:
        raise ArgumentException("offsets must hold n + 1 entries")
    if offsets.device != buf.device:
        raise ArgumentException("the buffer and the offsets must be on the same device")
    return buf.contiguous(), offsets.contiguous()


def check_device_spans(buf, begin, end):
    """chosen items of an arena on the device: a 1-D uint8 CUDA tensor and the int64 begin[m], end[m] of its spans"""
    if not is_device_vector(buf, "uint8"):
        raise ArgumentException("the buffer must be a 1-D uint8 CUDA tensor")
    for t in (begin, end):
        if not is_device_vector(t, "int64"):
            raise ArgumentException("begin and end must be 1-D int64 CUDA tensors")
        if t.device != buf.device:
            raise ArgumentException("the buffer and the spans must be on the same device")
    if begin.numel() != end.numel():
        raise ArgumentException("begin and end must have the same length")
    return buf.contiguous(), begin.contiguous(), end.contiguous()


def check_out(out, like):
    if not is_device_vector(out, "uint8") or not out.is_contiguous():
        raise ArgumentException("out must be a contiguous 1-D uint8 CUDA tensor")
    if out.device != like.device:
        raise ArgumentException("out must be on the source's device")
    return out


class DeviceCall:
    """One front-end call on the device of the tensor `like`: entered, that device is torch's current one; .lib is the library,
    .stream the handle of torch's current stream there, and u8 / i32 / i64 / record allocate what a call leaves its results in."""

    def __init__(self, like):
        import torch
        self._torch, self.device = torch, like.device
        self._guard = torch.cuda.device(like.device)

    def __enter__(self):
        self._guard.__enter__()
        self.lib = _lib.lib()
        self.stream = self._torch.cuda.current_stream(self.device).cuda_stream
        return self

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)

    def _new(self, n, dtype, zero):
        return (self._torch.zeros if zero else self._torch.empty)(n, dtype=dtype, device=self.device)

    def u8(self, n, zero: bool = False):
        return self._new(n, self._torch.uint8, zero)

    def i32(self, n, zero: bool = False):
        return self._new(n, self._torch.int32, zero)

    def i64(self, n, zero: bool = False):
        return self._new(n, self._torch.int64, zero)

    def record(self, cls):
        """room for one info record of the library, zeroed; read_record reads it back"""
        return self.u8(C.sizeof(cls), zero=True)

    def items(self, n):
        """what a batch call writes per item -> (out_off[n + 1], status[max(n, 1)])"""
        return self.i64(n + 1), self.i32(max(n, 1))


def read_record(t, cls):
    """The record a call left in the device tensor `t`, as its ctypes struct.  The one place that copies a record from the device,
    and it waits for the device."""
    return cls.from_buffer_copy(t.cpu().numpy().tobytes())


def settle(passes: int, guess, step):
    """Call, read the record, grow, call again: step(guess) -> (what the pass left, the next guess or None when this one held), at
    most `passes` times -> (what the last pass left, the guess after it).  A loop that runs out returns the guess its last pass asked
    for, with what that pass left for the one before: what that means is the caller's business."""
    for _ in range(passes):
        left, again = step(guess)
        if again is None:
            break
        guess = again
    return left, guess


def table_or_output(info, rows: str, table_full: int, guess):
    """The second half of a settle() step for a one-call decode that can outgrow its table or its output: the next (table rows,
    output bytes) after the record `info` -- the count in its field `rows` when info.error is `table_full`, else decoded_bytes when
    that exceeds the output -- or None when both held."""
    table, out_bytes = guess
    if info.error == table_full:
        return int(getattr(info, rows)), out_bytes
    if info.decoded_bytes > out_bytes:
        return table, int(info.decoded_bytes)
    return None
