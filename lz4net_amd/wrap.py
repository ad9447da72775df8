"""Batches of wrapped messages (LZ4Codec.Wrap / WrapHC / Unwrap, src/LZ4/LZ4Codec.cs:471-599) on the device: the lz4hip_wrap_* /
lz4hip_unwrap_* calls of include/lz4hip.h, kernels in csrc/lz4hip_wrap.hpp.

A batch of n messages is one 1-D uint8 buffer plus int64 offsets[n + 1]: message i is buf[offsets[i]:offsets[i + 1]].  wrap_* returns
the wrapped messages in that layout and unwrap_* reads it, so one's output is the other's input.  The bytes of each message are those
of LZ4Codec.Wrap / WrapHC / Unwrap; errors raise the exceptions Unwrap raises, with the failing message's index in .message_index.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, _plumbing as _p
from .codec import _CORRUPT, ArgumentException

_WRAP_INVALID = "inputBuffer size of inputLength is invalid"
_MESSAGES = {
    _lib.WRAP_SIZE_INVALID: "inputBuffer size is invalid",
    _lib.WRAP_CORRUPT_HEADER: "inputBuffer size is invalid or has been corrupted",
    _lib.WRAP_CORRUPT_BLOCK: _CORRUPT,
    _lib.E_ARGUMENT: _p.BAD_OFFSETS,
}


def unwrap_error(status: int, index: int) -> ArgumentException:
    """The exception LZ4Codec.Unwrap raises for a message with this status (LZ4HIP_WRAP_*, or LZ4HIP_E_ARGUMENT for bad offsets)."""
    e = ArgumentException(_MESSAGES.get(int(status), f"unwrap: unexpected status {int(status)}"))
    e.message_index = int(index)
    return e


# ---- device-resident batches (torch CUDA tensors, torch's current stream) ------------------------------------------------------

def wrap_device(src, offsets, high_compression: bool = False):
    """[LZ4Codec.Wrap(m) for m in messages] (WrapHC with high_compression) for the messages src[offsets[i]:offsets[i + 1]] of a CUDA
    tensor, on the device, on torch's current stream -> (packed, packed_offsets): packed_offsets[i] is where wrapped message i starts.
    Waits for the device once, to learn the total."""
    import torch
    src, offsets = _p.check_device_batch(src, offsets)
    with _p.DeviceCall(src) as d:
        n = offsets.numel() - 1
        bound = d.lib.lz4hip_wrap_bound(n, src.numel())
        out = d.u8(bound)
        out_off, result = d.items(n)
        scratch = d.u8(d.lib.lz4hip_wrap_scratch_bytes(n, src.numel()))
        _lib.check(d.lib.lz4hip_wrap_device(src.data_ptr(), src.numel(), offsets.data_ptr(), n, _p.mode(high_compression), out.data_ptr(), bound,
                                            out_off.data_ptr(), result.data_ptr(), scratch.data_ptr(), scratch.numel(), d.stream))
        lowest = result[:n].min().to(torch.int64).reshape(1) if n else d.i64(1, zero=True)
        total, lowest = torch.cat([out_off[n:], lowest]).tolist()
        if lowest < 0:
            raise ArgumentException(_WRAP_INVALID)
        return out[:total], out_off


def unwrap_device(packed, offsets, check: bool = True):
    """[LZ4Codec.Unwrap(w) for w in messages] for the wrapped messages packed[offsets[i]:offsets[i + 1]] of a CUDA tensor, on the device,
    on torch's current stream -> (data, data_offsets).  Every message with a valid header is decoded; with check=True the first failing
    message raises what Unwrap raises for it (ArgumentException, .message_index = its index), with check=False the per-message statuses
    (LZ4HIP_WRAP_*, 0 = fine) come back as a third value instead.  Waits for the device twice: to size the output, and for the outcome."""
    packed, offsets = _p.check_device_batch(packed, offsets)
    with _p.DeviceCall(packed) as d:
        n = offsets.numel() - 1
        out_off, status = d.items(n)
        scratch = d.u8(d.lib.lz4hip_unwrap_scratch_bytes(n))
        info_dev = d.record(_lib.UnwrapInfo)
        _lib.check(d.lib.lz4hip_unwrap_index_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, out_off.data_ptr(), status.data_ptr(),
                                                    scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(), d.stream))
        info = _p.read_record(info_dev, _lib.UnwrapInfo)
        out = d.u8(int(info.decoded_bytes))
        _lib.check(d.lib.lz4hip_unwrap_decode_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, C.byref(info), scratch.data_ptr(),
                                                     scratch.numel(), out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(),
                                                     info_dev.data_ptr(), d.stream))
        info = _p.read_record(info_dev, _lib.UnwrapInfo)
        if not check:
            return out, out_off, status[:n]
        if info.first_error >= 0:
            raise unwrap_error(info.error, info.first_error)
        return out, out_off


def _unwrap_into(entry, packed, where, n, out):
    """unwrap_into and unwrap_spans_into: the library call `entry` over the n messages that the tensors `where` locate in `packed`
    (offsets; or begin and end)"""
    out = _p.check_out(out, packed)
    with _p.DeviceCall(packed) as d:
        out_off, status = d.items(n)
        info, written = d.record(_lib.UnwrapInfo), d.i64(1, zero=True)
        scratch = d.u8(d.lib.lz4hip_unwrap_into_scratch_bytes(n))
        _lib.check(getattr(d.lib, entry)(packed.data_ptr(), packed.numel(), *(w.data_ptr() for w in where), n, scratch.data_ptr(), scratch.numel(),
                                         out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(), info.data_ptr(),
                                         written.data_ptr(), d.stream))
        return out_off, status[:n], info, written


def unwrap_into(packed, offsets, out):
    """unwrap_device into a tensor the caller already owns, in ONE device call on torch's current stream, without waiting for the
    device -> (out_off, status, info, written_messages), all device tensors: message i is out[out_off[i]:out_off[i + 1]], status is
    per message, info holds the lz4hip_unwrap_info_t record (read_unwrap_info, check_unwrap_into) and written_messages the int64 count
    of leading messages that fit `out`; the others are not written, and out_off and info.decoded_bytes are complete all the same."""
    packed, offsets = _p.check_device_batch(packed, offsets)
    return _unwrap_into("lz4hip_unwrap_into_device", packed, (offsets,), offsets.numel() - 1, out)


def select_spans(offsets, sel):
    """The spans of chosen entries of an arena, on the device, on torch's current stream, without waiting for it -> (begin, end):
    begin[j] = offsets[sel[j]], end[j] = offsets[sel[j] + 1] for the int64 CUDA tensors offsets[n + 1] and sel[m]; a sel[j] outside
    [0, n) gives (-1, -1), which unwrap_spans_into and stream.decompress_streams_spans_into answer with the bad-offsets status for that
    item.  (Through the library's kernel: what a C or C# caller, who has no torch to index with, calls.)"""
    for name, t in (("offsets", offsets), ("sel", sel)):
        if not _p.is_device_vector(t, "int64"):
            raise ArgumentException(f"{name} must be a 1-D int64 CUDA tensor")
    if offsets.numel() < 1:
        raise ArgumentException("offsets must hold n + 1 entries")
    if sel.device != offsets.device:
        raise ArgumentException("offsets and sel must be on the same device")
    offsets, sel = offsets.contiguous(), sel.contiguous()
    with _p.DeviceCall(offsets) as d:
        m = sel.numel()
        begin, end = d.i64(m), d.i64(m)
        _lib.check(d.lib.lz4hip_spans_select_device(offsets.data_ptr(), offsets.numel() - 1, sel.data_ptr(), m, begin.data_ptr(), end.data_ptr(),
                                                    d.stream))
        return begin, end


def unwrap_spans_into(packed, begin, end, out):
    """unwrap_into for CHOSEN messages of an arena: message j of the call is packed[begin[j]:end[j]] (int64 CUDA tensors of m entries,
    from select_spans or the caller's own index; any order, repeats, overlaps and holes), in ONE device call whose cost follows m ->
    (out_off, status, info, written_messages) as unwrap_into returns them, indexed by position in the call; check_unwrap_into reads
    them.  A span outside the buffer gets the bad-offsets status and no bytes."""
    packed, begin, end = _p.check_device_spans(packed, begin, end)
    return _unwrap_into("lz4hip_unwrap_spans_into_device", packed, (begin, end), begin.numel(), out)


def read_unwrap_info(info):
    """the lz4hip_unwrap_info_t an unwrap_into call left on the device (waits for the device)"""
    return _p.read_record(info, _lib.UnwrapInfo)


def check_unwrap_into(info, written_messages):
    """Waits for an unwrap_into call and raises what unwrap_device(check=True) raises for its outcome (.message_index), an
    ArgumentException when `out` was too small for the batch.  Returns the info record."""
    h = read_unwrap_info(info)
    if h.first_error >= 0:
        raise unwrap_error(h.error, h.first_error)
    if int(written_messages.item()) < h.messages:
        raise ArgumentException(f"out is too small: the batch unwraps to {h.decoded_bytes} bytes")
    return h


# ---- host-resident batches (numpy; the lz4hip_wrap_host / lz4hip_unwrap_host pair) -----------------------------------------------

def wrap_host(src, offsets, high_compression: bool = False):
    """wrap_device for host arrays, through lz4hip_wrap_host -> (packed, packed_offsets) as numpy arrays."""
    src, offsets = _p.check_host_batch(src, offsets)
    L = _lib.lib()
    n = offsets.size - 1
    bound = L.lz4hip_wrap_bound(n, src.size)
    out = np.empty(max(bound, 1), np.uint8)
    out_off = np.empty(n + 1, np.int64)
    result = np.empty(max(n, 1), np.int32)
    _lib.check(L.lz4hip_wrap_host(src.ctypes.data, src.size, offsets.ctypes.data, n, _p.mode(high_compression), out.ctypes.data, bound,
                                  out_off.ctypes.data, result.ctypes.data))
    if n and result[:n].min() < 0:
        raise ArgumentException(_WRAP_INVALID)
    return out[:int(out_off[n])], out_off


def unwrap_host(packed, offsets, check: bool = True):
    """unwrap_device for host arrays, through lz4hip_unwrap_host -> (data, data_offsets), or (data, data_offsets, status) with
    check=False."""
    packed, offsets = _p.check_host_batch(packed, offsets)
    L = _lib.lib()
    n = offsets.size - 1
    out_off = np.empty(n + 1, np.int64)
    status = np.empty(max(n, 1), np.int32)
    info = _lib.UnwrapInfo()
    out = _p.sized_decode_host(lambda dst, dst_cap: L.lz4hip_unwrap_host(
        packed.ctypes.data, packed.size, offsets.ctypes.data, n, dst, dst_cap, out_off.ctypes.data, status.ctypes.data, C.byref(info)), info)
    if not check:
        return out, out_off, status[:n]
    if info.first_error >= 0:
        raise unwrap_error(info.error, info.first_error)
    return out, out_off
