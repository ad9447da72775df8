"""Batches of wrapped messages (LZ4Codec.Wrap / WrapHC / Unwrap, src/LZ4/LZ4Codec.cs:471-599) on the device: the lz4hip_wrap_* /
lz4hip_unwrap_* calls of include/lz4hip.h, kernels in csrc/lz4hip_wrap.hpp.

A batch of n messages is one 1-D uint8 buffer plus int64 offsets[n + 1]: message i is buf[offsets[i]:offsets[i + 1]].  wrap_* returns
the wrapped messages in that layout and unwrap_* reads it, so one's output is the other's input.  The bytes of each message are those
of LZ4Codec.Wrap / WrapHC / Unwrap; errors raise the exceptions Unwrap raises, with the failing message's index in .message_index.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .codec import _CORRUPT, ArgumentException
from .stream import _check_device_batch, _check_device_spans, _check_host_batch, _check_out, _read_info

_WRAP_INVALID = "inputBuffer size of inputLength is invalid"
_MESSAGES = {
    _lib.WRAP_SIZE_INVALID: "inputBuffer size is invalid",
    _lib.WRAP_CORRUPT_HEADER: "inputBuffer size is invalid or has been corrupted",
    _lib.WRAP_CORRUPT_BLOCK: _CORRUPT,
    _lib.E_ARGUMENT: "offsets are invalid for the given buffer",
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
    src, offsets = _check_device_batch(src, offsets)
    with torch.cuda.device(src.device):
        L = _lib.lib()
        dev = src.device
        n = offsets.numel() - 1
        bound = L.lz4hip_wrap_bound(n, src.numel())
        out = torch.empty(bound, dtype=torch.uint8, device=dev)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        result = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        scratch = torch.empty(L.lz4hip_wrap_scratch_bytes(n, src.numel()), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_wrap_device(src.data_ptr(), src.numel(), offsets.data_ptr(), n, _lib.MODE_HC if high_compression else _lib.MODE_FAST,
                                        out.data_ptr(), bound, out_off.data_ptr(), result.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                        torch.cuda.current_stream(dev).cuda_stream))
        lowest = result[:n].min().to(torch.int64).reshape(1) if n else torch.zeros(1, dtype=torch.int64, device=dev)
        total, lowest = torch.cat([out_off[n:], lowest]).tolist()
        if lowest < 0:
            raise ArgumentException(_WRAP_INVALID)
        return out[:total], out_off


def unwrap_device(packed, offsets, check: bool = True):
    """[LZ4Codec.Unwrap(w) for w in messages] for the wrapped messages packed[offsets[i]:offsets[i + 1]] of a CUDA tensor, on the device,
    on torch's current stream -> (data, data_offsets).  Every message with a valid header is decoded; with check=True the first failing
    message raises what Unwrap raises for it (ArgumentException, .message_index = its index), with check=False the per-message statuses
    (LZ4HIP_WRAP_*, 0 = fine) come back as a third value instead.  Waits for the device twice: to size the output, and for the outcome."""
    import torch
    packed, offsets = _check_device_batch(packed, offsets)
    with torch.cuda.device(packed.device):
        L = _lib.lib()
        dev = packed.device
        s = torch.cuda.current_stream(dev).cuda_stream
        n = offsets.numel() - 1
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        scratch = torch.empty(L.lz4hip_unwrap_scratch_bytes(n), dtype=torch.uint8, device=dev)
        info_dev = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device=dev)

        def read_info():
            return _lib.UnwrapInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())

        _lib.check(L.lz4hip_unwrap_index_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, out_off.data_ptr(), status.data_ptr(),
                                                scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(), s))
        info = read_info()
        out = torch.empty(int(info.decoded_bytes), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_unwrap_decode_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, C.byref(info), scratch.data_ptr(),
                                                 scratch.numel(), out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(),
                                                 info_dev.data_ptr(), s))
        info = read_info()
        if not check:
            return out, out_off, status[:n]
        if info.first_error >= 0:
            raise unwrap_error(info.error, info.first_error)
        return out, out_off


def unwrap_into(packed, offsets, out):
    """unwrap_device into a tensor the caller already owns, in ONE device call on torch's current stream, without waiting for the
    device -> (out_off, status, info, written_messages), all device tensors: message i is out[out_off[i]:out_off[i + 1]], status is
    per message, info holds the lz4hip_unwrap_info_t record (read_unwrap_info, check_unwrap_into) and written_messages the int64 count
    of leading messages that fit `out`; the others are not written, and out_off and info.decoded_bytes are complete all the same."""
    import torch
    packed, offsets = _check_device_batch(packed, offsets)
    out = _check_out(out, packed)
    with torch.cuda.device(packed.device):
        L = _lib.lib()
        dev = packed.device
        n = offsets.numel() - 1
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        info = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device=dev)
        written = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(L.lz4hip_unwrap_into_scratch_bytes(n), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_unwrap_into_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, scratch.data_ptr(), scratch.numel(),
                                               out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(), info.data_ptr(),
                                               written.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return out_off, status[:n], info, written


def select_spans(offsets, sel):
    """The spans of chosen entries of an arena, on the device, on torch's current stream, without waiting for it -> (begin, end):
    begin[j] = offsets[sel[j]], end[j] = offsets[sel[j] + 1] for the int64 CUDA tensors offsets[n + 1] and sel[m]; a sel[j] outside
    [0, n) gives (-1, -1), which unwrap_spans_into and stream.decompress_streams_spans_into answer with the bad-offsets status for that
    item.  (Through the library's kernel: what a C or C# caller, who has no torch to index with, calls.)"""
    import torch
    for name, t in (("offsets", offsets), ("sel", sel)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 1:
            raise ArgumentException(f"{name} must be a 1-D int64 CUDA tensor")
    if offsets.numel() < 1:
        raise ArgumentException("offsets must hold n + 1 entries")
    if sel.device != offsets.device:
        raise ArgumentException("offsets and sel must be on the same device")
    offsets, sel = offsets.contiguous(), sel.contiguous()
    with torch.cuda.device(offsets.device):
        dev = offsets.device
        m = sel.numel()
        begin = torch.empty(m, dtype=torch.int64, device=dev)
        end = torch.empty(m, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().lz4hip_spans_select_device(offsets.data_ptr(), offsets.numel() - 1, sel.data_ptr(), m, begin.data_ptr(),
                                                         end.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return begin, end


def unwrap_spans_into(packed, begin, end, out):
    """unwrap_into for CHOSEN messages of an arena: message j of the call is packed[begin[j]:end[j]] (int64 CUDA tensors of m entries,
    from select_spans or the caller's own index; any order, repeats, overlaps and holes), in ONE device call whose cost follows m ->
    (out_off, status, info, written_messages) as unwrap_into returns them, indexed by position in the call; check_unwrap_into reads
    them.  A span outside the buffer gets the bad-offsets status and no bytes."""
    import torch
    packed, begin, end = _check_device_spans(packed, begin, end)
    out = _check_out(out, packed)
    with torch.cuda.device(packed.device):
        L = _lib.lib()
        dev = packed.device
        m = begin.numel()
        out_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
        status = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        info = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device=dev)
        written = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(L.lz4hip_unwrap_into_scratch_bytes(m), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_unwrap_spans_into_device(packed.data_ptr(), packed.numel(), begin.data_ptr(), end.data_ptr(), m, scratch.data_ptr(),
                                                     scratch.numel(), out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(),
                                                     info.data_ptr(), written.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return out_off, status[:m], info, written


def read_unwrap_info(info):
    """the lz4hip_unwrap_info_t an unwrap_into call left on the device (waits for the device)"""
    return _read_info(info, _lib.UnwrapInfo)


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
    src, offsets = _check_host_batch(src, offsets)
    L = _lib.lib()
    n = offsets.size - 1
    bound = L.lz4hip_wrap_bound(n, src.size)
    out = np.empty(max(bound, 1), np.uint8)
    out_off = np.empty(n + 1, np.int64)
    result = np.empty(max(n, 1), np.int32)
    _lib.check(L.lz4hip_wrap_host(src.ctypes.data, src.size, offsets.ctypes.data, n, _lib.MODE_HC if high_compression else _lib.MODE_FAST,
                                  out.ctypes.data, bound, out_off.ctypes.data, result.ctypes.data))
    if n and result[:n].min() < 0:
        raise ArgumentException(_WRAP_INVALID)
    return out[:int(out_off[n])], out_off


def unwrap_host(packed, offsets, check: bool = True):
    """unwrap_device for host arrays, through lz4hip_unwrap_host -> (data, data_offsets), or (data, data_offsets, status) with
    check=False."""
    packed, offsets = _check_host_batch(packed, offsets)
    L = _lib.lib()
    n = offsets.size - 1
    out_off = np.empty(n + 1, np.int64)
    status = np.empty(max(n, 1), np.int32)
    info = _lib.UnwrapInfo()
    # a size query first (dst_cap = 0: LZ4HIP_E_ARGUMENT with decoded_bytes filled in), then the call that decodes
    rc = L.lz4hip_unwrap_host(packed.ctypes.data, packed.size, offsets.ctypes.data, n, None, 0, out_off.ctypes.data, status.ctypes.data,
                              C.byref(info))
    out = np.empty(max(int(info.decoded_bytes), 1), np.uint8)
    if info.decoded_bytes > 0:
        rc = L.lz4hip_unwrap_host(packed.ctypes.data, packed.size, offsets.ctypes.data, n, out.ctypes.data, int(info.decoded_bytes),
                                  out_off.ctypes.data, status.ctypes.data, C.byref(info))
    if rc != info.error:                                              # (the outcome itself is info.error)
        _lib.check(rc)
    out = out[:int(info.decoded_bytes)]
    if not check:
        return out, out_off, status[:n]
    if info.first_error >= 0:
        raise unwrap_error(info.error, info.first_error)
    return out, out_off
