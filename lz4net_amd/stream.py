"""Batched LZ4Stream chunk framing -- the natural producer/consumer of block batches.

Mirrors the wire format of lz4net's ``LZ4Stream`` (src/LZ4/LZ4Stream.cs): a stream is a sequence of chunks

    varint(flags)  varint(originalLength)  [varint(compressedLength) if flags & Compressed]  payload

with ``ChunkFlags { None = 0, Compressed = 1, HighCompression = 2 }`` (src/LZ4/LZ4Stream.cs:43-59), varints
as in WriteVarInt / TryReadVarInt (:162-218), a chunk stored raw when the encoder returns <= 0 or does not
shrink it -- the encoder is called with ``outputLength = inputLength`` (FlushCurrentChunk, :239-269) -- and
``Decode(..., knownOutputLength: true)`` on the way back (AcquireNextChunk, :274-312).

The reference encodes and decodes one chunk per call; here all chunks of a buffer go through ONE
lz4hip_encode_batch_host / lz4hip_decode_batch_host call (include/lz4hip.h), i.e. one batch on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .codec import ArgumentException

FLAG_COMPRESSED, FLAG_HIGH_COMPRESSION = 1, 2
DEFAULT_BLOCK_SIZE = 1024 * 1024          # LZ4Stream's default (src/LZ4/LZ4Stream.cs:127-139); minimum 16


class EndOfStreamException(ArgumentException):
    """LZ4Stream.EndOfStream(): the stream is truncated or corrupted."""


def write_varint(value: int) -> bytes:
    out = bytearray()
    while True:
        b = value & 0x7F
        value >>= 7
        out.append(b | (0x80 if value else 0))
        if not value:
            return bytes(out)


def read_varint(buf, pos: int):
    """Returns (value, new_pos) or (None, pos) at a clean end of stream (TryReadVarInt)."""
    result, count, start = 0, 0, pos
    while True:
        if pos >= len(buf):
            if count == 0:
                return None, start
            raise EndOfStreamException("unexpected end of stream inside a varint")
        b = buf[pos]
        pos += 1
        result += (b & 0x7F) << count
        count += 7
        if (b & 0x80) == 0 or count >= 64:
            return result & 0xFFFFFFFFFFFFFFFF, pos             # (a ulong: of a tenth byte only bit 0 survives its shift by 63)


def _batch(src, src_off, src_len, dst, dst_off, dst_cap, result):
    n = len(src_len)
    return _lib.Batch(src=src.ctypes.data, src_off=src_off.ctypes.data, src_stride=0, src_len=src_len.ctypes.data,
                      dst=dst.ctypes.data, dst_off=dst_off.ctypes.data, dst_stride=0, dst_cap=dst_cap.ctypes.data,
                      dst_cap_all=0, src_len_all=0, result=result.ctypes.data, n_blocks=n)


def compress_stream(data, block_size: int = DEFAULT_BLOCK_SIZE, high_compression: bool = False) -> bytes:
    """LZ4Stream(Compress).Write(data) + Close(): every chunk of `data` encoded in one GPU batch."""
    block_size = max(16, int(block_size))
    raw = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    n = (raw.size + block_size - 1) // block_size
    if n == 0:
        return b""
    offs = np.arange(n, dtype=np.int64) * block_size
    lens = np.minimum(block_size, raw.size - offs).astype(np.int32)
    comp = np.zeros(raw.size, dtype=np.uint8)                  # outputLength = inputLength per chunk, packed at the same offsets
    res = np.zeros(n, dtype=np.int32)
    b = _batch(raw, offs, lens, comp, offs, lens, res)
    _lib.check(_lib.lib().lz4hip_encode_batch_host(C.byref(b), _lib.MODE_HC if high_compression else _lib.MODE_FAST))
    out = bytearray()
    for i in range(n):
        o, ln, cl = int(offs[i]), int(lens[i]), int(res[i])
        compressed = 0 < cl < ln
        flags = (FLAG_COMPRESSED if compressed else 0) | (FLAG_HIGH_COMPRESSION if high_compression else 0)
        out += write_varint(flags) + write_varint(ln)
        if compressed:
            out += write_varint(cl)
            out += comp[o:o + cl].tobytes()
        else:
            out += raw[o:o + ln].tobytes()
    return bytes(out)


def parse_chunks(stream):
    """Header walk of a framed stream -> list of (is_compressed, original_length, payload_offset, payload_length)."""
    buf = memoryview(stream) if not isinstance(stream, memoryview) else stream
    pos, chunks = 0, []
    while True:
        flags, pos = read_varint(buf, pos)
        if flags is None:
            return chunks
        original, pos = read_varint(buf, pos)
        if original is None:
            raise EndOfStreamException("missing chunk length")
        compressed = bool(flags & FLAG_COMPRESSED)
        if compressed:
            clen, pos = read_varint(buf, pos)
            if clen is None:
                raise EndOfStreamException("missing compressed length")
        else:
            clen = original
        original, clen = original & 0xFFFFFFFF, clen & 0xFFFFFFFF
        if original >= 1 << 31:
            original -= 1 << 32
        if clen >= 1 << 31:
            clen -= 1 << 32
        if clen > original or clen < 0:
            raise EndOfStreamException("corrupted chunk header")
        if pos + clen > len(buf):
            raise EndOfStreamException("truncated chunk payload")
        if compressed and ((flags & 0xFFFFFFFF) >> 2) != 0:      # (int)flags >> 2: bits 32..63 of the varint do not count
            raise NotImplementedError("Chunks with multiple passes are not supported.")
        chunks.append((compressed, original, pos, clen))
        pos += clen


def decompress_stream(stream) -> bytes:
    """LZ4Stream(Decompress).Read to end: all compressed chunks decoded in one GPU batch."""
    data = np.frombuffer(bytes(stream), dtype=np.uint8)
    chunks = parse_chunks(memoryview(bytes(stream)))
    total = sum(c[1] for c in chunks)
    out = np.zeros(total, dtype=np.uint8)
    out_off, pos = [], 0
    for _, original, _, _ in chunks:
        out_off.append(pos)
        pos += original
    idx = [i for i, c in enumerate(chunks) if c[0]]
    for i, (compressed, original, off, ln) in enumerate(chunks):
        if not compressed:
            out[out_off[i]:out_off[i] + original] = data[off:off + ln]
    if idx:
        src_off = np.array([chunks[i][2] for i in idx], dtype=np.int64)
        src_len = np.array([chunks[i][3] for i in idx], dtype=np.int32)
        dst_off = np.array([out_off[i] for i in idx], dtype=np.int64)
        dst_len = np.array([chunks[i][1] for i in idx], dtype=np.int32)
        res = np.zeros(len(idx), dtype=np.int32)
        b = _batch(data, src_off, src_len, out, dst_off, dst_len, res)
        _lib.check(_lib.lib().lz4hip_decode_batch_host(C.byref(b), 1))
        if not (res == src_len).all():                       # Decode64: consumed != inputLength (Unsafe.cs:373-378)
            raise ArgumentException("LZ4 block is corrupted, or invalid length has been given.")
    return out.tobytes()


# ---- device-resident streams (lz4hip_stream_* of include/lz4hip.h; kernels in csrc/lz4hip_stream.hpp) ------------------------------

def _check_device_bytes(t, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 1:
        raise ArgumentException(f"{name} must be a 1-D uint8 CUDA tensor")
    return t.contiguous()


def compress_stream_device(t, block_size: int = DEFAULT_BLOCK_SIZE, high_compression: bool = False):
    """compress_stream for a 1-D uint8 CUDA tensor, entirely on the device, on torch's current stream: the same bytes, returned as a
    1-D uint8 CUDA tensor.  Waits for the device once, to learn the stream's length."""
    import torch
    t = _check_device_bytes(t, "t")
    with torch.cuda.device(t.device):
        return _compress_stream_device(t, max(16, int(block_size)), high_compression)


def _compress_stream_device(t, block_size, high_compression):
    import torch
    L = _lib.lib()
    n = t.numel()
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=t.device)
    out = torch.empty(L.lz4hip_stream_bound(n, block_size), dtype=torch.uint8, device=t.device)
    scratch = torch.empty(L.lz4hip_stream_encode_scratch_bytes(n, block_size), dtype=torch.uint8, device=t.device)
    out_len = torch.empty(1, dtype=torch.int64, device=t.device)
    _lib.check(L.lz4hip_stream_encode_device(t.data_ptr(), n, block_size, _lib.MODE_HC if high_compression else _lib.MODE_FAST,
                                             out.data_ptr(), out.numel(), out_len.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                             torch.cuda.current_stream(t.device).cuda_stream))
    return out[:int(out_len.item())]


def _stream_error(info):
    """The exception parse_chunks / decompress_stream raise for an LZ4HIP_STREAM_* outcome, with the failing header's offset."""
    if info.error == _lib.STREAM_END_OF_STREAM:
        e = EndOfStreamException("truncated or corrupted stream")
    elif info.error == _lib.STREAM_PASSES:
        e = NotImplementedError("Chunks with multiple passes are not supported.")
    elif info.error == _lib.STREAM_CORRUPT_BLOCK:
        e = ArgumentException("LZ4 block is corrupted, or invalid length has been given.")
    else:
        e = _lib.Lz4HipError(f"stream decode: unexpected outcome {info.error}")
    e.error_offset = int(info.error_offset)
    return e


def decompress_stream_device(t):
    """decompress_stream for a 1-D uint8 CUDA tensor, on torch's current stream: the header walk, the block decode and the raw copies
    run on the device; the host reads the walk's result once (to size the output) and the final outcome once."""
    import torch
    t = _check_device_bytes(t, "t")
    with torch.cuda.device(t.device):
        return _decompress_stream_device(t)


def _decompress_stream_device(t):
    import torch
    L = _lib.lib()
    dev = t.device
    s = torch.cuda.current_stream(dev).cuda_stream
    n = t.numel()
    info_dev = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device=dev)

    def read_info():
        return _lib.StreamInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())

    max_chunks = (n + 4095) // 4096 + 16
    for _ in range(2):
        scratch = torch.empty(L.lz4hip_stream_decode_scratch_bytes(max_chunks), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_stream_index_device(t.data_ptr(), n, max_chunks, scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(), s))
        info = read_info()
        if info.error != _lib.STREAM_TABLE_FULL:
            break
        max_chunks = int(info.chunks)
    out = torch.empty(int(info.decoded_bytes), dtype=torch.uint8, device=dev)
    _lib.check(L.lz4hip_stream_decode_device(t.data_ptr(), C.byref(info), max_chunks, scratch.data_ptr(), scratch.numel(),
                                             out.data_ptr(), out.numel(), info_dev.data_ptr(), s))
    info = read_info()
    if info.error != _lib.STREAM_OK:
        raise _stream_error(info)
    return out


def _check_out(out, like):
    import torch
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ArgumentException("out must be a contiguous 1-D uint8 CUDA tensor")
    if out.device != like.device:
        raise ArgumentException("out must be on the source's device")
    return out


def _read_info(info, cls):
    """the one place that waits for the device: the info record a *_into call left there, as its ctypes struct"""
    return cls.from_buffer_copy(info.cpu().numpy().tobytes())


def decompress_stream_into(t, out, max_chunks=None, block_size: int = DEFAULT_BLOCK_SIZE):
    """decompress_stream for a 1-D uint8 CUDA tensor, into a tensor the caller already owns, in ONE device call on torch's current
    stream, without waiting for the device -> (info, written): device tensors holding the lz4hip_stream_info_t record (read it with
    read_stream_info, check it with check_stream_into) and the int64 count of bytes written.  The output is clipped at a chunk boundary
    when `out` is too small; info.decoded_bytes is the size needed all the same.  max_chunks is the chunk table's size: by default
    out.numel() // max(16, block_size) + 16, which holds anything compress_stream_device wrote into `out`'s size with that block size."""
    import torch
    t = _check_device_bytes(t, "t")
    out = _check_out(out, t)
    if max_chunks is None:
        max_chunks = out.numel() // max(16, int(block_size)) + 16
    with torch.cuda.device(t.device):
        L = _lib.lib()
        dev = t.device
        info = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device=dev)
        written = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(L.lz4hip_stream_decode_into_scratch_bytes(max_chunks), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_stream_decode_into_device(t.data_ptr(), t.numel(), max_chunks, scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                                      out.numel(), info.data_ptr(), written.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return info, written


def read_stream_info(info):
    """the lz4hip_stream_info_t a decompress_stream_into call left on the device (waits for the device)"""
    return _read_info(info, _lib.StreamInfo)


def check_stream_into(info, written):
    """Waits for a decompress_stream_into call and raises what decompress_stream_device raises for its outcome (.error_offset = the
    failing header's offset), an Lz4HipError naming the chunk count for a table that was too small, an ArgumentException when `out` was
    too small for the stream.  Returns the info record."""
    h = read_stream_info(info)
    if h.error == _lib.STREAM_TABLE_FULL:
        raise _lib.Lz4HipError(f"stream decode: the chunk table is too small, the stream has {h.chunks} chunks (max_chunks)")
    if h.error != _lib.STREAM_OK:
        raise _stream_error(h)
    if int(written.item()) < h.decoded_bytes:
        raise ArgumentException(f"out is too small: the stream decodes to {h.decoded_bytes} bytes")
    return h


# ---- batches of streams (lz4hip_streams_* of include/lz4hip.h; kernels in csrc/lz4hip_streams.hpp) ---------------------------------
# A batch of n streams is one 1-D uint8 buffer plus int64 offsets[n + 1]: item i is buf[offsets[i]:offsets[i + 1]].  compress_streams_*
# returns the framed streams in that layout and decompress_streams_* reads it, so one's output is the other's input.

_BAD_OFFSETS = "offsets are invalid for the given buffer"


def _check_device_batch(buf, offsets):
    """a batch on the device: a 1-D uint8 CUDA tensor and its int64 offsets[n + 1] (wrap.py's batches are the same)"""
    import torch
    if not isinstance(buf, torch.Tensor) or not buf.is_cuda or buf.dtype != torch.uint8 or buf.dim() != 1:
        raise ArgumentException("the buffer must be a 1-D uint8 CUDA tensor")
    if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.dtype != torch.int64 or offsets.dim() != 1:
        raise ArgumentException("offsets must be a 1-D int64 CUDA tensor")
    if offsets.numel() < 1:
        raise ArgumentException("offsets must hold n + 1 entries")
    if offsets.device != buf.device:
        raise ArgumentException("the buffer and the offsets must be on the same device")
    return buf.contiguous(), offsets.contiguous()


def _check_device_spans(buf, begin, end):
    """chosen items of an arena on the device: a 1-D uint8 CUDA tensor and the int64 begin[m], end[m] of its spans"""
    import torch
    if not isinstance(buf, torch.Tensor) or not buf.is_cuda or buf.dtype != torch.uint8 or buf.dim() != 1:
        raise ArgumentException("the buffer must be a 1-D uint8 CUDA tensor")
    for t in (begin, end):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 1:
            raise ArgumentException("begin and end must be 1-D int64 CUDA tensors")
        if t.device != buf.device:
            raise ArgumentException("the buffer and the spans must be on the same device")
    if begin.numel() != end.numel():
        raise ArgumentException("begin and end must have the same length")
    return buf.contiguous(), begin.contiguous(), end.contiguous()


def streams_error(status: int, index: int, error_offset: int = -1):
    """The exception a sequential [decompress_stream(s) for s in ...] raises at an item with this status (LZ4HIP_STREAM_*, or
    LZ4HIP_E_ARGUMENT for bad offsets), with the item's index in .item_index and the failing header's offset within it in .error_offset."""
    if int(status) == _lib.E_ARGUMENT:
        e = ArgumentException(_BAD_OFFSETS)
        e.error_offset = -1
    else:
        e = _stream_error(_lib.StreamInfo(error=int(status), error_offset=int(error_offset)))
    e.item_index = int(index)
    return e


def compress_streams_device(buf, offsets, block_size: int = DEFAULT_BLOCK_SIZE, high_compression: bool = False):
    """[compress_stream(item) for item in items] for the items buf[offsets[i]:offsets[i + 1]] of a CUDA tensor, in one call on the
    device, on torch's current stream -> (packed, packed_offsets): packed_offsets[i] is where item i's stream starts.  The chunks of
    all items are one batch of the block encoder.  Waits for the device once, to learn the total."""
    import torch
    buf, offsets = _check_device_batch(buf, offsets)
    block_size = max(16, int(block_size))
    with torch.cuda.device(buf.device):
        L = _lib.lib()
        dev = buf.device
        n = offsets.numel() - 1
        bound = L.lz4hip_streams_bound(n, buf.numel(), block_size)
        out = torch.empty(bound, dtype=torch.uint8, device=dev)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        scratch = torch.empty(L.lz4hip_streams_encode_scratch_bytes(n, buf.numel(), block_size), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_streams_encode_device(buf.data_ptr(), buf.numel(), offsets.data_ptr(), n, block_size,
                                                  _lib.MODE_HC if high_compression else _lib.MODE_FAST, out.data_ptr(), bound,
                                                  out_off.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                  torch.cuda.current_stream(dev).cuda_stream))
        bad = ((offsets[1:] < offsets[:-1]).any() | (offsets[0] < 0) | (offsets[-1] > buf.numel())).to(torch.int64).reshape(1)
        total, bad = torch.cat([out_off[n:], bad]).tolist()
        if bad:
            raise ArgumentException(_BAD_OFFSETS)
        return out[:total], out_off


def decompress_streams_device(packed, offsets, check: bool = True):
    """[decompress_stream(s) for s in streams] for the streams packed[offsets[i]:offsets[i + 1]] of a CUDA tensor, on the device, on
    torch's current stream -> (data, data_offsets).  Every item's headers are walked by a wavefront of its own, the compressed chunks
    of all items are one batch of the block decoder.  Every chunk before an item's first error is decoded; with check=True the first
    failing item raises what decompress_stream raises for it (.item_index = its index, .error_offset = the failing header's offset
    within the item), with check=False the per-item statuses (LZ4HIP_STREAM_*, 0 = fine; LZ4HIP_E_ARGUMENT for bad offsets) come back
    as a third value instead.  Waits for the device twice: to size the output, and for the outcome."""
    import torch
    packed, offsets = _check_device_batch(packed, offsets)
    with torch.cuda.device(packed.device):
        L = _lib.lib()
        dev = packed.device
        s = torch.cuda.current_stream(dev).cuda_stream
        n = offsets.numel() - 1
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        err_off = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        info_dev = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device=dev)

        def read_info():
            return _lib.StreamsInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())

        max_chunks = packed.numel() // 4096 + n + 16
        for _ in range(2):
            scratch = torch.empty(L.lz4hip_streams_decode_scratch_bytes(n, max_chunks), dtype=torch.uint8, device=dev)
            _lib.check(L.lz4hip_streams_index_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, max_chunks, out_off.data_ptr(),
                                                     status.data_ptr(), err_off.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                     info_dev.data_ptr(), s))
            info = read_info()
            if info.error != _lib.STREAM_TABLE_FULL:
                break
            max_chunks = int(info.chunks)
        out = torch.empty(int(info.decoded_bytes), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_streams_decode_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, C.byref(info), max_chunks,
                                                  scratch.data_ptr(), scratch.numel(), out.data_ptr(), out.numel(), out_off.data_ptr(),
                                                  status.data_ptr(), err_off.data_ptr(), info_dev.data_ptr(), s))
        info = read_info()
        if not check:
            return out, out_off, status[:n]
        if info.first_error >= 0:
            raise streams_error(info.error, info.first_error, info.error_offset)
        return out, out_off


def decompress_streams_into(packed, offsets, out, max_chunks=None, block_size: int = DEFAULT_BLOCK_SIZE):
    """decompress_streams_device into a tensor the caller already owns, in ONE device call on torch's current stream, without waiting
    for the device -> (out_off, status, error_offset, info, written_items), all device tensors: item i is out[out_off[i]:out_off[i + 1]],
    status and error_offset are per item, info holds the lz4hip_streams_info_t record (read_streams_info, check_streams_into) and
    written_items the int64 count of leading items that fit `out`; the others are not written, and out_off and info.decoded_bytes are
    complete all the same.  max_chunks is the chunk table's size for the whole batch: by default out.numel() // block + n + 16."""
    import torch
    packed, offsets = _check_device_batch(packed, offsets)
    out = _check_out(out, packed)
    n = offsets.numel() - 1
    if max_chunks is None:
        max_chunks = out.numel() // max(16, int(block_size)) + n + 16
    with torch.cuda.device(packed.device):
        L = _lib.lib()
        dev = packed.device
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        err_off = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        info = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device=dev)
        written = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(L.lz4hip_streams_decode_into_scratch_bytes(n, max_chunks), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_streams_decode_into_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, max_chunks, scratch.data_ptr(),
                                                       scratch.numel(), out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(),
                                                       err_off.data_ptr(), info.data_ptr(), written.data_ptr(),
                                                       torch.cuda.current_stream(dev).cuda_stream))
        return out_off, status[:n], err_off[:n], info, written


def decompress_streams_spans_into(packed, begin, end, out, max_chunks=None, block_size: int = DEFAULT_BLOCK_SIZE):
    """decompress_streams_into for CHOSEN items of an arena: item j of the call is packed[begin[j]:end[j]] (int64 CUDA tensors of m
    entries, from wrap.select_spans, a stream_directory or the caller's own index; any order, repeats, overlaps and holes), in ONE
    device call whose cost follows m -> (out_off, status, error_offset, info, written_items) as decompress_streams_into returns them,
    indexed by position in the call; check_streams_into reads them.  max_chunks counts the chunks of the chosen items, repeats
    included: by default out.numel() // block + m + 16."""
    import torch
    packed, begin, end = _check_device_spans(packed, begin, end)
    out = _check_out(out, packed)
    m = begin.numel()
    if max_chunks is None:
        max_chunks = out.numel() // max(16, int(block_size)) + m + 16
    with torch.cuda.device(packed.device):
        L = _lib.lib()
        dev = packed.device
        out_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
        status = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        err_off = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
        info = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device=dev)
        written = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(L.lz4hip_streams_decode_into_scratch_bytes(m, max_chunks), dtype=torch.uint8, device=dev)
        _lib.check(L.lz4hip_streams_decode_spans_into_device(packed.data_ptr(), packed.numel(), begin.data_ptr(), end.data_ptr(), m, max_chunks,
                                                             scratch.data_ptr(), scratch.numel(), out.data_ptr(), out.numel(),
                                                             out_off.data_ptr(), status.data_ptr(), err_off.data_ptr(), info.data_ptr(),
                                                             written.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return out_off, status[:m], err_off[:m], info, written


def stream_directory(t, max_chunks=None, block_size: int = DEFAULT_BLOCK_SIZE):
    """The chunk directory of ONE LZ4Stream buffer (a 1-D uint8 CUDA tensor), to keep beside a stream that is decoded more than once
    or in parts -> (hdr_off, out_off, out_off_host): device int64 tensors of chunks + 1 entries -- chunk k's header is at hdr_off[k]
    and its bytes are [out_off[k], out_off[k + 1]) of the plain text; the closing entries are the stream's length and its decoded size
    -- and a host copy of out_off as a numpy array.  t[hdr_off[k]:hdr_off[k + 1]] is a one-chunk item for
    decompress_streams_spans_into.  This is the once-per-stream step: the serial header walk, and it waits for the device (twice when
    the default table of t.numel() // block + 16 chunks was too small).  A header error raises what decompress_stream_device raises."""
    import torch
    t = _check_device_bytes(t, "t")
    if max_chunks is None:
        max_chunks = t.numel() // max(16, int(block_size)) + 16
    with torch.cuda.device(t.device):
        L = _lib.lib()
        dev = t.device
        info_dev = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device=dev)
        for _ in range(2):
            hdr_off = torch.empty(max_chunks + 1, dtype=torch.int64, device=dev)
            out_off = torch.empty(max_chunks + 1, dtype=torch.int64, device=dev)
            _lib.check(L.lz4hip_stream_directory_device(t.data_ptr(), t.numel(), max_chunks, hdr_off.data_ptr(), out_off.data_ptr(),
                                                        info_dev.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            info = _read_info(info_dev, _lib.StreamInfo)
            if info.error != _lib.STREAM_TABLE_FULL:
                break
            max_chunks = int(info.chunks)
        if info.error != _lib.STREAM_OK:
            raise _stream_error(info)
        k = int(info.chunks) + 1
        return hdr_off[:k], out_off[:k], out_off[:k].cpu().numpy()


def decompress_stream_range(t, directory, start: int, length: int):
    """Bytes [start, start + length) of the plain text of the LZ4Stream buffer t, given its stream_directory: decodes the chunks that
    cover the range -- whole chunks, as one-chunk spans in one decompress_streams_spans_into call into a chunk-aligned buffer -- and
    returns the length-byte view of it.  Waits for the device once, for the outcome."""
    import torch
    t = _check_device_bytes(t, "t")
    hdr_off, out_off, host = directory
    start, length = int(start), int(length)
    total = int(host[-1])
    if start < 0 or length < 0 or start + length > total:
        raise ArgumentException(f"the range is outside the stream's {total} decoded bytes")
    if length == 0:
        return torch.empty(0, dtype=torch.uint8, device=t.device)
    k0 = int(np.searchsorted(host, start, side="right")) - 1            # the chunk that holds `start`, and the one that holds the last byte
    k1 = int(np.searchsorted(host, start + length - 1, side="right")) - 1
    out = torch.empty(int(host[k1 + 1] - host[k0]), dtype=torch.uint8, device=t.device)
    res = decompress_streams_spans_into(t, hdr_off[k0:k1 + 1], hdr_off[k0 + 1:k1 + 2], out, max_chunks=k1 - k0 + 1)
    check_streams_into(res[3], res[4])
    return out[start - int(host[k0]):start - int(host[k0]) + length]


def read_streams_info(info):
    """the lz4hip_streams_info_t a decompress_streams_into call left on the device (waits for the device)"""
    return _read_info(info, _lib.StreamsInfo)


def check_streams_into(info, written_items):
    """Waits for a decompress_streams_into call and raises what decompress_streams_device(check=True) raises for its outcome
    (.item_index, .error_offset), an Lz4HipError naming the chunk count for a table that was too small, an ArgumentException when
    `out` was too small for the batch.  Returns the info record."""
    h = read_streams_info(info)
    if h.error == _lib.STREAM_TABLE_FULL:
        raise _lib.Lz4HipError(f"streams decode: the chunk table is too small, the batch has {h.chunks} chunks (max_chunks)")
    if h.first_error >= 0:
        raise streams_error(h.error, h.first_error, h.error_offset)
    if int(written_items.item()) < h.items:
        raise ArgumentException(f"out is too small: the batch decodes to {h.decoded_bytes} bytes")
    return h


def _check_host_batch(buf, offsets):
    """the same batch in host memory; bytes-like buffers are taken as uint8 arrays"""
    if isinstance(buf, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(buf, dtype=np.uint8)
    if not isinstance(buf, np.ndarray) or buf.dtype != np.uint8 or buf.ndim != 1:
        raise ArgumentException("the buffer must be a 1-D uint8 array")
    if not isinstance(offsets, np.ndarray) or offsets.dtype != np.int64 or offsets.ndim != 1:
        raise ArgumentException("offsets must be a 1-D int64 array")
    if offsets.size < 1:
        raise ArgumentException("offsets must hold n + 1 entries")
    return np.ascontiguousarray(buf), np.ascontiguousarray(offsets)


def compress_streams_host(buf, offsets, block_size: int = DEFAULT_BLOCK_SIZE, high_compression: bool = False):
    """compress_streams_device for host arrays, through lz4hip_streams_encode_host -> (packed, packed_offsets) as numpy arrays."""
    buf, offsets = _check_host_batch(buf, offsets)
    block_size = max(16, int(block_size))
    L = _lib.lib()
    n = offsets.size - 1
    if n and ((np.diff(offsets) < 0).any() or offsets[0] < 0 or offsets[-1] > buf.size):
        raise ArgumentException(_BAD_OFFSETS)
    bound = L.lz4hip_streams_bound(n, buf.size, block_size)
    out = np.empty(max(bound, 1), np.uint8)
    out_off = np.empty(n + 1, np.int64)
    _lib.check(L.lz4hip_streams_encode_host(buf.ctypes.data, buf.size, offsets.ctypes.data, n, block_size,
                                            _lib.MODE_HC if high_compression else _lib.MODE_FAST, out.ctypes.data, bound, out_off.ctypes.data))
    return out[:int(out_off[n])], out_off


def decompress_streams_host(packed, offsets, check: bool = True):
    """decompress_streams_device for host arrays, through lz4hip_streams_decode_host -> (data, data_offsets), or (data, data_offsets,
    status) with check=False."""
    packed, offsets = _check_host_batch(packed, offsets)
    L = _lib.lib()
    n = offsets.size - 1
    out_off = np.empty(n + 1, np.int64)
    status = np.empty(max(n, 1), np.int32)
    err_off = np.empty(max(n, 1), np.int64)
    info = _lib.StreamsInfo()
    # a size query first (dst_cap = 0: LZ4HIP_E_ARGUMENT with decoded_bytes filled in), then the call that decodes
    rc = L.lz4hip_streams_decode_host(packed.ctypes.data, packed.size, offsets.ctypes.data, n, None, 0, out_off.ctypes.data, status.ctypes.data,
                                      err_off.ctypes.data, C.byref(info))
    out = np.empty(max(int(info.decoded_bytes), 1), np.uint8)
    if info.decoded_bytes > 0:
        rc = L.lz4hip_streams_decode_host(packed.ctypes.data, packed.size, offsets.ctypes.data, n, out.ctypes.data, int(info.decoded_bytes),
                                          out_off.ctypes.data, status.ctypes.data, err_off.ctypes.data, C.byref(info))
    if rc != info.error:                                              # (the outcome itself is info.error)
        _lib.check(rc)
    out = out[:int(info.decoded_bytes)]
    if not check:
        return out, out_off, status[:n]
    if info.first_error >= 0:
        raise streams_error(info.error, info.first_error, info.error_offset)
    return out, out_off
