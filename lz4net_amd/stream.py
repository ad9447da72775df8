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

from . import _lib, _plumbing as _p
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
    b = _p.host_blocks(raw, offs, lens, comp, offs, lens, res)
    _lib.check(_lib.lib().lz4hip_encode_batch_host(C.byref(b), _p.mode(high_compression)))
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
        b = _p.host_blocks(data, src_off, src_len, out, dst_off, dst_len, res)
        _lib.check(_lib.lib().lz4hip_decode_batch_host(C.byref(b), 1))
        if not (res == src_len).all():                       # Decode64: consumed != inputLength (Unsafe.cs:373-378)
            raise ArgumentException("LZ4 block is corrupted, or invalid length has been given.")
    return out.tobytes()


# ---- device-resident streams (lz4hip_stream_* of include/lz4hip.h; kernels in csrc/lz4hip_stream.hpp) ------------------------------

def compress_stream_device(t, block_size: int = DEFAULT_BLOCK_SIZE, high_compression: bool = False):
    """compress_stream for a 1-D uint8 CUDA tensor, entirely on the device, on torch's current stream: the same bytes, returned as a
    1-D uint8 CUDA tensor.  Waits for the device once, to learn the stream's length."""
    t = _p.check_device_bytes(t, "t")
    block_size = max(16, int(block_size))
    with _p.DeviceCall(t) as d:
        n = t.numel()
        if n == 0:
            return d.u8(0)
        out = d.u8(d.lib.lz4hip_stream_bound(n, block_size))
        scratch = d.u8(d.lib.lz4hip_stream_encode_scratch_bytes(n, block_size))
        out_len = d.i64(1)
        _lib.check(d.lib.lz4hip_stream_encode_device(t.data_ptr(), n, block_size, _p.mode(high_compression), out.data_ptr(), out.numel(),
                                                     out_len.data_ptr(), scratch.data_ptr(), scratch.numel(), d.stream))
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


def _table_full(info):
    """the next table size for _p.settle: the chunk count a walk reported when its table was too small, else None"""
    return int(info.chunks) if info.error == _lib.STREAM_TABLE_FULL else None


def decompress_stream_device(t):
    """decompress_stream for a 1-D uint8 CUDA tensor, on torch's current stream: the header walk, the block decode and the raw copies
    run on the device; the host reads the walk's result once (to size the output) and the final outcome once."""
    t = _p.check_device_bytes(t, "t")
    with _p.DeviceCall(t) as d:
        n = t.numel()
        info_dev = d.record(_lib.StreamInfo)

        def index(max_chunks):
            scratch = d.u8(d.lib.lz4hip_stream_decode_scratch_bytes(max_chunks))
            _lib.check(d.lib.lz4hip_stream_index_device(t.data_ptr(), n, max_chunks, scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(),
                                                        d.stream))
            info = _p.read_record(info_dev, _lib.StreamInfo)
            return (scratch, info), _table_full(info)

        (scratch, info), max_chunks = _p.settle(2, (n + 4095) // 4096 + 16, index)      # (a table still too small: the decode's outcome says so)
        out = d.u8(int(info.decoded_bytes))
        _lib.check(d.lib.lz4hip_stream_decode_device(t.data_ptr(), C.byref(info), max_chunks, scratch.data_ptr(), scratch.numel(),
                                                     out.data_ptr(), out.numel(), info_dev.data_ptr(), d.stream))
        info = _p.read_record(info_dev, _lib.StreamInfo)
        if info.error != _lib.STREAM_OK:
            raise _stream_error(info)
        return out


def decompress_stream_into(t, out, max_chunks=None, block_size: int = DEFAULT_BLOCK_SIZE):
    """decompress_stream for a 1-D uint8 CUDA tensor, into a tensor the caller already owns, in ONE device call on torch's current
    stream, without waiting for the device -> (info, written): device tensors holding the lz4hip_stream_info_t record (read it with
    read_stream_info, check it with check_stream_into) and the int64 count of bytes written.  The output is clipped at a chunk boundary
    when `out` is too small; info.decoded_bytes is the size needed all the same.  max_chunks is the chunk table's size: by default
    out.numel() // max(16, block_size) + 16, which holds anything compress_stream_device wrote into `out`'s size with that block size."""
    t = _p.check_device_bytes(t, "t")
    out = _p.check_out(out, t)
    if max_chunks is None:
        max_chunks = out.numel() // max(16, int(block_size)) + 16
    with _p.DeviceCall(t) as d:
        info, written = d.record(_lib.StreamInfo), d.i64(1, zero=True)
        scratch = d.u8(d.lib.lz4hip_stream_decode_into_scratch_bytes(max_chunks))
        _lib.check(d.lib.lz4hip_stream_decode_into_device(t.data_ptr(), t.numel(), max_chunks, scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                                          out.numel(), info.data_ptr(), written.data_ptr(), d.stream))
        return info, written


def read_stream_info(info):
    """the lz4hip_stream_info_t a decompress_stream_into call left on the device (waits for the device)"""
    return _p.read_record(info, _lib.StreamInfo)


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

def streams_error(status: int, index: int, error_offset: int = -1):
    """The exception a sequential [decompress_stream(s) for s in ...] raises at an item with this status (LZ4HIP_STREAM_*, or
    LZ4HIP_E_ARGUMENT for bad offsets), with the item's index in .item_index and the failing header's offset within it in .error_offset."""
    if int(status) == _lib.E_ARGUMENT:
        e = ArgumentException(_p.BAD_OFFSETS)
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
    buf, offsets = _p.check_device_batch(buf, offsets)
    block_size = max(16, int(block_size))
    with _p.DeviceCall(buf) as d:
        n = offsets.numel() - 1
        bound = d.lib.lz4hip_streams_bound(n, buf.numel(), block_size)
        out, out_off = d.u8(bound), d.i64(n + 1)
        scratch = d.u8(d.lib.lz4hip_streams_encode_scratch_bytes(n, buf.numel(), block_size))
        _lib.check(d.lib.lz4hip_streams_encode_device(buf.data_ptr(), buf.numel(), offsets.data_ptr(), n, block_size, _p.mode(high_compression),
                                                      out.data_ptr(), bound, out_off.data_ptr(), scratch.data_ptr(), scratch.numel(), d.stream))
        bad = ((offsets[1:] < offsets[:-1]).any() | (offsets[0] < 0) | (offsets[-1] > buf.numel())).to(torch.int64).reshape(1)
        total, bad = torch.cat([out_off[n:], bad]).tolist()
        if bad:
            raise ArgumentException(_p.BAD_OFFSETS)
        return out[:total], out_off


def decompress_streams_device(packed, offsets, check: bool = True):
    """[decompress_stream(s) for s in streams] for the streams packed[offsets[i]:offsets[i + 1]] of a CUDA tensor, on the device, on
    torch's current stream -> (data, data_offsets).  Every item's headers are walked by a wavefront of its own, the compressed chunks
    of all items are one batch of the block decoder.  Every chunk before an item's first error is decoded; with check=True the first
    failing item raises what decompress_stream raises for it (.item_index = its index, .error_offset = the failing header's offset
    within the item), with check=False the per-item statuses (LZ4HIP_STREAM_*, 0 = fine; LZ4HIP_E_ARGUMENT for bad offsets) come back
    as a third value instead.  Waits for the device twice: to size the output, and for the outcome."""
    packed, offsets = _p.check_device_batch(packed, offsets)
    with _p.DeviceCall(packed) as d:
        n = offsets.numel() - 1
        out_off, status = d.items(n)
        err_off = d.i64(max(n, 1))
        info_dev = d.record(_lib.StreamsInfo)

        def index(max_chunks):
            scratch = d.u8(d.lib.lz4hip_streams_decode_scratch_bytes(n, max_chunks))
            _lib.check(d.lib.lz4hip_streams_index_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, max_chunks, out_off.data_ptr(),
                                                         status.data_ptr(), err_off.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                         info_dev.data_ptr(), d.stream))
            info = _p.read_record(info_dev, _lib.StreamsInfo)
            return (scratch, info), _table_full(info)

        (scratch, info), max_chunks = _p.settle(2, packed.numel() // 4096 + n + 16, index)  # (a table still too small: the decode's outcome says so)
        out = d.u8(int(info.decoded_bytes))
        _lib.check(d.lib.lz4hip_streams_decode_device(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, C.byref(info), max_chunks,
                                                      scratch.data_ptr(), scratch.numel(), out.data_ptr(), out.numel(), out_off.data_ptr(),
                                                      status.data_ptr(), err_off.data_ptr(), info_dev.data_ptr(), d.stream))
        info = _p.read_record(info_dev, _lib.StreamsInfo)
        if not check:
            return out, out_off, status[:n]
        if info.first_error >= 0:
            raise streams_error(info.error, info.first_error, info.error_offset)
        return out, out_off


def _streams_into(entry, packed, where, n, out, max_chunks, block_size):
    """decompress_streams_into and decompress_streams_spans_into: the library call `entry` over the n items that the tensors `where`
    locate in `packed` (offsets; or begin and end)"""
    out = _p.check_out(out, packed)
    if max_chunks is None:
        max_chunks = out.numel() // max(16, int(block_size)) + n + 16
    with _p.DeviceCall(packed) as d:
        out_off, status = d.items(n)
        err_off = d.i64(max(n, 1))
        info, written = d.record(_lib.StreamsInfo), d.i64(1, zero=True)
        scratch = d.u8(d.lib.lz4hip_streams_decode_into_scratch_bytes(n, max_chunks))
        _lib.check(getattr(d.lib, entry)(packed.data_ptr(), packed.numel(), *(w.data_ptr() for w in where), n, max_chunks, scratch.data_ptr(),
                                         scratch.numel(), out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(),
                                         err_off.data_ptr(), info.data_ptr(), written.data_ptr(), d.stream))
        return out_off, status[:n], err_off[:n], info, written


def decompress_streams_into(packed, offsets, out, max_chunks=None, block_size: int = DEFAULT_BLOCK_SIZE):
    """decompress_streams_device into a tensor the caller already owns, in ONE device call on torch's current stream, without waiting
    for the device -> (out_off, status, error_offset, info, written_items), all device tensors: item i is out[out_off[i]:out_off[i + 1]],
    status and error_offset are per item, info holds the lz4hip_streams_info_t record (read_streams_info, check_streams_into) and
    written_items the int64 count of leading items that fit `out`; the others are not written, and out_off and info.decoded_bytes are
    complete all the same.  max_chunks is the chunk table's size for the whole batch: by default out.numel() // block + n + 16."""
    packed, offsets = _p.check_device_batch(packed, offsets)
    return _streams_into("lz4hip_streams_decode_into_device", packed, (offsets,), offsets.numel() - 1, out, max_chunks, block_size)


def decompress_streams_spans_into(packed, begin, end, out, max_chunks=None, block_size: int = DEFAULT_BLOCK_SIZE):
    """decompress_streams_into for CHOSEN items of an arena: item j of the call is packed[begin[j]:end[j]] (int64 CUDA tensors of m
    entries, from wrap.select_spans, a stream_directory or the caller's own index; any order, repeats, overlaps and holes), in ONE
    device call whose cost follows m -> (out_off, status, error_offset, info, written_items) as decompress_streams_into returns them,
    indexed by position in the call; check_streams_into reads them.  max_chunks counts the chunks of the chosen items, repeats
    included: by default out.numel() // block + m + 16."""
    packed, begin, end = _p.check_device_spans(packed, begin, end)
    return _streams_into("lz4hip_streams_decode_spans_into_device", packed, (begin, end), begin.numel(), out, max_chunks, block_size)


def stream_directory(t, max_chunks=None, block_size: int = DEFAULT_BLOCK_SIZE):
    """The chunk directory of ONE LZ4Stream buffer (a 1-D uint8 CUDA tensor), to keep beside a stream that is decoded more than once
    or in parts -> (hdr_off, out_off, out_off_host): device int64 tensors of chunks + 1 entries -- chunk k's header is at hdr_off[k]
    and its bytes are [out_off[k], out_off[k + 1]) of the plain text; the closing entries are the stream's length and its decoded size
    -- and a host copy of out_off as a numpy array.  t[hdr_off[k]:hdr_off[k + 1]] is a one-chunk item for
    decompress_streams_spans_into.  This is the once-per-stream step: the serial header walk, and it waits for the device (twice when
    the default table of t.numel() // block + 16 chunks was too small).  A header error raises what decompress_stream_device raises."""
    t = _p.check_device_bytes(t, "t")
    if max_chunks is None:
        max_chunks = t.numel() // max(16, int(block_size)) + 16
    with _p.DeviceCall(t) as d:
        info_dev = d.record(_lib.StreamInfo)

        def walk(max_chunks):
            hdr_off, out_off = d.i64(max_chunks + 1), d.i64(max_chunks + 1)
            _lib.check(d.lib.lz4hip_stream_directory_device(t.data_ptr(), t.numel(), max_chunks, hdr_off.data_ptr(), out_off.data_ptr(),
                                                            info_dev.data_ptr(), d.stream))
            info = _p.read_record(info_dev, _lib.StreamInfo)
            return (hdr_off, out_off, info), _table_full(info)

        (hdr_off, out_off, info), _ = _p.settle(2, max_chunks, walk)
        if info.error != _lib.STREAM_OK:                               # (a table still too small is one of them)
            raise _stream_error(info)
        k = int(info.chunks) + 1
        return hdr_off[:k], out_off[:k], out_off[:k].cpu().numpy()


def decompress_stream_range(t, directory, start: int, length: int):
    """Bytes [start, start + length) of the plain text of the LZ4Stream buffer t, given its stream_directory: decodes the chunks that
    cover the range -- whole chunks, as one-chunk spans in one decompress_streams_spans_into call into a chunk-aligned buffer -- and
    returns the length-byte view of it.  Waits for the device once, for the outcome."""
    import torch
    t = _p.check_device_bytes(t, "t")
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
    return _p.read_record(info, _lib.StreamsInfo)


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


def compress_streams_host(buf, offsets, block_size: int = DEFAULT_BLOCK_SIZE, high_compression: bool = False):
    """compress_streams_device for host arrays, through lz4hip_streams_encode_host -> (packed, packed_offsets) as numpy arrays."""
    buf, offsets = _p.check_host_batch(buf, offsets)
    block_size = max(16, int(block_size))
    L = _lib.lib()
    n = offsets.size - 1
    if n and ((np.diff(offsets) < 0).any() or offsets[0] < 0 or offsets[-1] > buf.size):
        raise ArgumentException(_p.BAD_OFFSETS)
    bound = L.lz4hip_streams_bound(n, buf.size, block_size)
    out = np.empty(max(bound, 1), np.uint8)
    out_off = np.empty(n + 1, np.int64)
    _lib.check(L.lz4hip_streams_encode_host(buf.ctypes.data, buf.size, offsets.ctypes.data, n, block_size, _p.mode(high_compression),
                                            out.ctypes.data, bound, out_off.ctypes.data))
    return out[:int(out_off[n])], out_off


def decompress_streams_host(packed, offsets, check: bool = True):
    """decompress_streams_device for host arrays, through lz4hip_streams_decode_host -> (data, data_offsets), or (data, data_offsets,
    status) with check=False."""
    packed, offsets = _p.check_host_batch(packed, offsets)
    L = _lib.lib()
    n = offsets.size - 1
    out_off = np.empty(n + 1, np.int64)
    status = np.empty(max(n, 1), np.int32)
    err_off = np.empty(max(n, 1), np.int64)
    info = _lib.StreamsInfo()
    out = _p.sized_decode_host(lambda dst, dst_cap: L.lz4hip_streams_decode_host(
        packed.ctypes.data, packed.size, offsets.ctypes.data, n, dst, dst_cap, out_off.ctypes.data, status.ctypes.data, err_off.ctypes.data,
        C.byref(info)), info)
    if not check:
        return out, out_off, status[:n]
    if info.first_error >= 0:
        raise streams_error(info.error, info.first_error, info.error_offset)
    return out, out_off
