"""Legacy LZ4 command-line frame of the reference era, batched.

Wire format of the upstream demo CLI that ships with the reference (original/lz4demo.c):

    LE32 magic 0x184C2102 (:86)  { LE32 compressedSize  payload }*

The writer (compress_file, :166-249) cuts the input into 8 MiB chunks (CHUNKSIZE, :84), compresses each with
``LZ4_compress`` (or ``LZ4_compressHC``) into an ``LZ4_compressBound`` buffer and prefixes it with its size.
The reader (decode_file, :252-317) checks the magic, then per chunk reads the size -- a size equal to the magic
means "another frame was appended, keep going" (:289-290) -- and decodes with
``LZ4_uncompress_unknownOutputSize(in, out, size, CHUNKSIZE)``; a negative result is a corrupted file.

The reference handles one chunk per call; here all chunks of a buffer go through ONE
lz4hip_encode_batch_host / lz4hip_decode_batch_host call (include/lz4hip.h).  8 MiB chunks are above 64 KiB, so
the encoder takes the generic variant (``LZ4_compressCtx``, original/lz4.c:345-562) exactly like the reference.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, _plumbing as _p
from .codec import ArgumentException

MAGIC = 0x184C2102
CHUNK_SIZE = 8 << 20


_bound = _p.compress_bound


def compress_frame(data, high_compression: bool = False, chunk_size: int = CHUNK_SIZE) -> bytes:
    """compress_file(): magic + size-prefixed chunks, every chunk compressed in one GPU batch."""
    raw = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    out = bytearray(MAGIC.to_bytes(4, "little"))
    n = (raw.size + chunk_size - 1) // chunk_size
    if n == 0:
        return bytes(out)
    offs = np.arange(n, dtype=np.int64) * chunk_size
    lens = np.minimum(chunk_size, raw.size - offs).astype(np.int32)
    caps = np.array([_bound(int(l)) for l in lens], dtype=np.int32)
    dst_off = np.concatenate(([0], np.cumsum(caps[:-1], dtype=np.int64))).astype(np.int64)
    comp = np.zeros(int(caps.astype(np.int64).sum()), dtype=np.uint8)
    res = np.zeros(n, dtype=np.int32)
    b = _p.host_blocks(raw, offs, lens, comp, dst_off, caps, res)
    _lib.check(_lib.lib().lz4hip_encode_batch_host(C.byref(b), _p.mode(high_compression)))
    for i in range(n):
        size = int(res[i])
        if size <= 0:                                              # cannot happen with a compressBound-sized buffer
            raise ArgumentException("LZ4 compression failed")
        out += size.to_bytes(4, "little")
        out += comp[int(dst_off[i]):int(dst_off[i]) + size].tobytes()
    return bytes(out)


def parse_frame(frame):
    """Header walk -> list of (payload_offset, payload_length); raises on a bad magic or a truncated chunk."""
    buf = memoryview(frame)
    if len(buf) < 4 or int.from_bytes(buf[:4], "little") != MAGIC:
        raise ArgumentException("Unrecognized header : file cannot be decoded")
    pos, chunks = 4, []
    while pos < len(buf):
        if pos + 4 > len(buf):
            raise ArgumentException("truncated chunk header")
        size = int.from_bytes(buf[pos:pos + 4], "little")
        pos += 4
        if size == MAGIC:                                          # appended compressed stream (lz4demo.c:289-290)
            continue
        if pos + size > len(buf):
            raise ArgumentException("truncated chunk payload")
        chunks.append((pos, size))
        pos += size
    return chunks


def decompress_frame(frame, chunk_size: int = CHUNK_SIZE) -> bytes:
    """decode_file(): every chunk decoded (output size unknown, at most `chunk_size`) in one GPU batch."""
    data = np.frombuffer(bytes(frame), dtype=np.uint8)
    chunks = parse_frame(memoryview(bytes(frame)))
    n = len(chunks)
    if n == 0:
        return b""
    src_off = np.array([c[0] for c in chunks], dtype=np.int64)
    src_len = np.array([c[1] for c in chunks], dtype=np.int32)
    dst_off = np.arange(n, dtype=np.int64) * chunk_size
    caps = np.full(n, chunk_size, dtype=np.int32)
    out = np.zeros(n * chunk_size, dtype=np.uint8)
    res = np.zeros(n, dtype=np.int32)
    b = _p.host_blocks(data, src_off, src_len, out, dst_off, caps, res)
    _lib.check(_lib.lib().lz4hip_decode_batch_host(C.byref(b), 0))
    if (res < 0).any():
        raise ArgumentException("Decoding Failed ! Corrupted input !")
    return b"".join(out[int(dst_off[i]):int(dst_off[i]) + int(res[i])].tobytes() for i in range(n))


# ---- whole frames on the device (lz4hip_frame_* of include/lz4hip.h; kernels in csrc/lz4hip_frame.hpp) ---------------------------------

def _frame_error(status: int, error_offset: int = -1, frame_len: int = -1):
    """The exception parse_frame / decompress_frame raise for an LZ4HIP_FRAME_* outcome, with the failing size field's offset in
    .error_offset; frame_len tells a size field cut short from a payload cut short."""
    status, error_offset = int(status), int(error_offset)
    if status == _lib.FRAME_BAD_MAGIC:
        e = ArgumentException("Unrecognized header : file cannot be decoded")
    elif status == _lib.FRAME_TRUNCATED:
        e = ArgumentException("truncated chunk header" if error_offset + 4 > frame_len else "truncated chunk payload")
    elif status == _lib.FRAME_BAD_SIZE:
        e = ArgumentException("chunk size exceeds what a chunk can compress to")
    elif status == _lib.FRAME_CORRUPT_BLOCK:
        e = ArgumentException("Decoding Failed ! Corrupted input !")
    else:
        e = _lib.Lz4HipError(f"frame decode: unexpected outcome {status}")
    e.error_offset = int(error_offset)
    return e


def _check_chunk_size(chunk_size) -> int:
    chunk_size = int(chunk_size)
    if not 1 <= chunk_size <= 0x7E000000:
        raise ArgumentException("chunk_size must be 1 .. 0x7E000000")
    return chunk_size


def compress_frame_device(t, high_compression: bool = False, chunk_size: int = CHUNK_SIZE):
    """compress_frame for a 1-D uint8 CUDA tensor, entirely on the device, on torch's current stream: the same bytes, returned as a 1-D
    uint8 CUDA tensor.  Waits for the device once, to learn the frame's length."""
    t = _p.check_device_bytes(t, "t")
    chunk_size = _check_chunk_size(chunk_size)
    with _p.DeviceCall(t) as d:
        n = t.numel()
        out = d.u8(d.lib.lz4hip_frame_bound(n, chunk_size))
        scratch = d.u8(d.lib.lz4hip_frame_encode_scratch_bytes(n, chunk_size))
        out_len = d.i64(1)
        _lib.check(d.lib.lz4hip_frame_encode_device(t.data_ptr(), n, chunk_size, _p.mode(high_compression), out.data_ptr(), out.numel(),
                                                    out_len.data_ptr(), scratch.data_ptr(), scratch.numel(), d.stream))
        return out[:int(out_len.item())]


def decompress_frame_device(t, chunk_size: int = CHUNK_SIZE):
    """decompress_frame for a 1-D uint8 CUDA tensor, on torch's current stream: the size field walk, the size of every chunk and the block
    decode run on the device, into a buffer of exactly the decoded size; the host reads the index's result once (to size the output)
    and the final outcome once."""
    t = _p.check_device_bytes(t, "t")
    chunk_size = _check_chunk_size(chunk_size)
    with _p.DeviceCall(t) as d:
        n = t.numel()
        info_dev = d.record(_lib.FrameInfo)

        def index(max_chunks):
            scratch = d.u8(d.lib.lz4hip_frame_decode_scratch_bytes(max_chunks))
            _lib.check(d.lib.lz4hip_frame_index_device(t.data_ptr(), n, chunk_size, max_chunks, scratch.data_ptr(), scratch.numel(),
                                                       info_dev.data_ptr(), d.stream))
            info = _p.read_record(info_dev, _lib.FrameInfo)
            return (scratch, info), (int(info.chunks) if info.error == _lib.FRAME_TABLE_FULL else None)

        (scratch, info), max_chunks = _p.settle(2, n // chunk_size + 16, index)
        if info.error == _lib.FRAME_TABLE_FULL:
            raise _lib.Lz4HipError("frame decode: the size field walk did not settle")
        out = d.u8(int(info.decoded_bytes))
        _lib.check(d.lib.lz4hip_frame_decode_device(t.data_ptr(), C.byref(info), max_chunks, scratch.data_ptr(), scratch.numel(),
                                                    out.data_ptr(), out.numel(), info_dev.data_ptr(), d.stream))
        info = _p.read_record(info_dev, _lib.FrameInfo)
        if info.error != _lib.FRAME_OK:
            raise _frame_error(info.error, info.error_offset, n)
        return out


def decompress_frame_compact_device(t, chunk_size: int = CHUNK_SIZE, round_chunks: int = 0):
    """decompress_frame for a 1-D uint8 CUDA tensor through lz4hip_frame_decode_compact_device, on torch's current stream: ONE call walks
    the size fields, decodes every chunk with chunk_size bytes of room -- as the reference's reader does, so a chunk the two-call path of
    decompress_frame_device refuses for breaking the format's end rules at its own size decodes here as it does there -- and packs the
    chunks back to back; no chunk is sized before it is decoded.  The table is sized as decompress_frame_device sizes it.  The output
    buffer is a guess the host can make without waiting: four times the frame, at most chunk_size per chunk the frame can hold; the
    host reads the outcome once, and only a frame with more chunks than the table or more bytes than the guess is decoded again, into
    the count and the size that record gave.  round_chunks = K > 0 decodes K chunks at a time through a ring of K chunk_size slots instead
    of one slot per table row: less scratch, but the rounds do not overlap."""
    t = _p.check_device_bytes(t, "t")
    chunk_size = _check_chunk_size(chunk_size)
    with _p.DeviceCall(t) as d:
        n = t.numel()
        info_dev = d.record(_lib.FrameInfo)

        def decode(guess):
            max_chunks, out_bytes = guess
            need = _lib.check(d.lib.lz4hip_frame_decode_compact_scratch_bytes(chunk_size, max_chunks, round_chunks))
            scratch, out = d.u8(need), d.u8(out_bytes)
            _lib.check(d.lib.lz4hip_frame_decode_compact_device(t.data_ptr(), n, chunk_size, max_chunks, round_chunks, scratch.data_ptr(), need,
                                                                out.data_ptr(), out_bytes, info_dev.data_ptr(), d.stream))
            info = _p.read_record(info_dev, _lib.FrameInfo)
            return (out, info), _p.table_or_output(info, "chunks", _lib.FRAME_TABLE_FULL, guess)

        max_chunks = n // chunk_size + 16
        out_bytes = min(4 * n, min(max_chunks, n // 4) * chunk_size)           # (a chunk takes at least its 4-byte size field)
        (out, info), (max_chunks, out_bytes) = _p.settle(3, (max_chunks, out_bytes), decode)
        if info.error == _lib.FRAME_TABLE_FULL or info.decoded_bytes > out_bytes:
            raise _lib.Lz4HipError("frame decode: the size field walk did not settle")
        if info.error != _lib.FRAME_OK:
            raise _frame_error(info.error, info.error_offset, n)
        return out[:int(info.decoded_bytes)]


def compress_frame_host(data, high_compression: bool = False, chunk_size: int = CHUNK_SIZE) -> bytes:
    """compress_frame through lz4hip_frame_encode_host: one staged call, the frame packed on the device."""
    raw = _p.host_bytes(data)
    chunk_size = _check_chunk_size(chunk_size)
    L = _lib.lib()
    bound = L.lz4hip_frame_bound(raw.size, chunk_size)
    out = np.empty(bound, np.uint8)
    out_len = C.c_int64(0)
    _lib.check(L.lz4hip_frame_encode_host(raw.ctypes.data, raw.size, chunk_size, _p.mode(high_compression), out.ctypes.data, bound,
                                          C.byref(out_len)))
    return out[:out_len.value].tobytes()


def decompress_frame_host(frame, chunk_size: int = CHUNK_SIZE) -> bytes:
    """decompress_frame through lz4hip_frame_decode_host: a size query (dst_cap = 0), then the call that decodes into exactly that size."""
    buf = _p.host_bytes(frame)
    chunk_size = _check_chunk_size(chunk_size)
    L = _lib.lib()
    info = _lib.FrameInfo()
    out = _p.sized_decode_host(lambda dst, dst_cap: L.lz4hip_frame_decode_host(buf.ctypes.data, buf.size, chunk_size, dst, dst_cap, C.byref(info)),
                               info, after_e_argument_only=True)
    if info.error != _lib.FRAME_OK:
        raise _frame_error(info.error, info.error_offset, buf.size)
    return out.tobytes()
