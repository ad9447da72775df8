"""The LZ4 frame format (magic 0x184D2204, LZ4 Frame format v1.6.x): what every `lz4` tool since r120, LZ4F_compressFrame,
K4os.Compression.LZ4.Streams and python-lz4 write and read.

    LE32 0x184D2204   FLG  BD  [LE64 contentSize if FLG.3]  [LE32 dictID if FLG.0]  HC
    { LE32 blockSize (bit 31: stored raw)  data  [LE32 xxh32(data) if FLG.4] }*
    LE32 0 (EndMark)   [LE32 xxh32(content) if FLG.2]

The blocks are the block format the library encodes and decodes anyway; the framing, the xxHash32 checksums and the packing run on
the device (lz4hip_lz4f_* of include/lz4hip.h).  Frames written here hold independent blocks.  The encoders take dictionary=...,
dict_id=... (LZ4F_compressFrame_usingCDict with independent blocks: every block is encoded against the same dictionary, in fast mode;
dict_id != 0 is written into the descriptor), and the decoders take
dictionary=..., dict_id=... (LZ4F_decompress_usingDict: ONE dictionary per call, in front of every frame's first byte); without one,
frames with a dictionary ID are refused with a clear message, not decoded wrongly, and so are frames with linked blocks (FLG.5 clear)
unless the caller passes accept_linked=True.  Skippable frames (magic 0x184D2A50 .. 0x184D2A5F) are skipped, appended frames decoded one after
the other.

Many frames at once -- the buffers of an Arrow IPC stream, the record batches of a Kafka log, a service's pickled messages -- go
through the batch calls (lz4hip_lz4f_batch_*): compress_frames_device / decompress_frames_device and their host forms take one buffer
and int64 offsets[n + 1], as the batches of stream.py and wrap.py do, and treat every item as ONE frame."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, _plumbing as _p
from .codec import ArgumentException

MAGIC = 0x184D2204
SKIPPABLE_MAGIC = 0x184D2A50
BLOCK_SIZES = {65536: 4, 262144: 5, 1048576: 6, 4194304: 7}
HEADER_PEEK = 19                                                       # magic + FLG + BD + content size + dictID + HC

_TEXT = {
    _lib.LZ4F_BAD_MAGIC: "not an LZ4 frame: unknown magic number",
    _lib.LZ4F_BAD_HEADER: "frame descriptor: wrong version, reserved bit set or invalid block size",
    _lib.LZ4F_HEADER_CHECKSUM: "frame descriptor: header checksum mismatch",
    _lib.LZ4F_UNSUPPORTED_LINKED: "frames with linked blocks are not supported: their blocks decode only in order",
    _lib.LZ4F_UNSUPPORTED_DICT: "frames with a dictionary ID are not supported",
    _lib.LZ4F_SLOT_TOO_SMALL: "the frame's block maximum exceeds the slot it was given",
    _lib.LZ4F_TRUNCATED: "truncated frame",
    _lib.LZ4F_BAD_BLOCK_SIZE: "block size exceeds the frame's block maximum",
    _lib.LZ4F_CORRUPT_BLOCK: "Decoding Failed ! Corrupted input !",
    _lib.LZ4F_BLOCK_CHECKSUM_ERROR: "block checksum mismatch",
    _lib.LZ4F_CONTENT_SIZE_ERROR: "decoded size differs from the frame's content size",
    _lib.LZ4F_CONTENT_CHECKSUM_ERROR: "content checksum mismatch",
}
# ... and of a call with a dictionary, the only ones that know the outcome
_DICT_TEXT = dict(_TEXT)
_DICT_TEXT[_lib.LZ4F_DICT_ID_MISMATCH] = "the frame's dictionary ID is not the one the caller expects"


def _frame_error(status: int, error_offset: int = -1, texts=_TEXT):
    """The exception the decoders raise for an LZ4HIP_LZ4F_* outcome, with where it was met in .error_offset and the code in .status."""
    status = int(status)
    e = ArgumentException(texts[status]) if status in texts else _lib.Lz4HipError(f"lz4 frame decode: unexpected outcome {status}")
    e.error_offset, e.status = int(error_offset), status
    return e


def _xxh32_small(data: bytes) -> int:
    """XXH32 (seed 0) of fewer than 16 bytes: the descriptor's HC byte"""
    P1, P2, P3, P4, P5, M = 2654435761, 2246822519, 3266489917, 668265263, 374761393, 0xFFFFFFFF
    assert len(data) < 16
    h = (P5 + len(data)) & M
    i = 0
    while i + 4 <= len(data):
        h = (h + int.from_bytes(data[i:i + 4], "little") * P3) & M
        h = (((h << 17) | (h >> 15)) & M) * P4 & M
        i += 4
    for b in data[i:]:
        h = (h + b * P5) & M
        h = (((h << 11) | (h >> 21)) & M) * P1 & M
    h ^= h >> 15
    h = h * P2 & M
    h ^= h >> 13
    h = h * P3 & M
    return h ^ (h >> 16)


def parse_header(data) -> dict:
    """The start of a frame -> {"kind": "frame" | "skippable", "header_bytes", and for a frame "flg", "bd", "block_max", "independent",
    "block_checksum", "content_checksum", "content_size" (None if absent), "dict_id" (None if absent); for a skippable frame "size"}.
    Raises ArgumentException as the device walk would (magic, version, reserved bits, block size id, truncation, HC)."""
    data = bytes(data)
    if len(data) < 4:
        raise _frame_error(_lib.LZ4F_BAD_MAGIC, 0)
    magic = int.from_bytes(data[:4], "little")
    if magic & 0xFFFFFFF0 == SKIPPABLE_MAGIC:
        if len(data) < 8:
            raise _frame_error(_lib.LZ4F_TRUNCATED, 4)
        return {"kind": "skippable", "size": int.from_bytes(data[4:8], "little"), "header_bytes": 8}
    if magic != MAGIC:
        raise _frame_error(_lib.LZ4F_BAD_MAGIC, 0)
    if len(data) < 7:
        raise _frame_error(_lib.LZ4F_TRUNCATED, 4)
    flg, bd = data[4], data[5]
    dlen = 3 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
    if (flg >> 6) != 1 or flg & 0x02 or bd & 0x8F or ((bd >> 4) & 7) < 4:
        raise _frame_error(_lib.LZ4F_BAD_HEADER, 4)
    if 4 + dlen > len(data):
        raise _frame_error(_lib.LZ4F_TRUNCATED, 4)
    if data[4 + dlen - 1] != (_xxh32_small(data[4:4 + dlen - 1]) >> 8) & 0xFF:
        raise _frame_error(_lib.LZ4F_HEADER_CHECKSUM, 4 + dlen - 1)
    at = 6
    content_size = dict_id = None
    if flg & 0x08:
        content_size = int.from_bytes(data[at:at + 8], "little")
        at += 8
    if flg & 0x01:
        dict_id = int.from_bytes(data[at:at + 4], "little")
    return {"kind": "frame", "flg": flg, "bd": bd, "block_max": 1 << (8 + 2 * ((bd >> 4) & 7)), "independent": bool(flg & 0x20),
            "block_checksum": bool(flg & 0x10), "content_checksum": bool(flg & 0x04), "content_size": content_size, "dict_id": dict_id,
            "header_bytes": 4 + dlen}


def _block_id(block_size) -> int:
    if int(block_size) not in BLOCK_SIZES:
        raise ArgumentException("block_size must be 65536, 262144, 1048576 or 4194304")
    return BLOCK_SIZES[int(block_size)]


def _encode_flags(block_checksum, content_checksum, content_size) -> int:
    return ((_lib.LZ4F_BLOCK_CHECKSUM if block_checksum else 0) | (_lib.LZ4F_CONTENT_CHECKSUM if content_checksum else 0) |
            (_lib.LZ4F_CONTENT_SIZE if content_size else 0))


def _decode_flags(verify, accept_linked) -> int:
    return ((_lib.LZ4F_VERIFY_BLOCKS | _lib.LZ4F_VERIFY_CONTENT) if verify else 0) | (_lib.LZ4F_ACCEPT_LINKED if accept_linked else 0)


def _device_dictionary(dictionary, like, dict_id):
    """(pointer, length, ID, the tensor to keep alive) of a device call's dictionary: a 1-D uint8 CUDA tensor on the frames' device; None and
    an empty one are no dictionary"""
    if dictionary is None:
        return 0, 0, 0, None
    if not _p.is_device_vector(dictionary, "uint8"):
        raise ArgumentException("the dictionary must be a 1-D uint8 CUDA tensor")
    if dictionary.device != like.device:
        raise ArgumentException("the dictionary must be on the frames' device")
    d = dictionary.contiguous()
    return (d.data_ptr() if d.numel() else 0), d.numel(), _dict_id(dict_id), d


def _host_dictionary(dictionary, dict_id):
    """(pointer, length, ID, the array to keep alive) of a host call's dictionary: bytes-like; None and an empty one are no dictionary"""
    if dictionary is None:
        return 0, 0, 0, None
    d = _p.host_bytes(dictionary)
    return (d.ctypes.data if d.size else 0), d.size, _dict_id(dict_id), d


def _no_hc_with_dictionary(high_compression, dict_len):
    if high_compression and dict_len:
        raise ArgumentException("high_compression with a dictionary is not supported: the dictionary encoder has the fast mode only")


def _dict_id(dict_id) -> int:
    if not 0 <= int(dict_id) <= 0xFFFFFFFF:
        raise ArgumentException("dict_id must be 0 (no check) .. 2^32 - 1")
    return int(dict_id)


def compress_frame_device(t, block_size: int = 65536, high_compression: bool = False, block_checksum: bool = False,
                          content_checksum: bool = False, content_size: bool = True, dictionary=None, dict_id: int = 0):
    """One LZ4 frame of a 1-D uint8 CUDA tensor, entirely on the device, on torch's current stream, returned as a 1-D uint8 CUDA tensor:
    independent blocks of block_size bytes, a block that does not shrink stored raw.  The content checksum is ONE serial row of the
    checksum kernel over the whole source.  Waits for the device once, to learn the frame's length.  dictionary: a 1-D uint8 CUDA tensor
    on t's device against which EVERY block is encoded (lz4hip_lz4f_encode_dict_device, LZ4F_compressFrame_usingCDict with independent
    blocks; fast mode only: with high_compression=True it raises ArgumentException); dict_id != 0 is written into the descriptor.  None
    or empty: no dictionary, the plain call."""
    t = _p.check_device_bytes(t, "t")
    bid, flags = _block_id(block_size), _encode_flags(block_checksum, content_checksum, content_size)
    dict_ptr, dict_len, dict_id, keep_dict = _device_dictionary(dictionary, t, dict_id)
    _no_hc_with_dictionary(high_compression, dict_len)
    with _p.DeviceCall(t) as d:
        n = t.numel()
        if dict_len:
            out = d.u8(_lib.check(d.lib.lz4hip_lz4f_dict_bound(n, bid, flags, dict_len, dict_id)))
            scratch = d.u8(_lib.check(d.lib.lz4hip_lz4f_encode_dict_scratch_bytes(n, bid, dict_len)))
            out_len = d.i64(1)
            _lib.check(d.lib.lz4hip_lz4f_encode_dict_device(t.data_ptr(), n, dict_ptr, dict_len, dict_id, bid, flags, out.data_ptr(), out.numel(),
                                                            out_len.data_ptr(), scratch.data_ptr(), scratch.numel(), d.stream))
            return out[:int(out_len.item())]
        out = d.u8(d.lib.lz4hip_lz4f_bound(n, bid, flags))
        scratch = d.u8(max(d.lib.lz4hip_lz4f_encode_scratch_bytes(n, bid), 1))
        out_len = d.i64(1)
        _lib.check(d.lib.lz4hip_lz4f_encode_device(t.data_ptr(), n, bid, _p.mode(high_compression), flags, out.data_ptr(), out.numel(),
                                                   out_len.data_ptr(), scratch.data_ptr(), scratch.numel(), d.stream))
        return out[:int(out_len.item())]


def decompress_frame_device(t, verify: bool = True, round_blocks: int = 0, accept_linked: bool = False, dictionary=None, dict_id: int = 0):
    """The content of the LZ4 frames in a 1-D uint8 CUDA tensor -- appended frames one after the other, skippable frames skipped -- as a
    1-D uint8 CUDA tensor, decoded on the device on torch's current stream.  Per frame the host reads the first 19 bytes back (the block
    maximum sizes the decoder's slots, the content size the output and the table), calls lz4hip_lz4f_decode_device once and reads its
    record; only a frame without a content size whose output outgrows the guess, or with more blocks than the table, is decoded again.
    verify=True checks whatever checksums the frame carries, as every reader of this format does; verify=False skips both.  The
    content checksum is ONE row of the checksum kernel -- four serial chains over the whole output, bound by their latency whatever the
    device (DESIGN.md 7 records the measured single-row rate, or says that it has not been measured yet) -- so verify=False is worth it for large frames whose
    integrity is known.  round_blocks = K > 0 decodes K blocks at a time through a ring of K slots.  accept_linked=True decodes frames
    with linked blocks (LZ4HIP_LZ4F_ACCEPT_LINKED) instead of refusing them: such a frame is one serial chain on ONE wavefront, far
    slower for one large frame than a host core -- it pays in decompress_frames_device, many frames at once.  dictionary: a 1-D
    uint8 CUDA tensor on t's device whose bytes count as lying in front of EVERY frame's first byte (lz4hip_lz4f_decode_dict_device,
    LZ4F_decompress_usingDict); dict_id != 0 refuses a frame whose descriptor carries another ID.  None or empty: no dictionary, and a
    frame with a dictionary ID is refused.  Raises ArgumentException with the outcome's text."""
    import torch
    t = _p.check_device_bytes(t, "t")
    flags = _decode_flags(verify, accept_linked)
    dict_ptr, dict_len, dict_id, keep_dict = _device_dictionary(dictionary, t, dict_id)
    with _p.DeviceCall(t) as d:
        info_dev = d.record(_lib.Lz4fInfo)
        parts, pos, n = [], 0, t.numel()
        if n == 0:
            raise _frame_error(_lib.LZ4F_BAD_MAGIC, 0)
        while pos < n:
            try:
                head = parse_header(t[pos:pos + HEADER_PEEK].cpu().numpy().tobytes())
            except ArgumentException as e:
                e.error_offset += pos
                raise
            if head["kind"] == "skippable":
                if pos + 8 + head["size"] > n:
                    raise _frame_error(_lib.LZ4F_TRUNCATED, pos + 4)
                pos += 8 + head["size"]
                continue
            rest = n - pos

            def decode(guess):
                max_blocks, out_bytes = guess
                need = _lib.check(d.lib.lz4hip_lz4f_decode_scratch_bytes(head["block_max"], max_blocks, round_blocks))
                scratch, out = d.u8(need), d.u8(out_bytes)
                if dict_len:
                    _lib.check(d.lib.lz4hip_lz4f_decode_dict_device(t.data_ptr() + pos, rest, dict_ptr, dict_len, dict_id, head["block_max"], max_blocks,
                                                                    round_blocks, flags, scratch.data_ptr(), need, out.data_ptr(), out_bytes,
                                                                    info_dev.data_ptr(), d.stream))
                else:
                    _lib.check(d.lib.lz4hip_lz4f_decode_device(t.data_ptr() + pos, rest, head["block_max"], max_blocks, round_blocks, flags,
                                                               scratch.data_ptr(), need, out.data_ptr(), out_bytes, info_dev.data_ptr(), d.stream))
                info = _p.read_record(info_dev, _lib.Lz4fInfo)
                return (out, info), _p.table_or_output(info, "blocks", _lib.LZ4F_TABLE_FULL, guess)

            known = head["content_size"]
            out_bytes = known if known is not None and known <= 255 * rest else 4 * rest
            max_blocks = (out_bytes if known is not None else rest) // head["block_max"] + 16
            (out, info), (max_blocks, out_bytes) = _p.settle(3, (max_blocks, out_bytes), decode)
            if info.error == _lib.LZ4F_TABLE_FULL or info.decoded_bytes > out_bytes:
                raise _lib.Lz4HipError("lz4 frame decode: the size field walk did not settle")
            if info.error != _lib.LZ4F_OK:
                raise _frame_error(info.error, pos + info.error_offset if info.error_offset >= 0 else -1, _DICT_TEXT if dict_len else _TEXT)
            parts.append(out[:int(info.decoded_bytes)])
            pos += int(info.frame_bytes)
        if not parts:                                                 # (skippable frames only)
            return d.u8(0)
        return parts[0] if len(parts) == 1 else torch.cat(parts)


def compress_frame_host(data, block_size: int = 65536, high_compression: bool = False, block_checksum: bool = False,
                        content_checksum: bool = False, content_size: bool = True, dictionary=None, dict_id: int = 0) -> bytes:
    """compress_frame_device for host bytes, through lz4hip_lz4f_encode_host: one staged call, the frame packed on the device.  dictionary
    (bytes-like here, through lz4hip_lz4f_encode_dict_host) and dict_id as in compress_frame_device."""
    raw = _p.host_bytes(data)
    bid, flags = _block_id(block_size), _encode_flags(block_checksum, content_checksum, content_size)
    dict_ptr, dict_len, dict_id, keep_dict = _host_dictionary(dictionary, dict_id)
    _no_hc_with_dictionary(high_compression, dict_len)
    L = _lib.lib()
    if dict_len:
        bound = _lib.check(L.lz4hip_lz4f_dict_bound(raw.size, bid, flags, dict_len, dict_id))
        out = np.empty(bound, np.uint8)
        out_len = C.c_int64(0)
        _lib.check(L.lz4hip_lz4f_encode_dict_host(raw.ctypes.data, raw.size, dict_ptr, dict_len, dict_id, bid, flags, out.ctypes.data, bound, C.byref(out_len)))
        return out[:out_len.value].tobytes()
    bound = L.lz4hip_lz4f_bound(raw.size, bid, flags)
    out = np.empty(bound, np.uint8)
    out_len = C.c_int64(0)
    _lib.check(L.lz4hip_lz4f_encode_host(raw.ctypes.data, raw.size, bid, _p.mode(high_compression), flags, out.ctypes.data, bound,
                                         C.byref(out_len)))
    return out[:out_len.value].tobytes()


def decompress_frame_host(frame, verify: bool = True, accept_linked: bool = False, dictionary=None, dict_id: int = 0) -> bytes:
    """decompress_frame_device for host bytes, through lz4hip_lz4f_decode_host: per frame a size query (dst_cap = 0), then the call that
    decodes into exactly that size.  Appended frames follow each other; skippable frames are skipped.  accept_linked, dictionary
    (bytes-like here, through lz4hip_lz4f_decode_dict_host) and dict_id as in decompress_frame_device."""
    buf = _p.host_bytes(frame)
    flags = _decode_flags(verify, accept_linked)
    dict_ptr, dict_len, dict_id, keep_dict = _host_dictionary(dictionary, dict_id)
    L = _lib.lib()
    parts, pos = [], 0
    if buf.size == 0:
        raise _frame_error(_lib.LZ4F_BAD_MAGIC, 0)
    while pos < buf.size:
        info = _lib.Lz4fInfo()
        at, rest = buf.ctypes.data + pos, buf.size - pos
        if dict_len:
            call = lambda dst, dst_cap: L.lz4hip_lz4f_decode_dict_host(at, rest, dict_ptr, dict_len, dict_id, flags, dst, dst_cap, C.byref(info))
        else:
            call = lambda dst, dst_cap: L.lz4hip_lz4f_decode_host(at, rest, flags, dst, dst_cap, C.byref(info))
        out = _p.sized_decode_host(call, info, after_e_argument_only=True)
        if info.error != _lib.LZ4F_OK:
            raise _frame_error(info.error, pos + info.error_offset if info.error_offset >= 0 else -1, _DICT_TEXT if dict_len else _TEXT)
        parts.append(out.tobytes())
        pos += int(info.frame_bytes)
    return b"".join(parts)


def xxh32_rows_device(data, off, lens, seed: int = 0):
    """XXH32 of rows of a 1-D uint8 CUDA tensor on torch's current stream: row i is data[off[i] : off[i] + lens[i]] (off: int64 CUDA
    tensor, lens: int32 CUDA tensor).  Returns the hashes as an int32 CUDA tensor of uint32 bit patterns; launch-only."""
    import torch
    data = _p.check_device_bytes(data, "data")
    if off.dtype != torch.int64 or lens.dtype != torch.int32 or off.numel() != lens.numel() or not (off.is_cuda and lens.is_cuda):
        raise ArgumentException("off must be an int64 and lens an int32 CUDA tensor of the same length")
    with _p.DeviceCall(data) as d:
        n = off.numel()
        sums = d.i32(n)
        _lib.check(d.lib.lz4hip_xxh32_rows_device(data.data_ptr(), off.contiguous().data_ptr(), 0, lens.contiguous().data_ptr(), 0,
                                                  seed & 0xFFFFFFFF, sums.data_ptr(), n, d.stream))
        return sums


# ---- batches of frames: one buffer, offsets[n + 1], one frame per item ---------------------------------------------------------------------

def _item_error(batch, texts=_TEXT):
    """the exception of the first failing item of a batch record (lz4hip_lz4f_batch_info_t), with the item's index in .item"""
    i = int(batch.first_error)
    if batch.error == _lib.E_ARGUMENT:
        e = ArgumentException(_p.BAD_OFFSETS)
        e.error_offset, e.status = -1, int(batch.error)
    else:
        e = _frame_error(batch.error, batch.error_offset, texts)
    e.item = i
    return e


def compress_frames_device(t, offsets, block_size: int = 65536, high_compression: bool = False, block_checksum: bool = False,
                           content_checksum: bool = False, content_size: bool = True, dictionary=None, dict_id: int = 0):
    """[compress_frame_device(item) for item in items] for the items t[offsets[i]:offsets[i + 1]] of a 1-D uint8 CUDA tensor, in one
    call on the device, on torch's current stream -> (frames, frame_offsets): item i's frame is frames[frame_offsets[i]:
    frame_offsets[i + 1]], byte for byte the frame of that item alone.  The blocks of all items are one batch of the block encoder,
    the block checksums rows of one checksum launch, the n content checksums n rows of another.  Waits for the device once, to learn
    the total.  dictionary and dict_id as in compress_frame_device: ONE dictionary and one ID for all items
    (lz4hip_lz4f_batch_encode_dict_device); with it every block is encoded on the wavefront mapping."""
    import torch
    t, offsets = _p.check_device_batch(t, offsets)
    bid, flags = _block_id(block_size), _encode_flags(block_checksum, content_checksum, content_size)
    dict_ptr, dict_len, dict_id, keep_dict = _device_dictionary(dictionary, t, dict_id)
    _no_hc_with_dictionary(high_compression, dict_len)
    with _p.DeviceCall(t) as d:
        n = offsets.numel() - 1
        if dict_len:
            bound = _lib.check(d.lib.lz4hip_lz4f_batch_dict_bound(n, t.numel(), bid, flags, dict_len, dict_id))
            out, out_off = d.u8(bound), d.i64(n + 1)
            scratch = d.u8(max(_lib.check(d.lib.lz4hip_lz4f_batch_encode_dict_scratch_bytes(n, t.numel(), bid, dict_len)), 1))
            _lib.check(d.lib.lz4hip_lz4f_batch_encode_dict_device(t.data_ptr(), t.numel(), offsets.data_ptr(), n, dict_ptr, dict_len, dict_id, bid, flags,
                                                                  out.data_ptr(), bound, out_off.data_ptr(), scratch.data_ptr(), scratch.numel(), d.stream))
        else:
            bound = d.lib.lz4hip_lz4f_batch_bound(n, t.numel(), bid, flags)
            out, out_off = d.u8(bound), d.i64(n + 1)
            scratch = d.u8(max(d.lib.lz4hip_lz4f_batch_encode_scratch_bytes(n, t.numel(), bid), 1))
            _lib.check(d.lib.lz4hip_lz4f_batch_encode_device(t.data_ptr(), t.numel(), offsets.data_ptr(), n, bid, _p.mode(high_compression), flags,
                                                             out.data_ptr(), bound, out_off.data_ptr(), scratch.data_ptr(), scratch.numel(), d.stream))
        bad = ((offsets[1:] < offsets[:-1]).any() | (offsets[0] < 0) | (offsets[-1] > t.numel())).to(torch.int64).reshape(1)
        total, bad = torch.cat([out_off[n:], bad]).tolist()
        if bad:
            raise ArgumentException(_p.BAD_OFFSETS)
        return out[:total], out_off


def decompress_frames_device(t, offsets, slot_bytes: int = 65536, verify: bool = True, round_blocks: int = 0, max_blocks=None,
                             accept_linked: bool = False, dictionary=None, dict_id: int = 0):
    """[decompress_frame_device(item) for item in items] for items of ONE frame each, t[offsets[i]:offsets[i + 1]] of a 1-D uint8 CUDA
    tensor, in one call on the device, on torch's current stream -> (data, data_offsets).  Every item's size fields are walked by a
    wavefront of its own, the blocks of all items are one table of the block decoder, the content checksums n rows of one launch.
    slot_bytes bounds every item's block maximum (65536, 262144, 1048576 or 4194304): an item with larger blocks fails with "the frame's
    block maximum exceeds the slot".  max_blocks is the table's size for the whole batch (default: a guess from the bytes); a table
    that was too small, or an output that outgrew the guess of four times the input, is decoded once more from the record.  A skippable
    item gives no bytes; what lies behind an item's frame is left alone.  round_blocks = K > 0 decodes K blocks at a time through a
    ring of K slots instead of one slot per table row.  accept_linked=True decodes items whose blocks are linked (the default of
    LZ4F_compressFrame, python-lz4 and Arrow's LZ4_FRAME codec above one block) instead of failing them: each such item is decoded in
    order by ONE wavefront, so the flag pays in batches of many items.  dictionary and dict_id as in decompress_frame_device: ONE
    dictionary for all items (lz4hip_lz4f_batch_decode_dict_device); with it every compressed block decodes on the wavefront mapping.
    Raises the first failing item's ArgumentException, its index in .item."""
    t, offsets = _p.check_device_batch(t, offsets)
    flags = _decode_flags(verify, accept_linked)
    dict_ptr, dict_len, dict_id, keep_dict = _device_dictionary(dictionary, t, dict_id)
    if int(slot_bytes) not in BLOCK_SIZES:
        raise ArgumentException("slot_bytes must be 65536, 262144, 1048576 or 4194304")
    with _p.DeviceCall(t) as d:
        n = offsets.numel() - 1
        out_off, items_dev = d.i64(n + 1), d.u8(C.sizeof(_lib.Lz4fInfo) * max(n, 1), zero=True)
        info_dev, written = d.record(_lib.Lz4fBatchInfo), d.i64(1, zero=True)

        def decode(guess):
            rows, out_bytes = guess
            need = _lib.check(d.lib.lz4hip_lz4f_batch_decode_scratch_bytes(n, slot_bytes, rows, round_blocks))
            scratch, out = d.u8(max(need, 1)), d.u8(out_bytes)
            if dict_len:
                _lib.check(d.lib.lz4hip_lz4f_batch_decode_dict_device(t.data_ptr(), t.numel(), offsets.data_ptr(), n, dict_ptr, dict_len, dict_id, slot_bytes,
                                                                      rows, round_blocks, flags, scratch.data_ptr(), need, out.data_ptr(), out_bytes,
                                                                      out_off.data_ptr(), items_dev.data_ptr(), info_dev.data_ptr(), written.data_ptr(),
                                                                      d.stream))
            else:
                _lib.check(d.lib.lz4hip_lz4f_batch_decode_device(t.data_ptr(), t.numel(), offsets.data_ptr(), n, slot_bytes, rows, round_blocks, flags,
                                                                 scratch.data_ptr(), need, out.data_ptr(), out_bytes, out_off.data_ptr(),
                                                                 items_dev.data_ptr(), info_dev.data_ptr(), written.data_ptr(), d.stream))
            info = _p.read_record(info_dev, _lib.Lz4fBatchInfo)
            return (out, info), _p.table_or_output(info, "blocks", _lib.LZ4F_TABLE_FULL, guess)

        rows = int(max_blocks) if max_blocks is not None else t.numel() // 16384 + n + 16
        (out, info), (rows, out_bytes) = _p.settle(3, (rows, 4 * t.numel()), decode)
        if info.error == _lib.LZ4F_TABLE_FULL or info.decoded_bytes > out_bytes:
            raise _lib.Lz4HipError("lz4 frame batch decode: the size field walks did not settle")
        if info.first_error >= 0:
            raise _item_error(info, _DICT_TEXT if dict_len else _TEXT)
        return out[:int(info.decoded_bytes)], out_off


def compress_frames_host(buf, offsets, block_size: int = 65536, high_compression: bool = False, block_checksum: bool = False,
                         content_checksum: bool = False, content_size: bool = True, dictionary=None, dict_id: int = 0):
    """compress_frames_device for host arrays, through lz4hip_lz4f_batch_encode_host -> (frames, frame_offsets) as numpy arrays.
    dictionary (bytes-like here, through lz4hip_lz4f_batch_encode_dict_host) and dict_id as in compress_frame_device."""
    buf, offsets = _p.check_host_batch(buf, offsets)
    bid, flags = _block_id(block_size), _encode_flags(block_checksum, content_checksum, content_size)
    dict_ptr, dict_len, dict_id, keep_dict = _host_dictionary(dictionary, dict_id)
    _no_hc_with_dictionary(high_compression, dict_len)
    n = offsets.size - 1
    if n and ((np.diff(offsets) < 0).any() or offsets[0] < 0 or offsets[-1] > buf.size):
        raise ArgumentException(_p.BAD_OFFSETS)
    L = _lib.lib()
    if dict_len:
        bound = _lib.check(L.lz4hip_lz4f_batch_dict_bound(n, buf.size, bid, flags, dict_len, dict_id))
        out = np.empty(max(bound, 1), np.uint8)
        out_off = np.empty(n + 1, np.int64)
        _lib.check(L.lz4hip_lz4f_batch_encode_dict_host(buf.ctypes.data, buf.size, offsets.ctypes.data, n, dict_ptr, dict_len, dict_id, bid, flags,
                                                        out.ctypes.data, bound, out_off.ctypes.data))
        return out[:int(out_off[n])], out_off
    bound = L.lz4hip_lz4f_batch_bound(n, buf.size, bid, flags)
    out = np.empty(max(bound, 1), np.uint8)
    out_off = np.empty(n + 1, np.int64)
    _lib.check(L.lz4hip_lz4f_batch_encode_host(buf.ctypes.data, buf.size, offsets.ctypes.data, n, bid, _p.mode(high_compression), flags,
                                               out.ctypes.data, bound, out_off.ctypes.data))
    return out[:int(out_off[n])], out_off


def decompress_frames_host(packed, offsets, verify: bool = True, accept_linked: bool = False, dictionary=None, dict_id: int = 0):
    """decompress_frames_device for host arrays, through lz4hip_lz4f_batch_decode_host: a size query (dst_cap = 0), then the call that
    decodes into exactly that size -> (data, data_offsets) as numpy arrays.  The slots take the largest block maximum among the items'
    descriptors.  accept_linked, dictionary (bytes-like here) and dict_id as in decompress_frames_device.  Raises the first failing item's ArgumentException, its index in .item."""
    packed, offsets = _p.check_host_batch(packed, offsets)
    n = offsets.size - 1
    if n and ((np.diff(offsets) < 0).any() or offsets[0] < 0 or offsets[-1] > packed.size):
        raise ArgumentException(_p.BAD_OFFSETS)
    flags = _decode_flags(verify, accept_linked)
    dict_ptr, dict_len, dict_id, keep_dict = _host_dictionary(dictionary, dict_id)
    L = _lib.lib()
    out_off = np.zeros(n + 1, np.int64)
    items = (_lib.Lz4fInfo * max(n, 1))()
    info = _lib.Lz4fBatchInfo()
    if dict_len:
        call = lambda dst, dst_cap: L.lz4hip_lz4f_batch_decode_dict_host(
            packed.ctypes.data, packed.size, offsets.ctypes.data, n, dict_ptr, dict_len, dict_id, flags, dst, dst_cap, out_off.ctypes.data, items, C.byref(info))
    else:
        call = lambda dst, dst_cap: L.lz4hip_lz4f_batch_decode_host(
            packed.ctypes.data, packed.size, offsets.ctypes.data, n, flags, dst, dst_cap, out_off.ctypes.data, items, C.byref(info))
    out = _p.sized_decode_host(call, info, after_e_argument_only=True)
    if info.first_error >= 0:
        raise _item_error(info, _DICT_TEXT if dict_len else _TEXT)
    return out, out_off
