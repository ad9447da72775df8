"""Device-resident batches of independent LZ4 blocks on torch tensors, and round-robin sharding of a
batch across the GPUs of a node.

torch is plumbing here (device memory, streams, torch.distributed); every byte of codec work happens
in the HIP kernels behind lz4hip_encode_batch_device / lz4hip_decode_batch_device (include/lz4hip.h),
launched on torch's current stream.

Multi-GPU: blocks are independent (the reference allocates a fresh table per call,
original/lz4.c:583,780), so block i belongs to rank i % world_size, each rank keeps its own
src/dst/length arrays, and NO collective touches payload bytes.  Only the 4-byte per-block results
are gathered, on the host side.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _plumbing as _p
from ._plumbing import compress_bound

BLOCK = 65536
BOUND = BLOCK + BLOCK // 255 + 16          # MaximumOutputLength(65536) = 65809
BOUND_STRIDE = (BOUND + 15) // 16 * 16     # 65824: 16-byte aligned slot for one compressed block


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _lens(x, n, device):
    """int -> (None, value); tensor -> (int32 device tensor, upper-bound hint 0)."""
    if isinstance(x, int):
        return None, x
    assert x.dtype == torch.int32 and x.numel() == n and x.device.type == "cuda"
    return x, 0


def _make_batch(src, src_len, dst, dst_cap, result, src_len_hint=0):
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and src.dim() == 2 and dst.dim() == 2
    assert src.is_cuda and dst.is_cuda and src.stride(1) == 1 and dst.stride(1) == 1
    n = src.shape[0]
    assert dst.shape[0] == n and result.numel() == n and result.dtype == torch.int32
    sl, sl_all = _lens(src_len, n, src.device)
    dc, dc_all = _lens(dst_cap, n, src.device)
    if sl is not None:
        sl_all = src_len_hint
    b = _lib.Batch(src=src.data_ptr(), src_off=None, src_stride=src.stride(0), src_len=_ptr(sl),
                   dst=dst.data_ptr(), dst_off=None, dst_stride=dst.stride(0), dst_cap=_ptr(dc),
                   dst_cap_all=dc_all, src_len_all=sl_all, result=result.data_ptr(), n_blocks=n)
    return b, (sl, dc)      # keep the tensors alive until the launch has been enqueued


def encode(src: torch.Tensor, src_len, dst: torch.Tensor, dst_cap, hc: bool = False,
           result: torch.Tensor | None = None, src_len_hint: int = 0) -> torch.Tensor:
    """Compress row i of `src` (src_len bytes) into row i of `dst` (capacity dst_cap).  Returns the
    int32 per-block results (bytes written, 0 = did not fit) -- LZ4_compress[HC]_limitedOutput semantics."""
    if result is None:
        result = torch.empty(src.shape[0], dtype=torch.int32, device=src.device)
    b, keep = _make_batch(src, src_len, dst, dst_cap, result, src_len_hint)
    _lib.check(_lib.lib().lz4hip_encode_batch_device(C.byref(b), _lib.MODE_HC if hc else _lib.MODE_FAST, _stream()))
    return result


def decode(src: torch.Tensor, src_len, dst: torch.Tensor, out_size, known_output_size: bool = True,
           result: torch.Tensor | None = None) -> torch.Tensor:
    """Decompress row i of `src`.  known_output_size=True: out_size is the exact decoded size and the
    result is the number of source bytes consumed (LZ4_uncompress); False: out_size is a capacity and
    the result is the number of bytes produced (LZ4_uncompress_unknownOutputSize).  Negative = error."""
    if result is None:
        result = torch.empty(src.shape[0], dtype=torch.int32, device=src.device)
    b, keep = _make_batch(src, src_len, dst, out_size, result)
    _lib.check(_lib.lib().lz4hip_decode_batch_device(C.byref(b), 1 if known_output_size else 0, _stream()))
    return result


def _dictionary(dictionary, like):
    """(pointer, length, the tensor to keep alive) of the dictionary a batch shares: a 1-D uint8 CUDA tensor on the blocks' device; None
    and an empty one are no dictionary"""
    if dictionary is None:
        return 0, 0, None
    if not _p.is_device_vector(dictionary, "uint8"):
        raise _p.ArgumentException("the dictionary must be a 1-D uint8 CUDA tensor")
    if dictionary.device != like.device:
        raise _p.ArgumentException("the dictionary must be on the blocks' device")
    d = dictionary.contiguous()
    return (d.data_ptr() if d.numel() else 0), d.numel(), d


def decode_dict(src: torch.Tensor, src_len, dst: torch.Tensor, out_size, dictionary: torch.Tensor | None, known_output_size: bool = True,
                result: torch.Tensor | None = None) -> torch.Tensor:
    """decode() with ONE dictionary shared by every block (lz4hip_decode_batch_dict_device, LZ4_decompress_safe_usingDict in a loop):
    a match may start in `dictionary` (1-D uint8, on the device), whose bytes count as lying in front of each block's output; only its
    last 65 535 can be reached.  Results and rules are decode()'s.  The wavefront mapping decodes these batches at every size."""
    ptr, n_dict, keep_dict = _dictionary(dictionary, src)
    if result is None:
        result = torch.empty(src.shape[0], dtype=torch.int32, device=src.device)
    b, keep = _make_batch(src, src_len, dst, out_size, result)
    _lib.check(_lib.lib().lz4hip_decode_batch_dict_device(C.byref(b), ptr, n_dict, 1 if known_output_size else 0, _stream()))
    return result


def encode_dict(src: torch.Tensor, src_len, dst: torch.Tensor, dst_cap, dictionary: torch.Tensor | None,
                result: torch.Tensor | None = None) -> torch.Tensor:
    """encode() in fast mode with ONE dictionary shared by every block (lz4hip_encode_batch_dict_device, K4os's
    LZ4Codec.Encode(source, target, dictionary) in a loop): a match may start in `dictionary` (1-D uint8, on the device), of which only
    the last 65 535 bytes can be reached.  Results are encode()'s; the bytes decode with decode_dict() and the same dictionary.  No
    dictionary, or an empty one, is encode().  The wavefront mapping encodes these batches at every size; the call allocates its 16 KiB
    of scratch (the dictionary's primed table) itself."""
    ptr, n_dict, keep_dict = _dictionary(dictionary, src)
    if result is None:
        result = torch.empty(src.shape[0], dtype=torch.int32, device=src.device)
    b, keep = _make_batch(src, src_len, dst, dst_cap, result)
    need = _lib.lib().lz4hip_encode_dict_scratch_bytes(n_dict)
    scratch = torch.empty(need, dtype=torch.uint8, device=src.device) if need else None   # (the caching allocator keeps it until the stream has passed)
    _lib.check(_lib.lib().lz4hip_encode_batch_dict_device(C.byref(b), ptr, n_dict, _ptr(scratch), need, _stream()))
    return result


def synth(dist: int, seed: int, first_block: int, n_blocks: int, length: int = BLOCK, stride: int | None = None,
          out: torch.Tensor | None = None, device=None, block_step: int = 1) -> torch.Tensor:
    """Synthetic blocks generated on the device (bit-identical to oracle/synth.c); row i is synthetic block
    first_block + i * block_step, so (first_block=rank, block_step=world) is a rank's round-robin share."""
    stride = length if stride is None else stride
    if out is None:
        out = torch.empty((n_blocks, stride), dtype=torch.uint8, device=device or torch.device("cuda"))
    _lib.check(_lib.lib().lz4hip_synth_device(dist, seed, first_block, block_step, n_blocks, out.data_ptr(), out.stride(0),
                                              length, _stream()))
    return out


def checksum(data: torch.Tensor, lens) -> torch.Tensor:
    """Per-block 64-bit checksums (returned as int64 bit patterns)."""
    n = data.shape[0]
    sums = torch.empty(n, dtype=torch.int64, device=data.device)
    ln, ln_all = _lens(lens, n, data.device)
    _lib.check(_lib.lib().lz4hip_checksum_device(data.data_ptr(), None, data.stride(0), _ptr(ln), ln_all,
                                                 sums.data_ptr(), n, _stream()))
    return sums


def count_mismatches(a: torch.Tensor, b: torch.Tensor, lens) -> int:
    """Number of differing bytes between rows of a and b (synchronises)."""
    n = a.shape[0]
    bad = torch.zeros(1, dtype=torch.int64, device=a.device)
    ln, ln_all = _lens(lens, n, a.device)
    _lib.check(_lib.lib().lz4hip_compare_device(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), _ptr(ln), ln_all,
                                                n, bad.data_ptr(), _stream()))
    return int(bad.item())


# ---- sizing a batch before decoding it ---------------------------------------------------------------
def _source(src, src_len, src_off):
    """(n, lz4hip_batch_t without outputs, tensors to keep alive): rows of a 2-D tensor, or a 1-D buffer with int64 offsets."""
    assert src.dtype == torch.uint8 and src.is_cuda and src.stride(-1) == 1
    if src_off is None:
        assert src.dim() == 2
        n, stride = src.shape[0], src.stride(0)
    else:
        assert src.dim() == 1 and src_off.dtype == torch.int64 and src_off.is_cuda and src_off.is_contiguous()
        n, stride = src_off.numel(), 0
    sl, sl_all = _lens(src_len, n, src.device)
    b = _lib.Batch(src=src.data_ptr(), src_off=_ptr(src_off), src_stride=stride, src_len=_ptr(sl), dst=None, dst_off=None,
                   dst_stride=0, dst_cap=None, dst_cap_all=0, src_len_all=sl_all, result=None, n_blocks=n)
    return n, b, (sl, src_off)


def read_sizes_info(info: torch.Tensor) -> _lib.SizesInfo:
    """The lz4hip_sizes_info_t a decoded_sizes call left on the device (synchronises)."""
    return _p.read_record(info, _lib.SizesInfo)


def _dict_len(dict_len) -> int:
    if isinstance(dict_len, bool) or not isinstance(dict_len, int) or dict_len < 0:
        raise _p.ArgumentException("dict_len must be an int >= 0")
    return dict_len


def decoded_sizes_dict(src: torch.Tensor, src_len, dict_len: int, src_off: torch.Tensor | None = None, result: torch.Tensor | None = None):
    """decoded_sizes() for blocks that are decoded against a dictionary of dict_len bytes (lz4hip_decoded_sizes_dict_device): a match may
    start up to min(dict_len, 65 535) bytes before its block.  The walk needs the dictionary's length, not its bytes."""
    return _decoded_sizes(src, src_len, src_off, result, _dict_len(dict_len))


def decode_packed_dict(src: torch.Tensor, src_len, dictionary: torch.Tensor | None, src_off: torch.Tensor | None = None):
    """decode_packed() against a shared dictionary: decoded_sizes_dict, ONE synchronisation, then lz4hip_decode_batch_dict_device
    (unknown size) on the offsets and capacities the query wrote.  Returns (dst, offsets, results) as decode_packed does."""
    ptr, n_dict, keep_dict = _dictionary(dictionary, src)
    n, b, keep = _source(src, src_len, src_off)
    sizes, offsets, info = _decoded_sizes(src, src_len, src_off, None, n_dict)
    total = read_sizes_info(info).decoded_bytes
    dst = torch.empty(total, dtype=torch.uint8, device=src.device)
    results = torch.empty(n, dtype=torch.int32, device=src.device)
    if n == 0:
        return dst, offsets, results
    guard = dst if total > 0 else torch.empty(1, dtype=torch.uint8, device=src.device)      # (dst must be non-NULL even if nothing fits)
    b.dst, b.dst_off, b.dst_cap, b.result = guard.data_ptr(), offsets.data_ptr(), sizes.data_ptr(), results.data_ptr()
    _lib.check(_lib.lib().lz4hip_decode_batch_dict_device(C.byref(b), ptr, n_dict, 0, _stream()))
    return dst, offsets, results


def decoded_sizes(src: torch.Tensor, src_len, src_off: torch.Tensor | None = None, result: torch.Tensor | None = None):
    """What an unknown-size decode of every block would produce, without decoding it (lz4hip_decoded_sizes_device): block i is row i
    of a 2-D `src`, or src[src_off[i]:] of a 1-D one.  Returns (sizes, offsets, info), all on the device and not waited for:
    sizes[i] = max(result[i], 0) (int32), offsets (int64, n + 1) their exclusive scan -- the dst_cap and dst_off of a packed decode --
    and the lz4hip_sizes_info_t record as four int64 (read_sizes_info).  `result` (int32, n) receives the per-block results: bytes
    produced, or -(error position), as LZ4_uncompress_unknownOutputSize with an unbounded output."""
    return _decoded_sizes(src, src_len, src_off, result, None)


def _decoded_sizes(src, src_len, src_off, result, dict_len):
    """decoded_sizes (dict_len None) and decoded_sizes_dict"""
    n, b, keep = _source(src, src_len, src_off)
    sizes = torch.empty(n, dtype=torch.int32, device=src.device)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=src.device)
    info = torch.empty(4, dtype=torch.int64, device=src.device)
    if result is not None:
        assert result.dtype == torch.int32 and result.numel() == n and result.is_cuda and result.is_contiguous()
        b.result = result.data_ptr()
    need = _lib.lib().lz4hip_decoded_sizes_scratch_bytes(n)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=src.device)
    if dict_len is None:
        _lib.check(_lib.lib().lz4hip_decoded_sizes_device(C.byref(b), offsets.data_ptr(), sizes.data_ptr(), scratch.data_ptr(), need,
                                                          info.data_ptr(), _stream()))
    else:
        _lib.check(_lib.lib().lz4hip_decoded_sizes_dict_device(C.byref(b), dict_len, offsets.data_ptr(), sizes.data_ptr(), scratch.data_ptr(), need,
                                                               info.data_ptr(), _stream()))
    return sizes, offsets, info


def decode_packed(src: torch.Tensor, src_len, src_off: torch.Tensor | None = None):
    """Decode blocks of unknown size into a buffer of exactly the bytes they produce: the size query, ONE synchronisation to read its
    info, then lz4hip_decode_batch_device (unknown size) on the offsets and capacities the query wrote.  Returns (dst, offsets,
    results): block i is dst[offsets[i]:offsets[i + 1]] and results[i] its size, negative (and no byte written) for a corrupt one."""
    n, b, keep = _source(src, src_len, src_off)
    sizes, offsets, info = decoded_sizes(src, src_len, src_off)
    total = read_sizes_info(info).decoded_bytes
    dst = torch.empty(total, dtype=torch.uint8, device=src.device)
    results = torch.empty(n, dtype=torch.int32, device=src.device)
    if n == 0:
        return dst, offsets, results
    guard = dst if total > 0 else torch.empty(1, dtype=torch.uint8, device=src.device)      # (dst must be non-NULL even if nothing fits)
    b.dst, b.dst_off, b.dst_cap, b.result = guard.data_ptr(), offsets.data_ptr(), sizes.data_ptr(), results.data_ptr()
    _lib.check(_lib.lib().lz4hip_decode_batch_device(C.byref(b), 0, _stream()))
    return dst, offsets, results


# ---- a batch into one packed buffer: what encode_packed and decode_compact share ---------------------------------------------------
def _launch_packed(name, lead, n, b, device, round_blocks, dst, slot_bytes, dst_cap, block_cap):
    """encode_packed_launch and decode_compact_launch: lz4hip_<name>_scratch_bytes, then lz4hip_<name>_device on the sources in `b`;
    `lead` holds the scalar arguments the call takes between the batch and round_blocks."""
    offsets = torch.empty(n + 1, dtype=torch.int64, device=device)
    lengths = torch.empty(n, dtype=torch.int32, device=device)
    results = torch.empty(n, dtype=torch.int32, device=device)
    info = torch.empty(5, dtype=torch.int64, device=device)
    if block_cap is not None:
        assert block_cap.dtype == torch.int32 and block_cap.numel() == n and block_cap.is_cuda and block_cap.is_contiguous()
        b.dst_cap = block_cap.data_ptr()
    b.dst_cap_all, b.result = slot_bytes, results.data_ptr()
    need = _lib.check(getattr(_lib.lib(), f"lz4hip_{name}_scratch_bytes")(n, slot_bytes, round_blocks))
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    cap = (0 if dst is None else dst.numel()) if dst_cap is None else dst_cap
    _lib.check(getattr(_lib.lib(), f"lz4hip_{name}_device")(C.byref(b), *lead, round_blocks, _ptr(dst), cap, offsets.data_ptr(), lengths.data_ptr(),
                                                            scratch.data_ptr(), need, info.data_ptr(), _stream()))
    return offsets, lengths, results, info


def _two_tries(launch, read, total, n, dst, guess, device):
    """encode_packed and decode_compact: launch(dst) into the caller's `dst`, or into `guess` bytes and, only when not every block
    fit, once more into exactly the bytes the first try's record named in its field `total` -> (dst_view, offsets, lengths, results,
    record).  One wait for the device per try."""
    given = dst is not None
    if given:
        assert dst.dtype == torch.uint8 and dst.is_cuda and dst.dim() == 1 and dst.is_contiguous()
    else:
        dst = torch.empty(max(guess, 0), dtype=torch.uint8, device=device)
    offsets, lengths, results, info = launch(dst)
    h = read(info)
    if not given and h.written_blocks < n:
        dst = torch.empty(getattr(h, total), dtype=torch.uint8, device=device)
        offsets, lengths, results, info = launch(dst)
        h = read(info)
    return dst[:min(getattr(h, total), dst.numel())], offsets, lengths, results, h


# ---- encoding a batch into one packed buffer --------------------------------------------------------
def read_packed_info(info: torch.Tensor) -> _lib.PackedInfo:
    """The lz4hip_packed_info_t an encode_packed call left on the device (synchronises)."""
    return _p.read_record(info, _lib.PackedInfo)


def encode_packed_launch(src, src_len, src_off, hc, round_blocks, dst, slot_bytes, dst_cap=None, block_cap=None):
    """One lz4hip_encode_packed_device call on torch's current stream, not waited for -> (offsets, lengths, results, info), all on the
    device: int64 n + 1, int32 n, int32 n and the lz4hip_packed_info_t record as five int64 (read_packed_info).  dst_cap defaults to
    dst.numel(); block_cap (int32, n) gives per-block output limits."""
    n, b, keep = _source(src, src_len, src_off)
    if src.dim() == 2 and not isinstance(src_len, int):
        b.src_len_all = src.shape[1]                # the hint: no block is longer than its row
    return _launch_packed("encode_packed", (_p.mode(hc),), n, b, src.device, round_blocks, dst, slot_bytes, dst_cap, block_cap)


def encode_packed(src: torch.Tensor, src_len, src_off: torch.Tensor | None = None, hc: bool = False, round_blocks: int = 0,
                  dst: torch.Tensor | None = None, slot_bytes: int | None = None):
    """Compress a batch of blocks into ONE buffer of exactly the bytes they produce (lz4hip_encode_packed_device): block i is row i of
    a 2-D `src`, or src[src_off[i]:] of a 1-D one.  Returns (dst_view, offsets, lengths, results, info): block i's compressed bytes are
    dst_view[offsets[i]:offsets[i + 1]], lengths[i] = max(results[i], 0) their count, results the raw encoder results and info the
    lz4hip_packed_info_t read back (ONE synchronisation).  decode_packed(dst_view, lengths, offsets[:-1]) is the way back.

    round_blocks = K > 0 runs the batch in rounds of K blocks through a ring of K slots (device scratch that does not grow with the
    batch).  slot_bytes, the slot width and per-block limit, defaults to compressBound of the longest block there can be: an int
    src_len itself, the row width of a 2-D src; a 1-D src with a tensor of lengths must bring it.

    dst=None: the first attempt allocates the size a compressor's caller expects to beat, as far as it is known without waiting for
    the device: n * src_len for an int src_len; with a tensor of lengths the bytes `src` spans (n * row width, or src.numel() for a
    1-D src) -- an upper bound of sum(src_len), and far more than that where most blocks are much shorter than their rows; bring
    `dst` then.  Only
    when not every block fits (info.written_blocks < n) is there a second call, into exactly info.packed_bytes bytes: that pass
    ENCODES AGAIN, it does not reuse the first one's work.  With `dst` (1-D uint8) given there is never a second call: dst_view is
    dst[:min(packed_bytes, dst.numel())], the blocks before info.written_blocks are in it, and offsets, lengths, results and
    info.packed_bytes are complete."""
    assert src.dtype == torch.uint8 and src.is_cuda
    n = src.shape[0] if src_off is None else src_off.numel()
    if slot_bytes is None:
        if isinstance(src_len, int):
            slot_bytes = compress_bound(src_len)
        else:
            assert src.dim() == 2, "a 1-D src with per-block lengths needs slot_bytes"
            slot_bytes = compress_bound(src.shape[1])
    slot_bytes = max(int(slot_bytes), 1)
    guess = n * src_len if isinstance(src_len, int) else (n * src.shape[1] if src.dim() == 2 else src.numel())
    return _two_tries(lambda dst: encode_packed_launch(src, src_len, src_off, hc, round_blocks, dst, slot_bytes), read_packed_info,
                      "packed_bytes", n, dst, guess, src.device)


# ---- decoding a batch into one packed buffer without a size walk --------------------------------------
def read_compact_info(info: torch.Tensor) -> _lib.CompactInfo:
    """The lz4hip_compact_info_t a decode_compact call left on the device (synchronises)."""
    return _p.read_record(info, _lib.CompactInfo)


def decode_compact_launch(src, src_len, src_off, round_blocks, dst, slot_bytes, dst_cap=None, block_cap=None):
    """One lz4hip_decode_compact_device call on torch's current stream, not waited for -> (offsets, lengths, results, info), all on the
    device: int64 n + 1, int32 n, int32 n and the lz4hip_compact_info_t record as five int64 (read_compact_info).  dst_cap defaults to
    dst.numel() (0 for dst=None: a size query); block_cap (int32, n) gives per-block output limits below slot_bytes."""
    n, b, keep = _source(src, src_len, src_off)
    return _launch_packed("decode_compact", (), n, b, src.device, round_blocks, dst, slot_bytes, dst_cap, block_cap)


COMPACT_GUESS = 4        # decode_compact's first output buffer: this many times the compressed bytes


def decode_compact(src: torch.Tensor, src_len, src_off: torch.Tensor | None = None, slot_bytes: int = BLOCK, round_blocks: int = 0,
                   dst: torch.Tensor | None = None):
    """Decode blocks of unknown size, none longer than slot_bytes, into ONE buffer of exactly the bytes they produce without sizing
    them first (lz4hip_decode_compact_device): block i is row i of a 2-D `src`, or src[src_off[i]:] of a 1-D one.  Returns (dst_view,
    offsets, lengths, results, info): block i's bytes are dst_view[offsets[i]:offsets[i + 1]], lengths[i] = max(results[i], 0) their
    count, results the raw decoder results (negative, and no byte taken, for a corrupt block or one that decodes to more than
    slot_bytes) and info the lz4hip_compact_info_t read back (ONE synchronisation).

    round_blocks = K > 0 runs the batch in rounds of K blocks through a ring of K slots of slot_bytes (device scratch that does not
    grow with the batch); 0 takes n slots.

    dst=None: the first attempt allocates a guess that needs no wait for the device: COMPACT_GUESS (4) times the compressed bytes as
    far as they are known here -- n * src_len for an int src_len, else the bytes `src` spans -- capped at n * slot_bytes, which no
    batch exceeds.  Only when not every block fits (info.written_blocks < n) is there a second call, into exactly info.decoded_bytes
    bytes: that pass DECODES AGAIN, it does not reuse the first one's work.  With `dst` (1-D uint8) given there is never a second
    call: dst_view is dst[:min(decoded_bytes, dst.numel())], the blocks before info.written_blocks are in it, and offsets, lengths,
    results and info.decoded_bytes are complete."""
    assert src.dtype == torch.uint8 and src.is_cuda
    n = src.shape[0] if src_off is None else src_off.numel()
    slot_bytes = max(int(slot_bytes), 1)
    compressed = n * src_len if isinstance(src_len, int) else src.numel()
    return _two_tries(lambda dst: decode_compact_launch(src, src_len, src_off, round_blocks, dst, slot_bytes), read_compact_info,
                      "decoded_bytes", n, dst, min(COMPACT_GUESS * compressed, n * slot_bytes), src.device)


# ---- round-robin sharding -------------------------------------------------------------------------
def local_block_count(n_blocks: int, rank: int, world: int) -> int:
    """Blocks owned by `rank` when block i lives on rank i % world."""
    return (n_blocks - rank + world - 1) // world if n_blocks > rank else 0


def local_to_global(j, rank: int, world: int):
    return j * world + rank


def gather_results(local: torch.Tensor, n_blocks: int, group=None) -> torch.Tensor | None:
    """Host-side gather of the per-block int32 results of a round-robin sharded batch, in global block
    order, on rank 0 (None elsewhere).  This is metadata (4 B per block); payloads stay where they are."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local.cpu()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    per = (n_blocks + world - 1) // world
    pad = torch.full((per,), -(2 ** 31), dtype=torch.int32)
    pad[:local.numel()] = local.cpu()
    parts = [torch.empty_like(pad) for _ in range(world)] if rank == 0 else None
    dist.gather(pad, parts, dst=0, group=group)
    if rank != 0:
        return None
    out = torch.stack(parts, dim=1).reshape(-1)[:n_blocks]     # [j, r] -> global index j*world + r
    return out.contiguous()
