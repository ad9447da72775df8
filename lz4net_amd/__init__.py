"""lz4net_amd -- MI355X (gfx950) batched LZ4 block codec behind lz4net's LZ4Codec API.

  lz4net_amd.LZ4Codec      host-side mirror of LZ4.LZ4Codec (src/LZ4/LZ4Codec.cs) over the C ABI
  lz4net_amd.batch         device-resident batches on torch tensors (+ round-robin multi-GPU sharding)
  lz4net_amd.stream        LZ4Stream chunk framing with all chunks of a buffer in one GPU batch; compress_streams_* / decompress_streams_*
                           do the same for MANY buffers per call, the chunks of all of them in one batch (lz4hip_streams_*)
  lz4net_amd.wrap          batches of Wrap / WrapHC / Unwrap messages framed on the device (lz4hip_wrap_*)
  lz4net_amd.lz4_frame     LZ4 frames (magic 0x184D2204, what every current lz4 tool reads and writes) encoded and decoded on the
                           device in one call (lz4hip_lz4f_*), and XXH32 of rows of device bytes; compress_frames_* / decompress_frames_*
                           do the same for MANY frames per call, one frame per item (lz4hip_lz4f_batch_*)
  lz4net_amd._plumbing     what those modules do around every library call, once: argument checks, the per-call device context,
                           reading a record back, the retry loop, the host size query
  lz4net_amd._lib          ctypes binding of liblz4hip.so (include/lz4hip.h)

The codec itself is hand-written HIP (lz4net_amd/csrc); Python only moves pointers.
"""
from ._lib import Lz4HipError, lib  # noqa: F401
from .codec import LZ4Codec  # noqa: F401

__all__ = ["LZ4Codec", "Lz4HipError", "lib"]
