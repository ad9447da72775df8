"""ctypes binding of liblz4hip.so (the C ABI of include/lz4hip.h).

There is no fallback of any kind: if the shared library is missing it is built with hipcc, and if that
is impossible the import fails loudly.  Calls on a machine without a gfx950 device return
LZ4HIP_E_DEVICE, which the wrappers turn into Lz4HipError.
"""
from __future__ import annotations

import ctypes as C

from . import build as _build

E_DEVICE, E_ARGUMENT, E_MEMORY = -2000000001, -2000000002, -2000000003
MODE_FAST, MODE_HC = 0, 1


class Lz4HipError(RuntimeError):
    pass


class Batch(C.Structure):
    """struct lz4hip_batch (include/lz4hip.h)."""
    _fields_ = [("src", C.c_void_p), ("src_off", C.c_void_p), ("src_stride", C.c_int64), ("src_len", C.c_void_p),
                ("dst", C.c_void_p), ("dst_off", C.c_void_p), ("dst_stride", C.c_int64), ("dst_cap", C.c_void_p),
                ("dst_cap_all", C.c_int32), ("src_len_all", C.c_int32), ("result", C.c_void_p),
                ("n_blocks", C.c_int64)]


class StreamInfo(C.Structure):
    """struct lz4hip_stream_info (include/lz4hip.h)."""
    _fields_ = [("chunks", C.c_int64), ("compressed_chunks", C.c_int64), ("decoded_bytes", C.c_int64), ("error_offset", C.c_int64),
                ("error", C.c_int32), ("reserved", C.c_int32)]


STREAM_OK, STREAM_END_OF_STREAM, STREAM_PASSES, STREAM_CORRUPT_BLOCK, STREAM_TABLE_FULL = range(5)


class UnwrapInfo(C.Structure):
    """struct lz4hip_unwrap_info (include/lz4hip.h)."""
    _fields_ = [("messages", C.c_int64), ("compressed", C.c_int64), ("decoded_bytes", C.c_int64), ("first_error", C.c_int64),
                ("error", C.c_int32), ("reserved", C.c_int32)]


WRAP_OK, WRAP_SIZE_INVALID, WRAP_CORRUPT_HEADER, WRAP_CORRUPT_BLOCK = range(4)


class StreamsInfo(C.Structure):
    """struct lz4hip_streams_info (include/lz4hip.h)."""
    _fields_ = [("items", C.c_int64), ("chunks", C.c_int64), ("compressed_chunks", C.c_int64), ("decoded_bytes", C.c_int64),
                ("first_error", C.c_int64), ("error_offset", C.c_int64), ("error", C.c_int32), ("reserved", C.c_int32)]


class SizesInfo(C.Structure):
    """struct lz4hip_sizes_info (include/lz4hip.h)."""
    _fields_ = [("blocks", C.c_int64), ("decoded_bytes", C.c_int64), ("first_error", C.c_int64), ("error", C.c_int32), ("reserved", C.c_int32)]


class PackedInfo(C.Structure):
    """struct lz4hip_packed_info (include/lz4hip.h)."""
    _fields_ = [("blocks", C.c_int64), ("packed_bytes", C.c_int64), ("written_blocks", C.c_int64), ("first_failed", C.c_int64),
                ("error", C.c_int32), ("reserved", C.c_int32)]


class CompactInfo(C.Structure):
    """struct lz4hip_compact_info (include/lz4hip.h)."""
    _fields_ = [("blocks", C.c_int64), ("decoded_bytes", C.c_int64), ("written_blocks", C.c_int64), ("first_failed", C.c_int64),
                ("error", C.c_int32), ("reserved", C.c_int32)]


class FrameInfo(C.Structure):
    """struct lz4hip_frame_info (include/lz4hip.h)."""
    _fields_ = [("chunks", C.c_int64), ("decoded_bytes", C.c_int64), ("good_bytes", C.c_int64), ("error_offset", C.c_int64),
                ("error", C.c_int32), ("reserved", C.c_int32)]


FRAME_OK, FRAME_BAD_MAGIC, FRAME_TRUNCATED, FRAME_BAD_SIZE, FRAME_CORRUPT_BLOCK, FRAME_TABLE_FULL = range(6)


class Lz4fInfo(C.Structure):
    """struct lz4hip_lz4f_info (include/lz4hip.h)."""
    _fields_ = [("blocks", C.c_int64), ("decoded_bytes", C.c_int64), ("good_bytes", C.c_int64), ("error_offset", C.c_int64),
                ("content_size", C.c_int64), ("frame_bytes", C.c_int64), ("error", C.c_int32), ("kind", C.c_int32), ("block_max", C.c_int32),
                ("flg", C.c_int32), ("bd", C.c_int32), ("checks", C.c_int32)]


class Lz4fBatchInfo(C.Structure):
    """struct lz4hip_lz4f_batch_info (include/lz4hip.h)."""
    _fields_ = [("items", C.c_int64), ("blocks", C.c_int64), ("decoded_bytes", C.c_int64), ("first_error", C.c_int64), ("error_offset", C.c_int64),
                ("error", C.c_int32), ("reserved", C.c_int32)]


(LZ4F_OK, LZ4F_BAD_MAGIC, LZ4F_BAD_HEADER, LZ4F_HEADER_CHECKSUM, LZ4F_UNSUPPORTED_LINKED, LZ4F_UNSUPPORTED_DICT, LZ4F_SLOT_TOO_SMALL,
 LZ4F_TRUNCATED, LZ4F_BAD_BLOCK_SIZE, LZ4F_CORRUPT_BLOCK, LZ4F_BLOCK_CHECKSUM_ERROR, LZ4F_CONTENT_SIZE_ERROR, LZ4F_CONTENT_CHECKSUM_ERROR,
 LZ4F_TABLE_FULL, LZ4F_DICT_ID_MISMATCH) = range(15)
LZ4F_BLOCK_CHECKSUM, LZ4F_CONTENT_CHECKSUM, LZ4F_CONTENT_SIZE = 1, 2, 4
LZ4F_VERIFY_BLOCKS, LZ4F_VERIFY_CONTENT, LZ4F_ACCEPT_LINKED = 1, 2, 8
LZ4F_KIND_FRAME, LZ4F_KIND_SKIPPABLE = 0, 1
LZ4F_CHECK_ABSENT, LZ4F_CHECK_VERIFIED, LZ4F_CHECK_SKIPPED = 0, 1, 2


# every symbol include/lz4hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("lz4hip_codec_name", C.c_char_p, []),
    ("lz4hip_device_count", C.c_int, []),
    ("lz4hip_last_error", C.c_char_p, []),
    ("lz4hip_build_id", C.c_char_p, []),
    ("lz4hip_compressBound", C.c_int, [C.c_int]),
    ("lz4hip_dispatch_counts", C.c_int, [C.c_void_p, C.c_int]),
    ("lz4hip_release_workspaces", C.c_int, []),
    ("lz4hip_tuning_set", C.c_int, [C.c_char_p, C.c_int]),
    ("lz4hip_tuning_get", C.c_int, [C.c_char_p]),
    ("lz4hip_compress_limitedOutput", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("lz4hip_compress", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("lz4hip_compressHC_limitedOutput", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("lz4hip_compressHC", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("lz4hip_uncompress", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("lz4hip_uncompress_unknownOutputSize", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("lz4hip_uncompress_bounded", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("lz4hip_encode_batch_device", C.c_int, [C.POINTER(Batch), C.c_int, C.c_void_p]),
    ("lz4hip_decode_batch_device", C.c_int, [C.POINTER(Batch), C.c_int, C.c_void_p]),
    ("lz4hip_encode_batch_host", C.c_int, [C.POINTER(Batch), C.c_int]),
    ("lz4hip_decode_batch_host", C.c_int, [C.POINTER(Batch), C.c_int]),
    ("lz4hip_decode_batch_dict_device", C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    ("lz4hip_decode_batch_dict_host", C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int64, C.c_int]),
    ("lz4hip_encode_dict_scratch_bytes", C.c_int64, [C.c_int64]),
    ("lz4hip_encode_batch_dict_device", C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_encode_batch_dict_host", C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int64]),
    ("lz4hip_encode_batch_host_multi", C.c_int, [C.POINTER(Batch), C.c_int, C.c_uint64]),
    ("lz4hip_decode_batch_host_multi", C.c_int, [C.POINTER(Batch), C.c_int, C.c_uint64]),
    ("lz4hip_synth_device", C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    ("lz4hip_checksum_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_compare_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_stream_bound", C.c_int64, [C.c_int64, C.c_int32]),
    ("lz4hip_stream_encode_scratch_bytes", C.c_int64, [C.c_int64, C.c_int32]),
    ("lz4hip_stream_decode_scratch_bytes", C.c_int64, [C.c_int64]),
    ("lz4hip_stream_encode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_stream_index_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_stream_decode_device", C.c_int, [C.c_void_p, C.POINTER(StreamInfo), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_stream_decode_into_scratch_bytes", C.c_int64, [C.c_int64]),
    ("lz4hip_stream_decode_into_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]),
    ("lz4hip_stream_directory_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_stream_encode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("lz4hip_stream_decode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(StreamInfo)]),
    ("lz4hip_wrap_bound", C.c_int64, [C.c_int64, C.c_int64]),
    ("lz4hip_wrap_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64]),
    ("lz4hip_unwrap_scratch_bytes", C.c_int64, [C.c_int64]),
    ("lz4hip_wrap_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_unwrap_index_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_void_p, C.c_void_p]),
    ("lz4hip_unwrap_decode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(UnwrapInfo), C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_unwrap_into_scratch_bytes", C.c_int64, [C.c_int64]),
    ("lz4hip_unwrap_into_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_unwrap_spans_into_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_spans_select_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_wrap_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_unwrap_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.POINTER(UnwrapInfo)]),
    ("lz4hip_streams_bound", C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    ("lz4hip_streams_encode_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    ("lz4hip_streams_decode_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64]),
    ("lz4hip_streams_encode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                               C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_streams_index_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_streams_decode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(StreamsInfo), C.c_int64, C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_streams_decode_into_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64]),
    ("lz4hip_streams_decode_into_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_streams_decode_spans_into_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_streams_encode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_streams_decode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(StreamsInfo)]),
    ("lz4hip_decoded_sizes_scratch_bytes", C.c_int64, [C.c_int64]),
    ("lz4hip_decoded_sizes_device", C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_decoded_sizes_host", C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_void_p, C.POINTER(SizesInfo)]),
    ("lz4hip_decoded_sizes_dict_device", C.c_int, [C.POINTER(Batch), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_decoded_sizes_dict_host", C.c_int, [C.POINTER(Batch), C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(SizesInfo)]),
    ("lz4hip_encode_packed_scratch_bytes", C.c_int64, [C.c_int64, C.c_int32, C.c_int64]),
    ("lz4hip_encode_packed_device", C.c_int, [C.POINTER(Batch), C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p]),
    ("lz4hip_encode_packed_host", C.c_int, [C.POINTER(Batch), C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(PackedInfo)]),
    ("lz4hip_decode_compact_scratch_bytes", C.c_int64, [C.c_int64, C.c_int32, C.c_int64]),
    ("lz4hip_decode_compact_device", C.c_int, [C.POINTER(Batch), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_void_p]),
    ("lz4hip_decode_compact_host", C.c_int, [C.POINTER(Batch), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(CompactInfo)]),
    ("lz4hip_frame_bound", C.c_int64, [C.c_int64, C.c_int32]),
    ("lz4hip_frame_encode_scratch_bytes", C.c_int64, [C.c_int64, C.c_int32]),
    ("lz4hip_frame_decode_scratch_bytes", C.c_int64, [C.c_int64]),
    ("lz4hip_frame_encode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_frame_index_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_frame_decode_device", C.c_int, [C.c_void_p, C.POINTER(FrameInfo), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_frame_decode_compact_scratch_bytes", C.c_int64, [C.c_int32, C.c_int64, C.c_int64]),
    ("lz4hip_frame_decode_compact_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                     C.c_void_p, C.c_void_p]),
    ("lz4hip_frame_encode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("lz4hip_frame_decode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(FrameInfo)]),
    ("lz4hip_xxh32_rows_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_lz4f_bound", C.c_int64, [C.c_int64, C.c_int, C.c_uint]),
    ("lz4hip_lz4f_encode_scratch_bytes", C.c_int64, [C.c_int64, C.c_int]),
    ("lz4hip_lz4f_decode_scratch_bytes", C.c_int64, [C.c_int32, C.c_int64, C.c_int64]),
    ("lz4hip_lz4f_encode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_void_p]),
    ("lz4hip_lz4f_decode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_uint, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p]),
    ("lz4hip_lz4f_encode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("lz4hip_lz4f_decode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_uint, C.c_void_p, C.c_int64, C.POINTER(Lz4fInfo)]),
    ("lz4hip_lz4f_batch_bound", C.c_int64, [C.c_int64, C.c_int64, C.c_int, C.c_uint]),
    ("lz4hip_lz4f_batch_encode_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    ("lz4hip_lz4f_batch_encode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_lz4f_batch_decode_scratch_bytes", C.c_int64, [C.c_int64, C.c_int32, C.c_int64, C.c_int64]),
    ("lz4hip_lz4f_batch_decode_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_uint, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("lz4hip_lz4f_batch_encode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_lz4f_batch_decode_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                C.POINTER(Lz4fBatchInfo)]),
    # ... with a dictionary: dict, dict_len, dict_id behind the source arguments
    ("lz4hip_lz4f_decode_dict_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_int32, C.c_int64, C.c_int64, C.c_uint,
                                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("lz4hip_lz4f_decode_dict_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_uint, C.c_void_p, C.c_int64,
                                               C.POINTER(Lz4fInfo)]),
    ("lz4hip_lz4f_batch_decode_dict_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_int32, C.c_int64,
                                                       C.c_int64, C.c_uint, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]),
    ("lz4hip_lz4f_batch_decode_dict_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_uint, C.c_void_p,
                                                     C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(Lz4fBatchInfo)]),
    # the encode with a dictionary (fast mode only: no mode argument)
    ("lz4hip_lz4f_dict_bound", C.c_int64, [C.c_int64, C.c_int, C.c_uint, C.c_int64, C.c_uint32]),
    ("lz4hip_lz4f_encode_dict_scratch_bytes", C.c_int64, [C.c_int64, C.c_int, C.c_int64]),
    ("lz4hip_lz4f_encode_dict_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_int, C.c_uint, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_lz4f_encode_dict_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_int, C.c_uint, C.c_void_p, C.c_int64,
                                               C.POINTER(C.c_int64)]),
    ("lz4hip_lz4f_batch_dict_bound", C.c_int64, [C.c_int64, C.c_int64, C.c_int, C.c_uint, C.c_int64, C.c_uint32]),
    ("lz4hip_lz4f_batch_encode_dict_scratch_bytes", C.c_int64, [C.c_int64, C.c_int64, C.c_int, C.c_int64]),
    ("lz4hip_lz4f_batch_encode_dict_device", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_int, C.c_uint,
                                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("lz4hip_lz4f_batch_encode_dict_host", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint32, C.c_int, C.c_uint,
                                                     C.c_void_p, C.c_int64, C.c_void_p]),
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        try:
            # torch wheels bundle their own libamdhip64 / libhsa-runtime64.  Loading torch FIRST makes the
            # dynamic linker resolve our DT_NEEDED entries to those same copies, so the process has ONE
            # HIP/HSA runtime (two HSA runtimes in one process do not both see the GPU).
            import torch  # noqa: F401
        except ImportError:
            pass
        so = _build.build()                     # raises if the library cannot be produced
        handle = C.CDLL(so)
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(handle, name)          # AttributeError == ABI drift: fail loudly
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


K_DECODE_WAVE, K_DECODE_LANE, K_ENCODE_WAVE, K_ENCODE_LANE, K_HC_WAVE, K_HC_LANE, K_COUNT = range(7)


def dispatch_counts() -> list:
    """Launches per kernel family since the library was loaded (lz4hip_dispatch_counts)."""
    buf = (C.c_uint64 * K_COUNT)()
    n = lib().lz4hip_dispatch_counts(buf, K_COUNT)
    assert n == K_COUNT
    return list(buf)


_MAPPING = {"auto": 0, "wave": 1, "lane": 2}


def tuning_set(name: str, value) -> int:
    """lz4hip_tuning_set; mapping knobs also take "auto" / "wave" / "lane".  Returns the previous value."""
    v = _MAPPING[value] if isinstance(value, str) else int(value)
    return check(lib().lz4hip_tuning_set(name.encode(), v))


def tuning_get(name: str) -> int:
    return check(lib().lz4hip_tuning_get(name.encode()))


class tuning:
    """with tuning(decoder="lane", hc_groups=4): ...  -- sets knobs, restores the previous values on exit."""

    def __init__(self, **knobs):
        self.knobs, self.prev = knobs, {}

    def __enter__(self):
        for k, v in self.knobs.items():
            self.prev[k] = tuning_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            tuning_set(k, v)
        return False


def check(rc: int) -> int:
    """Raise on library-level failures (LZ4HIP_E_*); pass codec results through."""
    if rc <= E_DEVICE and rc >= E_MEMORY:
        raise Lz4HipError(f"liblz4hip error {rc}: {lib().lz4hip_last_error().decode(errors='replace')}")
    return rc
