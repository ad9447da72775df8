"""The local format library (liblz4, found with ctypes.util.find_library: nothing is downloaded) through ctypes, for
tests/test_lz4f_interop.py and tests/golden/make_lz4f_golden.py: LZ4F_compressFrame and LZ4F_decompress.  load() is None where the
library is absent."""
import ctypes as C
import ctypes.util
import functools


class FrameInfo(C.Structure):
    """LZ4F_frameInfo_t (lz4frame.h, v1.8.0+)"""
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int), ("frameType", C.c_int),
                ("contentSize", C.c_ulonglong), ("dictID", C.c_uint), ("blockChecksumFlag", C.c_int)]


class Preferences(C.Structure):
    """LZ4F_preferences_t"""
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint), ("favorDecSpeed", C.c_uint),
                ("reserved", C.c_uint * 3)]


@functools.lru_cache(maxsize=None)
def load():
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    try:
        L = C.CDLL(name)
        L.LZ4F_compressFrameBound.restype, L.LZ4F_compressFrameBound.argtypes = C.c_size_t, [C.c_size_t, C.c_void_p]
        L.LZ4F_compressFrame.restype, L.LZ4F_compressFrame.argtypes = C.c_size_t, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.LZ4F_isError.restype, L.LZ4F_isError.argtypes = C.c_uint, [C.c_size_t]
        L.LZ4F_getErrorName.restype, L.LZ4F_getErrorName.argtypes = C.c_char_p, [C.c_size_t]
        L.LZ4F_createDecompressionContext.restype, L.LZ4F_createDecompressionContext.argtypes = C.c_size_t, [C.POINTER(C.c_void_p), C.c_uint]
        L.LZ4F_freeDecompressionContext.restype, L.LZ4F_freeDecompressionContext.argtypes = C.c_size_t, [C.c_void_p]
        L.LZ4F_decompress.restype = C.c_size_t
        L.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
        L.LZ4F_createCompressionContext.restype, L.LZ4F_createCompressionContext.argtypes = C.c_size_t, [C.POINTER(C.c_void_p), C.c_uint]
        L.LZ4F_freeCompressionContext.restype, L.LZ4F_freeCompressionContext.argtypes = C.c_size_t, [C.c_void_p]
        L.LZ4F_compressBound.restype, L.LZ4F_compressBound.argtypes = C.c_size_t, [C.c_size_t, C.c_void_p]
        L.LZ4F_compressBegin.restype, L.LZ4F_compressBegin.argtypes = C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.LZ4F_compressUpdate.restype = C.c_size_t
        L.LZ4F_compressUpdate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.LZ4F_compressEnd.restype, L.LZ4F_compressEnd.argtypes = C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.LZ4_versionNumber.restype = C.c_int
        if L.LZ4_versionNumber() < 10800:                             # (block checksums and this layout of the preferences: v1.8.0)
            return None
        return L
    except (OSError, AttributeError):
        return None


def _preferences(n, block_id, level, block_checksum, content_checksum, content_size, linked):
    p = Preferences()
    p.frameInfo.blockSizeID = block_id
    p.frameInfo.blockMode = 0 if linked else 1
    p.frameInfo.contentChecksumFlag = int(content_checksum)
    p.frameInfo.blockChecksumFlag = int(block_checksum)
    p.frameInfo.contentSize = n if content_size else 0                # (0: none is written)
    p.compressionLevel = level
    return p


def compress_frame(src, block_id=4, level=0, block_checksum=False, content_checksum=False, content_size=False, linked=False) -> bytes:
    """LZ4F_compressFrame.  It lowers the block size id to the smallest that holds the source, and writes independent blocks when
    there is only one."""
    L = load()
    src = bytes(src)
    p = _preferences(len(src), block_id, level, block_checksum, content_checksum, content_size, linked)
    cap = L.LZ4F_compressFrameBound(len(src), C.byref(p))
    dst = C.create_string_buffer(cap)
    n = L.LZ4F_compressFrame(dst, cap, src, len(src), C.byref(p))
    assert not L.LZ4F_isError(n), L.LZ4F_getErrorName(n)
    return dst.raw[:n]


def compress_frame_stream(src, block_id=4, level=0, block_checksum=False, content_checksum=False, content_size=False, linked=False) -> bytes:
    """LZ4F_compressBegin / Update / End: the block size id and the block mode go into the descriptor as they are given"""
    L = load()
    src = bytes(src)
    p = _preferences(len(src), block_id, level, block_checksum, content_checksum, content_size, linked)
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(C.byref(ctx), 100))
    try:
        cap = L.LZ4F_compressBound(len(src), C.byref(p)) + 64
        dst = C.create_string_buffer(cap)
        base, at = C.addressof(dst), 0
        for step in (lambda: L.LZ4F_compressBegin(ctx, base + at, cap - at, C.byref(p)),
                     lambda: L.LZ4F_compressUpdate(ctx, base + at, cap - at, src, len(src), None) if src else 0,
                     lambda: L.LZ4F_compressEnd(ctx, base + at, cap - at, None)):
            n = step()
            assert not L.LZ4F_isError(n), L.LZ4F_getErrorName(n)
            at += n
        return dst.raw[:at]
    finally:
        L.LZ4F_freeCompressionContext(ctx)


def decompress(frame, expect_bytes):
    """LZ4F_decompress over ONE frame -> (content, bytes of `frame` consumed, error name or None)"""
    L = load()
    frame = bytes(frame)
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    try:
        out = C.create_string_buffer(max(expect_bytes, 1) + 64)
        got, pos = b"", 0
        while True:
            dn, sn = C.c_size_t(len(out)), C.c_size_t(len(frame) - pos)
            src = C.create_string_buffer(frame[pos:], len(frame) - pos + 1)
            hint = L.LZ4F_decompress(ctx, out, C.byref(dn), src, C.byref(sn), None)
            if L.LZ4F_isError(hint):
                return got, pos, L.LZ4F_getErrorName(hint).decode()
            got += out.raw[:dn.value]
            pos += sn.value
            if hint == 0:
                return got, pos, None
            if sn.value == 0 and dn.value == 0:
                return got, pos, "incomplete frame"
    finally:
        L.LZ4F_freeDecompressionContext(ctx)
