"""The local format library's dictionary calls (liblz4, found with ctypes.util.find_library: nothing is downloaded) through ctypes, for
tests/test_lz4f_dict_interop.py and tests/golden/make_lz4f_dict_golden.py: LZ4F_createCDict / LZ4F_compressFrame_usingCDict and
LZ4F_decompress_usingDict, beside tests/lz4f_lib.py's plain ones.  load() is None where the library or these calls are absent."""
import ctypes as C
import functools

import lz4f_lib


@functools.lru_cache(maxsize=None)
def load():
    L = lz4f_lib.load()
    if L is None:
        return None
    try:
        L.LZ4F_createCDict.restype, L.LZ4F_createCDict.argtypes = C.c_void_p, [C.c_void_p, C.c_size_t]
        L.LZ4F_freeCDict.restype, L.LZ4F_freeCDict.argtypes = None, [C.c_void_p]
        L.LZ4F_compressFrame_usingCDict.restype = C.c_size_t
        L.LZ4F_compressFrame_usingCDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.LZ4F_decompress_usingDict.restype = C.c_size_t
        L.LZ4F_decompress_usingDict.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t,
                                                C.c_void_p]
        return L
    except AttributeError:
        return None


def compress_frame(src, dictionary, dict_id=0, level=0, linked=False, block_checksum=False, content_checksum=False, content_size=False) -> bytes:
    """LZ4F_compressFrame_usingCDict with 64 KiB blocks; dict_id = 0 writes no ID"""
    L = load()
    src, dictionary = bytes(src), bytes(dictionary)
    p = lz4f_lib._preferences(len(src), 4, level, block_checksum, content_checksum, content_size, linked)
    p.frameInfo.dictID = dict_id
    cdict, ctx = L.LZ4F_createCDict(dictionary, len(dictionary)), C.c_void_p()
    assert cdict and not L.LZ4F_isError(L.LZ4F_createCompressionContext(C.byref(ctx), 100))
    try:
        cap = L.LZ4F_compressFrameBound(len(src), C.byref(p))
        dst = C.create_string_buffer(cap)
        n = L.LZ4F_compressFrame_usingCDict(ctx, dst, cap, src, len(src), cdict, C.byref(p))
        assert not L.LZ4F_isError(n), L.LZ4F_getErrorName(n)
        return dst.raw[:n]
    finally:
        L.LZ4F_freeCompressionContext(ctx)
        L.LZ4F_freeCDict(cdict)


def decompress(frame, dictionary, expect_bytes):
    """LZ4F_decompress_usingDict over ONE frame, in one call -> (content, error name or None)"""
    L = load()
    frame, dictionary = bytes(frame), bytes(dictionary)
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    try:
        out = C.create_string_buffer(max(expect_bytes, 1) + 64)
        dn, sn = C.c_size_t(len(out)), C.c_size_t(len(frame))
        hint = L.LZ4F_decompress_usingDict(ctx, out, C.byref(dn), frame, C.byref(sn), dictionary, len(dictionary), None)
        if L.LZ4F_isError(hint):
            return out.raw[:0], L.LZ4F_getErrorName(hint).decode()
        return out.raw[:dn.value], None if hint == 0 else "incomplete frame"
    finally:
        L.LZ4F_freeDecompressionContext(ctx)
