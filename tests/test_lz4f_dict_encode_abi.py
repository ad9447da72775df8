"""CPU-only, through the built library: the calls that encode LZ4 frames with a dictionary (lz4hip_lz4f_dict_bound,
lz4hip_lz4f_encode_dict_scratch_bytes, lz4hip_lz4f_encode_dict_device / _host and their batch forms) are exported with the header's
signatures, check their arguments before they look for a device -- every refusal is LZ4HIP_E_ARGUMENT, never LZ4HIP_E_DEVICE -- their
queries equal the plain ones without a dictionary, and the Python fronts over them refuse what they must before they reach the library."""
import ctypes as C
import inspect

import numpy as np
import pytest

from lz4net_amd import _lib, lz4_frame
from lz4net_amd.codec import ArgumentException

E_ARGUMENT, E_DEVICE = _lib.E_ARGUMENT, _lib.E_DEVICE
NAMES = ("lz4hip_lz4f_dict_bound", "lz4hip_lz4f_encode_dict_scratch_bytes", "lz4hip_lz4f_encode_dict_device", "lz4hip_lz4f_encode_dict_host",
         "lz4hip_lz4f_batch_dict_bound", "lz4hip_lz4f_batch_encode_dict_scratch_bytes", "lz4hip_lz4f_batch_encode_dict_device",
         "lz4hip_lz4f_batch_encode_dict_host")


def test_the_library_exports_the_calls_with_the_headers_signatures():
    L = _lib.lib()
    symbols = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    header = " ".join(open(__file__.rsplit("/tests/", 1)[0] + "/include/lz4hip.h").read().split())
    ctype = {"int64_t": C.c_int64, "int": C.c_int, "unsigned": C.c_uint, "uint32_t": C.c_uint32}
    for name in NAMES:
        assert hasattr(L, name) and name in symbols
        at = header.index(name + "(")
        result = header[:at].split()[-1]
        params = header[at + len(name) + 1:header.index(");", at)].split(",")
        want = [C.c_void_p if "*" in p else ctype[p.split()[0]] for p in params]
        res, args = symbols[name]
        assert res is ctype[result], name
        # (a pointer to a record may be typed: what counts is that it is a pointer where the header has one)
        assert len(args) == len(want) and all(a is w or (w is C.c_void_p and hasattr(a, "contents")) for a, w in zip(args, want)), name
    assert "fast mode only" in header and "LZ4HC against a dictionary is out of scope" in header and "LZ4HIP_K_ENCODE_WAVE only" in header


def test_the_queries():
    L = _lib.lib()
    for flags in range(8):
        for n in (0, 1, 300, 65537, 300000):
            for bid in (0, 4, 5, 7):
                plain = L.lz4hip_lz4f_bound(n, bid, flags)
                assert L.lz4hip_lz4f_dict_bound(n, bid, flags, 0, 99) == plain == L.lz4hip_lz4f_dict_bound(n, bid, flags, 13, 0)
                assert L.lz4hip_lz4f_dict_bound(n, bid, flags, 13, 7) == plain + 4 == L.lz4hip_lz4f_dict_bound(n, bid, flags, 1 << 20, 0xFFFFFFFF)
                bplain = L.lz4hip_lz4f_batch_bound(5, n, bid, flags)
                assert L.lz4hip_lz4f_batch_dict_bound(5, n, bid, flags, 0, 99) == bplain == L.lz4hip_lz4f_batch_dict_bound(5, n, bid, flags, 13, 0)
                assert L.lz4hip_lz4f_batch_dict_bound(5, n, bid, flags, 13, 7) == bplain + 4 * 5
                scratch, bscratch = L.lz4hip_lz4f_encode_scratch_bytes(n, bid), L.lz4hip_lz4f_batch_encode_scratch_bytes(5, n, bid)
                assert L.lz4hip_lz4f_encode_dict_scratch_bytes(n, bid, 0) == scratch and L.lz4hip_lz4f_batch_encode_dict_scratch_bytes(5, n, bid, 0) == bscratch
                # the primed table (16 KiB) and the descriptors' three words each, in pieces of 256 bytes
                assert L.lz4hip_lz4f_encode_dict_scratch_bytes(n, bid, 13) == scratch + 16384 + 256
                assert L.lz4hip_lz4f_batch_encode_dict_scratch_bytes(5, n, bid, 70000) == bscratch + 16384 + 256
    assert L.lz4hip_lz4f_batch_encode_dict_scratch_bytes(0, 0, 4, 13) == 0
    for bad in (L.lz4hip_lz4f_dict_bound(300, 4, 0, -1, 0), L.lz4hip_lz4f_dict_bound(300, 4, 8, 13, 0), L.lz4hip_lz4f_dict_bound(300, 3, 0, 13, 0),
                L.lz4hip_lz4f_batch_dict_bound(1, 300, 4, 0, -1, 0), L.lz4hip_lz4f_batch_dict_bound(1, 300, 8, 0, 13, 0),
                L.lz4hip_lz4f_encode_dict_scratch_bytes(300, 4, -1), L.lz4hip_lz4f_encode_dict_scratch_bytes(300, 1, 13),
                L.lz4hip_lz4f_batch_encode_dict_scratch_bytes(1, 300, 4, -1), L.lz4hip_lz4f_batch_encode_dict_scratch_bytes(1, 300, 9, 13)):
        assert bad == E_ARGUMENT


def test_every_argument_error_comes_before_the_device():
    """host memory stands in for device memory: every call below is refused before anything is launched or staged"""
    L = _lib.lib()
    keep = np.full(1 << 18, 0xA7, np.uint8)
    p = keep.ctypes.data + (-keep.ctypes.data) % 256
    src, d, dst, scratch, off = p, p + 4096, p + 8192, p + 65536, np.array([0, 300], np.int64)
    out_len = C.c_int64(-1)
    bound, need = L.lz4hip_lz4f_dict_bound(300, 4, 7, 13, 7), L.lz4hip_lz4f_encode_dict_scratch_bytes(300, 4, 13)
    bbound, bneed = L.lz4hip_lz4f_batch_dict_bound(1, 300, 4, 7, 13, 7), L.lz4hip_lz4f_batch_encode_dict_scratch_bytes(1, 300, 4, 13)

    def one(dict_ptr=d, dict_len=13, bid=4, flags=7, cap=bound, sb=need):
        return [L.lz4hip_lz4f_encode_dict_device(src, 300, dict_ptr, dict_len, 7, bid, flags, dst, cap, C.byref(out_len), scratch, sb, None),
                L.lz4hip_lz4f_encode_dict_host(src, 300, dict_ptr, dict_len, 7, bid, flags, dst, cap, C.byref(out_len))]

    def batch(dict_ptr=d, dict_len=13, bid=4, flags=7, cap=bbound, sb=bneed):
        return [L.lz4hip_lz4f_batch_encode_dict_device(src, 300, off.ctypes.data, 1, dict_ptr, dict_len, 7, bid, flags, dst, cap, scratch, scratch + 65536, sb, None),
                L.lz4hip_lz4f_batch_encode_dict_host(src, 300, off.ctypes.data, 1, dict_ptr, dict_len, 7, bid, flags, dst, cap, scratch)]

    for call, short in ((one, bound - 1), (batch, bbound - 1)):
        assert call(dict_len=-1) == [E_ARGUMENT] * 2 and b"dict_len < 0" in L.lz4hip_last_error()
        assert call(dict_ptr=None) == [E_ARGUMENT] * 2 and b"dict is NULL" in L.lz4hip_last_error()
        assert call(flags=8) == [E_ARGUMENT] * 2
        assert call(bid=3) == [E_ARGUMENT] * 2 and call(bid=8) == [E_ARGUMENT] * 2
        assert call(cap=short) == [E_ARGUMENT] * 2 and b"dst_cap <" in L.lz4hip_last_error()
    assert L.lz4hip_lz4f_encode_dict_device(src, 300, d, 13, 7, 4, 7, dst, bound, C.byref(out_len), scratch, need - 1, None) == E_ARGUMENT
    assert b"lz4hip_lz4f_encode_dict_scratch_bytes" in L.lz4hip_last_error()
    assert L.lz4hip_lz4f_batch_encode_dict_device(src, 300, off.ctypes.data, 1, d, 13, 7, 4, 7, dst, bbound, scratch, scratch + 65536, bneed - 1, None) == E_ARGUMENT
    assert b"lz4hip_lz4f_batch_encode_dict_scratch_bytes" in L.lz4hip_last_error()
    assert (keep == 0xA7).all() and out_len.value == -1, "a refused call writes nothing"
    if L.lz4hip_device_count() == 0:                                                    # what is not refused goes on to the device
        assert one() == [E_DEVICE] * 2 and batch() == [E_DEVICE] * 2
        assert one(dict_ptr=None, dict_len=0, cap=L.lz4hip_lz4f_bound(300, 4, 7), sb=L.lz4hip_lz4f_encode_scratch_bytes(300, 4)) == [E_DEVICE] * 2


def test_the_python_keywords():
    for f in (lz4_frame.compress_frame_device, lz4_frame.compress_frame_host, lz4_frame.compress_frames_device, lz4_frame.compress_frames_host):
        names = list(inspect.signature(f).parameters)
        assert names[-2:] == ["dictionary", "dict_id"] and inspect.signature(f).parameters["dictionary"].default is None
        assert inspect.signature(f).parameters["dict_id"].default == 0
    off = np.array([0, 3], np.int64)
    with pytest.raises(ArgumentException, match="high_compression with a dictionary"):
        lz4_frame.compress_frame_host(b"abc", high_compression=True, dictionary=b"xyz")
    with pytest.raises(ArgumentException, match="high_compression with a dictionary"):
        lz4_frame.compress_frames_host(b"abc", off, high_compression=True, dictionary=b"xyz", dict_id=7)
    for bad_id in (-1, 1 << 32):
        with pytest.raises(ArgumentException, match="dict_id"):
            lz4_frame.compress_frame_host(b"abc", dictionary=b"xyz", dict_id=bad_id)
        with pytest.raises(ArgumentException, match="dict_id"):
            lz4_frame.compress_frames_host(b"abc", off, dictionary=b"xyz", dict_id=bad_id)
    with pytest.raises(ArgumentException, match="block_size"):
        lz4_frame.compress_frame_host(b"abc", block_size=1000, dictionary=b"xyz")


def test_the_device_fronts_refuse_a_dictionary_that_is_no_device_vector():
    torch = pytest.importorskip("torch")
    like = torch.zeros(16, dtype=torch.uint8)
    for bad in (b"xyz", np.zeros(4, np.uint8), torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ArgumentException):
            lz4_frame._device_dictionary(bad, like, 0)
    assert lz4_frame._device_dictionary(None, like, 5) == (0, 0, 0, None)
    with pytest.raises(ArgumentException, match="high_compression with a dictionary"):
        lz4_frame._no_hc_with_dictionary(True, 3)
    lz4_frame._no_hc_with_dictionary(True, 0)
    lz4_frame._no_hc_with_dictionary(False, 3)
