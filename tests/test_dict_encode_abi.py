"""CPU-only, through the built library: the calls that encode a block batch against a shared dictionary (lz4hip_encode_dict_scratch_bytes,
lz4hip_encode_batch_dict_device / _host) check their arguments before they look for a device -- every refusal is LZ4HIP_E_ARGUMENT, never
LZ4HIP_E_DEVICE -- and the Python fronts over them (batch.encode_dict, LZ4Codec.encode_many_with_dictionary) refuse what they must before
they reach the library."""
import ctypes as C

import numpy as np
import pytest

from lz4net_amd import _lib
from lz4net_amd.codec import ArgumentException, ArgumentNullException, LZ4Codec

E_ARGUMENT, E_DEVICE = _lib.E_ARGUMENT, _lib.E_DEVICE


def host_batch(n=2):
    """host memory standing in for a batch: the calls below are refused before anything is launched or staged"""
    keep = np.zeros(1 << 15, np.uint8)
    p = keep.ctypes.data + (-keep.ctypes.data) % 16
    b = _lib.Batch(src=p, src_off=None, src_stride=64, src_len=None, dst=p, dst_off=None, dst_stride=64, dst_cap=None, dst_cap_all=64, src_len_all=32,
                   result=p, n_blocks=n)
    return keep, p, b


def test_the_library_exports_the_calls_with_their_prototypes():
    L = _lib.lib()
    names = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("lz4hip_encode_dict_scratch_bytes", "lz4hip_encode_batch_dict_device", "lz4hip_encode_batch_dict_host"):
        assert hasattr(L, name) and name in names
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/lz4hip.h").read()
    assert "int64_t lz4hip_encode_dict_scratch_bytes(int64_t dict_len);" in header
    assert ("int lz4hip_encode_batch_dict_device(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, void* scratch, int64_t scratch_bytes, "
            "void* stream);") in header
    assert "int lz4hip_encode_batch_dict_host(const lz4hip_batch_t* b, const void* dict, int64_t dict_len);" in header
    assert "FAST MODE ONLY" in header and "LZ4HIP_K_ENCODE_WAVE only" in header


def test_the_scratch_is_the_primed_table():
    L = _lib.lib()
    assert [L.lz4hip_encode_dict_scratch_bytes(n) for n in (-1, 0, 1, 3, 4, 65535, 65536, 1 << 40)] == [0, 0] + [16384] * 6


def test_encode_dict_arguments():
    L = _lib.lib()
    keep, p, b = host_batch()
    need = L.lz4hip_encode_dict_scratch_bytes(16)
    dev = lambda bp, d, n, scratch=p, sb=need: L.lz4hip_encode_batch_dict_device(bp, d, n, scratch, sb, None)   # noqa: E731
    for call in (dev, lambda bp, d, n: L.lz4hip_encode_batch_dict_host(bp, d, n)):
        assert call(None, p, 16) == E_ARGUMENT
        assert call(C.byref(b), p, -1) == E_ARGUMENT and b"dict_len < 0" in L.lz4hip_last_error()
        assert call(C.byref(b), None, 1) == E_ARGUMENT and b"dict is NULL" in L.lz4hip_last_error()
        assert call(C.byref(b), None, -5) == E_ARGUMENT
        for field in ("src", "dst", "result"):
            _, _, bad = host_batch()
            setattr(bad, field, None)
            assert call(C.byref(bad), p, 16) == E_ARGUMENT
        _, _, bad = host_batch(n=-1)
        assert call(C.byref(bad), p, 16) == E_ARGUMENT
        _, _, bad = host_batch(n=-1)
        assert call(C.byref(bad), None, 0) == E_ARGUMENT
    assert dev(C.byref(b), p, 16, scratch=None) == E_ARGUMENT and b"scratch is NULL" in L.lz4hip_last_error()
    assert dev(C.byref(b), p, 16, sb=need - 1) == E_ARGUMENT and b"scratch_bytes" in L.lz4hip_last_error()
    assert dev(C.byref(b), p, 16, scratch=p + 4) == E_ARGUMENT and b"16-byte aligned" in L.lz4hip_last_error()
    _, _, empty = host_batch(n=0)
    assert L.lz4hip_encode_batch_dict_host(C.byref(empty), p, 16) == 0                    # (nothing to do: no device is looked for)
    if L.lz4hip_device_count() == 0:                                                    # what is not refused goes on to the device
        assert dev(C.byref(b), p, 16) == E_DEVICE
        assert dev(C.byref(b), None, 0, scratch=None, sb=0) == E_DEVICE                   # (no dictionary: the scratch may be NULL)
        assert L.lz4hip_encode_batch_dict_host(C.byref(b), p, 16) == E_DEVICE
        assert L.lz4hip_encode_batch_dict_host(C.byref(b), None, 0) == E_DEVICE


def test_codec_front_refusals():
    with pytest.raises(ArgumentNullException):
        LZ4Codec.encode_many_with_dictionary(None, b"abc")
    with pytest.raises(ArgumentNullException):
        LZ4Codec.encode_many_with_dictionary([b"abc"], None)
    with pytest.raises((ArgumentException, TypeError)):
        LZ4Codec.encode_many_with_dictionary([b"abc"], 7)
    with pytest.raises((ArgumentException, TypeError)):
        LZ4Codec.encode_many_with_dictionary([3.5], b"abc")
    assert LZ4Codec.encode_many_with_dictionary([], b"abc") == []                         # (no block: the library is not reached)


def test_batch_front_refusals():
    torch = pytest.importorskip("torch")
    from lz4net_amd import _plumbing, batch
    like = torch.zeros((1, 16), dtype=torch.uint8)
    for bad in (np.zeros(4, np.uint8), torch.zeros(4, dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(_plumbing.ArgumentException):
            batch._dictionary(bad, like)
    assert batch._dictionary(None, like) == (0, 0, None)
    assert callable(batch.encode_dict)
