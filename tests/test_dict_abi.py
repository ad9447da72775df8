"""CPU-only, through the built library: the calls that decode a block batch against a shared dictionary (lz4hip_decode_batch_dict_device /
_host, lz4hip_decoded_sizes_dict_device / _host) check their arguments before they look for a device -- every refusal is
LZ4HIP_E_ARGUMENT, never LZ4HIP_E_DEVICE -- and the Python fronts over them (batch.decode_dict, decoded_sizes_dict, decode_packed_dict,
LZ4Codec.decode_many_with_dictionary) refuse what they must before they reach the library."""
import ctypes as C

import numpy as np
import pytest

from lz4net_amd import _lib
from lz4net_amd.codec import ArgumentException, ArgumentNullException, LZ4Codec

E_ARGUMENT, E_DEVICE = _lib.E_ARGUMENT, _lib.E_DEVICE


def host_batch(n=2):
    """host memory standing in for a batch: the calls below are refused before anything is launched or staged"""
    keep = np.zeros(1 << 12, np.uint8)
    p = keep.ctypes.data
    b = _lib.Batch(src=p, src_off=None, src_stride=64, src_len=None, dst=p, dst_off=None, dst_stride=64, dst_cap=None, dst_cap_all=64, src_len_all=32,
                   result=p, n_blocks=n)
    return keep, p, b


def test_the_library_exports_the_calls_with_their_prototypes():
    L = _lib.lib()
    names = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("lz4hip_decode_batch_dict_device", "lz4hip_decode_batch_dict_host", "lz4hip_decoded_sizes_dict_device", "lz4hip_decoded_sizes_dict_host"):
        assert hasattr(L, name) and name in names
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/lz4hip.h").read()
    assert "int lz4hip_decode_batch_dict_device(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, int known_output_size, void* stream);" in header
    assert "int lz4hip_decode_batch_dict_host(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, int known_output_size);" in header


@pytest.mark.parametrize("known", [0, 1])
def test_decode_dict_arguments(known):
    L = _lib.lib()
    keep, p, b = host_batch()
    for call in (lambda bp, d, n: L.lz4hip_decode_batch_dict_device(bp, d, n, known, None), lambda bp, d, n: L.lz4hip_decode_batch_dict_host(bp, d, n, known)):
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
    _, _, empty = host_batch(n=0)
    assert L.lz4hip_decode_batch_dict_host(C.byref(empty), None, 0, known) == 0          # (nothing to do: no device is looked for)
    if L.lz4hip_device_count() == 0:                                                    # what is not refused goes on to the device
        assert L.lz4hip_decode_batch_dict_device(C.byref(b), p, 16, known, None) == E_DEVICE
        assert L.lz4hip_decode_batch_dict_device(C.byref(b), None, 0, known, None) == E_DEVICE
        assert L.lz4hip_decode_batch_dict_host(C.byref(b), p, 16, known) == E_DEVICE


def test_decoded_sizes_dict_arguments():
    L = _lib.lib()
    keep, p, b = host_batch()
    need = L.lz4hip_decoded_sizes_scratch_bytes(2)
    assert 0 < need <= keep.size
    dev = lambda bp, n, scratch=p, sb=need: L.lz4hip_decoded_sizes_dict_device(bp, n, p, p, scratch, sb, p, None)   # noqa: E731
    assert dev(None, 16) == E_ARGUMENT
    assert dev(C.byref(b), -1) == E_ARGUMENT and b"dict_len < 0" in L.lz4hip_last_error()
    assert dev(C.byref(b), 16, sb=need - 1) == E_ARGUMENT and b"scratch_bytes" in L.lz4hip_last_error()
    _, _, bad = host_batch(n=-1)
    assert dev(C.byref(bad), 16) == E_ARGUMENT
    info = _lib.SizesInfo()
    assert L.lz4hip_decoded_sizes_dict_host(None, 16, p, p, C.byref(info)) == E_ARGUMENT
    assert L.lz4hip_decoded_sizes_dict_host(C.byref(b), -1, p, p, C.byref(info)) == E_ARGUMENT
    assert L.lz4hip_decoded_sizes_dict_host(C.byref(bad), 16, p, p, C.byref(info)) == E_ARGUMENT
    _, _, empty = host_batch(n=0)
    assert L.lz4hip_decoded_sizes_dict_device(C.byref(empty), 70000, None, None, None, 0, None, None) == 0     # (nothing to write)
    if L.lz4hip_device_count() == 0:
        assert dev(C.byref(b), 16) == E_DEVICE and dev(C.byref(b), 0) == E_DEVICE and dev(C.byref(b), 1 << 40) == E_DEVICE


def test_batch_fronts_refuse_a_bad_dictionary():
    import torch
    from lz4net_amd import batch
    rows = torch.zeros((2, 64), dtype=torch.uint8)                     # (never looked at: the dictionary is checked first)
    for bad in (torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.int32), np.zeros(16, np.uint8), b"abc", torch.zeros((2, 8), dtype=torch.uint8)):
        with pytest.raises(ArgumentException, match="dictionary"):
            batch.decode_dict(rows, 32, rows, 64, bad)
        with pytest.raises(ArgumentException, match="dictionary"):
            batch.decode_packed_dict(rows, 32, bad)
    for bad in (-1, 1.5, None, True, "4"):
        with pytest.raises(ArgumentException, match="dict_len"):
            batch.decoded_sizes_dict(rows, 32, bad)


def test_codec_front_checks():
    with pytest.raises(ArgumentNullException):
        LZ4Codec.decode_many_with_dictionary(None, b"dictionary")
    with pytest.raises(ArgumentNullException):
        LZ4Codec.decode_many_with_dictionary([b"\x00"], None)
    with pytest.raises(ArgumentNullException):
        LZ4Codec.decode_many_with_dictionary([None], b"dictionary")
    with pytest.raises(ArgumentException):
        LZ4Codec.decode_many_with_dictionary([b"\x00", b"\x00"], b"dictionary", out_sizes=[1])
    with pytest.raises(ArgumentException):
        LZ4Codec.decode_many_with_dictionary([b"\x00"], b"dictionary", out_sizes=[-1])
    with pytest.raises(ArgumentException):
        LZ4Codec.decode_many_with_dictionary([b"\x00"], np.zeros((2, 2), np.uint8))
    assert LZ4Codec.decode_many_with_dictionary([], b"dictionary") == []
    assert LZ4Codec.decode_many_with_dictionary([], b"", out_sizes=[]) == []
