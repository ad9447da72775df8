"""CPU-only, through the built library: the one-call decodes (lz4hip_stream_decode_into_device, lz4hip_streams_decode_into_device,
lz4hip_unwrap_into_device) check their arguments before they look for a device -- every refusal is LZ4HIP_E_ARGUMENT, never
LZ4HIP_E_DEVICE -- and their scratch sizes grow with their arguments and are 0 where the two-call pair's are."""
import ctypes as C

import numpy as np

from lz4net_amd import _lib

E_ARGUMENT, E_DEVICE = _lib.E_ARGUMENT, _lib.E_DEVICE
BIG = 1 << 31


def buffers():
    """host memory standing in for device pointers: the calls below are refused before anything is launched"""
    a = np.zeros(1 << 16, np.uint8)
    return a, a.ctypes.data


def test_stream_decode_into_arguments():
    L = _lib.lib()
    keep, p = buffers()
    need = L.lz4hip_stream_decode_into_scratch_bytes(8)
    assert need <= keep.size
    good = dict(src=p, src_len=100, max_chunks=8, scratch=p, scratch_bytes=need, dst=p, dst_cap=100, info=p, written=p)

    def call(**over):
        a = dict(good, **over)
        return L.lz4hip_stream_decode_into_device(a["src"], a["src_len"], a["max_chunks"], a["scratch"], a["scratch_bytes"], a["dst"], a["dst_cap"],
                                                  a["info"], a["written"], None)
    for over in (dict(src_len=-1), dict(max_chunks=-1), dict(dst_cap=-1), dict(src=None), dict(dst=None), dict(info=None), dict(scratch=None),
                 dict(scratch_bytes=need - 1), dict(scratch_bytes=-1), dict(max_chunks=BIG, scratch_bytes=1 << 62)):
        assert call(**over) == E_ARGUMENT, over
        assert b"stream decode into" in L.lz4hip_last_error()
    if L.lz4hip_device_count() == 0:                                       # what is not refused goes on to the device
        assert call() == E_DEVICE and call(written=None) == E_DEVICE and call(src=None, src_len=0) == E_DEVICE and call(dst=None, dst_cap=0) == E_DEVICE


def test_streams_decode_into_arguments():
    L = _lib.lib()
    keep, p = buffers()
    need = L.lz4hip_streams_decode_into_scratch_bytes(3, 8)
    assert need <= keep.size
    good = dict(src=p, src_len=100, src_off=p, n=3, max_chunks=8, scratch=p, scratch_bytes=need, dst=p, dst_cap=100, dst_off=p, status=p,
                error_offset=p, info=p, written=p)

    def call(**over):
        a = dict(good, **over)
        return L.lz4hip_streams_decode_into_device(a["src"], a["src_len"], a["src_off"], a["n"], a["max_chunks"], a["scratch"], a["scratch_bytes"],
                                                   a["dst"], a["dst_cap"], a["dst_off"], a["status"], a["error_offset"], a["info"], a["written"], None)
    for over in (dict(src_len=-1), dict(n=-1), dict(max_chunks=-1), dict(dst_cap=-1), dict(src=None), dict(dst=None), dict(info=None),
                 dict(scratch=None), dict(src_off=None), dict(dst_off=None), dict(status=None), dict(error_offset=None),
                 dict(scratch_bytes=need - 1), dict(n=BIG, scratch_bytes=1 << 62), dict(max_chunks=BIG, scratch_bytes=1 << 62)):
        assert call(**over) == E_ARGUMENT, over
        assert b"streams decode into" in L.lz4hip_last_error()
    if L.lz4hip_device_count() == 0:
        assert call() == E_DEVICE and call(written=None) == E_DEVICE and call(dst=None, dst_cap=0) == E_DEVICE
        assert call(n=0, scratch=None, scratch_bytes=0, src_off=None, status=None, error_offset=None) == E_DEVICE


def test_unwrap_into_arguments():
    L = _lib.lib()
    keep, p = buffers()
    need = L.lz4hip_unwrap_into_scratch_bytes(3)
    assert need <= keep.size
    good = dict(src=p, src_len=100, src_off=p, n=3, scratch=p, scratch_bytes=need, dst=p, dst_cap=100, dst_off=p, status=p, info=p, written=p)

    def call(**over):
        a = dict(good, **over)
        return L.lz4hip_unwrap_into_device(a["src"], a["src_len"], a["src_off"], a["n"], a["scratch"], a["scratch_bytes"], a["dst"], a["dst_cap"],
                                           a["dst_off"], a["status"], a["info"], a["written"], None)
    for over in (dict(src_len=-1), dict(n=-1), dict(dst_cap=-1), dict(src=None), dict(dst=None), dict(info=None), dict(scratch=None),
                 dict(src_off=None), dict(dst_off=None), dict(status=None), dict(scratch_bytes=need - 1), dict(n=BIG, scratch_bytes=1 << 62)):
        assert call(**over) == E_ARGUMENT, over
        assert b"unwrap into" in L.lz4hip_last_error()
    if L.lz4hip_device_count() == 0:
        assert call() == E_DEVICE and call(written=None) == E_DEVICE and call(dst=None, dst_cap=0) == E_DEVICE


def test_scratch_sizes():
    L = _lib.lib()
    sizes = (-3, 0, 1, 63, 64, 65, 1000, 4096, 4097, 100000, 1 << 22)
    one = [L.lz4hip_stream_decode_into_scratch_bytes(m) for m in sizes]
    assert one == sorted(one) and all(a >= L.lz4hip_stream_decode_scratch_bytes(m) for a, m in zip(one, sizes))
    un = [L.lz4hip_unwrap_into_scratch_bytes(n) for n in sizes]
    assert un == sorted(un) and all(a >= L.lz4hip_unwrap_scratch_bytes(n) for a, n in zip(un, sizes))
    assert one[0] == one[1] and un[0] == un[1]                              # (negative counts are taken as 0)
    grid = [[L.lz4hip_streams_decode_into_scratch_bytes(n, m) for m in sizes] for n in sizes]
    for i, row in enumerate(grid):
        assert row == sorted(row), sizes[i]
        for j, v in enumerate(row):
            pair = L.lz4hip_streams_decode_scratch_bytes(sizes[i], sizes[j])
            assert (v == 0) == (pair == 0) and v >= pair, (sizes[i], sizes[j])
            assert i == 0 or v >= grid[i - 1][j], (sizes[i], sizes[j])
    assert all(v == 0 for v in grid[0]) and all(v == 0 for v in grid[1])    # no item: no scratch
    for m in sizes:                                                         # the pair's sizes are never 0 for these two: neither are these
        assert (L.lz4hip_stream_decode_into_scratch_bytes(m) == 0) == (L.lz4hip_stream_decode_scratch_bytes(m) == 0)
        assert (L.lz4hip_unwrap_into_scratch_bytes(m) == 0) == (L.lz4hip_unwrap_scratch_bytes(m) == 0)
