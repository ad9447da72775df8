"""CPU-only, through the built library: the span calls, the selection and the chunk directory (lz4hip_unwrap_spans_into_device,
lz4hip_streams_decode_spans_into_device, lz4hip_spans_select_device, lz4hip_stream_directory_device) check their arguments before
they look for a device -- every refusal is LZ4HIP_E_ARGUMENT, never LZ4HIP_E_DEVICE, on a machine with or without a GPU.  (No call here
passes the checks: nothing is launched and no pointer is followed.)"""
import numpy as np

from lz4net_amd import _lib

E_ARGUMENT = _lib.E_ARGUMENT


def test_span_calls_check_arguments_first():
    L = _lib.lib()
    m, mc = 3, 8
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    need_u, need_s = L.lz4hip_unwrap_into_scratch_bytes(m), L.lz4hip_streams_decode_into_scratch_bytes(m, mc)
    good = dict(src=p, src_len=100, begin=p, end=p, m=m, max_chunks=mc, scratch=p, dst=p, dst_cap=64, dst_off=p, status=p, eo=p, info=p, written=None)

    def unwrap(**change):
        a = dict(dict(good, scratch_bytes=need_u), **change)
        return L.lz4hip_unwrap_spans_into_device(a["src"], a["src_len"], a["begin"], a["end"], a["m"], a["scratch"], a["scratch_bytes"], a["dst"],
                                                 a["dst_cap"], a["dst_off"], a["status"], a["info"], a["written"], None)

    def streams(**change):
        a = dict(dict(good, scratch_bytes=need_s), **change)
        return L.lz4hip_streams_decode_spans_into_device(a["src"], a["src_len"], a["begin"], a["end"], a["m"], a["max_chunks"], a["scratch"],
                                                         a["scratch_bytes"], a["dst"], a["dst_cap"], a["dst_off"], a["status"], a["eo"], a["info"],
                                                         a["written"], None)

    common = (dict(begin=None), dict(end=None), dict(status=None), dict(scratch=None), dict(src=None), dict(dst=None), dict(dst_off=None),
              dict(info=None), dict(src_len=-1), dict(m=-1), dict(dst_cap=-1), dict(m=1 << 31))
    for change in common + (dict(scratch_bytes=need_u - 1),):
        assert unwrap(**change) == E_ARGUMENT, change
    for change in common + (dict(scratch_bytes=need_s - 1), dict(eo=None), dict(max_chunks=-1), dict(max_chunks=1 << 31)):
        assert streams(**change) == E_ARGUMENT, change
    for args in ((None, 5, p, 3, p, p), (p, 5, None, 3, p, p), (p, 5, p, 3, None, p), (p, 5, p, 3, p, None), (p, -1, p, 3, p, p), (p, 5, p, -1, p, p)):
        assert L.lz4hip_spans_select_device(*args, None) == E_ARGUMENT, args
    for args in ((None, 8, 3, p, p, p), (p, -1, 3, p, p, p), (p, 8, -1, p, p, p), (p, 8, 3, None, p, p), (p, 8, 3, p, None, p), (p, 8, 3, p, p, None)):
        assert L.lz4hip_stream_directory_device(*args, None) == E_ARGUMENT, args
