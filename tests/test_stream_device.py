"""LZ4Stream buffers on the device (lz4hip_stream_* of include/lz4hip.h, lz4net_amd/stream.py compress_stream_device /
decompress_stream_device).  CPU: the bound and the scratch sizes.  GPU: byte parity with a stream framed by stream_cases.py from the oracle's
blocks, round trips on a non-default torch stream, foreign streams, error cases and the host-pointer pair.  The CPU twin of the GPU
part -- the framing kernels themselves under the SIMT emulator, without the block codec -- lives in test_simt_framing.py."""
import ctypes as C

import numpy as np
import pytest

from lz4net_amd import _lib
from lz4net_amd import stream as st
from lz4net_amd.codec import ArgumentException
from stream_cases import BLOCKS, KINDS, _bad_block, _nonminimal, _offsets, data_of, expected_stream, frame, wide_flags_streams


def _varint_len(v):
    return len(st.write_varint(v))


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_stream_bound_formula():
    L = _lib.lib()
    for B in (16, 127, 128, 16383, 16384, 65536, 1 << 20, (1 << 31) - 1):
        for n in (0, 1, B - 1, B, B + 1, 3 * B + 5):
            chunks = -(-n // B)
            assert L.lz4hip_stream_bound(n, B) == n + chunks * (1 + 2 * _varint_len(B)), (n, B)
    assert L.lz4hip_stream_bound(100, 1) == L.lz4hip_stream_bound(100, 16)      # block_size is clamped to >= 16
    assert L.lz4hip_stream_bound(1 << 40, 16) == (1 << 40) + (1 << 36) * 3       # 64-bit sizes


def test_stream_bound_covers_the_framing_of_any_chunk():
    """Worst case per chunk: flags (1 byte), original length, a compressed length below it -- or the raw payload."""
    L = _lib.lib()
    for B in (16, 128, 16384, 65536):
        worst_compressed = 1 + _varint_len(B) + _varint_len(B - 1) + (B - 1)
        worst_raw = 1 + _varint_len(B) + B
        assert L.lz4hip_stream_bound(B, B) >= max(worst_compressed, worst_raw)


def test_stream_scratch_sizes_are_monotonic():
    L = _lib.lib()
    assert L.lz4hip_stream_encode_scratch_bytes(0, 4096) == 0
    for B in (16, 4096, 65536, 1 << 20):
        prev = 0
        for n in (1, 15, 16, 17, 4095, 4096, 65536, 1 << 20, (1 << 20) + 1, 1 << 26, 1 << 30):
            s = L.lz4hip_stream_encode_scratch_bytes(n, B)
            assert s >= prev and s >= n, (n, B)
            prev = s
    for n in (1, 1000, 1 << 20, 1 << 30):
        prev = None
        for B in (16, 17, 4096, 65536, 1 << 20, (1 << 31) - 1):
            s = L.lz4hip_stream_encode_scratch_bytes(n, B)
            assert prev is None or s <= prev, (n, B)
            prev = s
    prev = 0
    for m in (0, 1, 2, 31, 32, 33, 4096, 1 << 20, 1 << 26):
        s = L.lz4hip_stream_decode_scratch_bytes(m)
        assert s >= prev and s >= 36 * m, m
        prev = s


def test_device_functions_reject_host_data():
    with pytest.raises(ArgumentException):
        st.compress_stream_device(b"abc")
    with pytest.raises(ArgumentException):
        st.decompress_stream_device(np.zeros(4, np.uint8))


# ---- GPU: the expected bytes come from the oracle and the tests' own framing (stream_cases.py) ------------------------------

def sizes_for(B, hc=False):
    k = {16: 200, 4096: 16, 65536: 4, 100003: 3, 1 << 20: 2}[B]
    if hc:
        k = {16: 64, 4096: 8, 65536: 2}[B]
    return [0, 1, k * B, k * B + B // 3 + 7]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, data):
    return torch.from_numpy(np.ascontiguousarray(data)).to("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("B", BLOCKS)
def test_encode_parity_fast(oracle, B):
    torch = _torch()
    for kind in KINDS:
        for size in sizes_for(B):
            data = data_of(oracle, kind, size)
            got = st.compress_stream_device(_dev(torch, data), B).cpu().numpy().tobytes()
            assert got == expected_stream(oracle, data, B, False), (kind, size)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [16, 4096, 65536])
def test_encode_parity_hc(oracle, B):
    torch = _torch()
    for kind in (1, 2, 3, "zeros", "real"):
        for size in sizes_for(B, hc=True):
            data = data_of(oracle, kind, size)
            got = st.compress_stream_device(_dev(torch, data), B, high_compression=True).cpu().numpy().tobytes()
            assert got == expected_stream(oracle, data, B, True), (kind, size)


@pytest.mark.gpu
def test_encode_device_leaves_bytes_past_the_stream_alone(oracle):
    """The C entry point on torch memory: guard bytes behind dst_len stay untouched."""
    torch = _torch()
    L = _lib.lib()
    for B, kind, size in ((16, 2, 3000), (4096, "random", 4096 * 5 + 3), (65536, 3, 65536 * 3 + 1), (100003, "real", 250000)):
        data = data_of(oracle, kind, size)
        src = _dev(torch, data)
        bound = L.lz4hip_stream_bound(size, B)
        dst = torch.full((bound + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(L.lz4hip_stream_encode_scratch_bytes(size, B), dtype=torch.uint8, device="cuda")
        nt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        assert L.lz4hip_stream_encode_device(src.data_ptr(), size, B, 0, dst.data_ptr(), bound, nt.data_ptr(), scratch.data_ptr(),
                                             scratch.numel(), None) == 0
        torch.cuda.synchronize()
        n = int(nt.item())
        host = dst.cpu().numpy()
        assert host[:n].tobytes() == expected_stream(oracle, data, B, False)
        assert (host[n:] == 0xA5).all(), (B, kind)
        # too small a destination or scratch is refused before anything runs
        assert L.lz4hip_stream_encode_device(src.data_ptr(), size, B, 0, dst.data_ptr(), bound - 1, nt.data_ptr(), scratch.data_ptr(),
                                             scratch.numel(), None) == _lib.E_ARGUMENT
        assert L.lz4hip_stream_encode_device(src.data_ptr(), size, B, 0, dst.data_ptr(), bound, nt.data_ptr(), scratch.data_ptr(),
                                             scratch.numel() - 1, None) == _lib.E_ARGUMENT


@pytest.mark.gpu
@pytest.mark.parametrize("B", BLOCKS)
def test_round_trip_on_a_side_stream(oracle, B):
    torch = _torch()
    side = torch.cuda.Stream()
    for hc in (False, True):
        if hc and B > 65536:
            continue
        for kind in KINDS:
            for size in sizes_for(B, hc):
                data = data_of(oracle, kind, size)
                x = _dev(torch, data)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    back = st.decompress_stream_device(st.compress_stream_device(x, B, hc))
                    ok = bool(torch.equal(back, x))
                assert ok, (kind, size, hc)


def _dev_decode(torch, stream_bytes):
    return st.decompress_stream_device(_dev(torch, np.frombuffer(stream_bytes, np.uint8).copy())).cpu().numpy().tobytes()


@pytest.mark.gpu
def test_foreign_streams(oracle):
    torch = _torch()
    rng = np.random.default_rng(5)
    chunks = []
    for i in range(40):
        n = int(rng.integers(1, 20000)) if i % 7 else 0
        data = data_of(oracle, [2, 3, "random", "zeros"][i % 4], n)
        kind = i % 3
        if n == 0:
            chunks.append((0, 0, b""))                                                       # empty chunk
        elif kind == 0:
            chunks.append((0, n, data))                                                      # raw
        elif kind == 1:
            chunks.append((st.FLAG_HIGH_COMPRESSION, n, data))                               # HC flag on a raw chunk
        else:
            r, buf = oracle.compress_raw(data, n + n // 255 + 16, hc=bool(i & 1))
            if r <= n:
                chunks.append((st.FLAG_COMPRESSED | (st.FLAG_HIGH_COMPRESSION if i & 1 else 0), n, buf[:r]))
            else:
                chunks.append((0, n, data))
    s = frame(chunks)
    assert _dev_decode(torch, s) == st.decompress_stream(s)
    # non-minimal varints (0x80 0x00 style) in every field
    a = data_of(oracle, 2, 5000)
    r, buf = oracle.compress_raw(a, 5000)
    s = (_nonminimal(1) + _nonminimal(5000) + _nonminimal(r) + buf[:r].tobytes() + b"\x80\x00" + _nonminimal(7) + b"1234567")
    assert _dev_decode(torch, s) == st.decompress_stream(s) == a.tobytes() + b"1234567"
    # more chunks than the first table holds (ceil(len / 4096) + 16 entries): the table is grown once
    s = frame([(0, 1, bytes([i & 0xFF])) for i in range(3000)])
    assert _dev_decode(torch, s) == st.decompress_stream(s) == bytes(i & 0xFF for i in range(3000))
    assert _dev_decode(torch, b"") == b""
    # flags varints with bits the reference drops: it casts the varint to an int-based enum, so bit 35 and a tenth byte's bits 1..6
    # are not "multiple passes" (src/LZ4/LZ4Stream.cs:167-187, 280, 301)
    for s in wide_flags_streams(oracle):
        assert _dev_decode(torch, s) == st.decompress_stream(s) == data_of(oracle, 2, 5000).tobytes() + b"1234567"


def _expect_same_error(torch, s, offset, want=None):
    try:
        st.decompress_stream(s)
        host_exc = None
    except Exception as e:  # noqa: BLE001  (the class is what is compared)
        host_exc = type(e)
    want = want or host_exc
    assert want is not None
    with pytest.raises(Exception) as ei:
        _dev_decode(torch, s)
    assert type(ei.value) is want, (type(ei.value), want)
    assert ei.value.error_offset == offset


@pytest.mark.gpu
def test_stream_errors(oracle):
    torch = _torch()
    a = data_of(oracle, 2, 3000)
    r, buf = oracle.compress_raw(a, 3000)
    good = [(st.FLAG_COMPRESSED, 3000, buf[:r]), (0, 5, b"hello")]
    head = frame(good)
    # a truncated varint
    _expect_same_error(torch, head + b"\x80", len(head), st.EndOfStreamException)
    _expect_same_error(torch, head + b"\x01\x85", len(head), st.EndOfStreamException)
    # a truncated payload
    _expect_same_error(torch, head + frame([(0, 10, b"0123456789")])[:-3], len(head), st.EndOfStreamException)
    # clen > original
    _expect_same_error(torch, head + frame([(st.FLAG_COMPRESSED, 4, b"123456789")]), len(head), st.EndOfStreamException)
    # passes bits on a compressed chunk
    _expect_same_error(torch, head + frame([(st.FLAG_COMPRESSED | 4, 3000, buf[:r])]), len(head), NotImplementedError)
    # ... which a raw chunk may carry
    s = head + frame([(4, 3, b"abc")])
    assert _dev_decode(torch, s) == st.decompress_stream(s)
    # a corrupt block alone
    chunks = good + [_bad_block()] + good
    _expect_same_error(torch, frame(chunks), _offsets(chunks)[2], ArgumentException)
    # a corrupt block at chunk 2 and a truncated header at chunk 5: chunk 2 comes first in the stream and wins
    chunks = good + [_bad_block()] + good
    s = frame(chunks) + b"\x81"
    assert len(chunks) == 5
    with pytest.raises(st.EndOfStreamException):
        st.parse_chunks(s)
    _expect_same_error(torch, s, _offsets(chunks)[2], ArgumentException)


@pytest.mark.gpu
def test_host_pair(oracle):
    L = _lib.lib()
    for hc, B, kind, size in ((False, 4096, 2, 4096 * 9 + 5), (True, 65536, 3, 65536 * 2 + 77), (False, 16, "real", 999), (False, 1 << 20, 1, 0)):
        data = data_of(oracle, kind, size)
        bound = L.lz4hip_stream_bound(size, B)
        dst = np.full(bound + 64, 0xA5, np.uint8)
        n = C.c_int64(-1)
        assert L.lz4hip_stream_encode_host(data.ctypes.data, size, B, 1 if hc else 0, dst.ctypes.data, bound, C.byref(n)) == 0
        want = expected_stream(oracle, data, B, hc)
        assert n.value == len(want) and dst[:n.value].tobytes() == want and (dst[n.value:] == 0xA5).all()
        comp = dst[:n.value].copy()
        info = _lib.StreamInfo()
        # size query first, then the real call
        rc = L.lz4hip_stream_decode_host(comp.ctypes.data, comp.size, None, 0, C.byref(info))
        assert rc == (_lib.E_ARGUMENT if size else 0) and info.decoded_bytes == size and info.error == 0
        out = np.full(size + 64, 0xA5, np.uint8)
        assert L.lz4hip_stream_decode_host(comp.ctypes.data, comp.size, out.ctypes.data, size, C.byref(info)) == 0
        assert out[:size].tobytes() == data.tobytes() and (out[size:] == 0xA5).all()
        assert info.error == 0 and info.error_offset == -1 and info.decoded_bytes == size
    # an error through the host pair: the outcome code is returned and reported
    s = np.frombuffer(frame([(0, 5, b"hello")]) + b"\x80", np.uint8).copy()
    out = np.zeros(16, np.uint8)
    assert L.lz4hip_stream_decode_host(s.ctypes.data, s.size, out.ctypes.data, out.size, C.byref(info)) == _lib.STREAM_END_OF_STREAM
    assert info.error_offset == 7 and info.chunks == 1 and out[:5].tobytes() == b"hello"
