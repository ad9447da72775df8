"""Batches of LZ4Stream buffers on the device (lz4hip_streams_* of include/lz4hip.h, lz4net_amd/stream.py compress_streams_* /
decompress_streams_*).  CPU: the bound, the scratch sizes, the argument checks.  GPU: every item's bytes against a stream framed by
the test from the oracle's blocks AND against the one-stream call on that item alone; round trips, foreign streams, per-item errors,
guard bytes, the dispatch counters of one large batch, the host pair and a 1 GiB round trip.  Everything is exact equality.  The CPU
twin of the GPU part -- the framing kernels themselves under the SIMT emulator, without the block codec -- lives in
test_simt_framing.py."""
import ctypes as C

import numpy as np
import pytest

from lz4net_amd import _lib
from lz4net_amd import stream as st
from lz4net_amd.codec import ArgumentException

from conftest import ForcedMapping
from stream_cases import BLOCKS, KINDS, _bad_block, _nonminimal, _offsets, data_of, expected_stream, frame, wide_flags_streams


def _varint_len(v):
    return len(st.write_varint(v))


def concat(items):
    """list of uint8 arrays / bytes -> (buffer, int64 offsets[n + 1])"""
    items = [np.frombuffer(bytes(m), np.uint8) if not isinstance(m, np.ndarray) else m for m in items]
    offs = np.zeros(len(items) + 1, np.int64)
    if items:
        offs[1:] = np.cumsum([m.size for m in items])
    data = np.concatenate(items) if items else np.zeros(0, np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8), offs


def split(buf, offs):
    buf, offs = np.asarray(buf), np.asarray(offs)
    return [buf[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(offs) - 1)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_streams_bound_covers_every_partition():
    L = _lib.lib()
    rng = np.random.default_rng(3)
    for B in (16, 127, 128, 4096, 65536, 100003, 1 << 20):
        per_chunk = 1 + 2 * _varint_len(B)
        for n in (1, 2, 7, 100):
            for src_len in (0, 1, B - 1, B, B + 1, 5 * B + 3, 40 * B):
                assert L.lz4hip_streams_bound(n, src_len, B) == src_len + (src_len // B + n) * per_chunk, (B, n, src_len)
                for _ in range(4):
                    cuts = np.sort(rng.integers(0, src_len + 1, n - 1)) if n > 1 else np.zeros(0, np.int64)
                    if n > 2:
                        cuts[1] = cuts[0]                                  # an empty item
                    lens = np.diff(np.concatenate([[0], cuts, [src_len]]))
                    assert lens.sum() == src_len and (lens >= 0).all()
                    assert sum(-(-int(x) // B) for x in lens) <= src_len // B + n
                    assert L.lz4hip_streams_bound(n, src_len, B) >= sum(L.lz4hip_stream_bound(int(x), B) for x in lens)
    assert L.lz4hip_streams_bound(5, 1000, 1) == L.lz4hip_streams_bound(5, 1000, 16)          # block_size is clamped to >= 16
    assert L.lz4hip_streams_bound(3, 1000, -5) == L.lz4hip_streams_bound(3, 1000, 16)
    assert L.lz4hip_streams_bound(1 << 33, 1 << 40, 16) == (1 << 40) + ((1 << 36) + (1 << 33)) * 3   # 64-bit sizes
    assert L.lz4hip_streams_bound(0, 0, 4096) == 0


def test_streams_scratch_sizes_are_monotonic():
    L = _lib.lib()
    assert L.lz4hip_streams_encode_scratch_bytes(0, 0, 4096) == 0 and L.lz4hip_streams_encode_scratch_bytes(0, 1 << 20, 4096) == 0
    assert L.lz4hip_streams_decode_scratch_bytes(0, 0) == 0 and L.lz4hip_streams_decode_scratch_bytes(0, 1000) == 0
    sizes = (0, 1, 15, 16, 17, 4095, 4096, 65536, 1 << 20, (1 << 20) + 1, 1 << 26, 1 << 33)
    counts = (1, 2, 63, 64, 65, 4096, 4097, 1 << 20, 1 << 24)
    for B in (16, 4096, 65536, 1 << 20):
        for n in counts:
            prev = 0
            for src_len in sizes:
                s = L.lz4hip_streams_encode_scratch_bytes(n, src_len, B)
                assert s >= prev and s >= src_len + 8 * n, (B, n, src_len)
                prev = s
        for src_len in sizes:
            prev = 0
            for n in counts:
                s = L.lz4hip_streams_encode_scratch_bytes(n, src_len, B)
                assert s >= prev, (B, n, src_len)
                prev = s
    for n in counts:
        prev = 0
        for m in (0, 1, 2, 31, 32, 33, 4096, 1 << 20, 1 << 26):
            s = L.lz4hip_streams_decode_scratch_bytes(n, m)
            assert s >= prev and s >= 40 * m + 24 * n, (n, m)
            prev = s
    for m in (0, 1, 4096, 1 << 20):
        prev = 0
        for n in counts:
            s = L.lz4hip_streams_decode_scratch_bytes(n, m)
            assert s >= prev, (n, m)
            prev = s


def test_streams_info_layout():
    assert C.sizeof(_lib.StreamsInfo) == 56 and _lib.StreamsInfo.first_error.offset == 32 and _lib.StreamsInfo.error.offset == 48


def test_device_functions_reject_host_data():
    import torch
    offs = np.array([0, 3], np.int64)
    for fn in (st.compress_streams_device, st.decompress_streams_device):
        with pytest.raises(ArgumentException):
            fn(b"abc", offs)
        with pytest.raises(ArgumentException):
            fn(np.zeros(3, np.uint8), offs)
        with pytest.raises(ArgumentException):
            fn(torch.zeros(3, dtype=torch.uint8), torch.tensor([0, 3]))               # host tensors
        with pytest.raises(ArgumentException):
            fn(torch.zeros(3, dtype=torch.float32), torch.tensor([0, 3]))
    for fn in (st.compress_streams_host, st.decompress_streams_host):
        with pytest.raises(ArgumentException):
            fn(np.zeros(3, np.uint8), np.array([0, 3], np.int32))                     # wrong dtype
        with pytest.raises(ArgumentException):
            fn(np.zeros(3, np.float32), offs)
        with pytest.raises(ArgumentException):
            fn(np.zeros(3, np.uint8), np.zeros(0, np.int64))                          # offsets must hold n + 1 entries
        with pytest.raises(ArgumentException):
            fn(np.zeros((3, 1), np.uint8), offs)


# ---- GPU --------------------------------------------------------------------------------------------------------------------

def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def item_lengths(B, hc=False):
    k = {16: 200, 4096: 16, 65536: 4, 100003: 3, 1 << 20: 2}[B]
    if hc:
        k = {16: 64, 4096: 8, 65536: 2}[B]
    return [0, 1, B - 1, B, B + 1, k * B + B // 3 + 7]


def parity_items(oracle, B, hc):
    """Every kind at every length, several empty items in a row at the start, in the middle and at the end."""
    kinds = (1, 2, 3, "zeros", "real") if hc else KINDS
    empty = np.zeros(0, np.uint8)
    items = [empty, empty]
    for j, kind in enumerate(kinds):
        for size in item_lengths(B, hc):
            items.append(data_of(oracle, kind, size))
        if j == 1:
            items += [empty, empty, empty]
    return items + [empty, empty, empty]


def _check_encode_parity(oracle, B, hc):
    torch = _torch()
    items = parity_items(oracle, B, hc)
    data, offs = concat(items)
    packed, poff = st.compress_streams_device(_dev(torch, data), _dev(torch, offs), B, high_compression=hc)
    poff_h = poff.cpu().numpy()
    assert poff_h[0] == 0 and poff_h[-1] == packed.numel() and (np.diff(poff_h) >= 0).all()
    got = split(packed.cpu().numpy(), poff_h)
    for i, m in enumerate(items):
        assert got[i] == expected_stream(oracle, m, B, hc), (B, hc, i, m.size)
        alone = st.compress_stream_device(_dev(torch, m), B, hc).cpu().numpy().tobytes()
        assert got[i] == alone, (B, hc, i, m.size)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BLOCKS)
def test_encode_parity_fast(oracle, B):
    _check_encode_parity(oracle, B, False)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [16, 4096, 65536])
def test_encode_parity_hc(oracle, B):
    _check_encode_parity(oracle, B, True)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BLOCKS)
def test_round_trip_on_a_side_stream(oracle, B):
    torch = _torch()
    side = torch.cuda.Stream()
    for hc in (False, True):
        if hc and B > 65536:
            continue
        data, offs = concat(parity_items(oracle, B, hc))
        x, o = _dev(torch, data), _dev(torch, offs)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            back, boff = st.decompress_streams_device(*st.compress_streams_device(x, o, B, hc))
            ok = bool(torch.equal(back, x)) and bool(torch.equal(boff, o))
        assert ok, (B, hc)
    # empty batches and batches of empty items
    for items in ([], [b""], [b""] * 5):
        data, offs = concat(items)
        with torch.cuda.stream(side):
            packed, poff = st.compress_streams_device(_dev(torch, data), _dev(torch, offs), B)
            back, boff = st.decompress_streams_device(packed, poff)
        assert packed.numel() == 0 and back.numel() == 0 and poff.cpu().tolist() == boff.cpu().tolist() == [0] * (len(items) + 1)


def foreign_items(oracle):
    rng = np.random.default_rng(5)
    streams = []
    for s_i in range(6):
        chunks = []
        for i in range(4 + 9 * s_i):
            n = int(rng.integers(1, 20000)) if (i + s_i) % 7 else 0
            data = data_of(oracle, [2, 3, "random", "zeros"][i % 4], n)
            kind = (i + s_i) % 3
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
        streams.append(frame(chunks))
    a = data_of(oracle, 2, 5000)
    r, buf = oracle.compress_raw(a, 5000)
    # non-minimal varints (0x80 0x00 style) in every field
    streams.append(_nonminimal(1) + _nonminimal(5000) + _nonminimal(r) + buf[:r].tobytes() + b"\x80\x00" + _nonminimal(7) + b"1234567")
    streams.append(frame([(st.FLAG_COMPRESSED, 5000, buf[:r]), (4, 3, b"abc")]))                 # a passes bit on a raw chunk
    streams.append(b"")
    streams.append(frame([(0, 0, b""), (0, 0, b"")]))                                            # nothing but empty chunks
    streams += wide_flags_streams(oracle)                                                        # flags bits the reference drops
    return streams


@pytest.mark.gpu
def test_foreign_streams(oracle):
    torch = _torch()
    streams = foreign_items(oracle)
    want = [st.decompress_stream(s) for s in streams]
    packed, poff = concat(streams)
    out, ooff = st.decompress_streams_device(_dev(torch, packed), _dev(torch, poff))
    assert split(out.cpu().numpy(), ooff.cpu().numpy()) == want
    # one item of thousands of 1-byte raw chunks: the first table guess (len // 4096 + n + 16) is too small, the tables grow once
    tiny = frame([(0, 1, bytes([i & 0xFF])) for i in range(3000)])
    streams = streams[:3] + [tiny] + streams[3:]
    want = want[:3] + [bytes(i & 0xFF for i in range(3000))] + want[3:]
    packed, poff = concat(streams)
    p, o = _dev(torch, packed), _dev(torch, poff)
    n = len(streams)
    needed = sum(sum(1 for c in st.parse_chunks(s) if c[1] != 0) for s in streams)
    guess = packed.size // 4096 + n + 16
    assert needed > guess
    r = c_decode(torch, p, o, max_chunks=guess)
    assert r["index_info"].error == _lib.STREAM_TABLE_FULL and r["index_info"].chunks == needed and r["index_info"].first_error == -1
    out, ooff = st.decompress_streams_device(p, o)
    assert split(out.cpu().numpy(), ooff.cpu().numpy()) == want
    r = c_decode(torch, p, o, max_chunks=needed)                       # exactly enough
    assert r["info"].error == 0 and r["info"].chunks == needed and split(r["out"], r["dst_off"]) == want


GUARD = 64


def c_decode(torch, p, o, max_chunks=None, guard=False):
    """The two C calls on torch memory with guard bytes / entries behind everything the caller owns."""
    L = _lib.lib()
    n = o.numel() - 1
    if max_chunks is None:
        max_chunks = p.numel() // 4 + n + 16
    dst_off = torch.full((n + 1 + GUARD,), -0x5A5A5A5A, dtype=torch.int64, device="cuda")
    status = torch.full((n + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    err_off = torch.full((n + GUARD,), -0x5A5A5A5A, dtype=torch.int64, device="cuda")
    info_dev = torch.full((C.sizeof(_lib.StreamsInfo) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    sbytes = L.lz4hip_streams_decode_scratch_bytes(n, max_chunks)
    scratch = torch.full((sbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def read_info():
        torch.cuda.synchronize()
        return _lib.StreamsInfo.from_buffer_copy(info_dev.cpu().numpy()[:C.sizeof(_lib.StreamsInfo)].tobytes())

    index_args = (p.data_ptr(), p.numel(), o.data_ptr(), n, max_chunks, dst_off.data_ptr(), status.data_ptr(), err_off.data_ptr(), scratch.data_ptr())
    if guard and n:
        assert L.lz4hip_streams_index_device(*index_args, sbytes - 1, info_dev.data_ptr(), None) == _lib.E_ARGUMENT
    assert L.lz4hip_streams_index_device(*index_args, sbytes, info_dev.data_ptr(), None) == 0
    index_info = read_info()
    r = {"index_info": index_info, "index_status": status.cpu().numpy()[:n].copy(), "index_error_offset": err_off.cpu().numpy()[:n].copy()}
    if index_info.error == _lib.STREAM_TABLE_FULL:
        return r
    size = int(index_info.decoded_bytes)
    out = torch.full((size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def decode(dst_cap, scratch_bytes):
        return L.lz4hip_streams_decode_device(p.data_ptr(), p.numel(), o.data_ptr(), n, C.byref(index_info), max_chunks, scratch.data_ptr(), scratch_bytes,
                                              out.data_ptr(), dst_cap, dst_off.data_ptr(), status.data_ptr(), err_off.data_ptr(), info_dev.data_ptr(), None)

    if guard:                                                           # refused before anything runs
        if size:
            assert decode(size - 1, sbytes) == _lib.E_ARGUMENT
        if n:
            assert decode(size, sbytes - 1) == _lib.E_ARGUMENT
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xA5).all()
    assert decode(size, sbytes) == 0
    r["info"] = read_info()
    out_h, doff_h, st_h, eo_h = out.cpu().numpy(), dst_off.cpu().numpy(), status.cpu().numpy(), err_off.cpu().numpy()
    assert (out_h[size:] == 0xA5).all() and (doff_h[n + 1:] == -0x5A5A5A5A).all() and (st_h[n:] == 0x5A5A5A5A).all()
    assert (eo_h[n:] == -0x5A5A5A5A).all() and (scratch.cpu().numpy()[sbytes:] == 0xA5).all()
    assert (info_dev.cpu().numpy()[C.sizeof(_lib.StreamsInfo):] == 0xA5).all()
    r.update(out=out_h[:size], dst_off=doff_h[:n + 1], status=st_h[:n], error_offset=eo_h[:n])
    return r


def one_stream_outcome(s):
    """The merged one-stream path on this item alone -> (error, error_offset, the bytes before the error)."""
    L = _lib.lib()
    src = np.frombuffer(bytes(s), np.uint8).copy() if len(s) else np.zeros(1, np.uint8)
    info = _lib.StreamInfo()
    L.lz4hip_stream_decode_host(src.ctypes.data, len(s), None, 0, C.byref(info))
    out = np.zeros(int(info.decoded_bytes) + 1, np.uint8)
    rc = L.lz4hip_stream_decode_host(src.ctypes.data, len(s), out.ctypes.data, int(info.decoded_bytes), C.byref(info))
    assert rc == info.error
    return info.error, info.error_offset, out[:int(info.decoded_bytes)].tobytes()


def error_items(oracle):
    """Each failure test_stream_errors builds, at known indices among good items."""
    a = data_of(oracle, 2, 3000)
    r, buf = oracle.compress_raw(a, 3000)
    good = [(st.FLAG_COMPRESSED, 3000, buf[:r]), (0, 5, b"hello")]
    head = frame(good)
    corrupt = good + [_bad_block()] + good
    items = [
        head,                                                              # 0 good
        head + head,                                                       # 1 good
        head + b"\x80",                                                    # 2 a truncated varint
        frame(good * 3),                                                   # 3 good
        head + b"\x01\x85",                                                # 4 a truncated varint
        head + frame([(0, 10, b"0123456789")])[:-3],                       # 5 a truncated payload
        b"",                                                               # 6 good (empty)
        head + frame([(st.FLAG_COMPRESSED, 4, b"123456789")]),             # 7 clen > original
        head + frame([(st.FLAG_COMPRESSED | 4, 3000, buf[:r])]),           # 8 passes bits on a compressed chunk
        head + frame([(4, 3, b"abc")]),                                    # 9 good: a raw chunk may carry them
        frame(corrupt),                                                    # 10 a corrupt block alone
        frame(corrupt) + b"\x81",                                          # 11 a corrupt block before a truncated header
        head,                                                              # 12 good
    ]
    failing = {2: len(head), 4: len(head), 5: len(head), 7: len(head), 8: len(head), 10: _offsets(corrupt)[2], 11: _offsets(corrupt)[2]}
    return items, failing


@pytest.mark.gpu
def test_errors_per_item(oracle):
    torch = _torch()
    items, failing = error_items(oracle)
    packed, poff = concat(items)
    p, o = _dev(torch, packed), _dev(torch, poff)
    r = c_decode(torch, p, o)
    got = split(r["out"], r["dst_off"])
    for i, s in enumerate(items):
        err, err_off, data = one_stream_outcome(s)
        assert (int(r["status"][i]), int(r["error_offset"][i])) == (err, err_off), i
        assert (err != 0) == (i in failing) and (err == 0 or err_off == failing[i]), i
        if err != _lib.STREAM_CORRUPT_BLOCK:
            assert got[i] == data, i                                      # the good items intact, the bytes before a header error present
        else:                                                             # (the corrupt block's own range is unspecified)
            assert len(got[i]) == len(data)
            good_prefix = st.decompress_stream(s[:failing[i]])
            assert got[i][:len(good_prefix)] == data[:len(good_prefix)] == good_prefix, i
            tail = len(data) - len(good_prefix) - 100
            assert tail >= 0 and (tail == 0 or got[i][-tail:] == data[-tail:]), i
    assert r["info"].first_error == min(failing) and r["info"].error == r["status"][min(failing)] and r["info"].error_offset == failing[min(failing)]
    assert r["info"].items == len(items) and r["info"].decoded_bytes == r["dst_off"][-1]
    # the index alone reports the header errors; corrupt blocks are found by the decode
    assert r["index_status"][10] == 0 and r["index_status"][11] == _lib.STREAM_END_OF_STREAM and r["status"][11] == _lib.STREAM_CORRUPT_BLOCK
    # check=False: the statuses; check=True: what the host twin raises for the first failing item, then for every other one in front
    out, ooff, status = st.decompress_streams_device(p, o, check=False)
    assert status.cpu().tolist() == r["status"].tolist() and np.array_equal(ooff.cpu().numpy(), r["dst_off"])
    for first in sorted(failing):
        sub = [items[i] for i in range(len(items)) if i >= first or i not in failing]
        index = sub.index(items[first])
        with pytest.raises(Exception) as host:
            st.decompress_stream(items[first])
        # (item 11: the host twin parses every header before it decodes a block, a sequential LZ4Stream.Read meets the corrupt block first)
        want = ArgumentException if first == 11 else type(host.value)
        sp, so = concat(sub)
        with pytest.raises(Exception) as ei:
            st.decompress_streams_device(_dev(torch, sp), _dev(torch, so))
        assert type(ei.value) is want, (first, type(ei.value), want)
        assert ei.value.item_index == index and ei.value.error_offset == failing[first]


@pytest.mark.gpu
def test_bad_offsets(oracle):
    torch = _torch()
    items = [data_of(oracle, 2, 5000), data_of(oracle, 3, 70000), data_of(oracle, "real", 3000), data_of(oracle, 2, 100)]
    data, offs = concat(items)
    packed, poff = st.compress_streams_device(_dev(torch, data), _dev(torch, offs), 4096)
    ph, oh = packed.cpu().numpy(), poff.cpu().numpy()
    # items 1 and 5 are bad: offsets that decrease (behind an empty item, so that no two items overlap), an end past the buffer
    bad = np.array([oh[1], oh[1], oh[0], oh[1], oh[2], oh[3], ph.size + 1], np.int64)
    want_bad = [0, _lib.E_ARGUMENT, 0, 0, 0, _lib.E_ARGUMENT]
    r = c_decode(torch, packed, _dev(torch, bad))
    assert r["status"].tolist() == want_bad and r["info"].first_error == 1 and r["info"].error == _lib.E_ARGUMENT
    assert r["error_offset"].tolist() == [-1] * 6 and r["info"].error_offset == -1
    assert split(r["out"], r["dst_off"]) == [b"", b"", items[0].tobytes(), items[1].tobytes(), items[2].tobytes(), b""]
    with pytest.raises(ArgumentException) as ei:
        st.decompress_streams_device(packed, _dev(torch, bad))
    assert ei.value.item_index == 1
    # encode: a bad item takes no bytes and leaves the others as they are
    L = _lib.lib()
    src = _dev(torch, data)
    so = np.array([offs[1], offs[1], offs[0], offs[1], offs[2], offs[3], data.size + 1], np.int64)
    n = so.size - 1
    bound = L.lz4hip_streams_bound(n, data.size, 4096)
    dst = torch.full((bound + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.lz4hip_streams_encode_scratch_bytes(n, data.size, 4096), dtype=torch.uint8, device="cuda")
    sod = _dev(torch, so)
    assert L.lz4hip_streams_encode_device(src.data_ptr(), data.size, sod.data_ptr(), n, 4096, 0, dst.data_ptr(), bound, doff.data_ptr(),
                                          scratch.data_ptr(), scratch.numel(), None) == 0
    torch.cuda.synchronize()
    d = doff.cpu().numpy()
    got = split(dst.cpu().numpy(), d)
    assert got == [b"", b""] + [expected_stream(oracle, items[i], 4096, False) for i in range(3)] + [b""]
    assert (dst.cpu().numpy()[max(int(d[n]), 0):][-GUARD:] == 0xA5).all()
    with pytest.raises(ArgumentException):
        st.compress_streams_device(src, sod, 4096)
    with pytest.raises(ArgumentException):
        st.compress_streams_device(src, torch.zeros(0, dtype=torch.int64, device="cuda"))        # offsets must hold n + 1 entries
    with pytest.raises(ArgumentException):
        st.decompress_streams_device(src, sod.to(torch.int32))


@pytest.mark.gpu
def test_guard_bytes_through_the_c_calls(oracle):
    torch = _torch()
    L = _lib.lib()
    for B, hc in ((16, False), (4096, True), (65536, False), (100003, False)):
        items = parity_items(oracle, B, hc)[:16]
        data, offs = concat(items)
        n = len(items)
        src, so = _dev(torch, data), _dev(torch, offs)
        bound = L.lz4hip_streams_bound(n, data.size, B)
        dst = torch.full((bound + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        doff = torch.full((n + 1 + GUARD,), -0x5A5A5A5A, dtype=torch.int64, device="cuda")
        sbytes = L.lz4hip_streams_encode_scratch_bytes(n, data.size, B)
        scratch = torch.full((sbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

        def encode(dst_cap, scratch_bytes):
            return L.lz4hip_streams_encode_device(src.data_ptr(), data.size, so.data_ptr(), n, B, 1 if hc else 0, dst.data_ptr(), dst_cap,
                                                  doff.data_ptr(), scratch.data_ptr(), scratch_bytes, None)

        # too small a destination or scratch is refused before anything runs
        assert encode(bound - 1, sbytes) == _lib.E_ARGUMENT and encode(bound, sbytes - 1) == _lib.E_ARGUMENT
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 0xA5).all() and (doff.cpu().numpy() == -0x5A5A5A5A).all()
        assert encode(bound, sbytes) == 0
        torch.cuda.synchronize()
        d = doff.cpu().numpy()
        host = dst.cpu().numpy()
        total = int(d[n])
        assert split(host, d[:n + 1]) == [expected_stream(oracle, m, B, hc) for m in items]
        assert (host[total:] == 0xA5).all() and (d[n + 1:] == -0x5A5A5A5A).all() and (scratch.cpu().numpy()[sbytes:] == 0xA5).all()
        r = c_decode(torch, dst[:total].clone(), doff[:n + 1].clone(), guard=True)
        assert split(r["out"], r["dst_off"]) == [m.tobytes() for m in items] and np.array_equal(r["dst_off"], offs)
        assert (r["status"] == 0).all() and (r["error_offset"] == -1).all() and r["info"].first_error == -1 and r["info"].error == 0


def _moved(before, after):
    return [a - b for a, b in zip(after, before)]


@pytest.mark.gpu
def test_it_really_is_one_batch():
    """20 000 one-chunk items cost the block codecs what ONE stream of 20 000 chunks costs them: the same launches, the same mappings."""
    torch = _torch()
    from lz4net_amd import batch
    n, size = 20000, 4096
    x = batch.synth(2, 41, 0, n, length=size).reshape(-1)
    assert x.numel() == n * size
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * size
    # the reference point: the merged one-stream path on a single stream of 20 000 chunks of 4 KiB
    c0 = _lib.dispatch_counts()
    one = st.compress_stream_device(x, size)
    c1 = _lib.dispatch_counts()
    back_one = st.decompress_stream_device(one)
    c2 = _lib.dispatch_counts()
    packed, poff = st.compress_streams_device(x, offs, 1 << 20)
    c3 = _lib.dispatch_counts()
    back, boff = st.decompress_streams_device(packed, poff)
    c4 = _lib.dispatch_counts()
    assert torch.equal(back_one, x) and torch.equal(back, x) and torch.equal(boff, offs)
    # a chunk of 4 KiB is framed alike under both block sizes, so the two outputs are the same bytes
    assert torch.equal(packed, one)
    for ref, got in ((_moved(c0, c1), _moved(c2, c3)), (_moved(c1, c2), _moved(c3, c4))):
        assert sum(ref) > 0
        for k in range(_lib.K_COUNT):
            assert got[k] <= ref[k], (k, ref, got)
            assert (got[k] > 0) == (ref[k] > 0), (k, ref, got)
    # both encoder and both decoder mappings: identical bytes
    m = 2048
    xs, os_ = x[:m * size], offs[:m + 1]
    want_packed, want_off = packed[:int(poff[m])], poff[:m + 1]
    for mapping in ("wave", "lane"):
        with ForcedMapping("LZ4HIP_ENCODER", mapping):
            p, o = st.compress_streams_device(xs, os_, 1 << 20)
            torch.cuda.synchronize()
        assert torch.equal(p, want_packed) and torch.equal(o, want_off), mapping
        with ForcedMapping("LZ4HIP_DECODER", mapping):
            b, bo = st.decompress_streams_device(want_packed.clone(), want_off.clone())
            torch.cuda.synchronize()
        assert torch.equal(b, xs) and torch.equal(bo, os_), mapping


@pytest.mark.gpu
def test_host_pair(oracle):
    torch = _torch()
    L = _lib.lib()
    for hc, B in ((False, 4096), (True, 65536), (False, 16), (False, 1 << 20)):
        items = parity_items(oracle, B if B < (1 << 20) else 65536, hc)[:20]
        data, offs = concat(items)
        n = len(items)
        bound = L.lz4hip_streams_bound(n, data.size, B)
        dst = np.full(bound + 64, 0xA5, np.uint8)
        doff = np.full(n + 1 + 8, -7, np.int64)
        assert L.lz4hip_streams_encode_host(data.ctypes.data, data.size, offs.ctypes.data, n, B, 1 if hc else 0, dst.ctypes.data, bound,
                                            doff.ctypes.data) == 0
        total = int(doff[n])
        assert split(dst, doff[:n + 1]) == [expected_stream(oracle, m, B, hc) for m in items]
        assert (dst[total:] == 0xA5).all() and (doff[n + 1:] == -7).all()
        assert L.lz4hip_streams_encode_host(data.ctypes.data, data.size, offs.ctypes.data, n, B, 0, dst.ctypes.data, bound - 1,
                                            doff.ctypes.data) == _lib.E_ARGUMENT
        comp, coff = dst[:total].copy(), doff[:n + 1].copy()
        # the Python twins agree with the device functions
        ph, oh = st.compress_streams_host(data, offs, B, hc)
        assert ph.tobytes() == comp.tobytes() and np.array_equal(oh, coff)
        pd, od = st.compress_streams_device(_dev(torch, data), _dev(torch, offs), B, hc)
        assert pd.cpu().numpy().tobytes() == comp.tobytes() and np.array_equal(od.cpu().numpy(), coff)
        # size query first, then the real call
        info = _lib.StreamsInfo()
        ooff, status, eoff = np.full(n + 1 + 8, -7, np.int64), np.full(n + 8, 77, np.int32), np.full(n + 8, -7, np.int64)
        rc = L.lz4hip_streams_decode_host(comp.ctypes.data, comp.size, coff.ctypes.data, n, None, 0, ooff.ctypes.data, status.ctypes.data,
                                          eoff.ctypes.data, C.byref(info))
        assert rc == _lib.E_ARGUMENT and info.decoded_bytes == data.size and info.error == 0 and np.array_equal(ooff[:n + 1], offs)
        out = np.full(data.size + 64, 0xA5, np.uint8)
        assert L.lz4hip_streams_decode_host(comp.ctypes.data, comp.size, coff.ctypes.data, n, out.ctypes.data, data.size, ooff.ctypes.data,
                                            status.ctypes.data, eoff.ctypes.data, C.byref(info)) == 0
        assert out[:data.size].tobytes() == data.tobytes() and (out[data.size:] == 0xA5).all()
        assert np.array_equal(ooff[:n + 1], offs) and (ooff[n + 1:] == -7).all() and (status[:n] == 0).all() and (status[n:] == 77).all()
        assert (eoff[:n] == -1).all() and (eoff[n:] == -7).all()
        assert info.error == 0 and info.first_error == -1 and info.error_offset == -1 and info.items == n and info.decoded_bytes == data.size
        back, boff = st.decompress_streams_host(comp, coff)
        assert back.tobytes() == data.tobytes() and np.array_equal(boff, offs)
    # an empty batch
    info = _lib.StreamsInfo()
    z = np.zeros(1, np.int64)
    o1 = np.full(1, -7, np.int64)
    assert L.lz4hip_streams_decode_host(None, 0, z.ctypes.data, 0, None, 0, o1.ctypes.data, None, None, C.byref(info)) == 0
    assert o1[0] == 0 and info.first_error == -1 and info.items == 0
    # errors through the host pair: the outcome code is returned and reported
    items, failing = error_items(oracle)
    packed, poff = concat(items)
    hd, hof, hst = st.decompress_streams_host(packed, poff, check=False)
    dd, dof, dst_ = st.decompress_streams_device(_dev(torch, packed), _dev(torch, poff), check=False)
    assert hst.tolist() == dst_.cpu().tolist() and np.array_equal(hof, dof.cpu().numpy())
    assert [i for i, s in enumerate(hst.tolist()) if s] == sorted(failing)
    good = [i for i in range(len(items)) if i not in failing]
    assert [split(hd, hof)[i] for i in good] == [st.decompress_stream(items[i]) for i in good]
    with pytest.raises(st.EndOfStreamException) as ei:
        st.decompress_streams_host(packed, poff)
    assert ei.value.item_index == 2 and ei.value.error_offset == failing[2]
    n = len(items)
    out = np.zeros(int(hof[n]) + 16, np.uint8)
    o, s, e, info = np.zeros(n + 1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int64), _lib.StreamsInfo()
    assert L.lz4hip_streams_decode_host(packed.ctypes.data, packed.size, poff.ctypes.data, n, out.ctypes.data, out.size, o.ctypes.data,
                                        s.ctypes.data, e.ctypes.data, C.byref(info)) == _lib.STREAM_END_OF_STREAM
    assert info.first_error == 2 and info.error_offset == failing[2] and np.array_equal(o, hof)
    assert [int(e[i]) for i in sorted(failing)] == [failing[i] for i in sorted(failing)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [65536, 1 << 20])
def test_scale_d2_round_trip(B):
    """16 384 items x 64 KiB of D2 (1 GiB), verified on the device."""
    torch = _torch()
    from lz4net_amd import batch
    n, size = 16384, 65536
    x2 = batch.synth(2, 78, 0, n)
    x = x2.reshape(-1)
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * size
    before = _lib.dispatch_counts()
    packed, poff = st.compress_streams_device(x, offs, B)
    back, boff = st.decompress_streams_device(packed, poff)
    after = _lib.dispatch_counts()
    assert torch.equal(boff, offs) and back.numel() == x.numel()
    assert batch.count_mismatches(x2, back.reshape(n, size), size) == 0
    assert after[_lib.K_DECODE_LANE] > before[_lib.K_DECODE_LANE]
    assert int(poff[n]) < x.numel()
