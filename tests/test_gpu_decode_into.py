"""GPU: LZ4Stream buffers, batches of them and wrapped messages decoded in ONE device call into a buffer of any capacity
(lz4hip_stream_decode_into_device, lz4hip_streams_decode_into_device, lz4hip_unwrap_into_device and their Python wrappers): parity with
the two-call pair and with the source under both decoder mappings, clipping at dst_cap between guard bytes, a table too small, a corrupt
block, a header error, and tables with rows to spare so that empty rows reach the real decoders."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpu_helpers import GUARD, dev, guarded, host, i64, intact_from, mapping_ran, s0, synth_bytes
from lz4net_amd import _lib, stream as st, wrap
from lz4net_amd.codec import ArgumentException

pytestmark = pytest.mark.gpu

SPARE = 37
CORRUPT = [0x0F, 0xFF, 0xFF]                                             # no literal, a match 65 535 bytes back: before the output


def cap_values(spans, total):
    caps = {0, 1, total - 1, total, total + 4096}
    for a, b in spans:
        caps |= {a, b}
    return sorted(caps)


# ---- one stream ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_input():
    """about 40 chunks with block sizes 256 .. 4096, raw (D1) and compressed (D2, D3), with empty chunks between the parts
    -> (stream bytes, plain bytes, [(compressed, original, payload offset, payload length, header offset, output offset)])"""
    import torch
    parts, plain = [], []
    for k, B in enumerate((256, 1000, 4096, 512)):
        data = torch.cat([synth_bytes(2, 4 * B + 17, 10 + k), synth_bytes(1, 3 * B, 20 + k), synth_bytes(3, 3 * B, 30 + k)])
        parts += [host(st.compress_stream_device(data, B)), b"\x00\x00"]
        plain.append(host(data))
    stream = b"".join(parts)
    rows, out = [], 0
    for c in st.parse_chunks(stream):
        hdr = c[2] - len(st.write_varint(1 if c[0] else 0)) - len(st.write_varint(c[1])) - (len(st.write_varint(c[3])) if c[0] else 0)
        if c[1]:
            rows.append((c[0], c[1], c[2], c[3], hdr, out))
        out += c[1]
    assert 40 <= len(rows) <= 50 and sum(1 for r in rows if r[0]) >= 20 and sum(1 for r in rows if not r[0]) >= 8
    return stream, b"".join(plain), rows


def pair_stream(t, max_chunks):
    """lz4hip_stream_index_device, the read-back, lz4hip_stream_decode_device -> (index info, final info bytes, output bytes)"""
    import torch
    L = _lib.lib()
    info_dev = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(L.lz4hip_stream_decode_scratch_bytes(max_chunks), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_stream_index_device(t.data_ptr(), t.numel(), max_chunks, scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(), s0()) == 0
    first = _lib.StreamInfo.from_buffer_copy(host(info_dev))
    if first.error == _lib.STREAM_TABLE_FULL:
        return first, host(info_dev), b""
    out = torch.empty(int(first.decoded_bytes), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_stream_decode_device(t.data_ptr(), C.byref(first), max_chunks, scratch.data_ptr(), scratch.numel(), out.data_ptr(), out.numel(),
                                         info_dev.data_ptr(), s0()) == 0
    return first, host(info_dev), host(out)


def into_stream(t, max_chunks, dst_cap):
    """the one call, into dst_cap bytes between guard bytes -> (info bytes, written, the whole guarded buffer)"""
    import torch
    L = _lib.lib()
    info_dev = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device="cuda")
    written = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.lz4hip_stream_decode_into_scratch_bytes(max_chunks), dtype=torch.uint8, device="cuda")
    buf = guarded(dst_cap)
    assert L.lz4hip_stream_decode_into_device(t.data_ptr(), t.numel(), max_chunks, scratch.data_ptr(), scratch.numel(), buf.data_ptr() + GUARD, dst_cap,
                                              info_dev.data_ptr(), written.data_ptr(), s0()) == 0
    return host(info_dev), int(written.item()), host(buf)


@pytest.mark.parametrize("mapping", ["wave", "lane"])
def test_stream_parity(mapping):
    stream, plain, rows = stream_input()
    t = dev(stream)
    with mapping_ran(mapping):
        for mc in (len(rows), len(rows) + SPARE):
            first, pair_info, pair_out = pair_stream(t, mc)
            assert (first.error, first.chunks, first.decoded_bytes) == (_lib.STREAM_OK, len(rows), len(plain)) and pair_out == plain
            for cap in (len(plain), len(plain) + 4096):
                info, written, raw = into_stream(t, mc, cap)
                assert info == pair_info and written == len(plain), (mc, cap)
                assert raw[GUARD:GUARD + written] == plain and intact_from(raw, written, cap), (mc, cap)


def test_stream_clipping():
    stream, plain, rows = stream_input()
    t = dev(stream)
    ck, rk = [r for r in rows if r[0]][7], [r for r in rows if not r[0]][4]
    _, pair_info, _ = pair_stream(t, len(rows) + SPARE)
    for cap in cap_values([(r[5], r[5] + r[1]) for r in (ck, rk)], len(plain)):
        info, written, raw = into_stream(t, len(rows) + SPARE, cap)
        want = max([r[5] + r[1] for r in rows if r[5] + r[1] <= cap], default=0)
        assert written == want and info == pair_info, (cap, written, want)          # the counts and decoded_bytes are complete
        assert raw[GUARD:GUARD + written] == plain[:written] and intact_from(raw, written, cap), cap


def test_stream_table_full_and_errors():
    stream, plain, rows = stream_input()
    t = dev(stream)
    first, pair_info, _ = pair_stream(t, len(rows) - 1)
    assert (first.error, first.chunks) == (_lib.STREAM_TABLE_FULL, len(rows))
    info, written, raw = into_stream(t, len(rows) - 1, len(plain))
    assert info == pair_info and written == 0 and intact_from(raw, 0, len(plain))
    # a corrupt block: the host path rejects the same chunk
    victim = [r for r in rows if r[0]][5]
    bad = bytearray(stream)
    bad[victim[2]:victim[2] + 3] = bytes(CORRUPT)
    with pytest.raises(ArgumentException, match="corrupted"):
        st.decompress_stream(bytes(bad))
    for tail in (b"", b"\x81"):                                             # ... alone, and in front of a header error
        tb = dev(bytes(bad) + tail)
        first, pair_info, pair_out = pair_stream(tb, len(rows) + SPARE)
        final = _lib.StreamInfo.from_buffer_copy(pair_info)
        assert (final.error, final.error_offset) == (_lib.STREAM_CORRUPT_BLOCK, victim[4])
        info, written, raw = into_stream(tb, len(rows) + SPARE, len(plain) + 100)
        assert info == pair_info and written == len(plain)
        good = plain[:victim[5]], plain[victim[5] + victim[1]:]
        assert raw[GUARD:GUARD + victim[5]] == good[0] and raw[GUARD + victim[5] + victim[1]:GUARD + written] == good[1]
        assert intact_from(raw, written, len(plain) + 100)
        # clipped in front of the corrupt chunk, the block is not decoded: the index's outcome
        info, written, raw = into_stream(tb, len(rows) + SPARE, victim[5] + victim[1] - 1)
        h = _lib.StreamInfo.from_buffer_copy(info)
        assert written == victim[5] and (h.error, h.error_offset) == (first.error, first.error_offset) and h.decoded_bytes == len(plain)
    # a header error alone
    tb = dev(stream + b"\x81")
    first, pair_info, pair_out = pair_stream(tb, len(rows) + SPARE)
    assert (first.error, first.error_offset) == (_lib.STREAM_END_OF_STREAM, len(stream))
    info, written, raw = into_stream(tb, len(rows) + SPARE, len(plain))
    assert info == pair_info and written == len(plain) and raw[GUARD:GUARD + written] == plain == pair_out


# ---- a batch of streams ----------------------------------------------------------------------------------------------------------
N_ITEMS = 300


@functools.lru_cache(maxsize=None)
def streams_input():
    """300 items of 0 .. 3 chunks of 1 KiB, raw and compressed -> (packed tensor, its offsets, plain bytes, plain offsets as a list)"""
    import torch
    B = 1024
    sizes = [(0, 1, 700, 1024, 1025, 2500, 3072, 100)[(i + i // 8) % 8] for i in range(N_ITEMS)]
    offs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    total = int(offs[-1])
    data = torch.cat([synth_bytes(2, total, 41), synth_bytes(1, total, 42), synth_bytes(3, total, 43)])
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    for i in range(N_ITEMS):                                                # item i from D2, D1 or D3 by turns
        a, b = int(offs[i]), int(offs[i + 1])
        src[a:b] = data[(i % 3) * total + a:(i % 3) * total + b]
    packed, poff = st.compress_streams_device(src, i64(offs), B)
    return packed, poff, host(src), offs.tolist()


def pair_streams(packed, poff, max_chunks):
    import torch
    L = _lib.lib()
    n = poff.numel() - 1
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    err_off = torch.empty(n, dtype=torch.int64, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(L.lz4hip_streams_decode_scratch_bytes(n, max_chunks), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_streams_index_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, max_chunks, out_off.data_ptr(), status.data_ptr(),
                                         err_off.data_ptr(), scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(), s0()) == 0
    first = _lib.StreamsInfo.from_buffer_copy(host(info_dev))
    index = (host(info_dev), host(out_off), host(status), host(err_off))
    if first.error == _lib.STREAM_TABLE_FULL:
        return first, index, index, b""
    out = torch.empty(int(first.decoded_bytes), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_streams_decode_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, C.byref(first), max_chunks, scratch.data_ptr(),
                                          scratch.numel(), out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(), err_off.data_ptr(),
                                          info_dev.data_ptr(), s0()) == 0
    return first, index, (host(info_dev), host(out_off), host(status), host(err_off)), host(out)


def into_streams(packed, poff, max_chunks, dst_cap):
    import torch
    L = _lib.lib()
    n = poff.numel() - 1
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    err_off = torch.empty(n, dtype=torch.int64, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device="cuda")
    written = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.lz4hip_streams_decode_into_scratch_bytes(n, max_chunks), dtype=torch.uint8, device="cuda")
    buf = guarded(dst_cap)
    assert L.lz4hip_streams_decode_into_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, max_chunks, scratch.data_ptr(), scratch.numel(),
                                               buf.data_ptr() + GUARD, dst_cap, out_off.data_ptr(), status.data_ptr(), err_off.data_ptr(),
                                               info_dev.data_ptr(), written.data_ptr(), s0()) == 0
    return (host(info_dev), host(out_off), host(status), host(err_off)), int(written.item()), host(buf)


@pytest.mark.parametrize("mapping", ["wave", "lane"])
def test_streams_parity(mapping):
    packed, poff, plain, offs = streams_input()
    chunks = sum(-(-(offs[i + 1] - offs[i]) // 1024) for i in range(N_ITEMS))
    with mapping_ran(mapping):
        for mc in (chunks, chunks + SPARE):
            first, _, pair, pair_out = pair_streams(packed, poff, mc)
            assert (first.error, first.chunks, first.decoded_bytes) == (_lib.STREAM_OK, chunks, len(plain)) and pair_out == plain
            assert np.frombuffer(pair[1], np.int64).tolist() == offs
            got, written, raw = into_streams(packed, poff, mc, len(plain) + 4096)
            assert got == pair and written == N_ITEMS, mc
            assert raw[GUARD:GUARD + len(plain)] == plain and intact_from(raw, len(plain), len(plain) + 4096), mc


def cut_item(packed, poff, k):
    """the batch with the last byte of item k's stream taken out"""
    import torch
    end = int(poff[k + 1].item())
    shift = torch.zeros_like(poff)
    shift[k + 1:] = 1
    return torch.cat([packed[:end - 1], packed[end:]]), poff - shift


def test_streams_clipping_table_full_and_errors():
    import torch
    packed, poff, plain, offs = streams_input()
    chunks = sum(-(-(offs[i + 1] - offs[i]) // 1024) for i in range(N_ITEMS))
    mc = chunks + SPARE
    _, _, pair, _ = pair_streams(packed, poff, mc)
    ci = next(i for i in range(140, N_ITEMS) if i % 3 == 0 and offs[i + 1] - offs[i] >= 1024)      # D2: compressed chunks
    ri = next(i for i in range(140, N_ITEMS) if i % 3 == 1 and offs[i + 1] - offs[i] >= 1024)      # D1: raw chunks
    for cap in cap_values([(offs[i], offs[i + 1]) for i in (ci, ri)], len(plain)):
        got, written, raw = into_streams(packed, poff, mc, cap)
        want = sum(1 for i in range(N_ITEMS) if offs[i + 1] <= cap)
        assert written == want and got == pair, (cap, written, want)        # offsets, statuses and the info are complete
        end = offs[written]
        assert raw[GUARD:GUARD + end] == plain[:end] and intact_from(raw, end, cap), cap
    first, index, _, _ = pair_streams(packed, poff, chunks - 1)
    assert (first.error, first.chunks) == (_lib.STREAM_TABLE_FULL, chunks)
    got, written, raw = into_streams(packed, poff, chunks - 1, len(plain))
    assert got == index and written == 0 and intact_from(raw, 0, len(plain))
    # item ci's first block corrupt, a later item cut short inside its last chunk: failing items between good ones
    p_off = poff.cpu().tolist()
    c = st.parse_chunks(host(packed[p_off[ci]:p_off[ci + 1]]))[0]
    assert c[0]
    hurt = packed.clone()
    hurt[p_off[ci] + c[2]:p_off[ci] + c[2] + 3] = torch.tensor(CORRUPT, dtype=torch.uint8, device="cuda")
    with pytest.raises(ArgumentException, match="corrupted"):
        st.decompress_stream(host(hurt[p_off[ci]:p_off[ci + 1]]))
    cut = next(i for i in range(200, N_ITEMS) if offs[i + 1] > offs[i])
    hurt, hurt_off = cut_item(hurt, poff, cut)
    first, _, pair, pair_out = pair_streams(hurt, hurt_off, mc)
    final = _lib.StreamsInfo.from_buffer_copy(pair[0])
    assert (final.first_error, final.error) == (ci, _lib.STREAM_CORRUPT_BLOCK)
    st_pair = np.frombuffer(pair[2], np.int32)
    assert st_pair[ci] == _lib.STREAM_CORRUPT_BLOCK and st_pair[cut] == _lib.STREAM_END_OF_STREAM and (np.delete(st_pair, [ci, cut]) == 0).all()
    total = int(final.decoded_bytes)
    got, written, raw = into_streams(hurt, hurt_off, mc, total + 64)
    assert got == pair and written == N_ITEMS
    o = np.frombuffer(pair[1], np.int64).tolist()
    assert raw[GUARD:GUARD + o[ci]] == pair_out[:o[ci]] == plain[:o[ci]] and raw[GUARD + o[ci + 1]:GUARD + total] == pair_out[o[ci + 1]:]
    assert intact_from(raw, total, total + 64)
    # clipped in front of item ci, its block is not decoded: the header statuses alone
    got, written, raw = into_streams(hurt, hurt_off, mc, o[ci + 1] - 1)
    st_got = np.frombuffer(got[2], np.int32)
    assert written == ci and st_got[ci] == _lib.STREAM_OK and st_got[cut] == _lib.STREAM_END_OF_STREAM
    assert _lib.StreamsInfo.from_buffer_copy(got[0]).first_error == cut


# ---- wrapped messages ----------------------------------------------------------------------------------------------------------------
N_MSGS = 300


@functools.lru_cache(maxsize=None)
def wrap_input():
    """300 messages of 0 .. 5000 bytes, stored raw (D1) and compressed (D2, D3)"""
    import torch
    sizes = [(0, 1, 700, 4096, 5000, 64, 333, 2048)[(i + i // 8) % 8] for i in range(N_MSGS)]
    offs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    total = int(offs[-1])
    data = torch.cat([synth_bytes(2, total, 51), synth_bytes(1, total, 52), synth_bytes(3, total, 53)])
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    for i in range(N_MSGS):
        a, b = int(offs[i]), int(offs[i + 1])
        src[a:b] = data[(i % 3) * total + a:(i % 3) * total + b]
    packed, poff = wrap.wrap_device(src, i64(offs))
    return packed, poff, host(src), offs.tolist()


def pair_unwrap(packed, poff):
    import torch
    L = _lib.lib()
    n = poff.numel() - 1
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(L.lz4hip_unwrap_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_unwrap_index_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, out_off.data_ptr(), status.data_ptr(), scratch.data_ptr(),
                                        scratch.numel(), info_dev.data_ptr(), s0()) == 0
    first = _lib.UnwrapInfo.from_buffer_copy(host(info_dev))
    out = torch.empty(int(first.decoded_bytes), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_unwrap_decode_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, C.byref(first), scratch.data_ptr(), scratch.numel(),
                                         out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(), info_dev.data_ptr(), s0()) == 0
    return first, (host(info_dev), host(out_off), host(status)), host(out)


def into_unwrap(packed, poff, dst_cap):
    import torch
    L = _lib.lib()
    n = poff.numel() - 1
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device="cuda")
    written = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.lz4hip_unwrap_into_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    buf = guarded(dst_cap)
    assert L.lz4hip_unwrap_into_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, scratch.data_ptr(), scratch.numel(), buf.data_ptr() + GUARD,
                                       dst_cap, out_off.data_ptr(), status.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s0()) == 0
    return (host(info_dev), host(out_off), host(status)), int(written.item()), host(buf)


@pytest.mark.parametrize("mapping", ["wave", "lane"])
def test_unwrap_parity(mapping):
    packed, poff, plain, offs = wrap_input()
    with mapping_ran(mapping):
        first, pair, pair_out = pair_unwrap(packed, poff)
        assert (first.error, first.messages, first.decoded_bytes) == (_lib.WRAP_OK, N_MSGS, len(plain)) and pair_out == plain
        assert 100 <= first.compressed < N_MSGS                               # rows past the count reach the decoder as empty blocks
        assert np.frombuffer(pair[1], np.int64).tolist() == offs
        for cap in (len(plain), len(plain) + 4096):
            got, written, raw = into_unwrap(packed, poff, cap)
            assert got == pair and written == N_MSGS, cap
            assert raw[GUARD:GUARD + len(plain)] == plain and intact_from(raw, len(plain), cap), cap


def test_unwrap_clipping_and_errors():
    import torch
    packed, poff, plain, offs = wrap_input()
    _, pair, _ = pair_unwrap(packed, poff)
    p_off = poff.cpu().tolist()
    heads = [np.frombuffer(host(packed[p_off[i]:p_off[i] + 8]), np.int32) for i in range(N_MSGS)]
    ci = next(i for i in range(140, N_MSGS) if heads[i][1] < heads[i][0])
    ri = next(i for i in range(140, N_MSGS) if heads[i][1] == heads[i][0] > 0)
    for cap in cap_values([(offs[i], offs[i + 1]) for i in (ci, ri)], len(plain)):
        got, written, raw = into_unwrap(packed, poff, cap)
        want = sum(1 for i in range(N_MSGS) if offs[i + 1] <= cap)
        assert written == want and got == pair, (cap, written, want)
        end = offs[written]
        assert raw[GUARD:GUARD + end] == plain[:end] and intact_from(raw, end, cap), cap
    # message ci's block corrupt, message 30 with a payload length past its end
    hurt = packed.clone()
    hurt[p_off[ci] + 8:p_off[ci] + 11] = torch.tensor(CORRUPT, dtype=torch.uint8, device="cuda")
    hurt[p_off[30] + 4:p_off[30] + 8] = torch.tensor([0xFF, 0xFF, 0xFF, 0x3F], dtype=torch.uint8, device="cuda")
    first, pair, pair_out = pair_unwrap(hurt, poff)
    final = _lib.UnwrapInfo.from_buffer_copy(pair[0])
    st_pair = np.frombuffer(pair[2], np.int32)
    assert (final.first_error, final.error) == (30, _lib.WRAP_CORRUPT_HEADER) and st_pair[ci] == _lib.WRAP_CORRUPT_BLOCK
    total = int(final.decoded_bytes)
    got, written, raw = into_unwrap(hurt, poff, total + 64)
    assert got == pair and written == N_MSGS and intact_from(raw, total, total + 64)
    o = np.frombuffer(pair[1], np.int64).tolist()
    assert raw[GUARD:GUARD + o[ci]] == pair_out[:o[ci]] and raw[GUARD + o[ci + 1]:GUARD + total] == pair_out[o[ci + 1]:]
    # clipped in front of message ci, its block is not decoded: the header statuses alone
    got, written, raw = into_unwrap(hurt, poff, o[ci + 1] - 1)
    st_got = np.frombuffer(got[2], np.int32)
    assert written == ci and st_got[ci] == _lib.WRAP_OK and st_got[30] == _lib.WRAP_CORRUPT_HEADER


# ---- the Python wrappers -----------------------------------------------------------------------------------------------------------
def test_python_wrappers():
    import torch
    stream, plain, rows = stream_input()
    t = dev(stream)
    out = torch.empty(len(plain) + 100, dtype=torch.uint8, device="cuda")
    info, written = st.decompress_stream_into(t, out, block_size=256)       # (the smallest block size of the stream sizes the table)
    h = st.check_stream_into(info, written)
    assert (h.chunks, h.decoded_bytes, int(written.item())) == (len(rows), len(plain), len(plain)) and host(out[:len(plain)]) == plain
    info, written = st.decompress_stream_into(t, out, max_chunks=3)
    with pytest.raises(_lib.Lz4HipError, match=str(len(rows))):
        st.check_stream_into(info, written)
    info, written = st.decompress_stream_into(t, out[:1000], max_chunks=len(rows))
    assert st.read_stream_info(info).decoded_bytes == len(plain)
    with pytest.raises(ArgumentException, match="too small"):
        st.check_stream_into(info, written)
    info, written = st.decompress_stream_into(dev(stream + b"\x81"), out, max_chunks=len(rows))
    with pytest.raises(st.EndOfStreamException) as e:
        st.check_stream_into(info, written)
    assert e.value.error_offset == len(stream)

    packed, poff, plain, offs = streams_input()
    out = torch.empty(len(plain), dtype=torch.uint8, device="cuda")
    out_off, status, err_off, info, written = st.decompress_streams_into(packed, poff, out, block_size=1024)
    h = st.check_streams_into(info, written)
    assert h.items == N_ITEMS and out_off.tolist() == offs and host(out) == plain and not bool(status.any()) and bool((err_off == -1).all())
    # (the default table follows `out`: one sized for the whole batch, so that a short `out` clips instead of filling the table)
    res = st.decompress_streams_into(packed, poff, out[:offs[100]], max_chunks=len(plain) // 1024 + N_ITEMS + 16)
    assert int(res[4].item()) == sum(1 for i in range(N_ITEMS) if offs[i + 1] <= offs[100])
    with pytest.raises(ArgumentException, match="too small"):
        st.check_streams_into(res[3], res[4])
    res = st.decompress_streams_into(packed, poff, out, max_chunks=5)
    with pytest.raises(_lib.Lz4HipError, match="chunk table"):
        st.check_streams_into(res[3], res[4])
    last = max(i for i in range(N_ITEMS) if offs[i + 1] > offs[i])
    cut = st.decompress_streams_into(*cut_item(packed, poff, last), out, block_size=1024)
    with pytest.raises(st.EndOfStreamException) as e:
        st.check_streams_into(cut[3], cut[4])
    assert e.value.item_index == last

    packed, poff, plain, offs = wrap_input()
    out = torch.empty(len(plain) + 7, dtype=torch.uint8, device="cuda")
    out_off, status, info, written = wrap.unwrap_into(packed, poff, out)
    h = wrap.check_unwrap_into(info, written)
    assert h.messages == N_MSGS and out_off.tolist() == offs and host(out[:len(plain)]) == plain and not bool(status.any())
    res = wrap.unwrap_into(packed, poff, out[:offs[77] + 1])
    assert wrap.read_unwrap_info(res[2]).decoded_bytes == len(plain)
    with pytest.raises(ArgumentException, match="too small"):
        wrap.check_unwrap_into(res[2], res[3])
    hurt = packed.clone()
    hurt[int(poff[30].item()) + 4:int(poff[30].item()) + 8] = torch.tensor([0xFF, 0xFF, 0xFF, 0x3F], dtype=torch.uint8, device="cuda")
    res = wrap.unwrap_into(hurt, poff, out)
    with pytest.raises(ArgumentException, match="corrupted") as e:
        wrap.check_unwrap_into(res[2], res[3])
    assert e.value.message_index == 30
