"""GPU: chosen items of a device arena decoded in ONE call (lz4hip_unwrap_spans_into_device, lz4hip_streams_decode_spans_into_device,
lz4hip_spans_select_device and their Python wrappers) and the chunk directory of one stream (lz4hip_stream_directory_device,
stream.stream_directory, stream.decompress_stream_range): a selection with repeats in descending order against the chosen items' source
bytes under both decoder mappings, identity with the consecutive calls byte for byte, a corrupt item between good ones, an output far
larger than 255 times the arena, and a directory's one-chunk spans against the whole stream's decode."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpu_helpers import FILL, GUARD, dev, guarded, host, i64, intact_from, mapping_ran, s0, synth_bytes
from lz4net_amd import _lib, stream as st, wrap
from lz4net_amd.codec import ArgumentException

pytestmark = pytest.mark.gpu

SPARE = 37
CORRUPT = [0x0F, 0xFF, 0xFF]                                             # no literal, a match 65 535 bytes back: before the output


def mixed_source(sizes, seed):
    """items of the given sizes back to back, item i from D2, D1 (incompressible) or D3 by turns -> (device bytes, offsets as a list)"""
    import torch
    offs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    total = int(offs[-1])
    data = torch.cat([synth_bytes(2, total, seed), synth_bytes(1, total, seed + 1), synth_bytes(3, total, seed + 2)])
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    for i in range(len(sizes)):
        a, b = int(offs[i]), int(offs[i + 1])
        src[a:b] = data[(i % 3) * total + a:(i % 3) * total + b]
    return src, offs.tolist()


# ---- wrapped messages ----------------------------------------------------------------------------------------------------------------
N_MSGS = 48
MSG_SEL = [47, 47, 45, 41, 40, 40, 40, 38, 33, 32, 27, 25, 20, 13, 9, 8, 6, 2, 1, 0]     # 20 positions, repeats, descending


@functools.lru_cache(maxsize=None)
def wrap_arena():
    """48 wrapped messages: lengths 0, 1, 8, 100 raw, 4 KiB D2, 64 KiB D3, 70 000 D2, cycled -> (packed, offsets, plain bytes, plain offsets)"""
    import torch
    kinds = [(0, 2), (1, 2), (8, 2), (100, 1), (4096, 2), (65536, 3), (70000, 2)]
    sizes = [kinds[i % 7][0] for i in range(N_MSGS)]
    offs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    src = torch.cat([synth_bytes(kinds[i % 7][1], sizes[i], 60 + i) for i in range(N_MSGS) if sizes[i]])
    packed, poff = wrap.wrap_device(src, i64(offs))
    heads = [np.frombuffer(host(packed[int(poff[i]):int(poff[i]) + 8]), np.int32) for i in range(N_MSGS)]
    assert all(heads[i][1] == heads[i][0] for i in range(N_MSGS) if i % 7 == 3)         # the 100-byte messages are stored raw
    assert all(heads[i][1] < heads[i][0] for i in range(N_MSGS) if i % 7 >= 4)          # the large ones are compressed
    return packed, poff, host(src), offs.tolist()


def unwrap_spans(packed, begin, end, dst_cap):
    """the span call, into dst_cap bytes between guard bytes -> ((info, dst_off, status) as bytes, written, the whole guarded buffer)"""
    import torch
    L = _lib.lib()
    m = begin.numel()
    out_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(m, dtype=torch.int32, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device="cuda")
    written = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.lz4hip_unwrap_into_scratch_bytes(m), dtype=torch.uint8, device="cuda")
    buf = guarded(dst_cap)
    assert L.lz4hip_unwrap_spans_into_device(packed.data_ptr(), packed.numel(), begin.data_ptr(), end.data_ptr(), m, scratch.data_ptr(), scratch.numel(),
                                             buf.data_ptr() + GUARD, dst_cap, out_off.data_ptr(), status.data_ptr(), info_dev.data_ptr(),
                                             written.data_ptr(), s0()) == 0
    return (host(info_dev), host(out_off), host(status)), int(written.item()), host(buf)


def unwrap_consecutive(packed, poff, dst_cap):
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
def test_unwrap_selection_and_identity(mapping):
    packed, poff, plain, offs = wrap_arena()
    begin, end = wrap.select_spans(poff, i64(MSG_SEL))
    p_off = poff.tolist()
    assert begin.tolist() == [p_off[i] for i in MSG_SEL] and end.tolist() == [p_off[i + 1] for i in MSG_SEL]
    want = b"".join(plain[offs[i]:offs[i + 1]] for i in MSG_SEL)
    want_off = np.concatenate(([0], np.cumsum([offs[i + 1] - offs[i] for i in MSG_SEL]))).tolist()
    with mapping_ran(mapping):
        got, written, raw = unwrap_spans(packed, begin, end, len(want) + 4096)
        info = _lib.UnwrapInfo.from_buffer_copy(got[0])
        assert (info.messages, info.decoded_bytes, info.first_error, info.error) == (len(MSG_SEL), len(want), -1, _lib.WRAP_OK)
        assert info.compressed == sum(1 for i in MSG_SEL if i % 7 >= 4)
        assert np.frombuffer(got[1], np.int64).tolist() == want_off and not np.frombuffer(got[2], np.int32).any() and written == len(MSG_SEL)
        assert raw[GUARD:GUARD + len(want)] == want and intact_from(raw, len(want), len(want) + 4096)
        # clipped in call order: a prefix of the selection
        cap = want_off[7] + 5
        got, written, raw = unwrap_spans(packed, begin, end, cap)
        assert written == 7 and raw[GUARD:GUARD + want_off[7]] == want[:want_off[7]] and intact_from(raw, want_off[7], cap)
        # the arena's own offsets as spans: the consecutive call, byte for byte
        for cap in (len(plain) + 4096, offs[30] + 1, 0):
            assert unwrap_spans(packed, poff[:-1].contiguous(), poff[1:].contiguous(), cap) == unwrap_consecutive(packed, poff, cap), cap
    assert unwrap_consecutive(packed, poff, len(plain))[2][GUARD:GUARD + len(plain)] == plain


def test_unwrap_bad_selection_and_wrappers():
    import torch
    packed, poff, plain, offs = wrap_arena()
    sel = [5, -1, N_MSGS, 4]
    begin, end = wrap.select_spans(poff, i64(sel))
    assert begin.tolist()[1:3] == [-1, -1] and end.tolist()[1:3] == [-1, -1]
    size = offs[6] - offs[5] + offs[5] - offs[4]
    out = torch.full((size + 9,), FILL, dtype=torch.uint8, device="cuda")
    out_off, status, info, written = wrap.unwrap_spans_into(packed, begin, end, out)
    assert status.tolist() == [0, _lib.E_ARGUMENT, _lib.E_ARGUMENT, 0] and out_off.tolist() == [0, 65536, 65536, 65536, size]
    assert host(out[:size]) == plain[offs[5]:offs[6]] + plain[offs[4]:offs[5]] and host(out[size:]) == bytes([FILL]) * 9
    with pytest.raises(ArgumentException) as e:
        wrap.check_unwrap_into(info, written)
    assert e.value.message_index == 1
    begin, end = wrap.select_spans(poff, i64([4, 5]))
    res = wrap.unwrap_spans_into(packed, begin, end, out)
    assert wrap.check_unwrap_into(res[2], res[3]).messages == 2
    res = wrap.unwrap_spans_into(packed, begin, end, out[:4096 + 7])
    with pytest.raises(ArgumentException, match="too small"):
        wrap.check_unwrap_into(res[2], res[3])
    with pytest.raises(ArgumentException):
        wrap.unwrap_spans_into(packed, begin, end[:1], out)


def test_unwrap_output_not_bounded_by_the_arena():
    """one raw message of 100 incompressible bytes chosen 4 096 times: 409 600 bytes out of a 108-byte arena"""
    import torch
    src = synth_bytes(1, 100, 7)
    packed, poff = wrap.wrap_device(src, i64([0, 100]))
    assert packed.numel() == 108
    times = 4096
    begin, end = torch.zeros(times, dtype=torch.int64, device="cuda"), torch.full((times,), 108, dtype=torch.int64, device="cuda")
    got, written, raw = unwrap_spans(packed, begin, end, 100 * times)
    info = _lib.UnwrapInfo.from_buffer_copy(got[0])
    assert (info.messages, info.compressed, info.decoded_bytes, info.first_error, written) == (times, 0, 100 * times, -1, times)
    assert raw[GUARD:GUARD + 100 * times] == host(src) * times and intact_from(raw, 100 * times, 100 * times)


# ---- batches of streams ----------------------------------------------------------------------------------------------------------
N_ITEMS, BLOCK = 24, 4096
HURT_ITEM = 12
ITEM_SEL = [23, 21, 21, 18, 14, 13, 12, 12, 11, 8, 5, 0]                    # 12 positions, repeats, descending, the corrupt item between good ones


@functools.lru_cache(maxsize=None)
def streams_arena():
    """24 items of 0 .. 40 000 bytes at block size 4096, raw and compressed chunks; item HURT_ITEM's first block made corrupt in the
    second arena -> (packed, hurt packed, offsets, plain bytes, plain offsets)"""
    import torch
    sizes = [(0, 1, 4096, 5000, 12288, 40000, 300, 20000)[(i + i // 8) % 8] for i in range(N_ITEMS)]
    src, offs = mixed_source(sizes, 71)
    packed, poff = st.compress_streams_device(src, i64(offs), BLOCK)
    p_off = poff.tolist()
    c = st.parse_chunks(host(packed[p_off[HURT_ITEM]:p_off[HURT_ITEM + 1]]))[0]
    assert c[0] and offs[HURT_ITEM + 1] - offs[HURT_ITEM] > BLOCK
    hurt = packed.clone()
    hurt[p_off[HURT_ITEM] + c[2]:p_off[HURT_ITEM] + c[2] + 3] = torch.tensor(CORRUPT, dtype=torch.uint8, device="cuda")
    return packed, hurt, poff, host(src), offs


def chunks_of(offs, sel):
    return sum(-(-(offs[i + 1] - offs[i]) // BLOCK) for i in sel)


def streams_spans(packed, begin, end, max_chunks, dst_cap):
    import torch
    L = _lib.lib()
    m = begin.numel()
    out_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(m, dtype=torch.int32, device="cuda")
    err_off = torch.empty(m, dtype=torch.int64, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device="cuda")
    written = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.lz4hip_streams_decode_into_scratch_bytes(m, max_chunks), dtype=torch.uint8, device="cuda")
    buf = guarded(dst_cap)
    assert L.lz4hip_streams_decode_spans_into_device(packed.data_ptr(), packed.numel(), begin.data_ptr(), end.data_ptr(), m, max_chunks,
                                                     scratch.data_ptr(), scratch.numel(), buf.data_ptr() + GUARD, dst_cap, out_off.data_ptr(),
                                                     status.data_ptr(), err_off.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s0()) == 0
    return (host(info_dev), host(out_off), host(status), host(err_off)), int(written.item()), host(buf)


def streams_consecutive(packed, poff, max_chunks, dst_cap):
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
def test_streams_selection_and_identity(mapping):
    packed, hurt, poff, plain, offs = streams_arena()
    begin, end = wrap.select_spans(poff, i64(ITEM_SEL))
    want = b"".join(plain[offs[i]:offs[i + 1]] for i in ITEM_SEL)
    want_off = np.concatenate(([0], np.cumsum([offs[i + 1] - offs[i] for i in ITEM_SEL]))).tolist()
    need = chunks_of(offs, ITEM_SEL)
    all_chunks = chunks_of(offs, range(N_ITEMS))
    with mapping_ran(mapping):
        for mc in (need, need + SPARE):
            got, written, raw = streams_spans(packed, begin, end, mc, len(want) + 4096)
            info = _lib.StreamsInfo.from_buffer_copy(got[0])
            assert (info.items, info.chunks, info.decoded_bytes, info.first_error, info.error) == (len(ITEM_SEL), need, len(want), -1, _lib.STREAM_OK)
            assert np.frombuffer(got[1], np.int64).tolist() == want_off and not np.frombuffer(got[2], np.int32).any() and written == len(ITEM_SEL)
            assert (np.frombuffer(got[3], np.int64) == -1).all()
            assert raw[GUARD:GUARD + len(want)] == want and intact_from(raw, len(want), len(want) + 4096), mc
        # repeats count: a table one row short of the selection's chunks is full
        got, written, raw = streams_spans(packed, begin, end, need - 1, len(want))
        info = _lib.StreamsInfo.from_buffer_copy(got[0])
        assert (info.error, info.chunks, written) == (_lib.STREAM_TABLE_FULL, need, 0) and intact_from(raw, 0, len(want))
        # the corrupt item, chosen twice, does not disturb its neighbours
        got, written, raw = streams_spans(hurt, begin, end, need + SPARE, len(want))
        info = _lib.StreamsInfo.from_buffer_copy(got[0])
        bad = [j for j, i in enumerate(ITEM_SEL) if i == HURT_ITEM]
        assert (info.first_error, info.error, info.error_offset, written) == (bad[0], _lib.STREAM_CORRUPT_BLOCK, 0, len(ITEM_SEL))
        status = np.frombuffer(got[2], np.int32)
        assert [j for j in range(len(ITEM_SEL)) if status[j] != 0] == bad and (status[bad] == _lib.STREAM_CORRUPT_BLOCK).all()
        for j in range(len(ITEM_SEL)):
            if j not in bad:
                assert raw[GUARD + want_off[j]:GUARD + want_off[j + 1]] == want[want_off[j]:want_off[j + 1]], j
        assert intact_from(raw, len(want), len(want))
        # the arena's own offsets as spans: the consecutive call, byte for byte -- clean, clipped, sized only, and with the corrupt item
        b_all, e_all = poff[:-1].contiguous(), poff[1:].contiguous()
        for cap in (len(plain) + 4096, offs[15] + 1, 0):
            assert streams_spans(packed, b_all, e_all, all_chunks + SPARE, cap) == streams_consecutive(packed, poff, all_chunks + SPARE, cap), cap
        a, b = streams_spans(hurt, b_all, e_all, all_chunks, len(plain)), streams_consecutive(hurt, poff, all_chunks, len(plain))
        lo, hi = GUARD + offs[HURT_ITEM], GUARD + offs[HURT_ITEM + 1]      # (a corrupt block's own output is unspecified)
        assert a[:2] == b[:2] and a[2][:lo] == b[2][:lo] and a[2][hi:] == b[2][hi:]
    assert streams_consecutive(packed, poff, all_chunks, len(plain))[2][GUARD:GUARD + len(plain)] == plain


# ---- the chunk directory of one stream, and ranges of it ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_input():
    """about 40 chunks with block sizes 256 .. 4096, raw (D1) and compressed (D2, D3), with empty chunks between the parts
    -> (stream bytes, plain bytes, header offsets and output offsets of the non-empty chunks with their closing entries)"""
    import torch
    parts, plain = [], []
    for k, B in enumerate((256, 1000, 4096, 512)):
        data = torch.cat([synth_bytes(2, 4 * B + 17, 10 + k), synth_bytes(1, 3 * B, 20 + k), synth_bytes(3, 3 * B, 30 + k)])
        parts += [host(st.compress_stream_device(data, B)), b"\x00\x00"]
        plain.append(host(data))
    stream = b"".join(parts)
    hdr_off, out_off, out = [], [], 0
    for c in st.parse_chunks(stream):
        hdr = c[2] - len(st.write_varint(1 if c[0] else 0)) - len(st.write_varint(c[1])) - (len(st.write_varint(c[3])) if c[0] else 0)
        if c[1]:
            hdr_off.append(hdr)
            out_off.append(out)
        out += c[1]
    assert 40 <= len(hdr_off) <= 50
    return stream, b"".join(plain), hdr_off + [len(stream)], out_off + [out]


def test_directory_and_ranges():
    import torch
    stream, plain, want_hdr, want_out = stream_input()
    t = dev(stream)
    count = len(want_hdr) - 1
    for mc in (None, 3, count):                                             # the default table, one that is grown once, the exact one
        hdr_off, out_off, out_host = st.stream_directory(t, max_chunks=mc, block_size=256)
        assert hdr_off.tolist() == want_hdr and out_off.tolist() == want_out and out_host.tolist() == want_out
    directory = (hdr_off, out_off, out_host)
    k = 20
    for start, length in ((want_out[k] + 3, 10), (want_out[k] - 5, want_out[k + 1] - want_out[k] + 9), (len(plain) - 1, 1), (0, len(plain)),
                          (want_out[k], 0)):
        got = st.decompress_stream_range(t, directory, start, length)
        assert got.numel() == length and host(got) == plain[start:start + length], (start, length)
    for start, length in ((-1, 2), (len(plain), 1), (5, len(plain))):
        with pytest.raises(ArgumentException):
            st.decompress_stream_range(t, directory, start, length)
    # the whole stream as one-chunk spans: what the one-stream decode gives
    whole = host(st.decompress_stream_device(t))
    assert whole == plain
    got, written, raw = streams_spans(t, hdr_off[:-1].contiguous(), hdr_off[1:].contiguous(), count, len(plain))
    info = _lib.StreamsInfo.from_buffer_copy(got[0])
    assert (info.items, info.chunks, info.first_error, written) == (count, count, -1, count)
    assert np.frombuffer(got[1], np.int64).tolist() == want_out and raw[GUARD:GUARD + len(plain)] == whole and intact_from(raw, len(plain), len(plain))
    # the raw call: the info is the index's, a table too small keeps its first entries and writes no closing one
    L = _lib.lib()
    hdr = torch.full((count + 2,), -77, dtype=torch.int64, device="cuda")
    out = torch.full((count + 2,), -77, dtype=torch.int64, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device="cuda")
    index_dev = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device="cuda")
    for mc in (count, count - 1):
        hdr.fill_(-77)
        out.fill_(-77)
        assert L.lz4hip_stream_directory_device(t.data_ptr(), t.numel(), mc, hdr.data_ptr(), out.data_ptr(), info_dev.data_ptr(), s0()) == 0
        scratch = torch.empty(L.lz4hip_stream_decode_scratch_bytes(mc), dtype=torch.uint8, device="cuda")
        assert L.lz4hip_stream_index_device(t.data_ptr(), t.numel(), mc, scratch.data_ptr(), scratch.numel(), index_dev.data_ptr(), s0()) == 0
        assert host(info_dev) == host(index_dev)
        keep = mc + 1 if mc == count else mc
        assert hdr.tolist() == want_hdr[:keep] + [-77] * (count + 2 - keep) and out.tolist() == want_out[:keep] + [-77] * (count + 2 - keep), mc
    assert _lib.StreamInfo.from_buffer_copy(host(info_dev)).error == _lib.STREAM_TABLE_FULL
    with pytest.raises(st.EndOfStreamException) as e:
        st.stream_directory(dev(stream + b"\x81"), block_size=256)
    assert e.value.error_offset == len(stream)
