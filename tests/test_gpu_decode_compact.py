"""A block batch decoded into one packed buffer on the device without a size walk (lz4hip_decode_compact_device / _host,
batch.decode_compact) and the legacy frame decoded in one call on top of it (lz4hip_frame_decode_compact_device,
legacy_frame.decompress_frame_compact_device): parity with the existing path -- batch.decode, unknown size, into slot-strided rows of the
same blocks -- and with the source, rounds that take different decoder mappings, blocks that fail, clipping at dst_cap, the host-pointer
call and the automatic sizing of batch.decode_compact.  The blocks are encoded on the device from batch.synth.  The CPU twin -- the same
kernels and host code under the SIMT emulator -- is tests/test_simt_compact.py."""
import ctypes as C

import numpy as np
import pytest

from lz4net_amd import _lib, batch, legacy_frame as lf

pytestmark = pytest.mark.gpu

SEED, N = 20261018, 1000
LENGTHS = (1, 13, 4096, 65536)
SLOT = 65536
MAGIC = lf.MAGIC.to_bytes(4, "little")
_cache = {}


def blocks(dist):
    """N synthetic blocks of mixed lengths up to 64 KiB and what the device's fast encoder made of them: (rows, lengths, compressed
    rows, compressed lengths), once per distribution"""
    import torch
    if dist not in _cache:
        raw = batch.synth(dist, SEED, 0, N)
        lens = torch.tensor([LENGTHS[(i + i // 4) % 4] for i in range(N)], dtype=torch.int32, device="cuda")
        comp = torch.empty((N, batch.BOUND_STRIDE), dtype=torch.uint8, device="cuda")
        clen = batch.encode(raw, lens, comp, batch.BOUND, src_len_hint=65536)
        assert bool((clen > 0).all())
        _cache[dist] = (raw, lens, comp, clen)
    return _cache[dist]


def slot_decode(comp, clen, caps, slot=SLOT):
    """the existing path: batch.decode, unknown size, into slot-strided rows -> (results, the rows' produced bytes back to back)"""
    import torch
    n = comp.shape[0]
    rows = torch.zeros((n, slot + 64), dtype=torch.uint8, device="cuda")
    res = batch.decode(comp, clen, rows, caps, known_output_size=False)
    keep = torch.arange(slot + 64, device="cuda")[None, :] < res[:, None]
    return res, rows[keep]


def offsets_of(res):
    import torch
    return torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(res.clamp(min=0).to(torch.int64), 0)])


def flat(raw, lens):
    import torch
    return raw[torch.arange(raw.shape[1], device="cuda")[None, :] < lens[:, None]]


@pytest.mark.parametrize("mapping", ["wave", "lane"])
@pytest.mark.parametrize("dist", [2, 3])
def test_parity_with_the_slot_path_and_the_source(dist, mapping):
    import torch
    raw, lens, comp, clen = blocks(dist)
    if ("ref", dist) not in _cache:
        _cache["ref", dist] = slot_decode(comp, clen, SLOT)
    res, plain = _cache["ref", dist]
    assert torch.equal(res, lens) and torch.equal(plain, flat(raw, lens))
    knobs = dict(decoder="wave") if mapping == "wave" else dict(decoder="lane", decoder_groups=1)
    before = _lib.dispatch_counts()
    with _lib.tuning(**knobs):
        for k in (0, 64, 999):
            dst_view, offsets, lengths, results, h = batch.decode_compact(comp, clen, slot_bytes=SLOT, round_blocks=k)
            assert torch.equal(results, res) and torch.equal(lengths, res) and torch.equal(offsets, offsets_of(res))
            assert (h.blocks, h.decoded_bytes, h.written_blocks, h.first_failed, h.error, h.reserved) == (N, plain.numel(), N, -1, 0, 0)
            assert dst_view.numel() == plain.numel() and torch.equal(dst_view, plain)
    after = _lib.dispatch_counts()
    mine, other = (_lib.K_DECODE_WAVE, _lib.K_DECODE_LANE) if mapping == "wave" else (_lib.K_DECODE_LANE, _lib.K_DECODE_WAVE)
    assert after[mine] - before[mine] >= 1 + 16 + 2 and after[other] == before[other]        # one decode per round: 1, 16 and 2 rounds


def test_rounds_take_the_mapping_of_their_own_size():
    """20 480 blocks of 4 KiB in rounds of 16 384: the first round is large enough for the lane mapping, the second (4 096 blocks) is not
    and runs wavefront-mapped alone -- the dispatch rules see the round, not the batch"""
    import torch
    n, length = 20480, 4096
    raw = batch.synth(2, SEED, 0, n, length=length)
    comp = torch.empty((n, batch.compress_bound(length) + 15 & ~15), dtype=torch.uint8, device="cuda")
    clen = batch.encode(raw, length, comp, batch.compress_bound(length))
    before = _lib.dispatch_counts()
    dst_view, offsets, lengths, results, h = batch.decode_compact(comp, clen, slot_bytes=length, round_blocks=16384)
    after = _lib.dispatch_counts()
    assert after[_lib.K_DECODE_LANE] - before[_lib.K_DECODE_LANE] == 1, "the round of 16 384 blocks did not take the lane mapping"
    assert after[_lib.K_DECODE_WAVE] - before[_lib.K_DECODE_WAVE] == 2, "the round of 4 096 blocks did not run wavefront-mapped"
    assert (h.decoded_bytes, h.written_blocks, h.first_failed) == (n * length, n, -1) and bool((results == length).all())
    assert torch.equal(dst_view.view(n, length), raw)


@pytest.mark.parametrize("k", [0, 600])
def test_failed_blocks_take_no_bytes(k):
    """corrupted and over-limit blocks in both rounds of k = 600: the results are the batch decoder's, the neighbours are intact"""
    import torch
    raw, lens, comp, clen = blocks(2)
    comp = comp.clone()
    corrupt = [3, 599, 600, 999]                                       # 64 KiB blocks and short ones, on both sides of the round boundary
    for i in corrupt:
        comp[i, :3] = torch.tensor([0x0F, 0xFF, 0xFF], dtype=torch.uint8, device="cuda")      # no literal, a match 65 535 bytes back: before the output
    caps = torch.full((N,), SLOT + 5, dtype=torch.int32, device="cuda")         # (above the slot width: the slot width binds)
    short = [7, 11, 602, 998]                                          # blocks with one byte less room than they decode to
    for i in short:
        caps[i] = lens[i] - 1
    caps[20] = -4                                                      # no room at all
    res, plain = slot_decode(comp, clen, caps.clamp(min=0, max=SLOT))
    failed = torch.nonzero(res < 0).flatten().tolist()
    assert set(corrupt + short) <= set(failed) and len(failed) < 20
    dst = torch.full((plain.numel() + 64,), 0xA7, dtype=torch.uint8, device="cuda")
    offsets, lengths, results, info = batch.decode_compact_launch(comp, clen, None, k, dst, SLOT, dst_cap=plain.numel(), block_cap=caps)
    h = batch.read_compact_info(info)
    assert torch.equal(results, res) and torch.equal(lengths, res.clamp(min=0)) and torch.equal(offsets, offsets_of(res))
    assert (h.blocks, h.decoded_bytes, h.written_blocks, h.first_failed, h.error) == (N, plain.numel(), N, failed[0], int(res[failed[0]]))
    ok = res >= 0
    assert torch.equal(dst[:plain.numel()], flat(raw, torch.where(ok, lens, torch.zeros_like(lens)))), "a good block's bytes were disturbed"
    assert bool((dst[plain.numel():] == 0xA7).all())
    # through dst_cap_all: a slot of 4 096 bytes fails every 64 KiB block and keeps the rest
    res, plain = slot_decode(comp, clen, 4096, slot=4096)
    dst_view, offsets, lengths, results, h = batch.decode_compact(comp, clen, slot_bytes=4096, round_blocks=k)
    assert torch.equal(results, res) and torch.equal(dst_view, plain) and int((res < 0).sum()) >= N // 4
    assert h.first_failed == int(torch.nonzero(res < 0)[0]) and h.error == int(res[h.first_failed])


def test_dst_cap_clipping_and_size_query():
    import torch
    raw, lens, comp, clen = blocks(3)
    plain = flat(raw, lens)
    off = offsets_of(lens).cpu().numpy()
    total = int(off[N])
    # the size query: no dst at all
    offsets, lengths, results, info = batch.decode_compact_launch(comp, clen, None, 64, None, SLOT)
    h = batch.read_compact_info(info)
    assert (h.decoded_bytes, h.written_blocks, h.first_failed) == (total, 0, -1) and np.array_equal(offsets.cpu().numpy(), off)
    assert torch.equal(results, lens)
    for cap, written in ((total - 1, N - 1), (total, N), (int(off[500]) + 1, 500)):
        dst = torch.full((total + 64,), 0xA7, dtype=torch.uint8, device="cuda")
        offsets, lengths, results, info = batch.decode_compact_launch(comp, clen, None, 64, dst, SLOT, dst_cap=cap)
        h = batch.read_compact_info(info)
        assert (h.blocks, h.decoded_bytes, h.written_blocks, h.first_failed) == (N, total, written, -1)
        assert np.array_equal(offsets.cpu().numpy(), off) and torch.equal(results, lens)
        assert torch.equal(dst[:int(off[written])], plain[:int(off[written])])
        assert bool((dst[cap:] == 0xA7).all()), "a byte at or past dst_cap was written"


def test_host_call():
    n = 300
    L = _lib.lib()
    raw, lens, comp, clen = blocks(2)
    src, sl = comp[:n].cpu().numpy(), clen[:n].cpu().numpy().copy()
    want = lens[:n].cpu().numpy()
    plain = flat(raw[:n], lens[:n]).cpu().numpy()
    off = np.concatenate(([0], np.cumsum(want, dtype=np.int64)))
    sl[17] = -5                                                         # (the call's own result for that block, and no bytes)
    want = want.copy()
    want[17] = _lib.E_ARGUMENT
    keep = np.repeat(np.arange(n) != 17, np.maximum(lens[:n].cpu().numpy(), 0))
    plain = plain[keep]
    off = np.concatenate(([0], np.cumsum(np.maximum(want, 0), dtype=np.int64)))
    for k, cap in ((0, plain.size), (64, plain.size + 1000), (64, int(off[128]) + 1), (64, 0)):
        dst = np.full(cap + 64, 0xA7, np.uint8)
        dst_off = np.zeros(n + 1, np.int64)
        dlen, result = np.zeros(n, np.int32), np.zeros(n, np.int32)
        info = _lib.CompactInfo()
        b = _lib.Batch(src=src.ctypes.data, src_stride=src.strides[0], src_len=sl.ctypes.data, dst_cap_all=SLOT, result=result.ctypes.data, n_blocks=n)
        assert _lib.check(L.lz4hip_decode_compact_host(C.byref(b), k, dst.ctypes.data, cap, dst_off.ctypes.data, dlen.ctypes.data, C.byref(info))) == 0
        written = int(np.searchsorted(off, cap, side="right")) - 1
        assert (info.blocks, info.decoded_bytes, info.written_blocks, info.first_failed, info.error) == (n, plain.size, written, 17, _lib.E_ARGUMENT)
        assert np.array_equal(dst_off, off) and np.array_equal(dlen, np.maximum(want, 0)) and np.array_equal(result, want)
        assert np.array_equal(dst[:off[written]], plain[:off[written]]) and (dst[cap:] == 0xA7).all()
    # the arguments are checked before anything else
    assert L.lz4hip_decode_compact_host(None, 0, None, 0, dst_off.ctypes.data, None, None) == _lib.E_ARGUMENT
    assert L.lz4hip_decode_compact_host(C.byref(b), -1, dst.ctypes.data, cap, dst_off.ctypes.data, None, None) == _lib.E_ARGUMENT


def test_auto_sizing(monkeypatch):
    """dst=None: the first guess holds a batch that shrank to no less than a quarter in one call; a deliberately small guess is
    recovered from by the second call, into exactly decoded_bytes"""
    import torch
    calls = []
    launch = batch.decode_compact_launch
    monkeypatch.setattr(batch, "decode_compact_launch", lambda *a, **kw: (calls.append(1), launch(*a, **kw))[1])
    raw, lens, comp, clen = blocks(2)
    packed, poff, plen, _, _ = batch.encode_packed(raw, lens)
    plain = flat(raw, lens)
    assert packed.numel() < plain.numel() < 4 * packed.numel()
    dst_view, offsets, lengths, results, h = batch.decode_compact(packed, plen, poff[:-1], slot_bytes=SLOT, round_blocks=64)
    assert len(calls) == 1 and h.written_blocks == N and torch.equal(dst_view, plain)
    del calls[:]
    monkeypatch.setattr(batch, "COMPACT_GUESS", 1)                    # as many bytes as the compressed blocks: too few
    dst_view, offsets, lengths, results, h = batch.decode_compact(packed, plen, poff[:-1], slot_bytes=SLOT, round_blocks=64)
    assert len(calls) == 2 and h.written_blocks == N and dst_view.numel() == h.decoded_bytes == plain.numel()
    assert torch.equal(dst_view, plain) and torch.equal(results, lens) and torch.equal(offsets, offsets_of(lens))
    # with a dst given there is never a second call
    del calls[:]
    small = torch.empty(plain.numel() // 2, dtype=torch.uint8, device="cuda")
    dst_view, offsets, lengths, results, h = batch.decode_compact(packed, plen, poff[:-1], slot_bytes=SLOT, round_blocks=64, dst=small)
    assert len(calls) == 1 and 0 < h.written_blocks < N and h.decoded_bytes == plain.numel() and dst_view.numel() == small.numel()
    end = int(offsets[h.written_blocks])
    assert torch.equal(dst_view[:end], plain[:end])


# ---- the legacy frame in one call ---------------------------------------------------------------------------------------------------------
def frame_call(frame, chunk, max_chunks, k, dst_cap):
    """lz4hip_frame_decode_compact_device -> (info, output with 32 guard bytes after dst_cap)"""
    import torch
    L = _lib.lib()
    info_dev = torch.zeros(C.sizeof(_lib.FrameInfo), dtype=torch.uint8, device="cuda")
    need = _lib.check(L.lz4hip_frame_decode_compact_scratch_bytes(chunk, max_chunks, k))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((dst_cap + 32,), 0xA7, dtype=torch.uint8, device="cuda")
    assert L.lz4hip_frame_decode_compact_device(frame.data_ptr(), frame.numel(), chunk, max_chunks, k, scratch.data_ptr(), need, out.data_ptr(), dst_cap,
                                                info_dev.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    info = _lib.FrameInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    assert bool((out[dst_cap:] == 0xA7).all()), "a byte at or past dst_cap was written"
    return info, out[:dst_cap]


def info_tuple(i):
    return (i.chunks, i.decoded_bytes, i.good_bytes, i.error_offset, i.error)


@pytest.mark.parametrize("k", [0, 7])
def test_frames(k):
    import torch
    source = batch.synth(2, SEED + 1, 0, 48).reshape(-1)
    for chunk, n_bytes in ((65536, 39 * 65536 + 1000), (1 << 20, 3 << 20), (65536, 0)):
        data = source[:n_bytes]
        frame = lf.compress_frame_device(data, chunk_size=chunk)
        chunks = (n_bytes + chunk - 1) // chunk
        assert torch.equal(lf.decompress_frame_compact_device(frame, chunk_size=chunk, round_chunks=k), data)
        info, out = frame_call(frame, chunk, chunks + 5, k, n_bytes + 100)
        assert info_tuple(info) == (chunks, n_bytes, n_bytes, -1, _lib.FRAME_OK) and torch.equal(out[:n_bytes], data)
        info, out = frame_call(frame, chunk, chunks + 5, k, 0)          # the size query
        assert info_tuple(info) == (chunks, n_bytes, n_bytes, -1, _lib.FRAME_OK)
        both = torch.cat([frame, frame])                                 # an appended frame
        assert torch.equal(lf.decompress_frame_compact_device(both, chunk_size=chunk, round_chunks=k), torch.cat([data, data]))


@pytest.mark.parametrize("k", [0, 7])
def test_frame_with_a_corrupt_chunk_and_a_full_table(k):
    import torch
    chunk, n_chunks = 65536, 40
    data = batch.synth(2, SEED + 1, 0, n_chunks).reshape(-1)[:39 * 65536 + 1000]
    frame = lf.compress_frame_device(data, chunk_size=chunk)
    fields = [at - 4 for at, _ in lf.parse_frame(frame.cpu().numpy().tobytes())]
    bad = 20
    broken = frame.clone()
    broken[fields[bad] + 4:fields[bad] + 7] = torch.tensor([0x0F, 0xFF, 0xFF], dtype=torch.uint8, device="cuda")     # a match before the output
    info, out = frame_call(broken, chunk, n_chunks + 3, k, data.numel())
    total = data.numel() - chunk
    assert info_tuple(info) == (n_chunks, total, bad * chunk, fields[bad], _lib.FRAME_CORRUPT_BLOCK)
    assert torch.equal(out[:total], torch.cat([data[:bad * chunk], data[(bad + 1) * chunk:]])), "the neighbours do not pack around the bad chunk"
    with pytest.raises(lf.ArgumentException, match="Decoding Failed") as e:
        lf.decompress_frame_compact_device(broken, chunk_size=chunk, round_chunks=k)
    assert e.value.error_offset == fields[bad]
    # a table of fewer rows than the frame has chunks: the count needed comes back, and a table of that size decodes
    info, out = frame_call(frame, chunk, n_chunks - 1, k, data.numel())
    assert (info.error, info.chunks, info.error_offset) == (_lib.FRAME_TABLE_FULL, n_chunks, fields[n_chunks - 1])
    info, out = frame_call(frame, chunk, int(info.chunks), k, data.numel())
    assert info_tuple(info) == (n_chunks, data.numel(), data.numel(), -1, _lib.FRAME_OK) and torch.equal(out, data)
    # ... which is what the wrapper does for a frame read with a larger chunk_size than it was written with
    small = lf.compress_frame_device(data[:100000], chunk_size=1024)
    assert torch.equal(lf.decompress_frame_compact_device(small, chunk_size=65536, round_chunks=k), data[:100000])
