"""A block batch encoded into one packed buffer on the device (lz4hip_encode_packed_device / _host, batch.encode_packed): parity with
the existing path -- batch.encode into compressBound slots -- slice for slice and with the oracle on a sample, the round trip through
batch.decode_packed, clipping at dst_cap, the automatic sizing of batch.encode_packed, calls queued on a stream without
synchronisation, the host-pointer call and the argument checks.  The CPU twin -- the same kernels and host code under the SIMT
emulator -- is tests/test_simt_packed.py."""
import ctypes as C

import numpy as np
import pytest

from lz4net_amd import _lib, batch

pytestmark = pytest.mark.gpu

SEED, N_MAX = 20261018, 4097
LENGTHS = (1, 13, 4096, 65536)
_cache = {}


def rows(dist):
    """N_MAX synthetic 64 KiB blocks of a distribution, generated once"""
    if ("rows", dist) not in _cache:
        _cache["rows", dist] = batch.synth(dist, SEED, 0, N_MAX)
    return _cache["rows", dist]


def mixed_lengths(n):
    import torch
    if ("lens", n) not in _cache:
        _cache["lens", n] = torch.tensor([LENGTHS[(i + i // 4) % 4] for i in range(n)], dtype=torch.int32, device="cuda")
    return _cache["lens", n]


def reference(dist, n, hc):
    """the existing path on the first n blocks: batch.encode into BOUND_STRIDE slots -> (results, the slots' bytes back to back), once"""
    import torch
    key = ("ref", dist, n, hc)
    if key not in _cache:
        slots = torch.empty((n, batch.BOUND_STRIDE), dtype=torch.uint8, device="cuda")
        res = batch.encode(rows(dist)[:n], mixed_lengths(n), slots, batch.BOUND, hc=hc, src_len_hint=65536)
        keep = torch.arange(batch.BOUND_STRIDE, device="cuda")[None, :] < res[:, None]
        _cache[key] = (res, slots[keep])                                # (row-major: block 0's bytes, then block 1's, ...)
    return _cache[key]


def check_against(ref, dst_view, offsets, lengths, results, info, n):
    import torch
    res, packed = ref
    assert torch.equal(results, res) and torch.equal(lengths, res.clamp(min=0))
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(res.clamp(min=0).to(torch.int64), 0)])
    assert torch.equal(offsets, want_off)
    assert (info.blocks, info.packed_bytes, info.written_blocks, info.first_failed, info.error, info.reserved) == (n, packed.numel(), n, -1, 0, 0)
    assert dst_view.numel() == packed.numel() and torch.equal(dst_view, packed)


@pytest.mark.parametrize("hc", [False, True])
@pytest.mark.parametrize("dist", [0, 1, 2, 3])
def test_parity_with_the_slot_path(oracle, dist, hc):
    for n in ((3, 257) if hc else (3, 257, N_MAX)):
        ref = reference(dist, n, hc)
        for k in (0, 64, 1000):
            out = batch.encode_packed(rows(dist)[:n], mixed_lengths(n), hc=hc, round_blocks=k)
            check_against(ref, *out, n)
    # ... and the oracle's bytes on a sample of 16 blocks
    n = 257
    dst_view, offsets, lengths, results, info = batch.encode_packed(rows(dist)[:n], mixed_lengths(n), hc=hc, round_blocks=64)
    got, off, lens = dst_view.cpu().numpy(), offsets.cpu().numpy(), mixed_lengths(n).cpu().numpy()
    for i in range(0, n, 17)[:16]:
        raw = oracle.gen(dist, SEED, i, 1)[0, :lens[i]]
        ret, buf = oracle.compress_raw(raw, batch.BOUND, hc)
        assert ret == off[i + 1] - off[i] and bytes(got[off[i]:off[i + 1]]) == bytes(buf[:ret]), i


@pytest.mark.parametrize("dist,hc,k", [(0, False, 0), (1, False, 64), (2, False, 1000), (3, False, 64), (2, True, 64), (3, True, 0)])
def test_round_trip(dist, hc, k):
    import torch
    n = 257 if hc else N_MAX
    src, lens = rows(dist)[:n], mixed_lengths(n)
    dst_view, offsets, lengths, results, info = batch.encode_packed(src, lens, hc=hc, round_blocks=k)
    out, out_off, out_res = batch.decode_packed(dst_view, lengths, offsets[:-1])
    assert torch.equal(out_res, lens)
    # the decoded blocks lie back to back: lay them out in rows again and compare on the device
    back = torch.zeros_like(src)
    keep = torch.arange(src.shape[1], device="cuda")[None, :] < lens[:, None]
    back[keep] = out
    assert batch.count_mismatches(src, back, lens) == 0


def test_dst_cap_clipping_and_size_query():
    import torch
    n, k, dist = 257, 64, 2
    src, lens = rows(dist)[:n], mixed_lengths(n)
    res, packed = reference(dist, n, False)
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(res.to(torch.int64), 0)]).cpu().numpy()
    total = int(off[n])
    for cap, written in ((int(off[128]) - 1, 127), (int(off[128]), 128), (int(off[128]) + 1, 128), (total - 1, n - 1), (0, 0)):
        dst = torch.full((total + 64,), 0xA7, dtype=torch.uint8, device="cuda")
        offsets, lengths, results, info = batch.encode_packed_launch(src, lens, None, False, k, dst, batch.BOUND, dst_cap=cap)
        h = batch.read_packed_info(info)
        assert (h.blocks, h.packed_bytes, h.written_blocks, h.first_failed) == (n, total, written, -1)
        assert np.array_equal(offsets.cpu().numpy(), off) and torch.equal(results, res)
        assert torch.equal(dst[:int(off[written])], packed[:int(off[written])])
        assert bool((dst[cap:] == 0xA7).all()), "a byte at or past dst_cap was written"
    # the size query: no dst at all
    offsets, lengths, results, info = batch.encode_packed_launch(src, lens, None, False, k, None, batch.BOUND)
    h = batch.read_packed_info(info)
    assert (h.packed_bytes, h.written_blocks) == (total, 0) and np.array_equal(offsets.cpu().numpy(), off)
    # with a dst given, encode_packed never retries and returns what fit
    small = torch.empty(int(off[128]) + 5, dtype=torch.uint8, device="cuda")
    fit = int(np.searchsorted(off, small.numel(), side="right")) - 1   # the blocks that end at or before it (short ones after block 127 too)
    assert 128 <= fit < n
    dst_view, offsets, lengths, results, h = batch.encode_packed(src, lens, round_blocks=k, dst=small)
    assert h.written_blocks == fit and h.packed_bytes == total and dst_view.numel() == small.numel()
    assert torch.equal(dst_view[:int(off[fit])], packed[:int(off[fit])])


def test_per_block_limits():
    import torch
    n, dist = 257, 2
    src, lens = rows(dist)[:n], mixed_lengths(n)
    res, packed = reference(dist, n, False)
    caps = torch.full((n,), batch.BOUND, dtype=torch.int32, device="cuda")
    big = torch.nonzero(res > 1000).flatten().tolist()                 # the 64 KiB blocks
    short = [big[0], big[len(big) // 2], big[-1]]                      # ... three of them one byte short
    for i in short:
        caps[i] = res[i] - 1
    dst = torch.empty(packed.numel(), dtype=torch.uint8, device="cuda")
    offsets, lengths, results, info = batch.encode_packed_launch(src, lens, None, False, 64, dst, batch.BOUND, block_cap=caps)
    h = batch.read_packed_info(info)
    want = res.clone()
    want[short] = 0
    assert torch.equal(results, want) and (h.first_failed, h.error, h.written_blocks) == (short[0], 0, n)
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[short] = False
    ref_off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(res.to(torch.int64), 0)])
    mask = torch.repeat_interleave(keep, res.to(torch.int64))
    assert h.packed_bytes == int(mask.sum()) and torch.equal(dst[:h.packed_bytes], packed[mask]) and ref_off[n] > h.packed_bytes


def test_negative_length_never_reaches_the_encoder():
    """a negative src_len[i] is LZ4HIP_E_ARGUMENT for that block alone, on the real encoders, fast and HC, first row of a round included"""
    import torch
    n, dist = 257, 2
    src = rows(dist)[:n]
    for hc in (False, True):
        res, packed = reference(dist, n, hc)
        lens = mixed_lengths(n).clone()
        bad = [0, 64, 67, 256]                                         # rows 0 and 64 are the first of a round of 64
        lens[bad] = torch.tensor([-13, -1, -65536, -(2 ** 31)], dtype=torch.int32, device="cuda")
        want = res.clone()
        want[bad] = _lib.E_ARGUMENT
        keep = torch.ones(n, dtype=torch.bool, device="cuda")
        keep[bad] = False
        mask = torch.repeat_interleave(keep, res.to(torch.int64))
        for k in (0, 64):
            dst = torch.full((packed.numel() + 64,), 0xA7, dtype=torch.uint8, device="cuda")
            offsets, lengths, results, info = batch.encode_packed_launch(src, lens, None, hc, k, dst, batch.BOUND)
            h = batch.read_packed_info(info)
            assert torch.equal(results, want) and torch.equal(lengths, want.clamp(min=0))
            assert (h.first_failed, h.error, h.written_blocks, h.packed_bytes) == (0, _lib.E_ARGUMENT, n, int(mask.sum()))
            assert torch.equal(dst[:h.packed_bytes], packed[mask]) and bool((dst[h.packed_bytes:] == 0xA7).all())


def test_auto_sizing(monkeypatch):
    import torch
    calls = []
    launch = batch.encode_packed_launch
    monkeypatch.setattr(batch, "encode_packed_launch", lambda *a, **kw: (calls.append(1), launch(*a, **kw))[1])
    n = 257
    # D2, the reference fuzzer generator, shrinks to about half: the first attempt, as many bytes as the source has, fits
    dst_view, offsets, lengths, results, h = batch.encode_packed(rows(2)[:n], 65536, round_blocks=64)
    assert len(calls) == 1 and h.written_blocks == n and h.packed_bytes < n * 65536 * 0.6
    # D1 is incompressible: every block expands, the first attempt does not hold them and a second call of exactly packed_bytes does
    del calls[:]
    dst_view, offsets, lengths, results, h = batch.encode_packed(rows(1)[:n], 65536, round_blocks=64)
    assert len(calls) == 2 and h.written_blocks == n and h.packed_bytes > n * 65536 and dst_view.numel() == h.packed_bytes
    slots = torch.empty((n, batch.BOUND_STRIDE), dtype=torch.uint8, device="cuda")
    res = batch.encode(rows(1)[:n], 65536, slots, batch.BOUND)
    keep = torch.arange(batch.BOUND_STRIDE, device="cuda")[None, :] < res[:, None]
    assert torch.equal(results, res) and torch.equal(dst_view, slots[keep])


def test_launch_only_on_a_stream():
    """the device call queues behind unrelated work on a non-default stream and returns before that work is done"""
    import torch
    n, k, dist = 257, 64, 3
    src, lens = rows(dist)[:n], mixed_lengths(n)
    first = batch.encode_packed(src, lens, round_blocks=k)             # the default-stream run (and every first-use step)
    dst = torch.empty(first[0].numel(), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        busy = torch.randn(8192, 8192, device="cuda")
        for _ in range(30):
            busy = busy @ busy * 1e-4
        offsets, lengths, results, info = batch.encode_packed_launch(src, lens, None, False, k, dst, batch.BOUND)
        done = torch.cuda.Event()
        done.record(s)
        returned_early = not done.query()
    s.synchronize()
    assert returned_early, "the call waited for the stream"
    h = batch.read_packed_info(info)
    assert h.written_blocks == n and torch.equal(dst, first[0]) and torch.equal(offsets, first[1]) and torch.equal(results, first[3])


def test_host_call_parity():
    n, dist = 257, 2
    L = _lib.lib()
    src = rows(dist)[:n].cpu().numpy()
    lens = mixed_lengths(n).cpu().numpy()
    res, packed = reference(dist, n, False)
    res, packed = res.cpu().numpy(), packed.cpu().numpy()
    off = np.concatenate(([0], np.cumsum(res, dtype=np.int64)))
    for k, cap in ((0, packed.size), (64, packed.size + 1000), (64, int(off[128]) + 1)):
        dst = np.full(cap + 64, 0xA7, np.uint8)
        dst_off = np.zeros(n + 1, np.int64)
        plen, result = np.zeros(n, np.int32), np.zeros(n, np.int32)
        info = _lib.PackedInfo()
        b = _lib.Batch(src=src.ctypes.data, src_stride=src.strides[0], src_len=lens.ctypes.data, src_len_all=65536, dst_cap_all=batch.BOUND,
                       result=result.ctypes.data, n_blocks=n)
        assert _lib.check(L.lz4hip_encode_packed_host(C.byref(b), 0, k, dst.ctypes.data, cap, dst_off.ctypes.data, plen.ctypes.data, C.byref(info))) == 0
        written = n if cap >= packed.size else 128
        assert (info.blocks, info.packed_bytes, info.written_blocks, info.first_failed, info.error) == (n, packed.size, written, -1, 0)
        assert np.array_equal(dst_off, off) and np.array_equal(plen, res) and np.array_equal(result, res)
        assert np.array_equal(dst[:off[written]], packed[:off[written]]) and (dst[cap:] == 0xA7).all()


def test_argument_checks():
    import torch
    L = _lib.lib()
    n = 3
    src, lens = rows(2)[:n], mixed_lengths(n)
    need = L.lz4hip_encode_packed_scratch_bytes(n, batch.BOUND, 0)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n * batch.BOUND, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    info = torch.empty(5, dtype=torch.int64, device="cuda")

    def call(b, mode=0, k=0, cap=dst.numel(), off_ptr=off.data_ptr(), scratch_n=need):
        return L.lz4hip_encode_packed_device(None if b is None else C.byref(b), mode, k, dst.data_ptr(), cap, off_ptr, None, scratch.data_ptr(), scratch_n,
                                             info.data_ptr(), torch.cuda.current_stream().cuda_stream)

    def good(**kw):
        fields = dict(src=src.data_ptr(), src_stride=src.stride(0), src_len=lens.data_ptr(), src_len_all=65536, dst_cap_all=batch.BOUND, n_blocks=n)
        fields.update(kw)
        return _lib.Batch(**fields)

    assert call(good()) == 0
    assert call(None) == _lib.E_ARGUMENT
    assert call(good(n_blocks=-1)) == _lib.E_ARGUMENT and call(good(dst_cap_all=0)) == _lib.E_ARGUMENT and call(good(src=None)) == _lib.E_ARGUMENT
    assert call(good(), mode=2) == _lib.E_ARGUMENT and call(good(), k=-1) == _lib.E_ARGUMENT and call(good(), cap=-1) == _lib.E_ARGUMENT
    assert call(good(), off_ptr=None) == _lib.E_ARGUMENT and call(good(), scratch_n=need - 1) == _lib.E_ARGUMENT
    assert call(good(n_blocks=1 << 31), scratch_n=1 << 62) == _lib.E_ARGUMENT
    torch.cuda.synchronize()
    f = L.lz4hip_encode_packed_scratch_bytes
    assert f(0, batch.BOUND, 64) == 0 and f(16384, batch.BOUND, 16384) == f(262144, batch.BOUND, 16384) < f(262144, batch.BOUND, 65536)
    assert f(262144, batch.BOUND, 0) > 262144 * batch.BOUND
    # an empty batch
    b = _lib.Batch(dst_cap_all=batch.BOUND)
    off.fill_(-77)
    assert L.lz4hip_encode_packed_device(C.byref(b), 0, 0, None, 0, off.data_ptr(), None, None, 0, info.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    h = batch.read_packed_info(info)
    assert int(off[0]) == 0 and int(off[1]) == -77 and (h.blocks, h.packed_bytes, h.written_blocks, h.first_failed, h.error) == (0, 0, 0, -1, 0)
