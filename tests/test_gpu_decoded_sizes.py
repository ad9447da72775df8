"""The size query of a block batch on the device (lz4hip_decoded_sizes_device / _host, batch.decoded_sizes / decode_packed): parity with
the reference on the corpora of tests/test_decoded_sizes.py, the two-step decode into a buffer of exactly decoded_bytes, calls queued
on one stream without synchronisation, and a batch whose lanes walk many blocks each.  The CPU twin -- the same kernels and host code
under the SIMT emulator -- is tests/test_decoded_sizes.py."""
import ctypes as C

import numpy as np
import pytest

import sizes_helpers as sh
from lz4net_amd import _lib, batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpora(oracle):
    """every corpus of the CPU tests in one list, with the reference's results: computed once, never changed"""
    blocks = sh.encoder_corpus(oracle) + sh.hand_blocks() + sh.prefixes(oracle) + sh.window_blocks(64) + sh.fuzz_blocks(oracle)
    want = sh.reference_sizes(blocks)
    want.setflags(write=False)
    return blocks, want


def device_sizes(torch, buf, off, lens, wanted=("result", "dst_off", "dst_cap", "info"), stream=None, staged=None):
    """lz4hip_decoded_sizes_device on a packed layout (staged: already on the device); returns the outputs as device tensors (None for
    those left out)"""
    n = len(lens)
    d_buf, d_off, d_len = staged if staged else (torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda())
    res = torch.full((n,), -77, dtype=torch.int32, device="cuda") if "result" in wanted else None
    doff = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda") if "dst_off" in wanted else None
    cap = torch.full((n,), -77, dtype=torch.int32, device="cuda") if "dst_cap" in wanted else None
    info = torch.full((4,), -77, dtype=torch.int64, device="cuda") if "info" in wanted else None
    L = _lib.lib()
    need = L.lz4hip_decoded_sizes_scratch_bytes(n)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()                # noqa: E731
    b = _lib.Batch(src=d_buf.data_ptr(), src_off=d_off.data_ptr(), src_len=d_len.data_ptr(), result=ptr(res), n_blocks=n)
    s = stream if stream is not None else torch.cuda.current_stream()
    _lib.check(L.lz4hip_decoded_sizes_device(C.byref(b), ptr(doff), ptr(cap), scratch.data_ptr(), need, ptr(info), s.cuda_stream))
    return res, doff, cap, info, (d_buf, d_off, d_len, scratch)


def check_outputs(want, res, doff, cap, info):
    e_cap, e_off, total, first, error = sh.expected(want)
    if res is not None:
        got = res.cpu().numpy()
        wrong = np.flatnonzero(got != want)
        assert len(wrong) == 0, [(int(i), int(got[i]), int(want[i])) for i in wrong[:8]]
    if cap is not None:
        assert np.array_equal(cap.cpu().numpy(), e_cap)
    if doff is not None:
        assert np.array_equal(doff.cpu().numpy(), e_off)
    if info is not None:
        r = batch.read_sizes_info(info)
        assert (r.blocks, r.decoded_bytes, r.first_error, r.error, r.reserved) == (len(want), total, first, error, 0)


def test_parity_on_the_device(corpora):
    import torch
    blocks, want = corpora
    buf, off, lens = sh.pack_offsets(blocks)                            # odd byte offsets
    res, doff, cap, info, keep = device_sizes(torch, buf, off, lens)
    torch.cuda.synchronize()
    check_outputs(want, res, doff, cap, info)
    for wanted in (("dst_off",), ("dst_cap", "info"), ("result",)):     # the other outputs are NULL
        res, doff, cap, info, keep = device_sizes(torch, buf, off, lens, wanted)
        torch.cuda.synchronize()
        check_outputs(want, res, doff, cap, info)
    with _lib.tuning(sizes_groups=3):                                   # three wavefronts: every lane walks more than a hundred blocks
        res, doff, cap, info, keep = device_sizes(torch, buf, off, lens)
        torch.cuda.synchronize()
    check_outputs(want, res, doff, cap, info)


def test_parity_of_the_host_call(corpora):
    blocks, want = corpora
    buf, off, lens = sh.pack_offsets(blocks)
    n = len(blocks)
    L = _lib.lib()
    out = sh.Outputs(n)
    b = sh.make_batch(buf, off=off, lens=lens, n=n, result=out.ptr("result"))
    assert _lib.check(L.lz4hip_decoded_sizes_host(C.byref(b), out.ptr("dst_off"), out.ptr("dst_cap"), C.byref(out.info))) == 0
    out.check(want)
    out = sh.Outputs(n, ("dst_off", "info"))
    b = sh.make_batch(buf, off=off, lens=lens, n=n)
    assert _lib.check(L.lz4hip_decoded_sizes_host(C.byref(b), out.ptr("dst_off"), None, C.byref(out.info))) == 0
    out.check(want)
    # rows at a stride, one length for all, and an empty batch
    same = [b[:300] for b in blocks if len(b) >= 300][:70]
    assert len(same) == 70
    rows = np.full((70, 303), 0xEE, np.uint8)
    rows[:, :300] = np.stack(same)
    out = sh.Outputs(70)
    b = sh.make_batch(rows, stride=303, len_all=300, n=70, result=out.ptr("result"))
    assert _lib.check(L.lz4hip_decoded_sizes_host(C.byref(b), out.ptr("dst_off"), out.ptr("dst_cap"), C.byref(out.info))) == 0
    out.check(sh.reference_sizes(same))
    out = sh.Outputs(0)
    b = sh.make_batch(None, n=0)
    assert L.lz4hip_decoded_sizes_host(C.byref(b), out.ptr("dst_off"), None, C.byref(out.info)) == 0
    out.check(np.zeros(0, np.int32))


def mixed_batch(oracle, n=300):
    """a few hundred blocks of mixed sizes with their originals; every seventh is corrupt (a truncation or a bad offset)"""
    rng = np.random.default_rng(77)
    raws, comps, corrupt = [], [], []
    for i in range(n):
        length = int(rng.choice([0, 1, 13, 64, 700, 4096, 20000, 65536, 70000]))
        raw = sh.data(oracle, int(rng.integers(0, 4)), length, seed=100 + i).copy()
        comp = sh.compress(raw, hc=bool(i & 1))
        bad = i % 7 == 3
        if bad and len(comp) < 12:
            comp = np.concatenate([comp, np.zeros(1, np.uint8)])        # a byte behind the last literals
        elif bad:
            comp = comp[:-3].copy() if i & 1 else np.concatenate([np.array([0x00, 9, 9], np.uint8), comp])   # truncated; an offset before the block
        raws.append(raw); comps.append(comp); corrupt.append(bad)
    want = sh.reference_sizes(comps)
    corrupt = np.array(corrupt)
    assert (want[corrupt] < 0).all() and all(want[i] == len(raws[i]) for i in np.flatnonzero(~corrupt))
    return raws, comps, want


def check_round_trip(raws, want, dst, offsets, results, guard=0):
    e_cap, e_off, total, first, error = sh.expected(want)
    out = dst.cpu().numpy()
    assert out.size == total + guard and np.array_equal(offsets.cpu().numpy(), e_off)
    got = results.cpu().numpy()
    for i, raw in enumerate(raws):
        if want[i] < 0:
            assert got[i] < 0 and e_off[i + 1] == e_off[i], i          # a corrupt block fails again and owns no byte of the output
        else:
            assert got[i] == want[i] == len(raw), (i, got[i], want[i])
            assert np.array_equal(out[e_off[i]:e_off[i + 1]], raw), i
    return out


@pytest.mark.parametrize("decoder", ["auto", "wave", "lane"])
def test_two_step_decode(oracle, decoder):
    import torch
    raws, comps, want = mixed_batch(oracle)
    buf, off, lens = sh.pack_offsets(comps)
    n = len(comps)
    res, doff, cap, info, keep = device_sizes(torch, buf, off, lens)
    r = batch.read_sizes_info(info)                                     # the one synchronisation
    check_outputs(want, res, doff, cap, info)
    guard = 256
    dst = torch.full((r.decoded_bytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    results = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    d_buf, d_off, d_len, _ = keep
    b = _lib.Batch(src=d_buf.data_ptr(), src_off=d_off.data_ptr(), src_len=d_len.data_ptr(), dst=dst.data_ptr(), dst_off=doff.data_ptr(),
                   dst_cap=cap.data_ptr(), result=results.data_ptr(), n_blocks=n)
    with _lib.tuning(decoder=decoder):
        _lib.check(_lib.lib().lz4hip_decode_batch_device(C.byref(b), 0, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    out = check_round_trip(raws, want, dst, doff, results, guard)
    assert (out[r.decoded_bytes:] == 0xA5).all()                        # the guard bytes behind exactly decoded_bytes


def test_decode_packed(oracle):
    import torch
    raws, comps, want = mixed_batch(oracle)
    buf, off, lens = sh.pack_offsets(comps)
    d_buf, d_off, d_len = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    dst, offsets, results = batch.decode_packed(d_buf, d_len, d_off)
    torch.cuda.synchronize()
    check_round_trip(raws, want, dst, offsets, results)
    # rows of a 2-D tensor, one length for all
    same = [c for c in comps if len(c) > 40][:9]
    rows = torch.from_numpy(np.stack([c[:40] for c in same])).cuda()
    sizes, offsets, info = batch.decoded_sizes(rows, 40)
    r = batch.read_sizes_info(info)
    ref = sh.reference_sizes([c[:40] for c in same])
    assert np.array_equal(sizes.cpu().numpy(), np.maximum(ref, 0)) and r.blocks == 9 and r.decoded_bytes == int(np.maximum(ref, 0).sum())
    dst, offsets, results = batch.decode_packed(torch.zeros((0, 16), dtype=torch.uint8, device="cuda"), 16)
    assert dst.numel() == 0 and offsets.cpu().tolist() == [0] and results.numel() == 0


def test_launch_only_on_one_stream(corpora):
    import torch
    blocks, want = corpora
    parts = [(blocks[k::4], want[k::4]) for k in range(4)]
    stream = torch.cuda.Stream()
    layouts = [sh.pack_offsets(p) for p, _ in parts]
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(stream):
        staged = [(torch.from_numpy(b).cuda(), torch.from_numpy(o).cuda(), torch.from_numpy(ln).cuda()) for b, o, ln in layouts]
    stream.synchronize()
    for (buf, off, lens), on_device in zip(layouts, staged):            # four calls queued back to back, nothing waited for in between
        with torch.cuda.stream(stream):
            outs.append(device_sizes(torch, buf, off, lens, stream=stream, staged=on_device))
    stream.synchronize()
    for (p, w), (res, doff, cap, info, keep) in zip(parts, outs):
        check_outputs(w, res, doff, cap, info)


def test_chip_filling_batch():
    """65 536 blocks of 4 KiB, made and encoded on the device: 1 024 wavefronts under the library's grid, and sixteen of them with
    sixty-four blocks per lane; the sizes are those the encoder's inputs had"""
    import torch
    n, length = 65536, 4096
    cap = length + length // 255 + 16
    stride = (cap + 15) // 16 * 16
    raw = batch.synth(2, 4321, 0, n, length=length)
    comp = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    clen = batch.encode(raw, length, comp, cap)
    assert bool((clen > 0).all())
    for groups in (0, 16):
        with _lib.tuning(sizes_groups=groups):
            result = torch.full((n,), -77, dtype=torch.int32, device="cuda")
            sizes, offsets, info = batch.decoded_sizes(comp, clen, result=result)
            r = batch.read_sizes_info(info)
        assert (r.blocks, r.decoded_bytes, r.first_error, r.error) == (n, n * length, -1, 0)
        assert bool((result == length).all()) and bool((sizes == length).all())
        assert bool((offsets == torch.arange(n + 1, device="cuda", dtype=torch.int64) * length).all())
