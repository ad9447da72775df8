"""Block batches decoded against a shared dictionary on the device (lz4hip_decode_batch_dict_device / _host, lz4hip_decoded_sizes_dict_*):
the built blocks of tests/dict_cases.py -- every one on one side of an edge of the decoder's paths, checked against the spliced truth on the
CPU first -- through the device call one block per call and all of a dictionary's in one batch, both decoder kinds, guard bytes behind
every row, the dictionary at 0, 1 and 3 bytes from a 16-byte boundary, and lz4hip_dispatch_counts as the proof that the wavefront mapping
ran and the lane mapping did not; then the fixture liblz4 wrote (tests/golden/dict_blocks.json) through the host call, the sizes calls,
decode_packed_dict and the codec front, and tiled to 20 000 blocks.  That each built block reaches the path it was built for is proven
where the kernel's counters exist, under the emulator: tests/test_simt_dict_decode.py."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    return gpu_helpers


class wave_only:
    """lz4hip_dispatch_counts: the wavefront mapping's counter moved, the lane mapping's did not"""

    def __enter__(self):
        from lz4net_amd import _lib
        self.before = _lib.dispatch_counts()

    def __exit__(self, *exc):
        from lz4net_amd import _lib
        if exc[0] is None:
            after = _lib.dispatch_counts()
            assert after[_lib.K_DECODE_WAVE] > self.before[_lib.K_DECODE_WAVE]
            assert all(after[k] == self.before[k] for k in range(len(after)) if k != _lib.K_DECODE_WAVE), "another kernel family was launched"
        return False


def _dict_tensor(dic, align):
    """the dictionary on the device, its first byte `align` bytes behind a 16-byte boundary (None for an empty one)"""
    import torch
    if len(dic) == 0:
        return None
    buf = torch.zeros(len(dic) + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[align:align + len(dic)]
    t.copy_(torch.from_numpy(np.ascontiguousarray(dic)))
    assert t.data_ptr() % 16 == align
    return t


def _device_decoder(gpu, one_by_one):
    """dict_cases.check's decode over lz4hip_decode_batch_dict_device: rows and outputs uploaded once; one call for the batch, or one call
    per block"""
    import torch
    from lz4net_amd import _lib

    def decode(comps, caps, known, lens, dic, align):
        n = len(comps)
        src_h, _ = gpu.pack(comps)
        src = torch.from_numpy(src_h).cuda()
        sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        cp = torch.tensor(caps, dtype=torch.int32, device="cuda")
        dst = torch.full((n, max(caps) + 64), cases.HOLE, dtype=torch.uint8, device="cuda")
        res = torch.full((n,), -12345678, dtype=torch.int32, device="cuda")
        d = _dict_tensor(dic, align)
        dp, dn = (d.data_ptr(), d.numel()) if d is not None else (None, 0)
        for first, count in ([(i, 1) for i in range(n)] if one_by_one else [(0, n)]):
            b = _lib.Batch(src=src.data_ptr() + first * src.stride(0), src_off=None, src_stride=src.stride(0), src_len=sl.data_ptr() + 4 * first,
                           dst=dst.data_ptr() + first * dst.stride(0), dst_off=None, dst_stride=dst.stride(0), dst_cap=cp.data_ptr() + 4 * first,
                           dst_cap_all=0, src_len_all=0, result=res.data_ptr() + 4 * first, n_blocks=count)
            _lib.check(_lib.lib().lz4hip_decode_batch_dict_device(C.byref(b), dp, dn, int(known), gpu.s0()))
        torch.cuda.synchronize()
        return res.cpu().numpy(), dst.cpu().numpy()
    return decode


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("batch,align", [("single-block", 0), ("one-batch", 1), ("one-batch", 3)])
@pytest.mark.parametrize("name", cases.NAMES)
def test_built_blocks_match_the_spliced_truth(gpu, oracle, name, batch, align, known):
    with wave_only():
        cases.check(oracle, name, known, _device_decoder(gpu, batch == "single-block"), align=align)


def test_dict_len_zero_is_the_plain_call(gpu, oracle):
    """result for result and byte for byte, on valid and damaged blocks, with the wavefront mapping forced for the plain call"""
    f = cases.family("identity")
    comps = [np.frombuffer(c.block, np.uint8) for c in f.cases] + [c for c, _ in cases.plain_blocks()]
    caps = [c.cap for c in f.cases] + [raw.size for _, raw in cases.plain_blocks()]
    lens = [len(c) for c in comps]
    for known in (True, False):
        with gpu.mapping_ran("wave"):
            want_res, want_dst = gpu.decode(comps, caps, known=known)
        res, dst = _device_decoder(gpu, False)(comps, caps, known, lens, np.zeros(0, np.uint8), 0)
        assert list(res) == list(want_res)
        for i in range(len(comps)):
            # (the host call copies back what the result owns: a refused row keeps its fill there, and may hold a few bytes here)
            n = caps[i] if known and res[i] >= 0 else max(int(res[i]), 0) if not known else 0
            assert np.array_equal(dst[i, :n], want_dst[i, :n]) and (dst[i, caps[i]:caps[i] + 64] == cases.HOLE).all(), (known, i)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return cases.load_fixture()


def _host_batch(blocks, caps, canary=64):
    from lz4net_amd import _lib
    import gpu_helpers
    src, sl = gpu_helpers.pack([np.frombuffer(b, np.uint8) for b in blocks])
    cp = np.array(caps, np.int32)
    dst = np.full((len(blocks), int(cp.max()) + canary), cases.HOLE, np.uint8)
    res = np.full(len(blocks), -12345678, np.int32)
    b = _lib.Batch(src=src.ctypes.data, src_off=None, src_stride=src.strides[0], src_len=sl.ctypes.data, dst=dst.ctypes.data, dst_off=None,
                   dst_stride=dst.strides[0], dst_cap=cp.ctypes.data, dst_cap_all=0, src_len_all=0, result=res.ctypes.data, n_blocks=len(blocks))
    return b, (src, sl, cp), dst, res


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
def test_fixture_through_the_host_call(gpu, fixture, known):
    from lz4net_amd import _lib
    dic, records, _ = fixture
    b, keep, dst, res = _host_batch([blk for _, blk in records], [len(p) + (0 if known else 7) for p, _ in records])
    with wave_only():
        _lib.check(_lib.lib().lz4hip_decode_batch_dict_host(C.byref(b), dic.ctypes.data, dic.size, int(known)))
    assert list(res) == [len(blk) if known else len(p) for p, blk in records]
    for i, (p, _) in enumerate(records):
        assert bytes(dst[i, :len(p)]) == p and (dst[i, len(p) + (0 if known else 7):] == cases.HOLE).all(), i
    # without the dictionary the same blocks are refused: every one of them starts with a match into it or reaches it soon
    _lib.check(_lib.lib().lz4hip_decode_batch_dict_host(C.byref(b), None, 0, int(known)))
    assert (res < 0).sum() >= len(records) - 2


def test_fixture_sizes_and_packed_decode(gpu, fixture):
    import torch
    from lz4net_amd import _lib, batch
    dic, records, _ = fixture
    blocks = [blk for _, blk in records]
    src_h, sl_h = gpu.pack([np.frombuffer(b, np.uint8) for b in blocks])
    src, sl = torch.from_numpy(src_h).cuda(), torch.from_numpy(sl_h).cuda()
    want = [len(p) for p, _ in records]
    res = torch.empty(len(blocks), dtype=torch.int32, device="cuda")
    sizes, offsets, info = batch.decoded_sizes_dict(src, sl, dic.size, result=res)
    h = batch.read_sizes_info(info)
    assert sizes.tolist() == want and res.tolist() == want and offsets.tolist() == [0] + list(np.cumsum(want))
    assert (h.blocks, h.decoded_bytes, h.first_error, h.error) == (len(blocks), sum(want), -1, 0)
    # with no dictionary to reach into, the walk refuses them
    _, _, info0 = batch.decoded_sizes_dict(src, sl, 0)
    assert batch.read_sizes_info(info0).first_error >= 0
    # the host sizes call
    b, keep, _, hres = _host_batch(blocks, want)
    doff, dcap, hinfo = np.zeros(len(blocks) + 1, np.int64), np.zeros(len(blocks), np.int32), _lib.SizesInfo()
    _lib.check(_lib.lib().lz4hip_decoded_sizes_dict_host(C.byref(b), dic.size, doff.ctypes.data, dcap.ctypes.data, C.byref(hinfo)))
    assert list(hres) == want and list(dcap) == want and int(doff[-1]) == sum(want) and hinfo.first_error == -1
    # decode_packed_dict: the sizes, then the decode into exactly those bytes
    d = _dict_tensor(dic, 1)
    with wave_only():
        out, offs, results = batch.decode_packed_dict(src, sl, d)
        torch.cuda.synchronize()
    assert results.tolist() == want and out.cpu().numpy().tobytes() == b"".join(p for p, _ in records)
    # decode_dict, rows to rows
    rows = torch.full((len(blocks), 4096 + 64), cases.HOLE, dtype=torch.uint8, device="cuda")
    caps = torch.tensor(want, dtype=torch.int32, device="cuda")
    used = batch.decode_dict(src, sl, rows, caps, d)
    assert used.tolist() == [len(b) for b in blocks]
    back = rows.cpu().numpy()
    for i, (p, _) in enumerate(records):
        assert bytes(back[i, :len(p)]) == p and (back[i, len(p):] == cases.HOLE).all(), i


def test_codec_front_on_the_fixture(gpu, fixture):
    from lz4net_amd.codec import ArgumentException, LZ4Codec
    dic, records, _ = fixture
    blocks, plain = [b for _, b in records], [p for p, _ in records]
    assert LZ4Codec.decode_many_with_dictionary(blocks, dic) == plain
    assert LZ4Codec.decode_many_with_dictionary(blocks, dic.tobytes(), out_sizes=[len(p) for p in plain]) == plain
    with pytest.raises(ArgumentException):
        LZ4Codec.decode_many_with_dictionary(blocks, dic[:100])
    with pytest.raises(ArgumentException):
        LZ4Codec.decode_many_with_dictionary(blocks, dic, out_sizes=[len(p) + 1 for p in plain])


def test_twenty_thousand_blocks_stay_on_the_wavefront_mapping(gpu, fixture):
    """the fixture tiled to 20 000 blocks (more than the lane mapping's threshold): one device call, the wavefront mapping alone, every
    row right; and the host call, which cuts such a batch over two pipelines that share the one uploaded dictionary"""
    import torch
    from lz4net_amd import _lib, batch
    dic, records, _ = fixture
    n, m = 20000, len(records)
    src_h, sl_h = gpu.pack([np.frombuffer(b, np.uint8) for _, b in records])
    plain_h = np.full((m, 4096 + 16), cases.HOLE, np.uint8)
    for i, (p, _) in enumerate(records):
        plain_h[i, :len(p)] = np.frombuffer(p, np.uint8)
    pick = torch.arange(n, device="cuda") % m
    src, sl = torch.from_numpy(src_h).cuda()[pick].contiguous(), torch.from_numpy(sl_h).cuda()[pick].contiguous()
    want = torch.from_numpy(plain_h).cuda()[pick]
    caps = torch.tensor([len(p) for p, _ in records], dtype=torch.int32, device="cuda")[pick].contiguous()
    rows = torch.full((n, 4096 + 16), cases.HOLE, dtype=torch.uint8, device="cuda")
    d = _dict_tensor(dic, 3)
    with wave_only():
        used = batch.decode_dict(src, sl, rows, caps, d)
        torch.cuda.synchronize()
    assert torch.equal(used, sl) and torch.equal(rows, want)
    # the host call
    src_n, sl_n, cap_n = src.cpu().numpy(), sl.cpu().numpy(), caps.cpu().numpy()
    dst = np.full((n, 4096 + 16), cases.HOLE, np.uint8)
    res = np.zeros(n, np.int32)
    b = _lib.Batch(src=src_n.ctypes.data, src_off=None, src_stride=src_n.strides[0], src_len=sl_n.ctypes.data, dst=dst.ctypes.data, dst_off=None,
                   dst_stride=dst.strides[0], dst_cap=cap_n.ctypes.data, dst_cap_all=0, src_len_all=0, result=res.ctypes.data, n_blocks=n)
    with wave_only():
        _lib.check(_lib.lib().lz4hip_decode_batch_dict_host(C.byref(b), dic.ctypes.data, dic.size, 1))
    assert np.array_equal(res, sl_n) and np.array_equal(dst, want.cpu().numpy())
