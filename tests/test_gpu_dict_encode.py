"""Block batches encoded against a shared dictionary on the device (lz4hip_encode_batch_dict_device / _host): the built blocks of
tests/dict_encode_cases.py -- every one at an edge of the DICT mode, its parse asserted on the twin when it is built -- through the device
call one block per call and all of a dictionary's in one batch, guard bytes behind every row, the dictionary at 0, 1 and 3 bytes from a
16-byte boundary, bytes and results against the twin (tests/dict_encode_ref.py), and lz4hip_dispatch_counts as the proof that the
wavefront encoder's counter moved and no other; dict_len = 0 against the plain call; the round trip through the library's own
dictionary decode; then the records of tests/golden/dict_blocks.json through the host call, batch.encode_dict and the codec front, and
tiled to 20 000 blocks.  That each built block reaches the edge it was built for is proven where the kernel's counters exist, under the
emulator: tests/test_simt_dict_encode.py."""
import ctypes as C

import numpy as np
import pytest

import dict_cases
import dict_encode_cases as cases
import dict_encode_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    return gpu_helpers


class wave_only:
    """lz4hip_dispatch_counts: the wavefront encoder's counter moved, no other did"""

    def __enter__(self):
        from lz4net_amd import _lib
        self.before = _lib.dispatch_counts()

    def __exit__(self, *exc):
        from lz4net_amd import _lib
        if exc[0] is None:
            after = _lib.dispatch_counts()
            assert after[_lib.K_ENCODE_WAVE] > self.before[_lib.K_ENCODE_WAVE]
            assert all(after[k] == self.before[k] for k in range(len(after)) if k != _lib.K_ENCODE_WAVE), "another kernel family was launched"
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


def _device_encoder(gpu, one_by_one):
    """dict_encode_cases.check's encode over lz4hip_encode_batch_dict_device: rows uploaded once; one call for the batch, or one per block"""
    import torch
    from lz4net_amd import _lib

    def encode(blocks, caps, dic, align):
        n = len(blocks)
        src_h, sl_h = gpu.pack([np.frombuffer(b, np.uint8) for b in blocks])
        src, sl = torch.from_numpy(src_h).cuda(), torch.from_numpy(sl_h).cuda()
        cp = torch.tensor(caps, dtype=torch.int32, device="cuda")
        dst = torch.full((n, max(caps) + 64), cases.HOLE, dtype=torch.uint8, device="cuda")
        res = torch.full((n,), -12345678, dtype=torch.int32, device="cuda")
        d = _dict_tensor(dic, align)
        dp, dn = (d.data_ptr(), d.numel()) if d is not None else (None, 0)
        need = _lib.lib().lz4hip_encode_dict_scratch_bytes(dn)
        scratch = torch.full((need + 64,), 0x77, dtype=torch.uint8, device="cuda")
        for first, count in ([(i, 1) for i in range(n)] if one_by_one else [(0, n)]):
            b = _lib.Batch(src=src.data_ptr() + first * src.stride(0), src_off=None, src_stride=src.stride(0), src_len=sl.data_ptr() + 4 * first,
                           dst=dst.data_ptr() + first * dst.stride(0), dst_off=None, dst_stride=dst.stride(0), dst_cap=cp.data_ptr() + 4 * first,
                           dst_cap_all=0, src_len_all=0, result=res.data_ptr() + 4 * first, n_blocks=count)
            _lib.check(_lib.lib().lz4hip_encode_batch_dict_device(C.byref(b), dp, dn, scratch.data_ptr() if need else None, need, gpu.s0()))
        torch.cuda.synchronize()
        tail = scratch.cpu().numpy()
        assert (tail[need:] == 0x77).all(), "wrote behind the scratch"
        if need:
            assert np.array_equal(tail[:need].view(np.uint32), ref.primed_table(dic.tobytes())), "the primed table after the batch"
        out = dst.cpu().numpy()
        return res.cpu().numpy(), [out[i, :caps[i] + 64] for i in range(n)]
    return encode


@pytest.mark.parametrize("batch,align", [("single-block", 0), ("one-batch", 1), ("one-batch", 3)])
@pytest.mark.parametrize("group", [g for g in cases.GROUPS if g[1] > 0], ids=[i for g, i in zip(cases.GROUPS, cases.IDS) if g[1] > 0])
def test_built_blocks_match_the_twin(gpu, oracle, group, batch, align):
    with wave_only():
        cases.check(oracle, group, _device_encoder(gpu, batch == "single-block"), align=align)


def test_dict_len_zero_is_the_plain_call(gpu, oracle):
    """result for result and byte for byte on the same rows, short (the 64k variant) and long (the generic one), a NULL scratch included"""
    import torch
    from lz4net_amd import _lib, batch
    rng = np.random.default_rng(11)
    blocks = [c.block for c in cases.cases(("generic", 0))] + [bytes(rng.integers(0, 4, n, dtype=np.uint8)) for n in (4096, 65546, 65547, 70001)]
    caps = [c.cap for c in cases.cases(("generic", 0))] + [ref.bound(n) for n in (4096, 65546, 65547, 70001)]
    cases.check(oracle, ("generic", 0), _device_encoder(gpu, False))                  # (the reference's bytes)
    src_h, sl_h = gpu.pack([np.frombuffer(b, np.uint8) for b in blocks])
    src, sl = torch.from_numpy(src_h).cuda(), torch.from_numpy(sl_h).cuda()
    cp = torch.tensor(caps, dtype=torch.int32, device="cuda")
    want = torch.full((len(blocks), max(caps) + 64), cases.HOLE, dtype=torch.uint8, device="cuda")
    got = want.clone()
    want_res = batch.encode(src, sl, want, cp)
    got_res = batch.encode_dict(src, sl, got, cp, None)
    empty_res = batch.encode_dict(src, sl, got.clone(), cp, torch.zeros(0, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(want_res, got_res) and torch.equal(want_res, empty_res) and torch.equal(want, got)
    r = want_res.cpu().numpy()
    assert r[-1] > 0 and r[len(cases.cases(("generic", 0))) - 1] == 0
    long_one = np.frombuffer(blocks[-1], np.uint8)
    assert bytes(got[-1, :r[-1]].cpu().numpy()) == bytes(oracle.compress(long_one)) == ref.encode(blocks[-1])[1]


@pytest.mark.parametrize("group", [("generic", 17), ("generic", 4097), ("generic", 70000), ("far", 65536)], ids=["17", "4097", "70000", "far-65536"])
def test_round_trip_through_the_dictionary_decode(gpu, group):
    """batch.encode_dict, then batch.decode_dict with the same dictionary: every block that fitted comes back"""
    import torch
    from lz4net_amd import batch
    cs = [c for c in cases.cases(group) if c.cap >= ref.bound(len(c.block))]
    src_h, sl_h = gpu.pack([np.frombuffer(c.block, np.uint8) for c in cs])
    src, sl = torch.from_numpy(src_h).cuda(), torch.from_numpy(sl_h).cuda()
    comp = torch.full((len(cs), ref.bound(int(sl_h.max())) + 16), cases.HOLE, dtype=torch.uint8, device="cuda")
    cp = torch.tensor([c.cap for c in cs], dtype=torch.int32, device="cuda")
    d = _dict_tensor(cs[0].dic, 1)
    with wave_only():
        clen = batch.encode_dict(src, sl, comp, cp, d)
        torch.cuda.synchronize()
    assert (clen > 0).all()
    back = torch.full_like(src, cases.HOLE)
    used = batch.decode_dict(comp, clen, back, sl, d)
    torch.cuda.synchronize()
    assert torch.equal(used, clen)
    b = back.cpu().numpy()
    for i, c in enumerate(cs):
        assert bytes(b[i, :len(c.block)]) == c.block and (b[i, len(c.block):] == cases.HOLE).all(), c.note


# ---- the fixture's records -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    dic, records, _ = dict_cases.load_fixture()
    plains = [p for p, _ in records]
    return dic, plains, [ref.encode(p, dic.tobytes()) for p in plains]


def _decodes(dic, plain, block):
    import lz4f_ref
    assert lz4f_ref.decode_block(block, len(plain), history=ref.tail_of(dic.tobytes())) == (len(plain), plain)
    lz4 = dict_cases.liblz4()
    if lz4 is not None:
        assert dict_cases.using_dict(lz4, block, len(plain), dic) == (len(plain), plain)


def test_fixture_through_the_host_call(gpu, fixture):
    from lz4net_amd import _lib
    dic, plains, want = fixture
    src, sl = gpu.pack([np.frombuffer(p, np.uint8) for p in plains])
    cp = np.array([ref.bound(len(p)) for p in plains], np.int32)
    dst = np.full((len(plains), int(cp.max()) + 64), cases.HOLE, np.uint8)
    res = np.full(len(plains), -12345678, np.int32)
    b = _lib.Batch(src=src.ctypes.data, src_off=None, src_stride=src.strides[0], src_len=sl.ctypes.data, dst=dst.ctypes.data, dst_off=None,
                   dst_stride=dst.strides[0], dst_cap=cp.ctypes.data, dst_cap_all=0, src_len_all=0, result=res.ctypes.data, n_blocks=len(plains))
    with wave_only():
        _lib.check(_lib.lib().lz4hip_encode_batch_dict_host(C.byref(b), dic.ctypes.data, dic.size))
    for i, p in enumerate(plains):
        assert (int(res[i]), bytes(dst[i, :res[i]])) == want[i], i
        assert (dst[i, res[i]:] == cases.HOLE).all(), i
        _decodes(dic, p, bytes(dst[i, :res[i]]))
    # no dictionary: the plain host call's results and bytes
    plain_res, plain_dst = gpu.encode([np.frombuffer(p, np.uint8) for p in plains], list(cp))
    dst[:] = cases.HOLE
    _lib.check(_lib.lib().lz4hip_encode_batch_dict_host(C.byref(b), None, 0))
    assert list(res) == list(plain_res) and all(np.array_equal(dst[i, :res[i]], plain_dst[i, :res[i]]) for i in range(len(plains)))
    assert sum(int(r) for r in plain_res) > sum(r for r, _ in want)                    # (the dictionary pays)


def test_fixture_through_the_python_fronts(gpu, fixture):
    import torch
    from lz4net_amd import batch
    from lz4net_amd.codec import LZ4Codec
    dic, plains, want = fixture
    src_h, sl_h = gpu.pack([np.frombuffer(p, np.uint8) for p in plains])
    src, sl = torch.from_numpy(src_h).cuda(), torch.from_numpy(sl_h).cuda()
    comp = torch.full((len(plains), ref.bound(4096) + 64), cases.HOLE, dtype=torch.uint8, device="cuda")
    with wave_only():
        clen = batch.encode_dict(src, sl, comp, ref.bound(4096), _dict_tensor(dic, 3))
        torch.cuda.synchronize()
    out = comp.cpu().numpy()
    for i, p in enumerate(plains):
        assert (int(clen[i]), bytes(out[i, :int(clen[i])])) == want[i] and (out[i, int(clen[i]):] == cases.HOLE).all(), i
    blocks = LZ4Codec.encode_many_with_dictionary(plains, dic)
    assert blocks == [b for _, b in want]
    for p, blk in zip(plains, blocks):
        _decodes(dic, p, blk)
    assert LZ4Codec.decode_many_with_dictionary(blocks, dic, out_sizes=[len(p) for p in plains]) == plains
    assert LZ4Codec.encode_many_with_dictionary(plains[:3], dic.tobytes()) == blocks[:3]


def test_twenty_thousand_blocks_in_one_call(gpu, fixture):
    """the records tiled to 20 000 blocks -- several residency rounds, workgroups of five -- in ONE device call: the wavefront mapping
    alone, and every block is its first copy's bytes, which are the twin's"""
    import torch
    from lz4net_amd import batch
    dic, plains, want = fixture
    n, m = 20000, len(plains)
    src_h, sl_h = gpu.pack([np.frombuffer(p, np.uint8) for p in plains])
    pick = torch.arange(n, device="cuda") % m
    src, sl = torch.from_numpy(src_h).cuda()[pick].contiguous(), torch.from_numpy(sl_h).cuda()[pick].contiguous()
    stride = ref.bound(4096) + 16
    comp = torch.full((n, stride), cases.HOLE, dtype=torch.uint8, device="cuda")
    with wave_only():
        clen = batch.encode_dict(src, sl, comp, ref.bound(4096), _dict_tensor(dic, 1))
        torch.cuda.synchronize()
    assert torch.equal(clen, clen[:m][pick]) and torch.equal(comp, comp[:m][pick])
    first = comp[:m].cpu().numpy()
    for i in range(m):
        assert (int(clen[i]), bytes(first[i, :int(clen[i])])) == want[i] and (first[i, int(clen[i]):] == cases.HOLE).all(), i
