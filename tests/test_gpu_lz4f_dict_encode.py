"""GPU: LZ4 frames encoded against a dictionary on the device (lz4hip_lz4f_encode_dict_* and lz4hip_lz4f_batch_encode_dict_* of
include/lz4hip.h, dictionary=... on the Python encoders of lz4net_amd/lz4_frame.py), byte for byte against the twin
tests/lz4f_dict_encode_ref.py, and every frame decoded again by lz4hip_lz4f_batch_decode_dict_device with the same dictionary and ID.
Every output buffer is filled with 0xA7 first and has PAD bytes behind its bound, and what the call was not to write is still 0xA7
afterwards; the dictionary lies between guard bytes, at an even or an odd address."""
import ctypes as C

import numpy as np
import pytest

import lz4f_dict_encode_ref as twin
import lz4f_ref as ref
from gpu_helpers import dev, host, i64, s0
from lz4f_cases import offsets_of
from lz4f_gpu import FILL, PAD, DeviceDict, batch_call, dev_bytes
from lz4net_amd import _lib, lz4_frame as lz
from lz4net_amd.codec import ArgumentException

pytestmark = pytest.mark.gpu


def encode_one(src, dd, dict_id=0, block_id=4, flags=0, host_call=False, d=b""):
    """lz4hip_lz4f_encode_dict_device with the DeviceDict dd (None: a NULL dictionary of no bytes), or _host with the bytes d -> the frame"""
    import torch
    L = _lib.lib()
    dict_len = len(d) if host_call else (dd.n if dd else 0)
    bound = L.lz4hip_lz4f_dict_bound(len(src), block_id, flags, dict_len, dict_id)
    assert bound > 0
    if host_call:
        out, n, dh = np.full(bound + PAD, FILL, np.uint8), C.c_int64(-1), np.frombuffer(d, np.uint8)
        assert L.lz4hip_lz4f_encode_dict_host(src, len(src), dh.ctypes.data if d else None, len(d), dict_id, block_id, flags, out.ctypes.data, bound,
                                              C.byref(n)) == 0, L.lz4hip_last_error()
        n = n.value
    else:
        t = dev_bytes(src)
        need = L.lz4hip_lz4f_encode_dict_scratch_bytes(len(src), block_id, dict_len)
        assert need > 0
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        out_dev = torch.full((bound + PAD,), FILL, dtype=torch.uint8, device="cuda")
        out_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        assert L.lz4hip_lz4f_encode_dict_device(t.data_ptr(), len(src), dd.ptr if dd else None, dict_len, dict_id, block_id, flags, out_dev.data_ptr(), bound,
                                                out_len.data_ptr(), scratch.data_ptr(), need, s0()) == 0, L.lz4hip_last_error()
        out, n = out_dev.cpu().numpy(), int(out_len.item())
        assert dd is None or dd.intact()
    assert 0 < n <= bound and (out[n:] == FILL).all(), "bytes at or past the reported length were written"
    return out[:n].tobytes()


def encode_batch(src, off, dd, dict_id=0, block_id=4, flags=0, plain=False):
    """lz4hip_lz4f_batch_encode_dict_device (plain: lz4hip_lz4f_batch_encode_device in fast mode) -> (dst_off, the bytes [0, dst_off[n]))"""
    import torch
    L = _lib.lib()
    n, dict_len = len(off) - 1, dd.n if dd else 0
    t, o = dev_bytes(src), i64(off)
    bound = L.lz4hip_lz4f_batch_bound(n, len(src), block_id, flags) if plain else L.lz4hip_lz4f_batch_dict_bound(n, len(src), block_id, flags, dict_len, dict_id)
    need = L.lz4hip_lz4f_batch_encode_scratch_bytes(n, len(src), block_id) if plain else L.lz4hip_lz4f_batch_encode_dict_scratch_bytes(n, len(src), block_id, dict_len)
    assert bound > 0 and need > 0
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((bound + PAD,), FILL, dtype=torch.uint8, device="cuda")
    out_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    if plain:
        rc = L.lz4hip_lz4f_batch_encode_device(t.data_ptr(), len(src), o.data_ptr(), n, block_id, _lib.MODE_FAST, flags, out.data_ptr(), bound, out_off.data_ptr(),
                                               scratch.data_ptr(), need, s0())
    else:
        rc = L.lz4hip_lz4f_batch_encode_dict_device(t.data_ptr(), len(src), o.data_ptr(), n, dd.ptr if dd else None, dict_len, dict_id, block_id, flags,
                                                    out.data_ptr(), bound, out_off.data_ptr(), scratch.data_ptr(), need, s0())
    assert rc == 0, L.lz4hip_last_error()
    ends, got = out_off.cpu().numpy(), out.cpu().numpy()
    assert dd is None or dd.intact()
    assert 0 <= ends[-1] <= bound and (got[int(ends[-1]):] == FILL).all(), "bytes at or past the reported length were written"
    return ends, got[:int(ends[-1])].tobytes()


def check_decodes(frames, sources, dd, dict_id, slot=65536):
    """every frame through lz4hip_lz4f_batch_decode_dict_device with the same dictionary and ID"""
    total = sum(len(s) for s in sources)
    rows = sum(max(len(ref.cut(s, 4 if slot == 65536 else 5)), 1) for s in sources)
    got, recs, off, dst, written = batch_call(frames, slot, rows + 3, 0, 3, total, dd, dict_id)
    assert got["error"] == ref.OK and got["decoded_bytes"] == total and written == len(frames) and list(off) == list(offsets_of(sources))
    assert dst[:total].tobytes() == b"".join(sources) and (dst[total:] == FILL).all()


@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("n", [13, 4097, 65535, 70000])
def test_frames_against_every_dictionary(n, odd):
    d, dd = twin.dictionary(n), DeviceDict(twin.dictionary(n), odd)
    sizes = (0, 13, 300, 65537) + ((150000,) if (n, odd) in ((4097, 1), (70000, 0)) else ())
    frames, sources = [], []
    for k, size in enumerate(sizes):
        src, dict_id = twin.source(size, n), twin.DICT_IDS[(k + odd) % 3]
        frame = encode_one(src, dd, dict_id)
        assert frame == twin.write_frame_dict(src, d, dict_id)[0], (size, dict_id)
        if (k + odd) & 1:
            assert encode_one(src, None, dict_id, host_call=True, d=d) == frame
        if dict_id == 7:
            frames.append(frame)
            sources.append(src)
    check_decodes(frames, sources, dd, 7)


def test_a_block_above_64_kib_all_flags_and_the_three_ids():
    d, dd = twin.dictionary(70000), DeviceDict(twin.dictionary(70000), 1)
    src = twin.source(twin.BIG, 70000)
    frame = encode_one(src, dd, 0xFFFFFFFF, block_id=5, flags=7)
    assert frame == twin.write_frame_dict(src, d, 0xFFFFFFFF, 5, 7)[0] and len(frame) < twin.BIG // 2
    check_decodes([frame], [src], dd, 0xFFFFFFFF, slot=262144)
    src = twin.source(65537, 70000)
    for flags in range(8):
        dict_id = twin.DICT_IDS[flags % 3]
        frame = encode_one(src, dd, dict_id, flags=flags, host_call=bool(flags & 1), d=d)
        assert frame == twin.write_frame_dict(src, d, dict_id, 4, flags)[0], flags
        check_decodes([frame], [src], dd, dict_id)


def test_a_source_that_only_the_dictionary_compresses():
    d, src = twin.only_with_the_dictionary()
    dd = DeviceDict(d, 1)
    want, rets = twin.write_frame_dict(src, d)
    assert rets == [10]
    for host_call in (False, True):
        assert encode_one(src, dd, host_call=host_call, d=d) == want and len(want) == 7 + 4 + 10 + 4
        without = encode_one(src, None, host_call=host_call)
        assert without[7:11] == ref.le32(200 | 0x80000000) and without[11:211] == src and len(without) == 7 + 4 + 200 + 4
    check_decodes([want], [src], dd, 0)
    t = dev(src)
    assert host(lz.compress_frame_device(t, content_size=False, dictionary=dd.tensor)) == want
    assert len(lz.compress_frame_device(t, content_size=False)) == 215
    assert lz.compress_frame_host(src, content_size=False, dictionary=d) == want
    assert lz.decompress_frame_host(want, dictionary=d) == src


def mixed(n):
    items = [twin.source(size, n) for size in twin.SOURCE_LENGTHS] + [b"", twin.noise(200)]
    src, off = b"".join(items), list(offsets_of(items))
    off = off[:4] + [off[4], off[3]] + off[4:]                            # an item [off[4], off[3]): its offsets decrease, it takes no bytes
    return src, off, [src[a:b] if a <= b else None for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("n,odd", [(4097, 1), (70000, 0)])
def test_the_mixed_batch(n, odd):
    d, dd = twin.dictionary(n), DeviceDict(twin.dictionary(n), odd)
    flags = ref.F_CONTENT_SIZE | ref.F_BLOCK_CHECKSUM
    src, off, spans = mixed(n)
    frames = [b"" if s is None else twin.write_frame_dict(s, d, 7, 4, flags)[0] for s in spans]
    before = _lib.dispatch_counts()
    ends, got = encode_batch(src, off, dd, 7, 4, flags)
    after = _lib.dispatch_counts()
    assert [k for k in range(_lib.K_COUNT) if after[k] != before[k]] == [_lib.K_ENCODE_WAVE] and after[_lib.K_ENCODE_WAVE] == before[_lib.K_ENCODE_WAVE] + 1
    assert list(ends) == list(offsets_of(frames)) and got == b"".join(frames)
    kept = [(f, s) for f, s in zip(frames, spans) if s is not None]
    check_decodes([f for f, _ in kept], [s for _, s in kept], dd, 7)


@pytest.mark.parametrize("wg5", [1, 2])
def test_a_batch_of_1030_small_items_in_both_workgroup_shapes(wg5):
    """one block, then five blocks per workgroup (the knob forces each): 1 034 table rows, so the last group of five is ragged"""
    d, dd = twin.dictionary(4097), DeviceDict(twin.dictionary(4097), 1)
    kinds = [twin.source(300 * 8, 4097)[300 * k:300 * (k + 1)] for k in range(8)]
    items = [kinds[(k * 5 + k // 8) % 8] for k in range(1030)]
    frames = [twin.write_frame_dict(s, d, 7, 4, ref.F_CONTENT_SIZE)[0] for s in items]
    before = _lib.dispatch_counts()
    with _lib.tuning(encoder_wg5=wg5):
        ends, got = encode_batch(b"".join(items), offsets_of(items), dd, 7, 4, ref.F_CONTENT_SIZE)
    after = _lib.dispatch_counts()
    assert [k for k in range(_lib.K_COUNT) if after[k] != before[k]] == [_lib.K_ENCODE_WAVE]
    assert list(ends) == list(offsets_of(frames)) and got == b"".join(frames)
    check_decodes(frames, items, dd, 7)


def test_without_a_dictionary_the_call_is_the_plain_call():
    src, off, _ = mixed(4097)
    for flags in (0, 7):
        plain = encode_batch(src, off, None, flags=flags, plain=True)
        none = encode_batch(src, off, None, 99, flags=flags)
        assert list(plain[0]) == list(none[0]) and plain[1] == none[1]
    one = twin.source(65537)
    assert encode_one(one, None, 99, flags=7) == host(lz.compress_frame_device(dev(one), block_checksum=True, content_checksum=True))
    assert encode_one(one, None, 99, flags=7, host_call=True) == lz.compress_frame_host(one, block_checksum=True, content_checksum=True)


def test_the_python_calls():
    d, dd = twin.dictionary(4097), DeviceDict(twin.dictionary(4097), 1)
    items = [twin.source(size) for size in (300, 0, 65537, 13)]
    src, off = b"".join(items), offsets_of(items)
    frames = [twin.write_frame_dict(s, d, 7, 4, ref.F_CONTENT_SIZE | ref.F_CONTENT_CHECKSUM)[0] for s in items]
    for s, f in zip(items, frames):
        assert host(lz.compress_frame_device(dev_bytes(s), content_checksum=True, dictionary=dd.tensor, dict_id=7)) == f
        assert lz.compress_frame_host(s, content_checksum=True, dictionary=d, dict_id=7) == f
        assert lz.decompress_frame_host(f, dictionary=d, dict_id=7) == s
    out, out_off = lz.compress_frames_device(dev(src), i64(off), content_checksum=True, dictionary=dd.tensor, dict_id=7)
    assert host(out) == b"".join(frames) and list(out_off.cpu().numpy()) == list(offsets_of(frames))
    data, data_off = lz.decompress_frames_device(out, out_off, dictionary=dd.tensor, dict_id=7)
    assert host(data) == src and list(data_off.cpu().numpy()) == list(off)
    out, out_off = lz.compress_frames_host(src, off, content_checksum=True, dictionary=d, dict_id=7)
    assert out.tobytes() == b"".join(frames) and list(out_off) == list(offsets_of(frames))
    big = lz.compress_frame_host(twin.source(twin.BIG, 70000), block_size=262144, dictionary=twin.dictionary(70000))
    assert big == twin.write_frame_dict(twin.source(twin.BIG, 70000), twin.dictionary(70000), 0, 5, ref.F_CONTENT_SIZE)[0]
    assert dd.intact()
    for call in (lambda: lz.compress_frame_device(dev(src), high_compression=True, dictionary=dd.tensor),
                 lambda: lz.compress_frames_device(dev(src), i64(off), high_compression=True, dictionary=dd.tensor),
                 lambda: lz.compress_frame_host(src, high_compression=True, dictionary=d),
                 lambda: lz.compress_frames_host(src, off, high_compression=True, dictionary=d)):
        with pytest.raises(ArgumentException, match="high_compression with a dictionary"):
            call()
    assert lz.compress_frame_host(items[0], high_compression=True, dictionary=b"") == lz.compress_frame_host(items[0], high_compression=True)
