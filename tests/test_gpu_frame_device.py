"""GPU: whole legacy frames (original/lz4demo.c) encoded and decoded on the device in one call (lz4hip_frame_* of include/lz4hip.h):
byte parity with the existing host path (legacy_frame.compress_frame) and with the frames the reference's CLI wrote
(tests/golden/ref_records.json), round trips, corruption, stream order and the host-pointer calls."""
import ctypes as C

import numpy as np
import pytest

import ref_records as rr
from gpu_helpers import dev, host
from lz4net_amd import _lib, legacy_frame as lf

pytestmark = pytest.mark.gpu

FRAMES = rr.load()["frames"]
MAGIC = lf.MAGIC.to_bytes(4, "little")


@pytest.mark.parametrize("hc", [False, True])
def test_parity_with_the_host_path_and_the_cli(oracle, hc):
    for n_bytes, dist, _ in [c for c in rr.FRAME_INTEROP_CASES if c[2] == hc]:
        data = rr.frame_sample(oracle, n_bytes, dist)
        rec = FRAMES[rr.frame_key(n_bytes, dist, hc)]
        ours = host(lf.compress_frame_device(dev(data), high_compression=hc))
        assert ours == lf.compress_frame(data, high_compression=hc), n_bytes
        assert (len(ours), rr.sha(ours)) == (rec["len"], rec["sha"]), "not the reference CLI's frame"
        assert len(lf.parse_frame(ours)) == (n_bytes + lf.CHUNK_SIZE - 1) // lf.CHUNK_SIZE
        assert host(lf.decompress_frame_device(dev(ours))) == data
        assert host(lf.decompress_frame_device(dev(ours + ours))) == data + data


def test_small_chunks(oracle):
    data = rr.frame_sample(oracle, 500000, 2)
    for chunk in (4096, 65536, 100000):
        frame = host(lf.compress_frame_device(dev(data), chunk_size=chunk))
        assert frame == lf.compress_frame(data, chunk_size=chunk)
        assert host(lf.decompress_frame_device(dev(frame), chunk_size=chunk)) == data
    # a frame read with a larger chunk_size than it was written with: more chunks than the first table holds
    frame = lf.compress_frame(data[:100000], chunk_size=1024)
    assert host(lf.decompress_frame_device(dev(frame))) == data[:100000]


def test_empty_source_and_empty_chunks():
    import torch
    frame = lf.compress_frame_device(torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert host(frame) == MAGIC
    assert lf.decompress_frame_device(frame).numel() == 0
    assert lf.decompress_frame_device(dev(MAGIC + bytes(8) + MAGIC)).numel() == 0
    for bad, text in ((b"", "Unrecognized"), (b"abcd", "Unrecognized"), (MAGIC + b"\x01", "truncated chunk header"),
                      (MAGIC + (5).to_bytes(4, "little") + b"abc", "truncated chunk payload"), (MAGIC + b"\xff\xff\xff\x7f", "chunk size")):
        with pytest.raises(lf.ArgumentException, match=text):
            lf.decompress_frame_device(dev(bad))


def frame_calls(frame, chunk_size=0, stream=None, max_chunks=None):
    """index, one read-back, decode through the C calls -> (index info, final info, output tensor)"""
    import torch
    L = _lib.lib()
    t = dev(frame)
    s = 0 if stream is None else stream.cuda_stream
    info_dev = torch.zeros(C.sizeof(_lib.FrameInfo), dtype=torch.uint8, device="cuda")
    m = len(frame) // (chunk_size or lf.CHUNK_SIZE) + 16 if max_chunks is None else max_chunks
    scratch = torch.empty(L.lz4hip_frame_decode_scratch_bytes(m), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_frame_index_device(t.data_ptr(), t.numel(), chunk_size, m, scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(), s) == 0
    first = _lib.FrameInfo.from_buffer_copy(host(info_dev))
    out = torch.full((int(first.decoded_bytes) + 64,), 0xA7, dtype=torch.uint8, device="cuda")
    assert L.lz4hip_frame_decode_device(t.data_ptr(), C.byref(first), m, scratch.data_ptr(), scratch.numel(), out.data_ptr() + 32,
                                        int(first.decoded_bytes), info_dev.data_ptr(), s) == 0
    final = _lib.FrameInfo.from_buffer_copy(host(info_dev))
    raw = host(out)
    assert raw[:32] == b"\xA7" * 32 and raw[len(raw) - 32:] == b"\xA7" * 32, "bytes outside [0, decoded_bytes) were written"
    return first, final, raw[32:len(raw) - 32]


def test_corruption(oracle):
    data = rr.frame_sample(oracle, 500000, 2)
    bad = bytearray(lf.compress_frame(data[:70000]))
    bad[8] = 0xFF; bad[9] = 0xFF; bad[10] = 0xFF                        # (the corruption of test_frame_small_chunks_roundtrip)
    with pytest.raises(lf.ArgumentException, match="Decoding Failed"):
        lf.decompress_frame_device(dev(bad))
    first, final, _ = frame_calls(bytes(bad))
    assert (final.error, final.error_offset, final.chunks, final.good_bytes) == (_lib.FRAME_CORRUPT_BLOCK, 4, 1, 0)
    # one bad chunk among nine, of each kind: the size walk fails; it walks past chunk_size; it breaks the end rules and the decoder fails it
    chunk = 4096
    a = np.frombuffer(data, np.uint8)
    comps = [bytes(oracle.compress(a[k * chunk:(k + 1) * chunk])) for k in range(9)]
    kinds = {"walk": (b"\xFF\xFF\xFF" + comps[4][3:], 0), "long": (bytes(oracle.compress(a[4 * chunk:5 * chunk + 1])), 0),
             "end": (bytes([0x10, 0x30, 1, 0, 0x50, 1, 2, 3, 4, 5]), 10)}
    for kind, (payload, slot) in kinds.items():
        parts = comps[:4] + [payload] + comps[5:]
        frame = MAGIC + b"".join(len(c).to_bytes(4, "little") + c for c in parts) + b"\x01\x02"       # (and a truncated tail: the block comes first)
        first, final, out = frame_calls(frame, chunk_size=chunk)
        field = 4 + sum(4 + len(c) for c in comps[:4])
        assert first.error == (_lib.FRAME_TRUNCATED if kind == "end" else _lib.FRAME_CORRUPT_BLOCK), kind
        assert (final.chunks, final.decoded_bytes, final.good_bytes, final.error_offset, final.error) == \
            (9, 8 * chunk + slot, 4 * chunk, field, _lib.FRAME_CORRUPT_BLOCK), kind
        assert out[:4 * chunk] == data[:4 * chunk] and out[4 * chunk + slot:] == data[5 * chunk:9 * chunk], kind
        with pytest.raises(lf.ArgumentException, match="Decoding Failed"):
            lf.decompress_frame_host(frame, chunk_size=chunk)


def test_table_full_and_argument_checks(oracle):
    import torch
    L = _lib.lib()
    data = rr.frame_sample(oracle, 100000, 2)
    frame = lf.compress_frame(data, chunk_size=4096)
    n = len(lf.parse_frame(frame))
    t = dev(frame)
    info_dev = torch.zeros(C.sizeof(_lib.FrameInfo), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(L.lz4hip_frame_decode_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_frame_index_device(t.data_ptr(), t.numel(), 4096, n - 1, scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(), None) == 0
    info = _lib.FrameInfo.from_buffer_copy(host(info_dev))
    assert (info.error, info.chunks) == (_lib.FRAME_TABLE_FULL, n)
    out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_frame_decode_device(t.data_ptr(), C.byref(info), n - 1, scratch.data_ptr(), scratch.numel(), out.data_ptr(), out.numel(),
                                        info_dev.data_ptr(), None) == _lib.E_ARGUMENT
    first, final, got = frame_calls(frame, chunk_size=4096, max_chunks=n)
    assert final.error == _lib.FRAME_OK and got == data
    assert L.lz4hip_frame_index_device(t.data_ptr(), t.numel(), -1, n, scratch.data_ptr(), scratch.numel(), info_dev.data_ptr(), None) == _lib.E_ARGUMENT
    assert L.lz4hip_frame_encode_device(t.data_ptr(), t.numel(), 0, 0, out.data_ptr(), 3, info_dev.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                        None) == _lib.E_ARGUMENT


def test_stream_order(oracle):
    """encode, index and decode queued on a non-default stream behind an unrelated kernel; only the info read-back waits"""
    import torch
    L = _lib.lib()
    data = rr.frame_sample(oracle, 300000, 2)
    chunk = 65536
    want = lf.compress_frame(data, chunk_size=chunk)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        busy = torch.randn(2048, 2048, device="cuda")
        src = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
        staged = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).pin_memory()
        for _ in range(4):
            busy = busy @ busy * 1e-3                                 # the unrelated work the calls must queue behind
        src.copy_(staged, non_blocking=True)                           # the source itself arrives in stream order
        bound = L.lz4hip_frame_bound(len(data), chunk)
        frame = torch.empty(bound, dtype=torch.uint8, device="cuda")
        frame_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        scratch = torch.empty(L.lz4hip_frame_encode_scratch_bytes(len(data), chunk), dtype=torch.uint8, device="cuda")
        assert L.lz4hip_frame_encode_device(src.data_ptr(), len(data), chunk, 0, frame.data_ptr(), bound, frame_len.data_ptr(), scratch.data_ptr(),
                                            scratch.numel(), s.cuda_stream) == 0
        # the index reads the frame the encoder has only queued: bound bytes are more than the frame, so its length comes from the host
        m = 16
        table = torch.empty(L.lz4hip_frame_decode_scratch_bytes(m), dtype=torch.uint8, device="cuda")
        info_dev = torch.zeros(C.sizeof(_lib.FrameInfo), dtype=torch.uint8, device="cuda")
        assert L.lz4hip_frame_index_device(frame.data_ptr(), len(want), chunk, m, table.data_ptr(), table.numel(), info_dev.data_ptr(), s.cuda_stream) == 0
        info = _lib.FrameInfo.from_buffer_copy(host(info_dev))          # the one synchronisation
        assert (info.error, info.chunks, info.decoded_bytes) == (_lib.FRAME_OK, 5, len(data))
        out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
        assert L.lz4hip_frame_decode_device(frame.data_ptr(), C.byref(info), m, table.data_ptr(), table.numel(), out.data_ptr(), out.numel(),
                                            info_dev.data_ptr(), s.cuda_stream) == 0
    s.synchronize()
    assert int(frame_len.item()) == len(want) and host(frame[:len(want)]) == want
    assert host(out) == data and _lib.FrameInfo.from_buffer_copy(host(info_dev)).error == _lib.FRAME_OK


def test_host_calls(oracle):
    L = _lib.lib()
    data = rr.frame_sample(oracle, 500000, 2)
    for chunk, hc in ((65536, False), (100000, True), (lf.CHUNK_SIZE, False)):
        frame = lf.compress_frame_host(data, high_compression=hc, chunk_size=chunk)
        assert frame == host(lf.compress_frame_device(dev(data), high_compression=hc, chunk_size=chunk))
        assert lf.decompress_frame_host(frame, chunk_size=chunk) == data
        buf = np.frombuffer(frame, np.uint8)
        info = _lib.FrameInfo()
        assert L.lz4hip_frame_decode_host(buf.ctypes.data, buf.size, chunk, None, 0, C.byref(info)) == _lib.E_ARGUMENT     # the size query
        first, final, _ = frame_calls(frame, chunk_size=chunk)
        assert [(i.chunks, i.decoded_bytes, i.good_bytes, i.error_offset, i.error) for i in (info, first, final)] == \
            [((len(data) + chunk - 1) // chunk, len(data), len(data), -1, _lib.FRAME_OK)] * 3
    assert lf.compress_frame_host(b"") == MAGIC and lf.decompress_frame_host(MAGIC) == b""
    with pytest.raises(lf.ArgumentException, match="Unrecognized"):
        lf.decompress_frame_host(b"nope" + bytes(8))
