"""CPU-only, no emulator: the fronts of the batch of LZ4 frames (lz4hip_lz4f_batch_* of include/lz4hip.h and the Python calls of
lz4net_amd/lz4_frame.py over them) refuse bad arguments before a device is looked for -- LZ4HIP_E_ARGUMENT, not LZ4HIP_E_DEVICE, on a
machine without one -- and lz4hip_lz4f_batch_bound covers the frames of every partition of a buffer into items."""
import ctypes as C

import numpy as np
import pytest

from lz4net_amd import _lib, lz4_frame as lz
from lz4net_amd.codec import ArgumentException

E_ARGUMENT = _lib.E_ARGUMENT


def test_the_c_fronts_check_their_arguments_first():
    L = _lib.lib()
    a, off, dst, doff, scratch = np.zeros(64, np.uint8), np.array([0, 10, 20], np.int64), np.zeros(512, np.uint8), np.zeros(3, np.int64), np.zeros(1 << 20, np.uint8)
    assert L.lz4hip_lz4f_batch_encode_scratch_bytes(2, 20, 4) <= scratch.size and L.lz4hip_lz4f_batch_encode_scratch_bytes(2, 20, 3) == E_ARGUMENT
    assert L.lz4hip_lz4f_batch_encode_scratch_bytes(0, 20, 4) == 0
    assert L.lz4hip_lz4f_batch_bound(2, 20, 4, 0) <= dst.size
    enc_ok = ok = [a.ctypes.data, 20, off.ctypes.data, 2, 4, 0, 0, dst.ctypes.data, 512, doff.ctypes.data, scratch.ctypes.data, scratch.size, None]
    for at, bad in ((0, None), (1, -1), (2, None), (3, -1), (4, 3), (4, 8), (5, 2), (6, 8), (7, None), (8, 10), (9, None), (10, None), (11, 16)):
        args = list(ok)
        args[at] = bad
        assert L.lz4hip_lz4f_batch_encode_device(*args) == E_ARGUMENT, at
    assert b"lz4f batch encode" in L.lz4hip_last_error()
    recs, info, written = (_lib.Lz4fInfo * 2)(), _lib.Lz4fBatchInfo(), np.zeros(1, np.int64)
    assert 0 < L.lz4hip_lz4f_batch_decode_scratch_bytes(2, 65536, 4, 0) <= scratch.size
    for bad in ((-1, 65536, 4, 0), (2, 65535, 4, 0), (2, 65536, 0, 0), (2, 65536, 4, -1)):
        assert L.lz4hip_lz4f_batch_decode_scratch_bytes(*bad) == E_ARGUMENT, bad
    ok = [a.ctypes.data, 20, off.ctypes.data, 2, 65536, 4, 0, 3, scratch.ctypes.data, scratch.size, dst.ctypes.data, 64, doff.ctypes.data, recs, C.byref(info),
          written.ctypes.data, None]
    for at, bad in ((0, None), (1, -1), (2, None), (3, -1), (4, 1000), (5, 0), (6, -1), (7, 4), (8, None), (9, 100), (10, None), (11, -1), (12, None), (13, None),
                    (14, None), (15, None)):
        args = list(ok)
        args[at] = bad
        assert L.lz4hip_lz4f_batch_decode_device(*args) == E_ARGUMENT, at
    assert b"lz4f batch decode" in L.lz4hip_last_error()
    if L.lz4hip_device_count() == 0:                                   # sound arguments get as far as the device
        assert L.lz4hip_lz4f_batch_encode_device(*enc_ok) == _lib.E_DEVICE
        assert L.lz4hip_lz4f_batch_decode_device(*ok) == _lib.E_DEVICE


def test_the_python_fronts_check_their_arguments_first():
    buf, off = np.zeros(64, np.uint8), np.array([0, 10, 20], np.int64)
    for call in (lz.compress_frames_device, lz.decompress_frames_device):
        with pytest.raises(ArgumentException, match="CUDA tensor"):
            call(buf, off)
    for call in (lz.compress_frames_host, lz.decompress_frames_host):
        with pytest.raises(ArgumentException, match="int64"):
            call(buf, off.astype(np.int32))
        with pytest.raises(ArgumentException, match="uint8"):
            call(buf.astype(np.int16), off)
        with pytest.raises(ArgumentException, match="n \\+ 1"):
            call(buf, off[:0])
        for wrong in ([0, 10, 5], [-1, 10, 20], [0, 10, 65]):
            with pytest.raises(ArgumentException, match="offsets are invalid"):
                call(buf, np.array(wrong, np.int64))
    with pytest.raises(ArgumentException, match="block_size"):
        lz.compress_frames_host(buf, off, block_size=1000)


@pytest.mark.parametrize("block_id", [0, 4, 5, 6, 7])
def test_the_bound_covers_every_partition(block_id):
    L = _lib.lib()
    rng = np.random.default_rng(block_id)
    block = 1 << (8 + 2 * (block_id or 4))
    for flags in range(8):
        for total in (0, 1, block - 1, block, block + 1, 5 * block + 7, int(rng.integers(0, 8 * block))):
            for n in (1, 2, 3, 17, 400):
                cuts = np.sort(rng.integers(0, total + 1, n - 1))
                for cuts in (cuts, np.zeros(n - 1, np.int64), np.full(n - 1, total), (np.arange(1, n) * block).clip(0, total)):
                    lens = np.diff(np.concatenate([[0], cuts, [total]]))
                    assert lens.sum() == total and (lens >= 0).all()
                    alone = sum(L.lz4hip_lz4f_bound(int(k), block_id, flags) for k in lens)
                    assert alone <= L.lz4hip_lz4f_batch_bound(n, total, block_id, flags), (flags, total, n)
    assert L.lz4hip_lz4f_batch_bound(3, 10, 3, 0) == E_ARGUMENT and L.lz4hip_lz4f_batch_bound(3, 10, 4, 8) == E_ARGUMENT
    assert L.lz4hip_lz4f_batch_bound(0, 0, 4, 7) == 0
