"""What the -m gpu tests share: a numpy front-end over the HOST-pointer batch entry points of liblz4hip.so (everything goes through the
C ABI, include/lz4hip.h), and device buffers -- bytes up and down, an output between guard bytes, a forced decoder mapping.  torch is
imported inside the functions, so that the files are collected on a machine without a device."""
import ctypes as C

import numpy as np

from lz4net_amd import _lib


def pack(rows, pad=16):
    n = len(rows)
    stride = max([len(r) for r in rows] + [1]) + pad
    buf = np.zeros((n, stride), np.uint8)
    for i, r in enumerate(rows):
        buf[i, :len(r)] = r
    return buf, np.array([len(r) for r in rows], np.int32)


def _batch(src, sl, dst, caps, res):
    return _lib.Batch(src=src.ctypes.data, src_off=None, src_stride=src.strides[0], src_len=sl.ctypes.data,
                      dst=dst.ctypes.data, dst_off=None, dst_stride=dst.strides[0], dst_cap=caps.ctypes.data,
                      dst_cap_all=0, src_len_all=0, result=res.ctypes.data, n_blocks=src.shape[0])


def encode(blocks, caps=None, hc=False, canary=64, device_mask=None):
    src, sl = pack(blocks)
    if caps is None:
        caps = [len(b) + len(b) // 255 + 16 for b in blocks]
    caps = np.array(caps, np.int32)
    dst = np.full((len(blocks), max(int(caps.max()), 1) + canary), 0xA5, np.uint8)
    res = np.zeros(len(blocks), np.int32)
    b = _batch(src, sl, dst, caps, res)
    if device_mask is None:
        _lib.check(_lib.lib().lz4hip_encode_batch_host(C.byref(b), 1 if hc else 0))
    else:
        _lib.check(_lib.lib().lz4hip_encode_batch_host_multi(C.byref(b), 1 if hc else 0, device_mask))
    return res, dst


def decode(comps, out_sizes, known=True, src_lens=None, canary=64, device_mask=None):
    src, sl = pack(comps)
    if src_lens is not None:
        sl = np.array(src_lens, np.int32)
    caps = np.array(out_sizes, np.int32)
    dst = np.full((len(comps), max(int(caps.max()), 1) + canary), 0xA5, np.uint8)
    res = np.zeros(len(comps), np.int32)
    b = _batch(src, sl, dst, caps, res)
    if device_mask is None:
        _lib.check(_lib.lib().lz4hip_decode_batch_host(C.byref(b), 1 if known else 0))
    else:
        _lib.check(_lib.lib().lz4hip_decode_batch_host_multi(C.byref(b), 1 if known else 0, device_mask))
    return res, dst


# ---- device buffers ------------------------------------------------------------------------------------------------------------------
GUARD, FILL = 64, 0xA5


def dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).cuda()


def host(t):
    return t.cpu().numpy().tobytes()


def i64(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int64, device="cuda")


def synth_bytes(dist, n_bytes, seed):
    from lz4net_amd import batch
    rows = batch.synth(dist, seed, 0, (n_bytes + 4095) // 4096, length=4096)
    return rows.reshape(-1)[:n_bytes]


def s0():
    import torch
    return torch.cuda.current_stream().cuda_stream


def guarded(cap):
    """cap bytes between GUARD bytes of FILL on either side"""
    import torch
    return torch.full((cap + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")


def intact_from(raw, written, dst_cap):
    return raw[:GUARD] == bytes([FILL]) * GUARD and raw[GUARD + written:] == bytes([FILL]) * (dst_cap - written + GUARD)


class mapping_ran:
    """with mapping_ran("lane"): the decoder is forced to that mapping, and lz4hip_dispatch_counts proves that it ran and the other did not"""

    def __init__(self, mapping):
        self.mapping = mapping
        self.knobs = _lib.tuning(decoder="wave") if mapping == "wave" else _lib.tuning(decoder="lane", decoder_groups=1)

    def __enter__(self):
        self.before = _lib.dispatch_counts()
        self.knobs.__enter__()

    def __exit__(self, *exc):
        self.knobs.__exit__(*exc)
        if exc[0] is None:
            after = _lib.dispatch_counts()
            mine, other = (_lib.K_DECODE_WAVE, _lib.K_DECODE_LANE) if self.mapping == "wave" else (_lib.K_DECODE_LANE, _lib.K_DECODE_WAVE)
            assert after[mine] > self.before[mine] and after[other] == self.before[other], self.mapping
        return False
