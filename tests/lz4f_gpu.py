"""What the -m gpu tests of LZ4 frames share (tests/test_gpu_lz4f*.py): the device decode calls of include/lz4hip.h on one frame and on a
batch -- the plain entry points, or their _dict_ forms where a dictionary is given -- into an output filled with 0xA7 that starts at the
very start of its allocation and has PAD bytes behind dst_cap, and the batch call checked against the twin with the comparisons of
tests/lz4f_cases.py.  torch is imported inside the functions, so that the files are collected on a machine without a device."""
import ctypes as C

import numpy as np

from gpu_helpers import FILL as DICT_FILL, GUARD as DICT_GUARD, dev, guarded, host, i64, s0
from lz4f_cases import ACCEPT, BATCH_FIELDS, check_call, expect, items_of, records_of
from lz4net_amd import _lib

FILL, PAD = 0xA7, 64


def dev_bytes(b):
    import torch
    return dev(b) if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


class DeviceDict:
    """the dictionary between guard bytes on the device, at an even (odd = 0) or odd address"""
    def __init__(self, d, odd=0):
        import torch
        self.raw = guarded(len(d) + 1)
        self.at, self.n = DICT_GUARD + odd, len(d)
        self.raw[self.at:self.at + self.n] = torch.from_numpy(np.frombuffer(bytes(d), np.uint8).copy()).cuda()
        self.tensor = self.raw[self.at:self.at + self.n]
        self.ptr = self.raw.data_ptr() + self.at

    def intact(self):
        raw, end = host(self.raw), self.at + self.n
        return raw[:self.at] == bytes([DICT_FILL]) * self.at and raw[end:] == bytes([DICT_FILL]) * (len(raw) - end)


def _dict_args(dd, dict_id, dict_call):
    """the dictionary's arguments of a _dict_ entry point, or None for the plain entry point: the _dict_ one is called where a
    dictionary is given, or (dict_call) with a NULL dictionary of no bytes"""
    if dd is None and not dict_call:
        return None
    return [dd.ptr if dd else None, dd.n if dd else 0, dict_id]


def batch_call(frames, slot=65536, max_blocks=64, round_blocks=0, flags=3 | ACCEPT, cap=0, dd=None, dict_id=0, dict_call=False, off=None):
    """lz4hip_lz4f_batch_decode_device, or lz4hip_lz4f_batch_decode_dict_device with the DeviceDict dd, on the items `frames` (with off:
    on the items [off[i], off[i + 1]) of the buffer `frames`) -> (batch record, item records, dst_off, cap + PAD bytes of dst,
    written_items)"""
    import torch
    L = _lib.lib()
    blob, off, _ = items_of(frames, off)
    n = len(off) - 1
    t, o = dev_bytes(blob), i64(off)
    need = L.lz4hip_lz4f_batch_decode_scratch_bytes(n, slot, max_blocks, round_blocks)
    assert need > 0
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((cap + PAD,), FILL, dtype=torch.uint8, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    recs_dev = torch.zeros(C.sizeof(_lib.Lz4fInfo) * max(n, 1), dtype=torch.uint8, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.Lz4fBatchInfo), dtype=torch.uint8, device="cuda")
    written = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    dict_args = _dict_args(dd, dict_id, dict_call)
    entry = L.lz4hip_lz4f_batch_decode_device if dict_args is None else L.lz4hip_lz4f_batch_decode_dict_device
    rc = entry(t.data_ptr(), len(blob), o.data_ptr(), n, *(dict_args or []), slot, max_blocks, round_blocks, flags, scratch.data_ptr(), need, out.data_ptr(), cap,
               out_off.data_ptr(), recs_dev.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s0())
    assert rc == 0, L.lz4hip_last_error()
    info = _lib.Lz4fBatchInfo.from_buffer_copy(host(info_dev))
    assert dd is None or dd.intact()
    return ({f: int(getattr(info, f)) for f in BATCH_FIELDS}, records_of(host(recs_dev)[:C.sizeof(_lib.Lz4fInfo) * n], n), out_off.cpu().numpy(),
            out.cpu().numpy(), int(written.item()))


def frame_call(frame, slot, flags, cap, max_blocks=16, round_blocks=0, dd=None, dict_id=0, dict_call=False):
    """lz4hip_lz4f_decode_device, or lz4hip_lz4f_decode_dict_device with the DeviceDict dd -> (record, cap + PAD bytes of dst)"""
    import torch
    L = _lib.lib()
    t = dev_bytes(frame)
    need = L.lz4hip_lz4f_decode_scratch_bytes(slot, max_blocks, round_blocks)
    assert need > 0
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((cap + PAD,), FILL, dtype=torch.uint8, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.Lz4fInfo), dtype=torch.uint8, device="cuda")
    dict_args = _dict_args(dd, dict_id, dict_call)
    entry = L.lz4hip_lz4f_decode_device if dict_args is None else L.lz4hip_lz4f_decode_dict_device
    rc = entry(t.data_ptr(), t.numel(), *(dict_args or []), slot, max_blocks, round_blocks, flags, scratch.data_ptr(), need, out.data_ptr(), cap,
               info_dev.data_ptr(), s0())
    assert rc == 0, L.lz4hip_last_error()
    assert dd is None or dd.intact()
    return records_of(host(info_dev), 1)[0], out.cpu().numpy()


def check_batch(codec, frames, d=b"", dict_id=0, slot=65536, round_blocks=0, verify=3, dst_cap=None, odd=0):
    """the device call with the flag (with a dictionary d: the _dict_ call) against the twin: the batch's record, dst_off, every record
    field by field, the image of dst, written_items -> (records, batch record)"""
    frames = list(frames)
    want = expect(codec, frames, slot, verify, dst_cap, 1 << 30, True, d, dict_id)
    recs, _, rows, _, cap = want
    got = batch_call(frames, slot, max(len(rows), 1) + 3, round_blocks, verify | ACCEPT, cap, DeviceDict(d, odd) if d else None, dict_id)
    check_call(got, want, FILL)
    return recs, got[0]
