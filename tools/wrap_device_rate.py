"""Device-resident Wrap / Unwrap batches (lz4hip_wrap_device, lz4hip_unwrap_index_device + lz4hip_unwrap_decode_device) over 1 GiB of D2
data, with event timings; meant to run under `rocprofv3 --kernel-trace --stats` too, whose per-kernel totals split the calls into their
kernels.

Cases: 16 384 x 64 KiB, 1 048 576 x 1 KiB and 1 024 x 1 MiB messages (fast).  Each is wrapped and unwrapped, and timed against
lz4hip_encode_batch_device (outputLength = inputLength, as Wrap runs it) and lz4hip_decode_batch_device (known size, on the compressed
payloads inside the wrapped buffer) on the same blocks with their offsets known in advance.  framing_share_* is the part of the wrap /
unwrap time that is not the batch codec's.  Every unwrap is checked against the source.

    python tools/wrap_device_rate.py [reps] [out.json]
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lz4net_amd import _lib, batch  # noqa: E402
from lz4net_amd import wrap as wr  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_json = sys.argv[2] if len(sys.argv) > 2 else None
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream
TOTAL = 1 << 30
src = batch.synth(2, 7, 0, TOTAL // batch.BLOCK).reshape(-1)
torch.cuda.synchronize()


def timed(fn, n=reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def batch_of(src_t, src_off, src_len, dst_t, dst_off, dst_cap, res, n):
    return _lib.Batch(src=src_t.data_ptr(), src_off=src_off.data_ptr(), src_stride=0, src_len=src_len.data_ptr(), dst=dst_t.data_ptr(),
                      dst_off=dst_off.data_ptr(), dst_stride=0, dst_cap=dst_cap.data_ptr(), dst_cap_all=0, src_len_all=0,
                      result=res.data_ptr(), n_blocks=n)


results = {}
for M in (1 << 16, 1 << 10, 1 << 20):
    n = TOTAL // M
    r = results[f"{n}x{M // 1024}KiB"] = {"messages": n}
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * M

    # wrap
    bound = L.lz4hip_wrap_bound(n, TOTAL)
    packed = torch.empty(bound, dtype=torch.uint8, device="cuda")
    poff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    result = torch.empty(n, dtype=torch.int32, device="cuda")
    scratch = torch.empty(L.lz4hip_wrap_scratch_bytes(n, TOTAL), dtype=torch.uint8, device="cuda")

    def wrap():
        _lib.check(L.lz4hip_wrap_device(src.data_ptr(), TOTAL, offs.data_ptr(), n, 0, packed.data_ptr(), bound, poff.data_ptr(),
                                        result.data_ptr(), scratch.data_ptr(), scratch.numel(), s))
    r["wrap_ms"] = timed(wrap)
    total = int(poff[n])
    r["wrapped_bytes"] = total
    r["compressed_messages"] = int((result > 0).sum())
    r["wrap_end_to_end_ms"] = timed(lambda: wr.wrap_device(src, offs))
    del scratch

    # the same blocks through the batch encoder: outputLength = inputLength, offsets known in advance
    lens = torch.full((n,), M, dtype=torch.int32, device="cuda")
    comp = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")
    res = torch.empty(n, dtype=torch.int32, device="cuda")
    be = batch_of(src, offs, lens, comp, offs, lens, res, n)
    r["batch_encode_ms"] = timed(lambda: _lib.check(L.lz4hip_encode_batch_device(C.byref(be), 0, s)))
    assert torch.equal(torch.where((res > 0) & (res < M), res, 0), result), "wrap results != batch encode results"
    r["framing_share_wrap"] = 1 - r["batch_encode_ms"] / r["wrap_ms"]
    del comp

    # unwrap: index, one read-back, decode
    packed_t = packed[:total]
    out = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")
    doff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    uscratch = torch.empty(L.lz4hip_unwrap_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device="cuda")

    def index():
        _lib.check(L.lz4hip_unwrap_index_device(packed_t.data_ptr(), total, poff.data_ptr(), n, doff.data_ptr(), status.data_ptr(),
                                                uscratch.data_ptr(), uscratch.numel(), info_dev.data_ptr(), s))
    r["unwrap_index_ms"] = timed(index)
    info = _lib.UnwrapInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    assert info.first_error == -1 and info.decoded_bytes == TOTAL, (info.first_error, info.decoded_bytes)

    def decode():
        _lib.check(L.lz4hip_unwrap_decode_device(packed_t.data_ptr(), total, poff.data_ptr(), n, C.byref(info), uscratch.data_ptr(),
                                                 uscratch.numel(), out.data_ptr(), TOTAL, doff.data_ptr(), status.data_ptr(),
                                                 info_dev.data_ptr(), s))
    r["unwrap_decode_ms"] = timed(decode)
    done = _lib.UnwrapInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    assert done.first_error == -1 and torch.equal(out, src) and torch.equal(doff, offs), "unwrap"
    r["unwrap_ms"] = r["unwrap_index_ms"] + r["unwrap_decode_ms"]
    r["unwrap_end_to_end_ms"] = timed(lambda: wr.unwrap_device(packed_t, poff))
    del uscratch

    # the compressed payloads through the batch decoder, offsets known in advance
    hdr = packed_t[(poff[:-1, None] + torch.arange(8, device="cuda")).reshape(-1)].reshape(n, 8).contiguous()
    olen, plen = hdr[:, :4].view(torch.int32).reshape(-1), hdr[:, 4:].view(torch.int32).reshape(-1)
    cm = plen < olen
    nc = int(cm.sum())
    so, sl, do, dc = (poff[:-1] + 8)[cm].contiguous(), plen[cm].contiguous(), offs[:-1][cm].contiguous(), olen[cm].contiguous()
    bres = torch.empty(max(nc, 1), dtype=torch.int32, device="cuda")
    out.zero_()
    bd = batch_of(packed_t, so, sl, out, do, dc, bres, nc)
    r["batch_decode_ms"] = timed(lambda: _lib.check(L.lz4hip_decode_batch_device(C.byref(bd), 1, s)))
    assert bool((bres[:nc] == sl).all()) and (nc < n or torch.equal(out, src)), "batch decode"
    r["framing_share_unwrap"] = 1 - r["batch_decode_ms"] / r["unwrap_ms"]
    r["unwrap_over_batch_decode"] = r["unwrap_ms"] / r["batch_decode_ms"]
    del out, packed, packed_t
    torch.cuda.synchronize()
    print(json.dumps({k: v for k, v in results.items()}), flush=True)

if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(results, fh, indent=1)
