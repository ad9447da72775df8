"""Device-resident LZ4Stream encode / decode (lz4hip_stream_*_device) over 1 GiB of D2 data, with event timings; meant to run under
`rocprofv3 --kernel-trace --stats` too, whose per-kernel totals split the calls into their kernels.

Cases: stream encode of 16 384 x 64 KiB and 1 024 x 1 MiB chunks (fast); a hipMemcpyAsync device-to-device copy of each encoded stream's
byte count (the pack kernel's yardstick); stream decode (index + decode) of both streams against lz4hip_decode_batch_device on the same
chunks with their offsets known in advance.  Every decode is checked against the source.

    python tools/stream_device_rate.py [reps] [out.json]
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lz4net_amd import _lib, batch  # noqa: E402
from lz4net_amd import stream as st  # noqa: E402

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


results = {}
for B in (1 << 16, 1 << 20):
    r = results[f"{TOTAL // B}x{B // 1024}KiB"] = {}
    bound = L.lz4hip_stream_bound(TOTAL, B)
    enc = torch.empty(bound, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(L.lz4hip_stream_encode_scratch_bytes(TOTAL, B), dtype=torch.uint8, device="cuda")
    n_out = torch.empty(1, dtype=torch.int64, device="cuda")

    def encode():
        _lib.check(L.lz4hip_stream_encode_device(src.data_ptr(), TOTAL, B, 0, enc.data_ptr(), bound, n_out.data_ptr(),
                                                 scratch.data_ptr(), scratch.numel(), s))
    r["encode_ms"] = timed(encode)
    n = int(n_out.item())
    r["stream_bytes"] = n
    copy_dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    r["memcpy_d2d_ms"] = timed(lambda: copy_dst.copy_(enc[:n]))
    r["memcpy_d2d_GBps"] = n / r["memcpy_d2d_ms"] / 1e6
    del copy_dst, scratch

    # stream decode: index, one read-back, decode
    stream_t = enc[:n]
    max_chunks = (n + 4095) // 4096 + 16
    dscratch = torch.empty(L.lz4hip_stream_decode_scratch_bytes(max_chunks), dtype=torch.uint8, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device="cuda")
    out = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")

    def index():
        _lib.check(L.lz4hip_stream_index_device(stream_t.data_ptr(), n, max_chunks, dscratch.data_ptr(), dscratch.numel(),
                                                info_dev.data_ptr(), s))
    r["index_ms"] = timed(index)
    info = _lib.StreamInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    assert info.error == 0 and info.decoded_bytes == TOTAL, (info.error, info.decoded_bytes)
    r["chunks"], r["compressed_chunks"] = info.chunks, info.compressed_chunks
    r["index_us_per_chunk"] = r["index_ms"] * 1000 / info.chunks

    def decode():
        _lib.check(L.lz4hip_stream_decode_device(stream_t.data_ptr(), C.byref(info), max_chunks, dscratch.data_ptr(), dscratch.numel(),
                                                 out.data_ptr(), TOTAL, info_dev.data_ptr(), s))
    r["stream_decode_ms"] = timed(decode)
    done = _lib.StreamInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    assert done.error == 0 and torch.equal(out, src), "stream decode"
    r["stream_index_plus_decode_ms"] = r["index_ms"] + r["stream_decode_ms"]
    r["decode_end_to_end_ms"] = timed(lambda: st.decompress_stream_device(stream_t))

    # the same chunks through the batch decoder, offsets known in advance
    chunks = st.parse_chunks(memoryview(stream_t.cpu().numpy().tobytes()))
    comp = [c for c in chunks if c[0]]
    out_off, pos = [], 0
    for c in chunks:
        out_off.append(pos)
        pos += c[1]
    out_off = [o for o, c in zip(out_off, chunks) if c[0]]
    so = torch.tensor([c[2] for c in comp], dtype=torch.int64, device="cuda")
    sl = torch.tensor([c[3] for c in comp], dtype=torch.int32, device="cuda")
    do = torch.tensor(out_off, dtype=torch.int64, device="cuda")
    dc = torch.tensor([c[1] for c in comp], dtype=torch.int32, device="cuda")
    res = torch.empty(len(comp), dtype=torch.int32, device="cuda")
    out.zero_()
    bd = _lib.Batch(src=stream_t.data_ptr(), src_off=so.data_ptr(), src_stride=0, src_len=sl.data_ptr(), dst=out.data_ptr(),
                    dst_off=do.data_ptr(), dst_stride=0, dst_cap=dc.data_ptr(), dst_cap_all=0, src_len_all=0, result=res.data_ptr(),
                    n_blocks=len(comp))
    r["batch_decode_ms"] = timed(lambda: _lib.check(L.lz4hip_decode_batch_device(C.byref(bd), 1, s)))
    assert bool((res == sl).all()) and (len(comp) < len(chunks) or torch.equal(out, src)), "batch decode"
    r["stream_over_batch_decode"] = r["stream_index_plus_decode_ms"] / r["batch_decode_ms"]
    del out, dscratch, enc
    torch.cuda.synchronize()
    print(json.dumps({k: v for k, v in results.items()}), flush=True)

if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(results, fh, indent=1)
