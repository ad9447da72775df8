"""Batches of LZ4Stream buffers on the device (lz4hip_streams_*_device) over 1 GiB of D2 data cut into many small items, block_size
1 MiB (one chunk per item), fast mode, with event timings; meant to run under `rocprofv3 --kernel-trace --stats` too, whose per-kernel
totals split the calls into their kernels.

Cases: 16 384 items x 64 KiB and 262 144 items x 4 KiB.  Per case: the new encode call and the new index + decode calls; the only way
to do the same work without them -- a Python loop of compress_stream_device / decompress_stream_device over the items, timed on a
1 024-item slice and scaled; lz4hip_encode_batch_device / lz4hip_decode_batch_device on the same blocks with offsets known in advance
(the floor: what the framing costs on top); and the one-stream header walk (lz4hip_stream_index_device) of ONE stream with the same
number of chunks, against the two walk passes of the batch (the whole index call).  Every decode is checked against the source.

    python tools/streams_device_rate.py [reps] [out.json]
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lz4net_amd import _lib, batch  # noqa: E402
from lz4net_amd import stream as st  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_json = sys.argv[2] if len(sys.argv) > 2 else None
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream
TOTAL, B, SLICE = 1 << 30, 1 << 20, 1024


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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


results = {}
for size in (1 << 16, 1 << 12):
    n = TOTAL // size
    r = results[f"{n}x{size // 1024}KiB"] = {"items": n}
    src2 = batch.synth(2, 7, 0, n, length=size)
    src = src2.reshape(-1)
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * size
    torch.cuda.synchronize()

    # ---- encode: the new call
    bound = L.lz4hip_streams_bound(n, TOTAL, B)
    enc = torch.empty(bound, dtype=torch.uint8, device="cuda")
    enc_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.lz4hip_streams_encode_scratch_bytes(n, TOTAL, B), dtype=torch.uint8, device="cuda")

    def encode():
        _lib.check(L.lz4hip_streams_encode_device(src.data_ptr(), TOTAL, offs.data_ptr(), n, B, 0, enc.data_ptr(), bound, enc_off.data_ptr(),
                                                  scratch.data_ptr(), scratch.numel(), s))
    r["streams_encode_ms"] = timed(encode)
    total = int(enc_off[n].item())
    r["packed_bytes"] = total
    del scratch

    # the loop over the items: a slice, scaled
    items = [src[i * size:(i + 1) * size] for i in range(SLICE)]
    st.compress_stream_device(items[0], B)
    loop_streams = []
    r["loop_encode_slice_ms"] = wall_ms(lambda: loop_streams.extend(st.compress_stream_device(m, B) for m in items))
    r["loop_encode_scaled_ms"] = r["loop_encode_slice_ms"] * n / SLICE

    # the floor: the batch encoder on the same blocks, offsets known in advance
    comp = torch.empty((n, size), dtype=torch.uint8, device="cuda")
    clen = torch.empty(n, dtype=torch.int32, device="cuda")
    be = _lib.Batch(src=src.data_ptr(), src_off=None, src_stride=size, src_len=None, dst=comp.data_ptr(), dst_off=None, dst_stride=size,
                    dst_cap=None, dst_cap_all=size, src_len_all=size, result=clen.data_ptr(), n_blocks=n)
    r["batch_encode_ms"] = timed(lambda: _lib.check(L.lz4hip_encode_batch_device(C.byref(be), 0, s)))
    r["streams_over_batch_encode"] = r["streams_encode_ms"] / r["batch_encode_ms"]
    r["loop_over_streams_encode"] = r["loop_encode_scaled_ms"] / r["streams_encode_ms"]

    # ---- decode: the new calls
    packed, packed_off = enc[:total], enc_off
    max_chunks = n + 16
    dscratch = torch.empty(L.lz4hip_streams_decode_scratch_bytes(n, max_chunks), dtype=torch.uint8, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device="cuda")
    out = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    err_off = torch.empty(n, dtype=torch.int64, device="cuda")

    def index():
        _lib.check(L.lz4hip_streams_index_device(packed.data_ptr(), total, packed_off.data_ptr(), n, max_chunks, out_off.data_ptr(), status.data_ptr(),
                                                 err_off.data_ptr(), dscratch.data_ptr(), dscratch.numel(), info_dev.data_ptr(), s))
    r["streams_index_ms"] = timed(index)
    info = _lib.StreamsInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    assert info.error == 0 and info.decoded_bytes == TOTAL and info.chunks == n, (info.error, info.decoded_bytes, info.chunks)
    r["chunks"], r["compressed_chunks"] = info.chunks, info.compressed_chunks

    def decode():
        _lib.check(L.lz4hip_streams_decode_device(packed.data_ptr(), total, packed_off.data_ptr(), n, C.byref(info), max_chunks, dscratch.data_ptr(),
                                                  dscratch.numel(), out.data_ptr(), TOTAL, out_off.data_ptr(), status.data_ptr(), err_off.data_ptr(),
                                                  info_dev.data_ptr(), s))
    r["streams_decode_ms"] = timed(decode)
    done = _lib.StreamsInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    assert done.error == 0 and done.first_error == -1 and torch.equal(out_off, offs), "streams decode"
    assert batch.count_mismatches(src2, out.reshape(n, size), size) == 0, "streams decode"
    r["streams_index_plus_decode_ms"] = r["streams_index_ms"] + r["streams_decode_ms"]
    r["decode_end_to_end_ms"] = timed(lambda: st.decompress_streams_device(packed, packed_off))

    st.decompress_stream_device(loop_streams[0])
    loop_back = []
    r["loop_decode_slice_ms"] = wall_ms(lambda: loop_back.extend(st.decompress_stream_device(m) for m in loop_streams))
    assert all(torch.equal(a, b) for a, b in zip(loop_back[:8], items[:8]))
    r["loop_decode_scaled_ms"] = r["loop_decode_slice_ms"] * n / SLICE
    del loop_back, loop_streams

    # the floor: the batch decoder on the batch encoder's blocks
    out.zero_()
    used = torch.empty(n, dtype=torch.int32, device="cuda")
    bd = _lib.Batch(src=comp.data_ptr(), src_off=None, src_stride=size, src_len=clen.data_ptr(), dst=out.data_ptr(), dst_off=None, dst_stride=size,
                    dst_cap=None, dst_cap_all=size, src_len_all=0, result=used.data_ptr(), n_blocks=n)
    assert bool((clen > 0).all())
    r["batch_decode_ms"] = timed(lambda: _lib.check(L.lz4hip_decode_batch_device(C.byref(bd), 1, s)))
    assert bool((used == clen).all()) and batch.count_mismatches(src2, out.reshape(n, size), size) == 0, "batch decode"
    r["streams_over_batch_decode"] = r["streams_index_plus_decode_ms"] / r["batch_decode_ms"]
    r["loop_over_streams_decode"] = r["loop_decode_scaled_ms"] / r["decode_end_to_end_ms"]
    del comp, dscratch, enc

    # the one-stream walk of ONE stream with as many chunks (block_size = the item size)
    one = st.compress_stream_device(src, size)
    one_chunks = n + 16
    oscratch = torch.empty(L.lz4hip_stream_decode_scratch_bytes(one_chunks), dtype=torch.uint8, device="cuda")
    oinfo = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device="cuda")
    r["one_stream_index_ms"] = timed(lambda: _lib.check(L.lz4hip_stream_index_device(one.data_ptr(), one.numel(), one_chunks, oscratch.data_ptr(),
                                                                                     oscratch.numel(), oinfo.data_ptr(), s)))
    oi = _lib.StreamInfo.from_buffer_copy(oinfo.cpu().numpy().tobytes())
    assert oi.error == 0 and oi.chunks == n
    r["one_stream_index_us_per_chunk"] = r["one_stream_index_ms"] * 1000 / n
    r["one_stream_walk_over_streams_index"] = r["one_stream_index_ms"] / r["streams_index_ms"]
    del out, one, oscratch, src, src2
    torch.cuda.synchronize()
    print(json.dumps(results), flush=True)

if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(results, fh, indent=1)
