"""Legacy frames on the device (lz4hip_frame_*_device) over 1 GiB of D2 and of D3 data, at chunks of 8 MiB (the CLI's) and 64 KiB, fast
mode.  Per case:

  - compress_frame_device / decompress_frame_device: event timings of the Python calls as a user makes them (allocations and their
    one / two read-backs included);
  - the bare lz4hip_frame_encode_device / lz4hip_frame_index_device / lz4hip_frame_decode_device calls into preallocated buffers:
    event timings, launch-only -- what the framing's share is taken from;
  - compress_frame_host / decompress_frame_host, the host-staged calls: wall clock;
  - the existing legacy_frame.compress_frame / decompress_frame on the same bytes: wall clock (Python around lz4hip_*_batch_host);
  - the block codec alone on the same table -- lz4hip_encode_batch_device with compressBound capacities, lz4hip_decode_batch_device
    (unknown size) on the same chunks, every one of them (a shorter last chunk is a batch of its own, timed too) -- and with it the
    framing's own share: the bare device call's time minus the block codec's.

Best of five after one warm-up.  Every decode is checked against the source.

    python tools/frame_rate.py [--reps 5] [--bytes 1073741824] [--out profiles/frame_device/frame_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lz4net_amd import _lib, batch  # noqa: E402
from lz4net_amd import legacy_frame as lf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--bytes", type=int, default=1 << 30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = _lib.lib()


def event_ms(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(min(ts))


def wall_ms(fn):
    fn()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(min(ts))


def bound(n):
    return n + n // 255 + 16


results = {}
for dist in (2, 3):
    src = batch.synth(dist, 7, 0, args.bytes // 65536, length=65536).reshape(-1)
    host_src = src.cpu().numpy()
    for chunk in (8 << 20, 64 << 10):
        n = (src.numel() + chunk - 1) // chunk
        r = results[f"D{dist}/{chunk // 1024}KiB"] = {"bytes": src.numel(), "chunks": n}
        s = torch.cuda.current_stream().cuda_stream
        frame = lf.compress_frame_device(src, chunk_size=chunk)
        r["frame_bytes"] = frame.numel()
        r["encode_device_ms"] = event_ms(lambda: lf.compress_frame_device(src, chunk_size=chunk))
        r["decode_device_ms"] = event_ms(lambda: lf.decompress_frame_device(frame, chunk_size=chunk))
        assert torch.equal(lf.decompress_frame_device(frame, chunk_size=chunk), src)

        # the bare encode call into preallocated buffers: launch-only, like the block codec call it is held against
        cap = L.lz4hip_frame_bound(src.numel(), chunk)
        enc_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        enc_scratch = torch.empty(L.lz4hip_frame_encode_scratch_bytes(src.numel(), chunk), dtype=torch.uint8, device="cuda")
        enc_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        r["encode_call_ms"] = event_ms(lambda: _lib.check(L.lz4hip_frame_encode_device(
            src.data_ptr(), src.numel(), chunk, _lib.MODE_FAST, enc_out.data_ptr(), cap, enc_len.data_ptr(), enc_scratch.data_ptr(),
            enc_scratch.numel(), s)))
        assert int(enc_len.item()) == frame.numel() and torch.equal(enc_out[:frame.numel()], frame)
        del enc_out, enc_scratch

        # the block codec alone on the same chunks: the full ones as one batch, a shorter last one as a batch of its own
        full, rest = src.numel() // chunk, src.numel() % chunk
        r["encode_blocks_ms"] = 0.0
        if full:
            rows = src[:full * chunk].reshape(full, chunk)
            comp = torch.empty(full, bound(chunk), dtype=torch.uint8, device="cuda")
            r["encode_blocks_ms"] += event_ms(lambda: batch.encode(rows, chunk, comp, comp.shape[1]))
            del comp
        if rest:
            tail = src[full * chunk:].reshape(1, rest)
            comp = torch.empty(1, bound(rest), dtype=torch.uint8, device="cuda")
            r["encode_blocks_ms"] += event_ms(lambda: batch.encode(tail, rest, comp, comp.shape[1]))
            del comp
        info_dev = torch.zeros(C.sizeof(_lib.FrameInfo), dtype=torch.uint8, device="cuda")
        m = n + 16
        table = torch.empty(L.lz4hip_frame_decode_scratch_bytes(m), dtype=torch.uint8, device="cuda")
        out = torch.empty(src.numel(), dtype=torch.uint8, device="cuda")

        def index():
            _lib.check(L.lz4hip_frame_index_device(frame.data_ptr(), frame.numel(), chunk, m, table.data_ptr(), table.numel(), info_dev.data_ptr(), s))

        index()
        info = _lib.FrameInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
        assert info.error == _lib.FRAME_OK and info.decoded_bytes == src.numel()

        def decode():
            _lib.check(L.lz4hip_frame_decode_device(frame.data_ptr(), C.byref(info), m, table.data_ptr(), table.numel(), out.data_ptr(), out.numel(),
                                                    info_dev.data_ptr(), s))

        r["index_ms"] = event_ms(index)
        r["decode_call_ms"] = event_ms(decode)
        # the same rows through the block decoder with everything known in advance: offsets from the host's walk, capacity = chunk
        chunks = lf.parse_frame(frame.cpu().numpy().tobytes())
        off = torch.tensor([c[0] for c in chunks], dtype=torch.int64, device="cuda")
        lens = torch.tensor([c[1] for c in chunks], dtype=torch.int32, device="cuda")
        doff = torch.arange(n, dtype=torch.int64, device="cuda") * chunk
        caps = torch.full((n,), chunk, dtype=torch.int32, device="cuda")
        res = torch.empty(n, dtype=torch.int32, device="cuda")
        b = _lib.Batch(src=frame.data_ptr(), src_off=off.data_ptr(), src_stride=0, src_len=lens.data_ptr(), dst=out.data_ptr(), dst_off=doff.data_ptr(),
                       dst_stride=0, dst_cap=caps.data_ptr(), dst_cap_all=0, src_len_all=0, result=res.data_ptr(), n_blocks=n)
        r["decode_blocks_ms"] = event_ms(lambda: _lib.check(L.lz4hip_decode_batch_device(C.byref(b), 0, s)))
        r["encode_framing_ms"] = r["encode_call_ms"] - r["encode_blocks_ms"]
        r["decode_framing_ms"] = r["index_ms"] + r["decode_call_ms"] - r["decode_blocks_ms"]

        # the host-staged calls and the existing path, on the same bytes
        host_frame = frame.cpu().numpy()
        r["encode_host_ms"] = wall_ms(lambda: lf.compress_frame_host(host_src, chunk_size=chunk))
        r["decode_host_ms"] = wall_ms(lambda: lf.decompress_frame_host(host_frame, chunk_size=chunk))
        r["encode_existing_ms"] = wall_ms(lambda: lf.compress_frame(host_src, chunk_size=chunk))
        r["decode_existing_ms"] = wall_ms(lambda: lf.decompress_frame(host_frame.tobytes(), chunk_size=chunk))
        print(json.dumps({f"D{dist}/{chunk // 1024}KiB": r}), flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
