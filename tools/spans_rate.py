"""Chosen items of a device arena decoded in ONE call (lz4hip_unwrap_spans_into_device, lz4hip_streams_decode_spans_into_device) and
the chunk directory of one stream (lz4hip_stream_directory_device), against the existing calls on the same input:

  - --messages wrapped messages of 64 KiB (D2): 256, 4 096 and all of them chosen in order, against lz4hip_unwrap_into_device over
    the whole arena (and lz4hip_spans_select_device for each selection);
  - a stream of --stream-bytes bytes of D2 and of D3 in chunks of 64 KiB and of 1 MiB: the directory once, then all chunks as
    one-chunk spans against lz4hip_stream_decode_into_device, both with a table of the exact count + 16.

Event timings of the bare calls into preallocated buffers.  Best of five after one warm-up; the paths alternate inside a repetition.
Every output is compared with the source once per case.

    python tools/spans_rate.py [--reps 5] [--stream-bytes 1073741824] [--messages 16384] [--out profiles/spans/spans_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lz4net_amd import _lib, batch, stream as st, wrap  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--stream-bytes", type=int, default=1 << 30)
ap.add_argument("--messages", type=int, default=16384)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spans", "spans_rate.json"))
args = ap.parse_args()
L = _lib.lib()
KIB64 = 65536


def event_ms(fns):
    """best-of-reps event time of each function of `fns`, which take turns inside a repetition; one warm-up each"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    best = {}
    for _ in range(args.reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            best[name] = min(best.get(name, float("inf")), a.elapsed_time(b))
    return best


def dev_bytes(n):
    return torch.empty(n, dtype=torch.uint8, device="cuda")


def synth_bytes(dist, n_bytes):
    return batch.synth(dist, 7, 0, (n_bytes + KIB64 - 1) // KIB64).reshape(-1)[:n_bytes]


results = {}
s = torch.cuda.current_stream().cuda_stream

# ---- wrapped messages: a selection against the whole arena ---------------------------------------------------------------------------
if args.messages > 0:
    n = args.messages
    key = f"D2/unwrap/{n}"
    r = results[key] = {"messages": n, "decoded_bytes": n * KIB64}
    data = synth_bytes(2, n * KIB64)
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * KIB64
    packed, poff = wrap.wrap_device(data, offs)
    r["packed_bytes"] = packed.numel()
    out = dev_bytes(data.numel())
    out_off, status = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device="cuda")
    written = torch.zeros(1, dtype=torch.int64, device="cuda")
    read_info = lambda: _lib.UnwrapInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())  # noqa: E731
    need = L.lz4hip_unwrap_into_scratch_bytes(n)
    scratch = dev_bytes(need)
    fns = {"whole_arena_into_ms": lambda: _lib.check(L.lz4hip_unwrap_into_device(
        packed.data_ptr(), packed.numel(), poff.data_ptr(), n, scratch.data_ptr(), need, out.data_ptr(), out.numel(), out_off.data_ptr(),
        status.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s))}
    keep = {}
    for m in sorted({min(256, n), min(4096, n), n}):
        sel = (torch.arange(m, dtype=torch.int64, device="cuda") * (n // m)).contiguous()      # in order, spread over the arena
        begin, end = torch.empty(m, dtype=torch.int64, device="cuda"), torch.empty(m, dtype=torch.int64, device="cuda")
        mneed = L.lz4hip_unwrap_into_scratch_bytes(m)
        keep[m] = (sel, begin, end, dev_bytes(mneed), mneed)
        fns[f"select_{m}_ms"] = lambda m=m: _lib.check(L.lz4hip_spans_select_device(
            poff.data_ptr(), n, keep[m][0].data_ptr(), m, keep[m][1].data_ptr(), keep[m][2].data_ptr(), s))
        fns[f"spans_{m}_ms"] = lambda m=m: _lib.check(L.lz4hip_unwrap_spans_into_device(
            packed.data_ptr(), packed.numel(), keep[m][1].data_ptr(), keep[m][2].data_ptr(), m, keep[m][3].data_ptr(), keep[m][4], out.data_ptr(),
            out.numel(), out_off.data_ptr(), status.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s))
        out.zero_()
        fns[f"select_{m}_ms"]()
        fns[f"spans_{m}_ms"]()
        assert read_info().error == _lib.WRAP_OK and int(written.item()) == m
        want = data.reshape(n, KIB64)[sel].reshape(-1)
        assert torch.equal(out[:m * KIB64], want), m
        del want
    out.zero_()
    fns["whole_arena_into_ms"]()
    assert read_info().error == _lib.WRAP_OK and int(written.item()) == n and torch.equal(out, data)
    r.update(event_ms(fns))
    print(json.dumps({key: r}), flush=True)
    del data, packed, out, scratch, keep, fns

# ---- one stream: the directory once, then all chunks as one-chunk spans ----------------------------------------------------------------
for dist in (2, 3):
    if args.stream_bytes <= 0:
        break
    data = synth_bytes(dist, args.stream_bytes)
    for block in (KIB64, 1 << 20):
        key = f"D{dist}/stream/{block}"
        r = results[key] = {"decoded_bytes": data.numel(), "block_size": block}
        t = st.compress_stream_device(data, block)
        chunks = (data.numel() + block - 1) // block
        r["chunks"], r["stream_bytes"] = chunks, t.numel()
        out = dev_bytes(data.numel())
        rows = chunks + 16
        r["table_rows"] = rows
        sinfo = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device="cuda")
        binfo = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device="cuda")
        written = torch.zeros(1, dtype=torch.int64, device="cuda")
        hdr_off, out_off = torch.empty(rows + 1, dtype=torch.int64, device="cuda"), torch.empty(rows + 1, dtype=torch.int64, device="cuda")
        directory = lambda: _lib.check(L.lz4hip_stream_directory_device(t.data_ptr(), t.numel(), rows, hdr_off.data_ptr(), out_off.data_ptr(),  # noqa: E731
                                                                        sinfo.data_ptr(), s))
        directory()
        first = _lib.StreamInfo.from_buffer_copy(sinfo.cpu().numpy().tobytes())
        assert (first.error, first.chunks, first.decoded_bytes) == (_lib.STREAM_OK, chunks, data.numel())
        ineed = L.lz4hip_stream_decode_into_scratch_bytes(rows)
        iscratch = dev_bytes(ineed)
        into = lambda: _lib.check(L.lz4hip_stream_decode_into_device(t.data_ptr(), t.numel(), rows, iscratch.data_ptr(), ineed, out.data_ptr(), out.numel(),  # noqa: E731
                                                                     sinfo.data_ptr(), written.data_ptr(), s))
        out.zero_()
        into()
        assert int(written.item()) == data.numel() and torch.equal(out, data)
        sneed = L.lz4hip_streams_decode_into_scratch_bytes(chunks, rows)
        sscratch = dev_bytes(sneed)
        d_off, status, err_off = torch.empty(chunks + 1, dtype=torch.int64, device="cuda"), torch.empty(chunks, dtype=torch.int32, device="cuda"), torch.empty(chunks, dtype=torch.int64, device="cuda")
        spans = lambda: _lib.check(L.lz4hip_streams_decode_spans_into_device(  # noqa: E731
            t.data_ptr(), t.numel(), hdr_off.data_ptr(), hdr_off.data_ptr() + 8, chunks, rows, sscratch.data_ptr(), sneed, out.data_ptr(), out.numel(),
            d_off.data_ptr(), status.data_ptr(), err_off.data_ptr(), binfo.data_ptr(), written.data_ptr(), s))
        out.zero_()
        spans()
        final = _lib.StreamsInfo.from_buffer_copy(binfo.cpu().numpy().tobytes())
        assert (final.error, final.first_error, final.chunks) == (_lib.STREAM_OK, -1, chunks) and int(written.item()) == chunks and torch.equal(out, data)
        r.update(event_ms({"directory_ms": directory, "one_call_into_ms": into, "directory_spans_ms": spans}))
        r["directory_spans_over_one_call_into"] = r["directory_spans_ms"] / r["one_call_into_ms"]
        print(json.dumps({key: r}), flush=True)
        del t, out, iscratch, sscratch
    del data

if args.out:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
