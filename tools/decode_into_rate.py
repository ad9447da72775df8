"""LZ4Stream buffers, batches of them and wrapped messages decoded in ONE device call (lz4hip_stream_decode_into_device,
lz4hip_streams_decode_into_device, lz4hip_unwrap_into_device) against the two-call pair each replaces, on the same input:

  - a stream of --stream-bytes bytes of D2 and of D3 in chunks of 64 KiB and of 1 MiB,
  - --items one-chunk items of 64 KiB (D2),
  - --messages wrapped messages of 64 KiB (D2).

Per case, event timings of the bare calls into preallocated buffers -- the pair's index and decode apart and together (without the
read-back a caller needs between them), the one call with its table at the exact count + 16 and at the Python wrapper's default, and
for the stream of 1 MiB chunks with a table of 16 400 rows, which sends its 1 024 chunks to the lane mapping -- and the wall-clock of
the Python wrappers as a user calls them, to the end of the device's work: decompress_stream_device / decompress_streams_device /
unwrap_device (allocation and both read-backs included) against the *_into forms into a buffer that is already there.

Best of five after one warm-up; the paths alternate inside a repetition.  Every output is compared with the source once per case.

    python tools/decode_into_rate.py [--reps 5] [--stream-bytes 1073741824] [--items 20000] [--messages 16384] [--out profiles/decode_into/decode_into_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lz4net_amd import _lib, batch, stream as st, wrap  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--stream-bytes", type=int, default=1 << 30)
ap.add_argument("--items", type=int, default=20000)
ap.add_argument("--messages", type=int, default=16384)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decode_into", "decode_into_rate.json"))
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


def wall_ms(fns):
    """the same, by the host's clock from the call to the end of the device's work"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    best = {}
    for _ in range(args.reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best[name] = min(best.get(name, float("inf")), (time.perf_counter() - t0) * 1e3)
    return best


def dev_bytes(n):
    return torch.empty(n, dtype=torch.uint8, device="cuda")


def synth_bytes(dist, n_bytes):
    return batch.synth(dist, 7, 0, (n_bytes + KIB64 - 1) // KIB64).reshape(-1)[:n_bytes]


results = {}
s = torch.cuda.current_stream().cuda_stream

# ---- one stream ------------------------------------------------------------------------------------------------------------------
for dist in (2, 3):
    data = synth_bytes(dist, args.stream_bytes)
    for block in (KIB64, 1 << 20):
        key = f"D{dist}/stream/{block}"
        r = results[key] = {"decoded_bytes": data.numel(), "block_size": block}
        t = st.compress_stream_device(data, block)
        chunks = (data.numel() + block - 1) // block
        r["chunks"], r["stream_bytes"] = chunks, t.numel()
        out = dev_bytes(data.numel())
        info_dev = torch.zeros(C.sizeof(_lib.StreamInfo), dtype=torch.uint8, device="cuda")
        written = torch.zeros(1, dtype=torch.int64, device="cuda")
        read_info = lambda: _lib.StreamInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())  # noqa: E731
        m = chunks + 16
        pneed = L.lz4hip_stream_decode_scratch_bytes(m)
        pscratch = dev_bytes(pneed)
        index = lambda: _lib.check(L.lz4hip_stream_index_device(t.data_ptr(), t.numel(), m, pscratch.data_ptr(), pneed, info_dev.data_ptr(), s))  # noqa: E731
        index()
        first = read_info()
        assert (first.error, first.chunks, first.decoded_bytes) == (_lib.STREAM_OK, chunks, data.numel())
        decode = lambda: _lib.check(L.lz4hip_stream_decode_device(t.data_ptr(), C.byref(first), m, pscratch.data_ptr(), pneed, out.data_ptr(), out.numel(),  # noqa: E731
                                                                  info_dev.data_ptr(), s))
        decode()
        assert read_info().error == _lib.STREAM_OK and torch.equal(out, data)
        fns = {"index_ms": index, "decode_ms": decode, "index_plus_decode_ms": lambda: (index(), decode())}
        tables = {"exact": m, "python_default": out.numel() // block + 16}
        if block > KIB64:
            tables["oversized_16400"] = 16400
        scratches = {}
        for name, rows in tables.items():
            need = L.lz4hip_stream_decode_into_scratch_bytes(rows)
            scratches[name] = dev_bytes(need)
            r[f"into_{name}_rows"] = rows
            fns[f"into_{name}_ms"] = lambda name=name, rows=rows: _lib.check(L.lz4hip_stream_decode_into_device(
                t.data_ptr(), t.numel(), rows, scratches[name].data_ptr(), scratches[name].numel(), out.data_ptr(), out.numel(), info_dev.data_ptr(),
                written.data_ptr(), s))
            out.zero_()
            fns[f"into_{name}_ms"]()
            assert read_info().error == _lib.STREAM_OK and int(written.item()) == data.numel() and torch.equal(out, data), name
        r.update(event_ms(fns))
        r.update(wall_ms({"pair_python_wall_ms": lambda: st.decompress_stream_device(t),
                          "into_python_wall_ms": lambda: st.decompress_stream_into(t, out, block_size=block)}))
        r["into_exact_over_index_plus_decode"] = r["into_exact_ms"] / r["index_plus_decode_ms"]
        print(json.dumps({key: r}), flush=True)
        del t, out, pscratch, scratches, fns
    del data

# ---- a batch of one-chunk streams ----------------------------------------------------------------------------------------------------
if args.items > 0:
    n = args.items
    key = f"D2/streams/{n}"
    r = results[key] = {"items": n, "decoded_bytes": n * KIB64}
    data = synth_bytes(2, n * KIB64)
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * KIB64
    packed, poff = st.compress_streams_device(data, offs, KIB64)
    r["packed_bytes"] = packed.numel()
    out = dev_bytes(data.numel())
    out_off, status, err_off = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.StreamsInfo), dtype=torch.uint8, device="cuda")
    written = torch.zeros(1, dtype=torch.int64, device="cuda")
    read_info = lambda: _lib.StreamsInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())  # noqa: E731
    m = n + 16
    pneed = L.lz4hip_streams_decode_scratch_bytes(n, m)
    pscratch = dev_bytes(pneed)
    index = lambda: _lib.check(L.lz4hip_streams_index_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, m, out_off.data_ptr(), status.data_ptr(),  # noqa: E731
                                                             err_off.data_ptr(), pscratch.data_ptr(), pneed, info_dev.data_ptr(), s))
    index()
    first = read_info()
    assert (first.error, first.chunks, first.decoded_bytes) == (_lib.STREAM_OK, n, data.numel())
    decode = lambda: _lib.check(L.lz4hip_streams_decode_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, C.byref(first), m, pscratch.data_ptr(), pneed,  # noqa: E731
                                                               out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(), err_off.data_ptr(),
                                                               info_dev.data_ptr(), s))
    decode()
    assert read_info().error == _lib.STREAM_OK and torch.equal(out, data)
    fns = {"index_ms": index, "decode_ms": decode, "index_plus_decode_ms": lambda: (index(), decode())}
    scratches = {}
    for name, rows in {"exact": m, "python_default": out.numel() // KIB64 + n + 16}.items():
        need = L.lz4hip_streams_decode_into_scratch_bytes(n, rows)
        scratches[name] = dev_bytes(need)
        r[f"into_{name}_rows"] = rows
        fns[f"into_{name}_ms"] = lambda name=name, rows=rows: _lib.check(L.lz4hip_streams_decode_into_device(
            packed.data_ptr(), packed.numel(), poff.data_ptr(), n, rows, scratches[name].data_ptr(), scratches[name].numel(), out.data_ptr(), out.numel(),
            out_off.data_ptr(), status.data_ptr(), err_off.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s))
        out.zero_()
        fns[f"into_{name}_ms"]()
        assert read_info().error == _lib.STREAM_OK and int(written.item()) == n and torch.equal(out, data), name
    r.update(event_ms(fns))
    r.update(wall_ms({"pair_python_wall_ms": lambda: st.decompress_streams_device(packed, poff),
                      "into_python_wall_ms": lambda: st.decompress_streams_into(packed, poff, out, block_size=KIB64)}))
    r["into_exact_over_index_plus_decode"] = r["into_exact_ms"] / r["index_plus_decode_ms"]
    print(json.dumps({key: r}), flush=True)
    del data, packed, out, pscratch, scratches, fns

# ---- wrapped messages ----------------------------------------------------------------------------------------------------------------
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
    pneed = L.lz4hip_unwrap_scratch_bytes(n)
    pscratch = dev_bytes(pneed)
    index = lambda: _lib.check(L.lz4hip_unwrap_index_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, out_off.data_ptr(), status.data_ptr(),  # noqa: E731
                                                            pscratch.data_ptr(), pneed, info_dev.data_ptr(), s))
    index()
    first = read_info()
    assert (first.error, first.decoded_bytes) == (_lib.WRAP_OK, data.numel())
    decode = lambda: _lib.check(L.lz4hip_unwrap_decode_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, C.byref(first), pscratch.data_ptr(), pneed,  # noqa: E731
                                                              out.data_ptr(), out.numel(), out_off.data_ptr(), status.data_ptr(), info_dev.data_ptr(), s))
    decode()
    assert read_info().error == _lib.WRAP_OK and torch.equal(out, data)
    need = L.lz4hip_unwrap_into_scratch_bytes(n)
    scratch = dev_bytes(need)
    into = lambda: _lib.check(L.lz4hip_unwrap_into_device(packed.data_ptr(), packed.numel(), poff.data_ptr(), n, scratch.data_ptr(), need, out.data_ptr(),  # noqa: E731
                                                          out.numel(), out_off.data_ptr(), status.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s))
    out.zero_()
    into()
    assert read_info().error == _lib.WRAP_OK and int(written.item()) == n and torch.equal(out, data)
    r["compressed_messages"] = int(read_info().compressed)
    r.update(event_ms({"index_ms": index, "decode_ms": decode, "index_plus_decode_ms": lambda: (index(), decode()), "into_ms": into}))
    r.update(wall_ms({"pair_python_wall_ms": lambda: wrap.unwrap_device(packed, poff),
                      "into_python_wall_ms": lambda: wrap.unwrap_into(packed, poff, out)}))
    r["into_over_index_plus_decode"] = r["into_ms"] / r["index_plus_decode_ms"]
    print(json.dumps({key: r}), flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
