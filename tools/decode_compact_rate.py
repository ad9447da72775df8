"""A block batch decoded into one packed buffer without a size walk (lz4hip_decode_compact_device) against the two existing ways to decode
blocks of unknown size, on the same blocks: D2 and D3, 16 384 and 262 144 blocks of 64 KiB encoded on the device.  Per case, event
timings of the bare calls into preallocated buffers:

  - compact: lz4hip_decode_compact_device with round_blocks 0, 16 384 and 65 536 into a buffer of exactly decoded_bytes; the scratch
    each form needs is recorded next to it;
  - walk + decode: lz4hip_decoded_sizes_device, then lz4hip_decode_batch_device (unknown size) on the offsets and capacities it wrote --
    what batch.decode_packed runs, without its read-back between the two -- timed apart and together;
  - slots: batch.decode (unknown size) into slot-strided rows, n * slot bytes of output: the block decoder's own time.

and batch.decode_compact / batch.decode_packed as a user calls them (allocations and read-backs included).  Then the same for a legacy
frame of --frame-bytes bytes in chunks of 64 KiB and of 8 MiB: lz4hip_frame_decode_compact_device (round_chunks 0 and a ring of 16
chunks) against lz4hip_frame_index_device + lz4hip_frame_decode_device, and the two Python wrappers.

Best of five after one warm-up; the two paths alternate inside a repetition.  Every output is compared with the source once per case.

    python tools/decode_compact_rate.py [--reps 5] [--blocks 16384,262144] [--frame-bytes 1073741824] [--out profiles/decode_compact/decode_compact_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lz4net_amd import _lib, batch, legacy_frame as lf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--blocks", default="16384,262144")
ap.add_argument("--rounds", default="0,16384,65536")
ap.add_argument("--frame-bytes", type=int, default=1 << 30)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decode_compact", "decode_compact_rate.json"))
args = ap.parse_args()
L = _lib.lib()
SLOT = batch.BLOCK


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


results = {}
s = torch.cuda.current_stream().cuda_stream
for dist in (2, 3):
    for n in [int(x) for x in args.blocks.split(",") if x]:
        r = results[f"D{dist}/{n}"] = {"blocks": n, "decoded_bytes": n * SLOT}
        raw = batch.synth(dist, 7, 0, n)
        comp = torch.empty((n, batch.BOUND_STRIDE), dtype=torch.uint8, device="cuda")
        clen = batch.encode(raw, SLOT, comp, batch.BOUND)
        total = n * SLOT
        r["compressed_bytes"] = int(clen.to(torch.int64).sum().item())
        res = torch.empty(n, dtype=torch.int32, device="cuda")
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        dlen = torch.empty(n, dtype=torch.int32, device="cuda")
        info = torch.empty(5, dtype=torch.int64, device="cuda")
        dst = torch.empty(total, dtype=torch.uint8, device="cuda")
        fns = {}

        # compact: rounds through a ring, no walk
        src_side = dict(src=comp.data_ptr(), src_stride=comp.stride(0), src_len=clen.data_ptr(), result=res.data_ptr(), n_blocks=n)
        cb = _lib.Batch(dst_cap_all=SLOT, **src_side)
        rounds = [int(x) for x in args.rounds.split(",")]
        needs = {k: _lib.check(L.lz4hip_decode_compact_scratch_bytes(n, SLOT, k)) for k in rounds}
        scratch = torch.empty(max(needs.values()), dtype=torch.uint8, device="cuda")       # (one buffer, each form using its own share of it)
        for k in rounds:
            r[f"compact_k{k}_scratch_bytes"] = needs[k]
            fns[f"compact_k{k}_ms"] = lambda k=k: _lib.check(L.lz4hip_decode_compact_device(
                C.byref(cb), k, dst.data_ptr(), total, off.data_ptr(), dlen.data_ptr(), scratch.data_ptr(), needs[k], info.data_ptr(), s))
            fns[f"compact_k{k}_ms"]()
            h = batch.read_compact_info(info)
            assert (h.decoded_bytes, h.written_blocks, h.first_failed) == (total, n, -1) and torch.equal(dst.view(n, SLOT), raw), k
            dst.zero_()

        # walk + decode: the size query, then the batch decoder on what it wrote
        wneed = L.lz4hip_decoded_sizes_scratch_bytes(n)
        wscratch = torch.empty(wneed, dtype=torch.uint8, device="cuda")
        caps = torch.empty(n, dtype=torch.int32, device="cuda")
        winfo = torch.empty(4, dtype=torch.int64, device="cuda")
        wb = _lib.Batch(**src_side)
        db = _lib.Batch(dst=dst.data_ptr(), dst_off=off.data_ptr(), dst_cap=caps.data_ptr(), **src_side)
        walk = lambda: _lib.check(L.lz4hip_decoded_sizes_device(C.byref(wb), off.data_ptr(), caps.data_ptr(), wscratch.data_ptr(), wneed, winfo.data_ptr(), s))  # noqa: E731
        exact = lambda: _lib.check(L.lz4hip_decode_batch_device(C.byref(db), 0, s))  # noqa: E731
        walk(), exact()
        assert batch.read_sizes_info(winfo).decoded_bytes == total and torch.equal(dst.view(n, SLOT), raw)
        fns["walk_ms"], fns["decode_exact_ms"] = walk, exact
        fns["walk_plus_decode_ms"] = lambda: (walk(), exact())

        # slots: n * slot bytes of output
        rows = dst.view(n, SLOT)                                          # (blocks of exactly the slot width: the same bytes, laid out as rows)
        dst.zero_()
        fns["slots_ms"] = lambda: batch.decode(comp, clen, rows, SLOT, known_output_size=False, result=res)
        fns["slots_ms"]()
        assert torch.equal(rows, raw)
        r["slots_output_bytes"] = rows.numel()

        fns["decode_compact_python_ms"] = lambda: batch.decode_compact(comp, clen, slot_bytes=SLOT)
        fns["decode_packed_python_ms"] = lambda: batch.decode_packed(comp, clen)
        r.update(event_ms(fns))
        for k in rounds:
            r[f"compact_k{k}_over_walk_plus_decode"] = r[f"compact_k{k}_ms"] / r["walk_plus_decode_ms"]
            r[f"compact_k{k}_minus_slots_ms"] = r[f"compact_k{k}_ms"] - r["slots_ms"]
        print(json.dumps({f"D{dist}/{n}": r}), flush=True)
        del raw, comp, dst, rows, scratch, wscratch, fns

    # ---- a legacy frame ------------------------------------------------------------------------------------------------------------
    if args.frame_bytes <= 0:
        continue
    data = batch.synth(dist, 7, 0, (args.frame_bytes + SLOT - 1) // SLOT).reshape(-1)[:args.frame_bytes]
    for chunk in (65536, 8 << 20):
        r = results[f"D{dist}/frame/{chunk}"] = {"chunk_size": chunk, "decoded_bytes": data.numel()}
        frame = lf.compress_frame_device(data, chunk_size=chunk)
        chunks = (data.numel() + chunk - 1) // chunk
        m = chunks + 16
        r["chunks"], r["frame_bytes"] = chunks, frame.numel()
        out = torch.empty(data.numel(), dtype=torch.uint8, device="cuda")
        info_dev = torch.zeros(C.sizeof(_lib.FrameInfo), dtype=torch.uint8, device="cuda")
        read_info = lambda: _lib.FrameInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())  # noqa: E731
        fns, scratches = {}, {}
        for k in (0, 16):
            need = _lib.check(L.lz4hip_frame_decode_compact_scratch_bytes(chunk, m, k))
            scratches[k] = torch.empty(need, dtype=torch.uint8, device="cuda")
            r[f"compact_k{k}_scratch_bytes"] = need
            fns[f"compact_k{k}_ms"] = lambda k=k: _lib.check(L.lz4hip_frame_decode_compact_device(
                frame.data_ptr(), frame.numel(), chunk, m, k, scratches[k].data_ptr(), scratches[k].numel(), out.data_ptr(), out.numel(), info_dev.data_ptr(), s))
            fns[f"compact_k{k}_ms"]()
            h = read_info()
            assert (h.error, h.chunks, h.decoded_bytes) == (_lib.FRAME_OK, chunks, data.numel()) and torch.equal(out, data), k
            out.zero_()
        tneed = L.lz4hip_frame_decode_scratch_bytes(m)
        tscratch = torch.empty(tneed, dtype=torch.uint8, device="cuda")
        index = lambda: _lib.check(L.lz4hip_frame_index_device(frame.data_ptr(), frame.numel(), chunk, m, tscratch.data_ptr(), tneed, info_dev.data_ptr(), s))  # noqa: E731
        index()
        first = read_info()
        assert (first.error, first.decoded_bytes) == (_lib.FRAME_OK, data.numel())
        decode = lambda: _lib.check(L.lz4hip_frame_decode_device(frame.data_ptr(), C.byref(first), m, tscratch.data_ptr(), tneed, out.data_ptr(), out.numel(),  # noqa: E731
                                                                 info_dev.data_ptr(), s))
        decode()
        assert read_info().error == _lib.FRAME_OK and torch.equal(out, data)
        fns["index_ms"], fns["decode_ms"] = index, decode
        fns["index_plus_decode_ms"] = lambda: (index(), decode())      # (without the read-back the two-call path needs between them)
        fns["compact_python_ms"] = lambda: lf.decompress_frame_compact_device(frame, chunk_size=chunk)
        fns["two_call_python_ms"] = lambda: lf.decompress_frame_device(frame, chunk_size=chunk)
        r.update(event_ms(fns))
        for k in (0, 16):
            r[f"compact_k{k}_over_index_plus_decode"] = r[f"compact_k{k}_ms"] / r["index_plus_decode_ms"]
        print(json.dumps({f"D{dist}/frame/{chunk}": r}), flush=True)
        del frame, out, scratches, tscratch, fns
    del data

if args.out:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
