"""Batches of LZ4 frames (lz4hip_lz4f_batch_*_device) against what the same library offered before them, on the same content, after
tools/lz4f_rate.py's method: event timings of the bare calls into preallocated buffers, best of --reps after one warm-up, the paths
taking turns inside a repetition.  One --case per process (run every case under its own `timeout`, chained with &&):

  small   16 384 frames of 64 KiB content (one block each)
  large   1 024 frames of 1 MiB content (sixteen 64 KiB blocks each)

each for D2 and D3, with no checksums and with both.  Yardsticks, all existing code timed in the same run:

  loop     the loop of one-frame calls over the same frames as the Python front makes them (compress_frame_device /
           decompress_frame_device per item: read-backs included, so wall time between two synchronisations, not event time), over the
           first --loop-items items, reported per item and extrapolated to the batch -- the extrapolation is marked as one
  streams  lz4hip_streams_encode_device / lz4hip_streams_decode_into_device on the same content, every item a one-chunk item (64 KiB items)
           or sixteen chunks of 64 KiB (1 MiB items)
  blocks   the block codecs alone on the same table: lz4hip_encode_batch_device / lz4hip_decode_batch_device over the 64 KiB blocks at a
           compressBound stride

    python tools/lz4f_batch_rate.py --case small [--reps 5] [--loop-items 256] [--out profiles/lz4f_batch/small.json]

  linked  frames with LINKED blocks through the decode flag LZ4HIP_LZ4F_ACCEPT_LINKED: 4 096 frames of 256 KiB content in 64 KiB blocks
          (16 384 frames of 64 KiB would fit one block each, and such a frame cannot be linked), and 262 144 independent frames of 4 KiB
          as the all-independent control.  The linked frames are this library's own frames with the descriptor's FLG.5 cleared and HC
          recomputed -- valid linked frames whose matches happen not to reach back -- and, where liblz4 is found, LZ4F_compressFrame's,
          whose matches do.  Timed, decode only, taking turns:
            linked_flagged_ms            the flagged call on the linked batch        (liblz4_linked_flagged_ms: on liblz4's frames)
            independent_unflagged_ms     the unflagged call on the same content as independent frames
            control_flagged_ms / control_unflagged_ms    either call on the control: the flag must cost an independent batch nothing
            linked_size_query_ms - linked_refused_ms     the size pre-pass plus the plan alone, as a DIFFERENCE: the flagged call at
                                         dst_cap = 0 (walk, size pre-pass, plan, empty rounds, records; no block is decoded) minus the
                                         unflagged call on the linked batch (every item refused: walk, empty rounds, records)
          --unflagged-only times the unflagged rows alone, which a library from before the flag can run too: the parent's build beside
          this one in the same session (LZ4HIP_KEEP_LIBRARY over a copied library) is the check that the unflagged path is what it was.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lz4net_amd import _lib, batch, lz4_frame as lz  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=("small", "large", "linked"), required=True)
ap.add_argument("--unflagged-only", action="store_true", help="--case linked: only the rows that do not pass the flag")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--items", type=int, default=0, help="items of the case (default: 16384 small, 1024 large, 4096 linked)")
ap.add_argument("--loop-items", type=int, default=256)
ap.add_argument("--dists", default="2,3")
ap.add_argument("--out", default="")
args = ap.parse_args()
L = _lib.lib()
if L.lz4hip_device_count() <= 0:
    sys.exit("lz4f_batch_rate: no gfx950 device: nothing is measured without one")
ITEM = {"small": 65536, "large": 1 << 20, "linked": 262144}[args.case]
N = args.items or {"small": 16384, "large": 1024, "linked": 4096}[args.case]
BLOCK = 65536
out_path = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lz4f_batch", args.case + ".json")


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


def wall_ms(fn):
    """best-of-reps wall time of a function that reads values back itself"""
    fn()
    best = float("inf")
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def u8(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")


def i64(n):
    return torch.zeros(max(int(n), 1), dtype=torch.int64, device="cuda")


s = torch.cuda.current_stream().cuda_stream
results = {"_note": "every yardstick is timed in the SAME library and run as the batch calls; `loop` is wall time over --loop-items items and "
                    "its *_extrapolated_ms figures are per-item time times the item count, not measurements of the whole loop",
           "_library": L.lz4hip_build_id().decode(), "case": args.case, "items": N, "item_bytes": ITEM}


# ---- the linked case ---------------------------------------------------------------------------------------------------------------------
def encode_frames(data, n, item, eflags):
    """this library's frames of the n items of `item` bytes -> (frames, offsets)"""
    total = n * item
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * item
    bound = L.lz4hip_lz4f_batch_bound(n, total, 4, eflags)
    enc_out, enc_off, enc_scratch = u8(bound), i64(n + 1), u8(L.lz4hip_lz4f_batch_encode_scratch_bytes(n, total, 4))
    _lib.check(L.lz4hip_lz4f_batch_encode_device(data.data_ptr(), total, off.data_ptr(), n, 4, _lib.MODE_FAST, eflags, enc_out.data_ptr(), bound,
                                                 enc_off.data_ptr(), enc_scratch.data_ptr(), enc_scratch.numel(), s))
    return enc_out[:int(enc_off[n])].clone(), enc_off.clone()


def relinked(frames, frame_off, n, item, eflags):
    """the same frames with FLG.5 cleared and HC recomputed (every item has the same descriptor: the same size)"""
    out = frames.clone()
    flg = int(frames[4]) & ~0x20
    head = bytes([flg, int(frames[5])]) + (item.to_bytes(8, "little") if eflags & _lib.LZ4F_CONTENT_SIZE else b"")
    at = frame_off[:n]
    out[at + 4] = flg
    out[at + 4 + len(head)] = (lz._xxh32_small(head) >> 8) & 0xFF
    return out


def liblz4_frames(data, n, item):
    """LZ4F_compressFrame's linked frames of the items, or None where liblz4 is not found"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import lz4f_lib
    if lz4f_lib.load() is None:
        return None
    host = data.cpu().numpy()
    parts = [lz4f_lib.compress_frame(host[i * item:(i + 1) * item].tobytes(), 4, 0, False, False, True, linked=True) for i in range(n)]
    assert all(not p[4] & 0x20 for p in parts)
    lens = torch.tensor([0] + [len(p) for p in parts], dtype=torch.int64)
    import numpy as np
    return torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).cuda(), torch.cumsum(lens, 0).cuda()


def decoder(frames, frame_off, n, rows, flags, cap, out, scratch):
    """the bare batch decode call over preallocated buffers (the calls of one label share `out` and `scratch`: they take turns)
    -> (the call, a reader of its record)"""
    out_off, recs, info_dev, written = i64(n + 1), u8(C.sizeof(_lib.Lz4fInfo) * n), u8(256), i64(1)
    need = _lib.check(L.lz4hip_lz4f_batch_decode_scratch_bytes(n, 65536, rows, 0))
    assert need <= scratch.numel()
    call = lambda: _lib.check(L.lz4hip_lz4f_batch_decode_device(  # noqa: E731
        frames.data_ptr(), frames.numel(), frame_off.data_ptr(), n, 65536, rows, 0, flags, scratch.data_ptr(), need, out.data_ptr(), cap, out_off.data_ptr(),
        recs.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s))
    record = lambda: _lib.Lz4fBatchInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes()[:C.sizeof(_lib.Lz4fBatchInfo)])  # noqa: E731
    return call, record


def linked_case():
    small_item, small_n = 4096, N * ITEM // 4096
    accept = 0 if args.unflagged_only else _lib.LZ4F_ACCEPT_LINKED
    results.update(control_items=small_n, control_item_bytes=small_item, unflagged_only=bool(args.unflagged_only))
    for dist in [int(x) for x in args.dists.split(",") if x]:
        total = N * ITEM
        data = batch.synth(dist, 7, 0, total // batch.BLOCK).reshape(-1)
        rows = total // BLOCK
        for label, eflags, vflags in (("plain", 0, 0), ("both_checksums", _lib.LZ4F_BLOCK_CHECKSUM | _lib.LZ4F_CONTENT_CHECKSUM, 3)):
            eflags |= _lib.LZ4F_CONTENT_SIZE
            r = results[f"D{dist}/{label}"] = {"content_bytes": total, "blocks": rows}
            frames, frame_off = encode_frames(data, N, ITEM, eflags)
            linked = relinked(frames, frame_off, N, ITEM, eflags)
            control, control_off = encode_frames(data, small_n, small_item, eflags)
            fns = {}
            out = u8(total)
            scratch = u8(max(L.lz4hip_lz4f_batch_decode_scratch_bytes(N, 65536, rows, 0), L.lz4hip_lz4f_batch_decode_scratch_bytes(small_n, 65536, small_n, 0)))

            def add(name, fr, fo, n, nrows, flags, want_error, cap=None):
                call, record = decoder(fr, fo, n, nrows, flags, total if cap is None else cap, out, scratch)
                out.zero_()
                call()
                h = record()
                if want_error == 0:
                    assert (h.error, h.first_error, h.blocks, h.decoded_bytes) == (0, -1, nrows, total), (name, h.error, h.first_error, h.blocks, h.decoded_bytes)
                    assert cap is not None or torch.equal(out, data), name
                else:
                    assert h.error == want_error and h.first_error == 0 and h.decoded_bytes == 0, (name, h.error, h.decoded_bytes)
                fns[name] = call

            add("independent_unflagged_ms", frames, frame_off, N, rows, vflags, 0)
            add("control_unflagged_ms", control, control_off, small_n, small_n, vflags, 0)
            add("linked_refused_ms", linked, frame_off, N, rows, vflags, _lib.LZ4F_UNSUPPORTED_LINKED)
            if accept:
                add("linked_flagged_ms", linked, frame_off, N, rows, vflags | accept, 0)
                add("control_flagged_ms", control, control_off, small_n, small_n, vflags | accept, 0)
                add("linked_size_query_ms", linked, frame_off, N, rows, vflags | accept, 0, cap=0)
                theirs = liblz4_frames(data, N, ITEM) if label == "plain" else None
                if theirs is not None:
                    r["liblz4_frames_bytes"] = theirs[0].numel()
                    add("liblz4_linked_flagged_ms", theirs[0], theirs[1], N, rows, vflags | accept, 0)
            r["frames_bytes"] = frames.numel()
            r.update(event_ms(fns))
            if accept:
                r["prepass_plus_plan_ms_by_difference"] = r["linked_size_query_ms"] - r["linked_refused_ms"]
            for name in [k for k in r if k.endswith("flagged_ms")]:
                r[name.replace("_ms", "_GBps")] = total / r[name] / 1e6
            print(json.dumps({f"D{dist}/{label}": r}), flush=True)
            del frames, linked, control, fns, out, scratch
        del data


if args.case == "linked":
    linked_case()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
    sys.exit(0)

for dist in [int(x) for x in args.dists.split(",") if x]:
    total = N * ITEM
    data = batch.synth(dist, 7, 0, total // batch.BLOCK).reshape(-1)
    off = torch.arange(N + 1, dtype=torch.int64, device="cuda") * ITEM
    rows = total // BLOCK
    for label, eflags, vflags in (("plain", 0, 0), ("both_checksums", _lib.LZ4F_BLOCK_CHECKSUM | _lib.LZ4F_CONTENT_CHECKSUM, 3)):
        eflags |= _lib.LZ4F_CONTENT_SIZE
        r = results[f"D{dist}/{label}"] = {"content_bytes": total, "blocks": rows}
        # ---- encode -------------------------------------------------------------------------------------------------------------------
        bound = L.lz4hip_lz4f_batch_bound(N, total, 4, eflags)
        enc_out, enc_off = u8(bound), i64(N + 1)
        enc_scratch = u8(L.lz4hip_lz4f_batch_encode_scratch_bytes(N, total, 4))
        batch_encode = lambda: _lib.check(L.lz4hip_lz4f_batch_encode_device(  # noqa: E731
            data.data_ptr(), total, off.data_ptr(), N, 4, _lib.MODE_FAST, eflags, enc_out.data_ptr(), bound, enc_off.data_ptr(), enc_scratch.data_ptr(),
            enc_scratch.numel(), s))
        batch_encode()
        frame_off = enc_off.clone()
        frames = enc_out[:int(frame_off[N])].clone()
        r["frames_bytes"] = frames.numel()
        fns = {"batch_encode_ms": batch_encode}
        if label == "plain":
            sb = L.lz4hip_streams_bound(N, total, BLOCK)
            st_out, st_off = u8(sb), i64(N + 1)
            st_scratch = u8(L.lz4hip_streams_encode_scratch_bytes(N, total, BLOCK))
            streams_encode = lambda: _lib.check(L.lz4hip_streams_encode_device(  # noqa: E731
                data.data_ptr(), total, off.data_ptr(), N, BLOCK, _lib.MODE_FAST, st_out.data_ptr(), sb, st_off.data_ptr(), st_scratch.data_ptr(),
                st_scratch.numel(), s))
            streams_encode()
            packed_off = st_off.clone()
            packed = st_out[:int(packed_off[N])].clone()
            fns["streams_encode_ms"] = streams_encode
            stride = BLOCK + BLOCK // 255 + 16
            blk_out, blk_res = u8(rows * stride), torch.zeros(rows, dtype=torch.int32, device="cuda")
            eb = _lib.Batch(src=data.data_ptr(), src_off=None, src_stride=BLOCK, src_len=None, dst=blk_out.data_ptr(), dst_off=None, dst_stride=stride,
                            dst_cap=None, dst_cap_all=stride, src_len_all=BLOCK, result=blk_res.data_ptr(), n_blocks=rows)
            fns["blocks_encode_ms"] = lambda: _lib.check(L.lz4hip_encode_batch_device(C.byref(eb), _lib.MODE_FAST, s))
        r.update(event_ms(fns))
        k = min(args.loop_items, N)
        opts = dict(block_checksum=bool(eflags & 1), content_checksum=bool(eflags & 2))
        r["loop_items"] = k
        r["loop_encode_ms_per_item"] = wall_ms(lambda: [lz.compress_frame_device(data[i * ITEM:(i + 1) * ITEM], **opts) for i in range(k)]) / k
        r["loop_encode_extrapolated_ms"] = r["loop_encode_ms_per_item"] * N
        # ---- decode -------------------------------------------------------------------------------------------------------------------
        out, out_off = u8(total), i64(N + 1)
        recs, info_dev, written = u8(C.sizeof(_lib.Lz4fInfo) * N), u8(256), i64(1)
        need = _lib.check(L.lz4hip_lz4f_batch_decode_scratch_bytes(N, 65536, rows, 0))
        scratch = u8(need)
        r["batch_decode_scratch_bytes"] = need
        batch_decode = lambda: _lib.check(L.lz4hip_lz4f_batch_decode_device(  # noqa: E731
            frames.data_ptr(), frames.numel(), frame_off.data_ptr(), N, 65536, rows, 0, vflags, scratch.data_ptr(), need, out.data_ptr(), total,
            out_off.data_ptr(), recs.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s))
        out.zero_()
        batch_decode()
        h = _lib.Lz4fBatchInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes()[:C.sizeof(_lib.Lz4fBatchInfo)])
        assert (h.error, h.first_error, h.blocks, h.decoded_bytes) == (0, -1, rows, total) and torch.equal(out, data) and int(written.item()) == N, label
        fns = {"batch_decode_ms": batch_decode}
        if label == "plain":
            max_chunks = rows + 16
            sneed = L.lz4hip_streams_decode_into_scratch_bytes(N, max_chunks)
            sscratch, status, err_off, sinfo = u8(sneed), torch.zeros(N, dtype=torch.int32, device="cuda"), i64(N), u8(256)
            streams_decode = lambda: _lib.check(L.lz4hip_streams_decode_into_device(  # noqa: E731
                packed.data_ptr(), packed.numel(), packed_off.data_ptr(), N, max_chunks, sscratch.data_ptr(), sneed, out.data_ptr(), total, out_off.data_ptr(),
                status.data_ptr(), err_off.data_ptr(), sinfo.data_ptr(), written.data_ptr(), s))
            out.zero_()
            streams_decode()
            assert torch.equal(out, data), "streams"
            fns["streams_decode_ms"] = streams_decode
            lens = blk_res.clone()
            dec_out = u8(rows * BLOCK)
            db = _lib.Batch(src=blk_out.data_ptr(), src_off=None, src_stride=stride, src_len=lens.data_ptr(), dst=dec_out.data_ptr(), dst_off=None,
                            dst_stride=BLOCK, dst_cap=None, dst_cap_all=BLOCK, src_len_all=0, result=blk_res.data_ptr(), n_blocks=rows)
            fns["blocks_decode_ms"] = lambda: _lib.check(L.lz4hip_decode_batch_device(C.byref(db), 0, s))
        r.update(event_ms(fns))
        items = [frames[int(a):int(b)] for a, b in zip(frame_off[:k].tolist(), frame_off[1:k + 1].tolist())]
        r["loop_decode_ms_per_item"] = wall_ms(lambda: [lz.decompress_frame_device(f, verify=bool(vflags)) for f in items]) / k
        r["loop_decode_extrapolated_ms"] = r["loop_decode_ms_per_item"] * N
        for what in ("encode", "decode"):
            r[f"batch_{what}_GBps"] = total / r[f"batch_{what}_ms"] / 1e6
            r[f"loop_over_batch_{what}"] = r[f"loop_{what}_extrapolated_ms"] / r[f"batch_{what}_ms"]
        print(json.dumps({f"D{dist}/{label}": r}), flush=True)
        del enc_out, enc_scratch, out, scratch, frames, fns
    del data

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
