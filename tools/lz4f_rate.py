"""LZ4 frames (lz4hip_lz4f_*_device) against the legacy frame's calls on the same content at the same block / chunk sizes: D2 and D3,
--bytes of content (default 1 GiB), blocks of 64 KiB and of 4 MiB.  Event timings of the bare calls into preallocated buffers, best of
--reps after one warm-up, the paths taking turns inside a repetition:

  decode   lz4hip_lz4f_decode_device without verification against lz4hip_frame_decode_compact_device (the framing differs by a constant,
           the block decode is the same code).  The legacy call is timed TWICE under two names (legacy_a / legacy_b): their difference is
           what repetitions of one path alone give, and no difference between the formats below it means anything.
           + the same decode with LZ4HIP_LZ4F_VERIFY_BLOCKS on a frame that carries block checksums: the added time.
  encode   lz4hip_lz4f_encode_device (no options) against lz4hip_frame_encode_device (twice, as above), + with LZ4HIP_LZ4F_BLOCK_CHECKSUM.
  content  lz4hip_xxh32_rows_device on ONE row of --row-bytes (default 256 MiB) of the content: the single-row rate in GB/s that
           LZ4HIP_LZ4F_VERIFY_CONTENT / LZ4HIP_LZ4F_CONTENT_CHECKSUM pay per byte; and on the content as rows of 64 KiB: the many-rows rate.

The legacy frame's code is the parent commit's, unchanged, in the same library.  Every output is compared with the source once per case.

    python tools/lz4f_rate.py [--reps 5] [--bytes 1073741824] [--row-bytes 268435456] [--out profiles/lz4f/lz4f_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lz4net_amd import _lib, batch, legacy_frame as lf, lz4_frame as lz  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--bytes", type=int, default=1 << 30)
ap.add_argument("--row-bytes", type=int, default=1 << 28)
ap.add_argument("--dists", default="2,3")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lz4f", "lz4f_rate.json"))
args = ap.parse_args()
L = _lib.lib()
if L.lz4hip_device_count() <= 0:
    sys.exit("lz4f_rate: no gfx950 device: nothing is measured without one")


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


def u8(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")


results = {"_note": "the legacy frame's calls (legacy_a / legacy_b) are timed in the SAME library as the lz4f calls, not in a build of the "
                    "parent commit: their code is that commit's, unchanged.  This is not a cross-build comparison.",
           "_library": L.lz4hip_build_id().decode()}
s = torch.cuda.current_stream().cuda_stream
for dist in [int(x) for x in args.dists.split(",") if x]:
    data = batch.synth(dist, 7, 0, (args.bytes + batch.BLOCK - 1) // batch.BLOCK).reshape(-1)[:args.bytes]
    n = data.numel()

    # ---- the checksum kernel alone --------------------------------------------------------------------------------------------------
    r = results[f"D{dist}/xxh32"] = {"row_bytes": min(args.row_bytes, n), "rows_bytes": n}
    sums = torch.empty(n // 65536 + 1, dtype=torch.int32, device="cuda")
    one = lambda: _lib.check(L.lz4hip_xxh32_rows_device(data.data_ptr(), None, 0, None, r["row_bytes"], 0, sums.data_ptr(), 1, s))  # noqa: E731
    many = lambda: _lib.check(L.lz4hip_xxh32_rows_device(data.data_ptr(), None, 65536, None, 65536, 0, sums.data_ptr(), n // 65536, s))  # noqa: E731
    r.update(event_ms({"one_row_ms": one, "rows_64k_ms": many}))
    r["one_row_GBps"] = r["row_bytes"] / r["one_row_ms"] / 1e6
    r["rows_64k_GBps"] = (n // 65536) * 65536 / r["rows_64k_ms"] / 1e6
    print(json.dumps({f"D{dist}/xxh32": r}), flush=True)

    for block in (65536, 4 << 20):
        bid = lz.BLOCK_SIZES[block]
        r = results[f"D{dist}/{block}"] = {"block_bytes": block, "content_bytes": n}
        blocks = (n + block - 1) // block
        m = blocks + 16
        out_len = torch.zeros(1, dtype=torch.int64, device="cuda")

        # ---- encode -----------------------------------------------------------------------------------------------------------------
        frames = {}
        fns = {}
        enc_scratch = u8(max(L.lz4hip_lz4f_encode_scratch_bytes(n, bid), L.lz4hip_frame_encode_scratch_bytes(n, block)))
        enc_out = u8(max(L.lz4hip_lz4f_bound(n, bid, 7), L.lz4hip_frame_bound(n, block)))
        for name, flags in (("lz4f_encode_ms", 0), ("lz4f_encode_block_checksum_ms", _lib.LZ4F_BLOCK_CHECKSUM)):
            fns[name] = lambda flags=flags: _lib.check(L.lz4hip_lz4f_encode_device(
                data.data_ptr(), n, bid, _lib.MODE_FAST, flags, enc_out.data_ptr(), enc_out.numel(), out_len.data_ptr(), enc_scratch.data_ptr(),
                enc_scratch.numel(), s))
            fns[name]()
            frames[flags] = enc_out[:int(out_len.item())].clone()
        legacy_encode = lambda: _lib.check(L.lz4hip_frame_encode_device(data.data_ptr(), n, block, _lib.MODE_FAST, enc_out.data_ptr(), enc_out.numel(),  # noqa: E731
                                                                        out_len.data_ptr(), enc_scratch.data_ptr(), enc_scratch.numel(), s))
        legacy_encode()
        legacy = enc_out[:int(out_len.item())].clone()
        fns["legacy_a_encode_ms"] = fns["legacy_b_encode_ms"] = legacy_encode
        r["lz4f_frame_bytes"], r["legacy_frame_bytes"] = frames[0].numel(), legacy.numel()
        r.update(event_ms(fns))
        del enc_scratch, enc_out

        # ---- decode -----------------------------------------------------------------------------------------------------------------
        out = u8(n)
        info_dev = torch.zeros(max(C.sizeof(_lib.Lz4fInfo), C.sizeof(_lib.FrameInfo)), dtype=torch.uint8, device="cuda")
        need = _lib.check(L.lz4hip_lz4f_decode_scratch_bytes(block, m, 0))
        lneed = _lib.check(L.lz4hip_frame_decode_compact_scratch_bytes(block, m, 0))
        scratch = u8(max(need, lneed))
        r["lz4f_decode_scratch_bytes"], r["legacy_decode_scratch_bytes"] = need, lneed
        fns = {}
        for name, frame, flags in (("lz4f_decode_ms", frames[0], 0), ("lz4f_decode_verify_blocks_ms", frames[_lib.LZ4F_BLOCK_CHECKSUM], _lib.LZ4F_VERIFY_BLOCKS)):
            fns[name] = lambda frame=frame, flags=flags: _lib.check(L.lz4hip_lz4f_decode_device(
                frame.data_ptr(), frame.numel(), block, m, 0, flags, scratch.data_ptr(), need, out.data_ptr(), n, info_dev.data_ptr(), s))
            out.zero_()
            fns[name]()
            h = _lib.Lz4fInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes()[:C.sizeof(_lib.Lz4fInfo)])
            assert (h.error, h.blocks, h.decoded_bytes) == (_lib.LZ4F_OK, blocks, n) and torch.equal(out[:n], data), name
        legacy_decode = lambda: _lib.check(L.lz4hip_frame_decode_compact_device(legacy.data_ptr(), legacy.numel(), block, m, 0, scratch.data_ptr(), lneed,  # noqa: E731
                                                                                out.data_ptr(), n, info_dev.data_ptr(), s))
        out.zero_()
        legacy_decode()
        h = _lib.FrameInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes()[:C.sizeof(_lib.FrameInfo)])
        assert (h.error, h.decoded_bytes) == (_lib.FRAME_OK, n) and torch.equal(out[:n], data)
        fns["legacy_a_decode_ms"] = fns["legacy_b_decode_ms"] = legacy_decode
        r.update(event_ms(fns))
        for what in ("encode", "decode"):
            a, b = r[f"legacy_a_{what}_ms"], r[f"legacy_b_{what}_ms"]
            r[f"legacy_{what}_spread"] = abs(a - b) / min(a, b)
            r[f"lz4f_{what}_over_legacy"] = r[f"lz4f_{what}_ms"] / min(a, b)
        r["verify_blocks_added_ms"] = r["lz4f_decode_verify_blocks_ms"] - r["lz4f_decode_ms"]
        r["block_checksum_added_ms"] = r["lz4f_encode_block_checksum_ms"] - r["lz4f_encode_ms"]
        print(json.dumps({f"D{dist}/{block}": r}), flush=True)
        del out, scratch, frames, legacy, fns
    del data

if args.out:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
