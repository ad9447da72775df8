"""A block batch encoded into one packed buffer (lz4hip_encode_packed_device) against the existing path on the same blocks: D2 and D3,
16 384 and 262 144 blocks of 64 KiB, fast mode.  Per case:

  - batch.encode into BOUND_STRIDE slots: event timings of the bare call into preallocated buffers -- the existing path, and the
    block encoder's own time;
  - lz4hip_encode_packed_device with round_blocks 0, 16 384 and 65 536 into a preallocated buffer of exactly packed_bytes: event
    timings, launch-only.  The pack's share is that time minus the slot path's; the scratch each form needs is recorded next to it;
  - batch.encode_packed as a user calls it (allocations and its one read-back included): event timings.

Best of five after one warm-up.  The packed bytes are checked against the slots' once per case.

    python tools/encode_packed_rate.py [--reps 5] [--blocks 16384,262144] [--out profiles/encode_packed/encode_packed_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lz4net_amd import _lib, batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--blocks", default="16384,262144")
ap.add_argument("--rounds", default="0,16384,65536")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "encode_packed", "encode_packed_rate.json"))
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


results = {}
for dist in (2, 3):
    for n in [int(x) for x in args.blocks.split(",")]:
        r = results[f"D{dist}/{n}"] = {"blocks": n, "bytes": n * batch.BLOCK}
        src = batch.synth(dist, 7, 0, n)
        s = torch.cuda.current_stream().cuda_stream

        # the existing path: one compressBound slot per block
        slots = torch.empty((n, batch.BOUND_STRIDE), dtype=torch.uint8, device="cuda")
        res = torch.empty(n, dtype=torch.int32, device="cuda")
        r["slots_ms"] = event_ms(lambda: batch.encode(src, batch.BLOCK, slots, batch.BOUND, result=res))
        r["slots_output_bytes"] = slots.numel()
        total = int(res.to(torch.int64).sum().item())
        r["packed_bytes"] = total
        keep = torch.arange(batch.BOUND_STRIDE, device="cuda")[None, :] < res[:, None]
        want = slots[keep]
        del slots, keep

        dst = torch.empty(total, dtype=torch.uint8, device="cuda")
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        plen = torch.empty(n, dtype=torch.int32, device="cuda")
        info = torch.empty(5, dtype=torch.int64, device="cuda")
        b = _lib.Batch(src=src.data_ptr(), src_stride=src.stride(0), src_len_all=batch.BLOCK, dst_cap_all=batch.BOUND, result=res.data_ptr(), n_blocks=n)
        for k in [int(x) for x in args.rounds.split(",")]:
            need = _lib.check(L.lz4hip_encode_packed_scratch_bytes(n, batch.BOUND, k))
            scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
            ms = event_ms(lambda: _lib.check(L.lz4hip_encode_packed_device(C.byref(b), _lib.MODE_FAST, k, dst.data_ptr(), total, off.data_ptr(),
                                                                           plen.data_ptr(), scratch.data_ptr(), need, info.data_ptr(), s)))
            h = batch.read_packed_info(info)
            assert (h.packed_bytes, h.written_blocks, h.first_failed) == (total, n, -1) and torch.equal(dst, want)
            r[f"packed_k{k}_ms"] = ms
            r[f"packed_k{k}_scratch_bytes"] = need
            r[f"packed_k{k}_pack_share_ms"] = ms - r["slots_ms"]
            r[f"packed_k{k}_pack_share"] = (ms - r["slots_ms"]) / r["slots_ms"]
            del scratch
        del dst, want
        r["encode_packed_python_ms"] = event_ms(lambda: batch.encode_packed(src, batch.BLOCK))
        r["slots_gbps"] = r["bytes"] / r["slots_ms"] / 1e6
        print(json.dumps({f"D{dist}/{n}": r}), flush=True)
        del src

if args.out:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
