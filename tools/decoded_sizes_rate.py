"""lz4hip_decoded_sizes_device against the only other way to learn a batch's decoded sizes, an unknown-size decode
(lz4hip_decode_batch_device, known_output_size = 0), on device-resident batches of 64 KiB blocks: event timings, best of `reps` after a
warm-up.  The decoder gets a capacity of 64 KiB + 64 per block -- far less memory than the format's worst case a caller without the
sizes would have to reserve, and no slower for it.  Every size is checked.

    python tools/decoded_sizes_rate.py [reps] [out.json] [blocks ...]
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lz4net_amd import _lib, batch  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_json = sys.argv[2] if len(sys.argv) > 2 else None
sizes = [int(a) for a in sys.argv[3:]] or [16384, 262144]
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream


def best(fn, n=reps):
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
    return min(ts), sorted(ts)


results = {"build_id": L.lz4hip_build_id().decode(), "device": L.lz4hip_codec_name().decode(), "reps": reps, "cases": {}}
for n in sizes:
    for dist in (2, 3):
        comp = torch.empty((n, batch.BOUND_STRIDE), dtype=torch.uint8, device="cuda")
        clen = torch.empty(n, dtype=torch.int32, device="cuda")
        for first in range(0, n, 16384):                                # (the raw blocks are not kept: 16 384 at a time)
            k = min(16384, n - first)
            raw = batch.synth(dist, 7, first, k)
            batch.encode(raw, batch.BLOCK, comp[first:first + k], batch.BOUND, result=clen[first:first + k])
        torch.cuda.synchronize()
        del raw
        r = results["cases"][f"D{dist}_{n}x64KiB"] = {"blocks": n, "compressed_bytes": int(clen.sum().item())}
        need = L.lz4hip_decoded_sizes_scratch_bytes(n)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        res = torch.empty(n, dtype=torch.int32, device="cuda")
        cap = torch.empty(n, dtype=torch.int32, device="cuda")
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        info = torch.empty(4, dtype=torch.int64, device="cuda")
        b = _lib.Batch(src=comp.data_ptr(), src_stride=comp.stride(0), src_len=clen.data_ptr(), result=res.data_ptr(), n_blocks=n)
        r["sizes_ms"], r["sizes_ms_all"] = best(lambda: _lib.check(L.lz4hip_decoded_sizes_device(
            C.byref(b), off.data_ptr(), cap.data_ptr(), scratch.data_ptr(), need, info.data_ptr(), s)))
        i = batch.read_sizes_info(info)
        assert (i.blocks, i.decoded_bytes, i.first_error) == (n, n * batch.BLOCK, -1) and bool((res == batch.BLOCK).all())
        out = torch.empty((n, batch.BLOCK + 64), dtype=torch.uint8, device="cuda")
        r["decode_unknown_ms"], r["decode_unknown_ms_all"] = best(lambda: batch.decode(comp, clen, out, batch.BLOCK + 64, known_output_size=False, result=res))
        assert bool((res == batch.BLOCK).all())
        r["sizes_over_decode"] = r["sizes_ms"] / r["decode_unknown_ms"]
        r["sizes_blocks_per_us"] = n / r["sizes_ms"] / 1e3
        r["sizes_compressed_GBps"] = r["compressed_bytes"] / r["sizes_ms"] / 1e6
        del out, comp, scratch
        torch.cuda.synchronize()
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}), flush=True)

if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(results, fh, indent=1)
