"""LZ4 frames encoded against a dictionary (lz4hip_lz4f_batch_encode_dict_device), and the condition they were added under: the PLAIN
batch encode of frames takes what it took before.

  plain frames, parent against new   lz4hip_lz4f_batch_encode_device (fast mode) on --items records of 4 KiB, one frame each -- with
                                     --parent-lib, the parent commit's library: both libraries in this process, taking turns, each
                                     measured twice in the order parent, new, new, parent, so that the parent's two columns are its own
                                     run-to-run spread; the two builds must write the same bytes
  the dictionary call's own rate     the same records against the 64 KiB dictionary of tests/dict_cases.py through
                                     lz4hip_lz4f_batch_encode_dict_device; next to it lz4hip_encode_batch_dict_device on THE SAME blocks
                                     (capacity length - 1): the ratio is the cost of the frame bookkeeping around the same kernel

Event timings, best of --reps after one warm-up, the paths taking turns inside a repetition; the dictionary frames are decoded back with
lz4hip_lz4f_batch_decode_dict_device and compared with the records.  It needs a GPU.

    python tools/lz4f_dict_encode_rate.py [--items 16384] [--reps 30] [--parent-lib PATH] [--out profiles/lz4f_dict_encode/lz4f_dict_encode_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dict_cases as cases  # noqa: E402
from lz4net_amd import _lib, batch, lz4_frame as lz  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--unique", type=int, default=1024, help="records that are built; larger batches tile them")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4f_dict_encode", "lz4f_dict_encode_rate.json"))
args = ap.parse_args()
RECORD, BLOCK_ID, FLAGS = 4096, 4, 4                                    # (LZ4HIP_LZ4F_CONTENT_SIZE)


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


def typed(path):
    """another build of the library in this process, its calls typed"""
    lib = C.CDLL(path)
    for name, res, argtypes in _lib.SYMBOLS:
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, argtypes
    return lib


def main():
    L = _lib.lib()
    dic = cases.fixture_dictionary()
    d_dev = torch.from_numpy(dic).cuda()
    records = [cases.fixture_record(cases.FIXTURE_SEED, 1000 + k, RECORD) for k in range(args.unique)]
    n = args.items
    unique_dev = torch.from_numpy(np.frombuffer(b"".join(records), np.uint8).reshape(len(records), RECORD).copy()).cuda()
    src = unique_dev[torch.arange(n, device="cuda") % args.unique].contiguous()
    flat = src.reshape(-1)
    off = torch.arange(0, (n + 1) * RECORD, RECORD, dtype=torch.int64, device="cuda")
    report = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "record_bytes": RECORD, "dictionary_bytes": int(dic.size), "items": n,
              "note": "one box, one run"}

    # ---- the plain batch encode of frames, parent against new
    bound = L.lz4hip_lz4f_batch_bound(n, flat.numel(), BLOCK_ID, FLAGS)
    need = L.lz4hip_lz4f_batch_encode_scratch_bytes(n, flat.numel(), BLOCK_ID)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

    def plain(lib):
        _lib.check(lib.lz4hip_lz4f_batch_encode_device(flat.data_ptr(), flat.numel(), off.data_ptr(), n, BLOCK_ID, _lib.MODE_FAST, FLAGS, out.data_ptr(), bound,
                                                       out_off.data_ptr(), scratch.data_ptr(), need, batch._stream()))

    if args.parent_lib:
        parent = typed(args.parent_lib)
        images = []
        for lib in (parent, L):
            out.zero_()
            plain(lib)
            torch.cuda.synchronize()
            images.append((out_off.clone(), out[:int(out_off[n].item())].clone()))
        assert torch.equal(images[0][0], images[1][0]) and torch.equal(images[0][1], images[1][1]), "the two builds do not write the same bytes"
        ms = event_ms({"parent_a": lambda: plain(parent), "new_a": lambda: plain(L), "new_b": lambda: plain(L), "parent_b": lambda: plain(parent)})
        best_parent, best_new = min(ms["parent_a"], ms["parent_b"]), min(ms["new_a"], ms["new_b"])
        spread = abs(ms["parent_a"] - ms["parent_b"]) / best_parent
        report["plain_parent_vs_new"] = {"ms": ms, "parent_spread": spread, "new_over_parent_best": best_new / best_parent,
                                         "difference_within_parent_spread": abs(best_new - best_parent) / best_parent <= spread,
                                         "GB_per_s_in_new": flat.numel() / best_new / 1e6}
        print("plain", json.dumps(report["plain_parent_vs_new"]), flush=True)

    # ---- the dictionary call, and the block batch call on the same blocks
    dbound = L.lz4hip_lz4f_batch_dict_bound(n, flat.numel(), BLOCK_ID, FLAGS, dic.size, 7)
    dneed = L.lz4hip_lz4f_batch_encode_dict_scratch_bytes(n, flat.numel(), BLOCK_ID, dic.size)
    dout = torch.empty(dbound, dtype=torch.uint8, device="cuda")
    dscratch = torch.empty(dneed, dtype=torch.uint8, device="cuda")
    table = torch.empty(L.lz4hip_encode_dict_scratch_bytes(dic.size), dtype=torch.uint8, device="cuda")
    comp = torch.empty((n, RECORD), dtype=torch.uint8, device="cuda")
    res = torch.empty(n, dtype=torch.int32, device="cuda")

    def frames_dict():
        _lib.check(L.lz4hip_lz4f_batch_encode_dict_device(flat.data_ptr(), flat.numel(), off.data_ptr(), n, d_dev.data_ptr(), d_dev.numel(), 7, BLOCK_ID, FLAGS,
                                                          dout.data_ptr(), dbound, out_off.data_ptr(), dscratch.data_ptr(), dneed, batch._stream()))

    def blocks_dict():
        b, keep = batch._make_batch(src, RECORD, comp, RECORD - 1, res)
        _lib.check(L.lz4hip_encode_batch_dict_device(C.byref(b), d_dev.data_ptr(), d_dev.numel(), table.data_ptr(), table.numel(), batch._stream()))

    frames_dict()
    blocks_dict()
    torch.cuda.synchronize()
    total = int(out_off[n].item())
    data, data_off = lz.decompress_frames_device(dout[:total], out_off, max_blocks=n + 16, dictionary=d_dev, dict_id=7)
    assert torch.equal(data, flat), "the dictionary's frames do not decode to the records"
    assert bool((res > 0).all()) and total == int(res.sum().item()) + n * (19 + 4 + 4), "the frames hold the block call's blocks"
    ms = event_ms({"frames_dict": frames_dict, "blocks_dict": blocks_dict, "frames_plain": lambda: plain(L)})
    report["dictionary_call"] = {"ms": ms, "GB_per_s_in": {k: flat.numel() / v / 1e6 for k, v in ms.items()},
                                 "frames_dict_over_blocks_dict": ms["frames_dict"] / ms["blocks_dict"],
                                 "frames_dict_over_frames_plain": ms["frames_dict"] / ms["frames_plain"],
                                 "frame_bytes_per_record": total / n}
    print("dict", json.dumps(report["dictionary_call"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
