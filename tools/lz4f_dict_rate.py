"""LZ4 frames decoded with a dictionary (lz4hip_lz4f_batch_decode_dict_device), and the condition they were added under: the PLAIN batch
decode of frames takes what it took before.

  plain frames, parent against new   lz4hip_lz4f_batch_decode_device on an all-independent batch (--items records of 4 KiB, one frame
                                     each, written by the library) and on an all-linked batch (--linked-items frames of 150 000 bytes,
                                     three linked blocks each, written by liblz4) -- with --parent-lib, the parent commit's library: both
                                     libraries in this process, taking turns, each measured twice, so that the first pair of columns is
                                     the parent's own run-to-run spread
  the dictionary calls' own rate     --items frames of one 4 KiB record each, written by liblz4's LZ4F_compressFrame_usingCDict against the
                                     64 KiB dictionary of tests/dict_cases.py, through lz4hip_lz4f_batch_decode_dict_device; next to it
                                     lz4hip_decode_batch_dict_device on THE SAME blocks, taken out of the frames; and the linked batch
                                     written against the dictionary

Event timings, best of --reps after one warm-up, the paths taking turns inside a repetition; every decode is compared with the source.
It needs liblz4 (found with ctypes.util.find_library; nothing is downloaded) and a GPU.

    python tools/lz4f_dict_rate.py [--items 16384] [--linked-items 1024] [--reps 5] [--parent-lib PATH] [--out profiles/lz4f_dict/lz4f_dict_rate.json]
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
import lz4f_dict_lib  # noqa: E402
import lz4f_lib  # noqa: E402
from lz4net_amd import _lib, batch, lz4_frame as lz  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--linked-items", type=int, default=1024)
ap.add_argument("--unique", type=int, default=1024, help="records that are built; larger batches tile them")
ap.add_argument("--unique-linked", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4f_dict", "lz4f_dict_rate.json"))
args = ap.parse_args()
RECORD, LINKED_BYTES, ACCEPT = 4096, 150000, 8


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


def dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).cuda()


class FrameBatch:
    """n frames on the device (the unique ones tiled) with everything a decode call needs, allocated once"""
    def __init__(self, frames, contents, n, rows_per_item):
        pick = [k % len(frames) for k in range(n)]
        self.n, self.rows = n, n * rows_per_item + 16
        self.src = dev(b"".join(frames[k] for k in pick))
        self.off = torch.tensor(np.cumsum([0] + [len(frames[k]) for k in pick]), dtype=torch.int64, device="cuda")
        self.want = dev(b"".join(contents[k] for k in pick))
        self.need = _lib.lib().lz4hip_lz4f_batch_decode_scratch_bytes(n, 65536, self.rows, 0)
        self.scratch = torch.empty(self.need, dtype=torch.uint8, device="cuda")
        self.out = torch.empty(self.want.numel(), dtype=torch.uint8, device="cuda")
        self.out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        self.recs = torch.zeros(C.sizeof(_lib.Lz4fInfo) * n, dtype=torch.uint8, device="cuda")
        self.info = torch.zeros(C.sizeof(_lib.Lz4fBatchInfo), dtype=torch.uint8, device="cuda")
        self.written = torch.zeros(1, dtype=torch.int64, device="cuda")

    def plain(self, lib):
        _lib.check(lib.lz4hip_lz4f_batch_decode_device(self.src.data_ptr(), self.src.numel(), self.off.data_ptr(), self.n, 65536, self.rows, 0, ACCEPT,
                                                       self.scratch.data_ptr(), self.need, self.out.data_ptr(), self.out.numel(), self.out_off.data_ptr(),
                                                       self.recs.data_ptr(), self.info.data_ptr(), self.written.data_ptr(), batch._stream()))

    def with_dict(self, lib, d):
        _lib.check(lib.lz4hip_lz4f_batch_decode_dict_device(self.src.data_ptr(), self.src.numel(), self.off.data_ptr(), self.n, d.data_ptr(), d.numel(), 0,
                                                            65536, self.rows, 0, ACCEPT, self.scratch.data_ptr(), self.need, self.out.data_ptr(),
                                                            self.out.numel(), self.out_off.data_ptr(), self.recs.data_ptr(), self.info.data_ptr(),
                                                            self.written.data_ptr(), batch._stream()))

    def check(self, fn, name):
        self.out.zero_()
        fn()
        torch.cuda.synchronize()
        info = _lib.Lz4fBatchInfo.from_buffer_copy(self.info.cpu().numpy().tobytes())
        assert info.error == 0 and info.decoded_bytes == self.want.numel() and torch.equal(self.out, self.want), (name, info.error, info.first_error)


def parent_vs_new(fb, parent, new, name):
    for lib in (parent, new):
        fb.check(lambda: fb.plain(lib), name)
    # (parent, new, new, parent: neither library always runs behind the other)
    ms = event_ms({"parent_a": lambda: fb.plain(parent), "new_a": lambda: fb.plain(new), "new_b": lambda: fb.plain(new), "parent_b": lambda: fb.plain(parent)})
    row = {"ms": ms, "parent_spread": abs(ms["parent_a"] - ms["parent_b"]) / min(ms["parent_a"], ms["parent_b"]),
           "new_over_parent_best": min(ms["new_a"], ms["new_b"]) / min(ms["parent_a"], ms["parent_b"]),
           "GB_per_s_out_new": fb.want.numel() / min(ms["new_a"], ms["new_b"]) / 1e6}
    print(name, json.dumps(row), flush=True)
    return row


def linked_source(k):
    """150 000 bytes of the records' kind of text: three linked blocks whose matches reach back across the block boundaries"""
    return cases.fixture_record(cases.FIXTURE_SEED, 500000 + k, LINKED_BYTES)


def main():
    assert lz4f_dict_lib.load() is not None, "liblz4 >= 1.8.0 with the dictionary calls is needed to write the frames"
    L = _lib.lib()
    dic = cases.fixture_dictionary().tobytes()
    d_dev = dev(dic)
    records = [cases.fixture_record(cases.FIXTURE_SEED, 1000 + k, RECORD) for k in range(args.unique)]
    report = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "record_bytes": RECORD, "dictionary_bytes": len(dic), "items": args.items,
              "linked_items": args.linked_items, "linked_item_bytes": LINKED_BYTES, "writer": "liblz4 %d" % lz4f_lib.load().LZ4_versionNumber(),
              "note": "one box, one run"}

    # ---- the plain batch decode: independent items from the library's own writer, linked items from liblz4
    t = dev(b"".join(records))
    offs = torch.arange(0, (args.unique + 1) * RECORD, RECORD, dtype=torch.int64, device="cuda")
    packed, packed_off = lz.compress_frames_device(t, offs)
    packed_h, packed_off_h = packed.cpu().numpy().tobytes(), packed_off.cpu().numpy()
    independent = FrameBatch([packed_h[packed_off_h[k]:packed_off_h[k + 1]] for k in range(args.unique)], records, args.items, 1)
    linked_src = [linked_source(k) for k in range(args.unique_linked)]
    linked_frames = [lz4f_lib.compress_frame(s, 4, 0, linked=True) for s in linked_src]
    assert all(not f[4] & 0x20 for f in linked_frames)
    linked = FrameBatch(linked_frames, linked_src, args.linked_items, 3)
    if args.parent_lib:
        parent = typed(args.parent_lib)
        report["plain_parent_vs_new"] = {"independent": parent_vs_new(independent, parent, L, "independent"),
                                         "linked": parent_vs_new(linked, parent, L, "linked")}

    # ---- the dictionary calls: frames of one record each against the dictionary, and the same blocks through the block batch call
    frames = [lz4f_dict_lib.compress_frame(r, dic) for r in records]
    blocks = []
    for f in frames:
        assert f[4] & 0x20 and not f[4] & 0x09 and not f[10] & 0x80, "one compressed block behind a 7-byte descriptor"
        size = int.from_bytes(f[7:11], "little")
        blocks.append(f[11:11 + size])
    with_dict = FrameBatch(frames, records, args.items, 1)
    pick = torch.arange(args.items, device="cuda") % args.unique
    width = (max(len(b) for b in blocks) + 31) // 16 * 16
    h = np.zeros((len(blocks), width), np.uint8)
    for i, b in enumerate(blocks):
        h[i, :len(b)] = np.frombuffer(b, np.uint8)
    rows = torch.from_numpy(h).cuda()[pick].contiguous()
    lens = torch.tensor([len(b) for b in blocks], dtype=torch.int32, device="cuda")[pick].contiguous()
    out = torch.empty((args.items, RECORD), dtype=torch.uint8, device="cuda")
    res = torch.empty(args.items, dtype=torch.int32, device="cuda")

    def block_batch():
        b, keep = batch._make_batch(rows, lens, out, RECORD, res)
        _lib.check(L.lz4hip_decode_batch_dict_device(C.byref(b), d_dev.data_ptr(), d_dev.numel(), 0, batch._stream()))

    block_batch()
    torch.cuda.synchronize()
    assert bool((res == RECORD).all()) and torch.equal(out.reshape(-1), with_dict.want)
    linked_dict_frames = [lz4f_dict_lib.compress_frame(s, dic, linked=True) for s in linked_src]
    assert all(not f[4] & 0x20 for f in linked_dict_frames)
    linked_dict = FrameBatch(linked_dict_frames, linked_src, args.linked_items, 3)
    fns = {"frames_dict": lambda: with_dict.with_dict(L, d_dev), "blocks_dict": block_batch, "frames_plain_independent": lambda: independent.plain(L),
           "linked_dict": lambda: linked_dict.with_dict(L, d_dev), "linked_plain": lambda: linked.plain(L)}
    with_dict.check(fns["frames_dict"], "frames_dict")
    linked_dict.check(fns["linked_dict"], "linked_dict")
    ms = event_ms(fns)
    sizes = {"frames_dict": with_dict.want.numel(), "blocks_dict": with_dict.want.numel(), "frames_plain_independent": independent.want.numel(),
             "linked_dict": linked_dict.want.numel(), "linked_plain": linked.want.numel()}
    report["dictionary_calls"] = {"ms": ms, "GB_per_s_out": {k: sizes[k] / v / 1e6 for k, v in ms.items()},
                                  "frames_dict_over_blocks_dict": ms["frames_dict"] / ms["blocks_dict"],
                                  "compressed_bytes_per_record": {"with_dictionary": sum(map(len, blocks)) / len(blocks)}}
    print(json.dumps(report["dictionary_calls"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
