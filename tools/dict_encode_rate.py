"""Block batches encoded against a shared dictionary (lz4hip_encode_batch_dict_device) against what the library already had, on the
same records: --records (default 16 384 and 262 144) records of 4 KiB, JSON-like text (tests/dict_cases.py fixture_record), against
the fixture's 64 KiB dictionary.

  dict        the dictionary call (priming kernel and block kernel)
  plain       lz4hip_encode_batch_device, fast mode, default dispatch, on the same records
  dict_len_0  the dictionary call with dict_len = 0
  prime       the dictionary call on ONE 12-byte block: the priming kernel, the table's copy into one wavefront's LDS and two launches

Event timings, best of --reps after one warm-up, the paths taking turns inside a repetition; every dictionary encode is decoded back
with lz4hip_decode_batch_dict_device and compared with the source.  The compressed size per record is set beside what liblz4's
LZ4_loadDict + LZ4_compress_fast_continue gives for the same records where liblz4 is installed.  With --parent-lib, the parent commit's
library: the condition that the plain fast encode of the bench's D2 and D3 at 4 096 and 16 384 blocks takes what it takes with the
parent's build -- both libraries in this process, taking turns, each measured twice so that the parent's own spread is seen.

    python tools/dict_encode_rate.py [--records 16384 262144] [--reps 5] [--parent-lib PATH] [--out profiles/dict_encode/dict_encode_rate.json]
"""
import argparse
import ctypes as C
import ctypes.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dict_cases as cases  # noqa: E402
from lz4net_amd import _lib, batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, nargs="+", default=[16384, 262144])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--unique", type=int, default=2048, help="records that are built; larger batches tile them")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_encode", "dict_encode_rate.json"))
args = ap.parse_args()
RECORD = 4096
CAP = batch.compress_bound(RECORD)


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


def liblz4_sizes(plain, dic):
    """bytes per record from LZ4_loadDict + LZ4_compress_fast_continue, and from LZ4_compress_default (None: no liblz4 here)"""
    path = ctypes.util.find_library("lz4")
    if not path:
        return None
    lz4 = C.CDLL(path)
    lz4.LZ4_createStream.restype = C.c_void_p
    lz4.LZ4_freeStream.argtypes = [C.c_void_p]
    lz4.LZ4_loadDict.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lz4.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    lz4.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    cap = lz4.LZ4_compressBound(RECORD)
    out = C.create_string_buffer(cap)
    d = dic.tobytes()
    with_dict = without = 0
    for p in plain:
        stream = lz4.LZ4_createStream()
        lz4.LZ4_loadDict(stream, d, len(d))
        with_dict += lz4.LZ4_compress_fast_continue(stream, p, out, RECORD, cap, 1)
        lz4.LZ4_freeStream(stream)
        without += lz4.LZ4_compress_default(p, out, RECORD, cap)
    return {"version": lz4.LZ4_versionNumber(), "with_dictionary": with_dict / len(plain), "without": without / len(plain)}


def main():
    L = _lib.lib()
    dic = cases.fixture_dictionary()
    plain = [cases.fixture_record(cases.FIXTURE_SEED, 1000 + k, RECORD) for k in range(args.unique)]
    d_dev = torch.from_numpy(dic).cuda()
    scratch = torch.empty(L.lz4hip_encode_dict_scratch_bytes(dic.size), dtype=torch.uint8, device="cuda")
    plain_dev = torch.from_numpy(np.frombuffer(b"".join(plain), np.uint8).reshape(len(plain), RECORD).copy()).cuda()
    report = {"unique_records": args.unique, "record_bytes": RECORD, "dictionary_bytes": int(dic.size), "reps": args.reps,
              "device": torch.cuda.get_device_name(0), "batches": {}, "note": "one box, one run"}
    for n in args.records:
        pick = torch.arange(n, device="cuda") % args.unique
        src = plain_dev[pick].contiguous()
        comp = torch.empty((n, CAP + 16), dtype=torch.uint8, device="cuda")
        res = torch.empty(n, dtype=torch.int32, device="cuda")
        one_res = torch.empty(1, dtype=torch.int32, device="cuda")

        def dict_call(dict_len, blocks=None):
            if blocks is None:
                b, keep = batch._make_batch(src, RECORD, comp, CAP, res)
            else:
                b, keep = batch._make_batch(src[:1], 12, comp[:1], CAP, one_res)
            _lib.check(L.lz4hip_encode_batch_dict_device(C.byref(b), d_dev.data_ptr() if dict_len else None, dict_len,
                                                         scratch.data_ptr() if dict_len else None, scratch.numel() if dict_len else 0, batch._stream()))

        fns = {"dict": lambda: dict_call(dic.size), "plain": lambda: batch.encode(src, RECORD, comp, CAP, result=res), "dict_len_0": lambda: dict_call(0),
               "prime": lambda: dict_call(dic.size, 1)}
        sizes = {}
        for name in ("plain", "dict_len_0", "dict"):                   # (dict last: its blocks are the ones decoded back)
            comp.zero_()
            fns[name]()
            torch.cuda.synchronize()
            assert (res > 0).all(), name
            sizes[name] = float(res[:args.unique if n >= args.unique else n].double().mean())
        back = torch.zeros_like(src)
        used = batch.decode_dict(comp, res, back, RECORD, d_dev)
        torch.cuda.synchronize()
        assert torch.equal(used, res) and torch.equal(back, src), "the dictionary's blocks do not decode to the records"
        assert sizes["plain"] == sizes["dict_len_0"]
        ms = event_ms(fns)
        row = {"ms": ms, "GB_per_s_in": {k: n * RECORD / v / 1e6 for k, v in ms.items() if k != "prime"},
               "compressed_bytes_per_record": {"dict": sizes["dict"], "plain": sizes["plain"]},
               "dict_over_plain": ms["dict"] / ms["plain"], "dict_len_0_over_plain": ms["dict_len_0"] / ms["plain"]}
        report["batches"][str(n)] = row
        print(n, json.dumps(row), flush=True)
        del src, comp, back
    report["liblz4_bytes_per_record"] = liblz4_sizes(plain, dic)
    print(json.dumps(report["liblz4_bytes_per_record"]), flush=True)
    if args.parent_lib:
        report["plain_encode_parent_vs_new"] = parent_vs_new(typed(args.parent_lib), L)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


def parent_vs_new(parent, new):
    """lz4hip_encode_batch_device (fast mode, default dispatch) on the bench's D2 and D3 at 4 096 and 16 384 blocks of 64 KiB: the parent's
    build and this one take turns; each appears twice, so the first pair of columns is the parent's own run-to-run spread"""
    out = {}
    for dist in (2, 3):
        for n in (4096, 16384):
            raw = batch.synth(dist, 4242, 0, n)
            comp = torch.empty((n, batch.BOUND_STRIDE), dtype=torch.uint8, device="cuda")
            res = torch.empty(n, dtype=torch.int32, device="cuda")

            def call(lib):
                b, keep = batch._make_batch(raw, batch.BLOCK, comp, batch.BOUND, res)
                _lib.check(lib.lz4hip_encode_batch_device(C.byref(b), _lib.MODE_FAST, batch._stream()))
            sums = []
            for lib in (parent, new):
                comp.zero_()
                call(lib)
                torch.cuda.synchronize()
                sums.append((res.clone(), batch.checksum(comp, res).clone()))
            assert torch.equal(sums[0][0], sums[1][0]) and torch.equal(sums[0][1], sums[1][1]), "the two builds do not write the same bytes"
            ms = event_ms({"parent_a": lambda: call(parent), "new_a": lambda: call(new), "parent_b": lambda: call(parent), "new_b": lambda: call(new)})
            spread = abs(ms["parent_a"] - ms["parent_b"]) / min(ms["parent_a"], ms["parent_b"])
            ratio = min(ms["new_a"], ms["new_b"]) / min(ms["parent_a"], ms["parent_b"])
            diff = abs(min(ms["new_a"], ms["new_b"]) - min(ms["parent_a"], ms["parent_b"])) / min(ms["parent_a"], ms["parent_b"])
            out["D%d_%d" % (dist, n)] = {"ms": ms, "parent_spread": spread, "new_over_parent_best": ratio, "difference_within_parent_spread": diff <= spread}
            print("D%d %d" % (dist, n), json.dumps(out["D%d_%d" % (dist, n)]), flush=True)
            del raw, comp
    return out


if __name__ == "__main__":
    main()
