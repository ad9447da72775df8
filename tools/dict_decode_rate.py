"""Block batches decoded against a shared dictionary (lz4hip_decode_batch_dict_device) against what the library already had, on the
same records: --records (default 16 384 and 262 144) records of 4 KiB, JSON-like text (tests/dict_cases.py fixture_record), against
the fixture's 64 KiB dictionary -- compressed by liblz4 where it is installed (LZ4_loadDict + LZ4_compress_fast_continue per record;
LZ4_compress_default for the yardsticks' blocks without a dictionary), else the fixture's own blocks tiled and the yardsticks' blocks
from the library's fast encoder.  Which of the two is recorded.

  dict            the dictionary call on the dictionary's blocks
  dict_no_preload the same from a library built with -DLZ4HIP_DICT_PRELOAD=0 (--variant-lib), where one is given
  plain_wave      lz4hip_decode_batch_device, wavefront mapping forced, on the same records compressed WITHOUT a dictionary
  dict_len_0      the dictionary call with dict_len = 0 on those blocks

Event timings, best of --reps after one warm-up, the paths taking turns inside a repetition; every decode is compared with the source.
Also the emulator's share of sequences per path of the wavefront decoder on a sample of the dictionary's blocks, with the preload and
without it (an emulator build with -DLZ4HIP_DICT_PRELOAD=0), and -- with --parent-lib, the parent commit's library -- the condition
that the plain decode of the bench's D2 and D3 at 4 096 and 65 536 blocks takes what it takes with the parent's build: both libraries
in this process, taking turns, each measured twice so that the parent's own spread is seen.  --emulator-only writes the emulator's
shares alone (it needs liblz4 and no GPU); --skip-emulator leaves them out of a GPU run.

    python tools/dict_decode_rate.py [--records 16384 262144] [--reps 5] [--parent-lib PATH] [--variant-lib PATH] [--skip-emulator] [--out profiles/dict_decode/dict_decode_rate.json]
    python tools/dict_decode_rate.py --emulator-only --out profiles/dict_decode/emulator_path_shares.json
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
ap.add_argument("--emu-sample", type=int, default=64)
ap.add_argument("--emulator-only", action="store_true", help="only the emulator's path shares (needs liblz4, no GPU)")
ap.add_argument("--skip-emulator", action="store_true")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--variant-lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_decode", "dict_decode_rate.json"))
args = ap.parse_args()
RECORD = 4096


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
    """another build of the library in this process, the two calls typed"""
    lib = C.CDLL(path)
    for name, res, argtypes in _lib.SYMBOLS:
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, argtypes
    return lib


def build_records(n_unique):
    """(how they were built, plain rows, blocks against the dictionary, blocks without one, the dictionary)"""
    dic = cases.fixture_dictionary()
    path = ctypes.util.find_library("lz4")
    if path:
        lz4 = C.CDLL(path)
        lz4.LZ4_createStream.restype = C.c_void_p
        lz4.LZ4_freeStream.argtypes = [C.c_void_p]
        lz4.LZ4_loadDict.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        lz4.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        lz4.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        plain, with_dict, without = [], [], []
        cap = lz4.LZ4_compressBound(RECORD)
        out = C.create_string_buffer(cap)
        d = dic.tobytes()
        for k in range(n_unique):
            p = cases.fixture_record(cases.FIXTURE_SEED, 1000 + k, RECORD)
            stream = lz4.LZ4_createStream()
            lz4.LZ4_loadDict(stream, d, len(d))
            n = lz4.LZ4_compress_fast_continue(stream, p, out, RECORD, cap, 1)
            lz4.LZ4_freeStream(stream)
            with_dict.append(out.raw[:n])
            n = lz4.LZ4_compress_default(p, out, RECORD, cap)
            without.append(out.raw[:n])
            plain.append(p)
        return "liblz4 %d" % lz4.LZ4_versionNumber(), plain, with_dict, without, dic
    _, records, _ = cases.load_fixture()
    full = [(p, b) for p, b in records if len(p) == RECORD]
    plain = [full[k % len(full)][0] for k in range(n_unique)]
    with_dict = [full[k % len(full)][1] for k in range(n_unique)]
    rows = torch.from_numpy(np.frombuffer(b"".join(plain), np.uint8).reshape(n_unique, RECORD).copy()).cuda()
    comp = torch.empty((n_unique, batch.compress_bound(RECORD) + 16), dtype=torch.uint8, device="cuda")
    clen = batch.encode(rows, RECORD, comp, batch.compress_bound(RECORD)).cpu().numpy()
    comp_h = comp.cpu().numpy()
    without = [comp_h[i, :clen[i]].tobytes() for i in range(n_unique)]
    return "the fixture's %d full records, tiled; yardstick blocks from the library's fast encoder" % len(full), plain, with_dict, without, dic


def rows_of(blocks, pick):
    width = (max(len(b) for b in blocks) + 31) // 16 * 16
    h = np.zeros((len(blocks), width), np.uint8)
    for i, b in enumerate(blocks):
        h[i, :len(b)] = np.frombuffer(b, np.uint8)
    lens = torch.tensor([len(b) for b in blocks], dtype=torch.int32, device="cuda")
    return torch.from_numpy(h).cuda()[pick].contiguous(), lens[pick].contiguous()


def emulator_shares(blocks, dic, preload):
    """share of sequences per path of the wavefront decoder under the emulator (LZ4HIP_STAT 21, 24, 25 and LZ4HIP_STAT_PATH 31)"""
    from emu_lib import build_dict
    L = C.CDLL(build_dict() if preload else build_dict(["-DLZ4HIP_DICT_PRELOAD=0"], "libsimt_dict_no_preload.so"))
    n = len(blocks)
    width = max(len(b) for b in blocks) + 16
    src = np.zeros((n, width), np.uint8)
    for i, b in enumerate(blocks):
        src[i, :len(b)] = np.frombuffer(b, np.uint8)
    sl = np.array([len(b) for b in blocks], np.int32)
    cp = np.full(n, RECORD, np.int32)
    dst = np.zeros((n, RECORD + 64), np.uint8)
    res = np.zeros(n, np.int32)
    st = (C.c_ulonglong * 40)()
    L.emu_stats(st, 1)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    L.emu_dict_decode(1, p(src), C.c_int64(width), p(sl), p(dst), C.c_int64(RECORD + 64), p(cp), p(res), C.c_int64(n), 4, p(dic), C.c_int64(dic.size))
    L.emu_stats(st, 1)
    assert (res == sl).all()
    burst, short, general, long_ = int(st[21]), int(st[24]), int(st[25]) - int(st[31]), int(st[31])
    total = burst + short + general + long_
    return {"sequences": total, "burst": burst / total, "short": short / total, "general": general / total, "long": long_ / total,
            "failed_bursts_per_block": int(st[23]) / n}


def main():
    if args.emulator_only:
        how, plain, with_dict, without, dic = build_records(args.emu_sample)
        sample = with_dict[:args.emu_sample]
        shares = {"records_built": how, "sample_records": len(sample), "with_preload": emulator_shares(sample, dic, True),
                  "without_preload": emulator_shares(sample, dic, False)}
        print(json.dumps(shares, indent=1))
        with open(args.out, "w") as fh:
            json.dump(shares, fh, indent=1)
            fh.write("\n")
        return
    L = _lib.lib()
    variant = typed(args.variant_lib) if args.variant_lib else None
    how, plain, with_dict, without, dic = build_records(args.unique)
    d_dev = torch.from_numpy(dic).cuda()
    report = {"records_built": how, "unique_records": args.unique, "record_bytes": RECORD, "dictionary_bytes": int(dic.size), "reps": args.reps,
              "compressed_bytes_per_record": {"with_dictionary": sum(map(len, with_dict)) / len(with_dict), "without": sum(map(len, without)) / len(without)},
              "device": torch.cuda.get_device_name(0), "batches": {}, "note": "one box, one run"}
    plain_dev = torch.from_numpy(np.frombuffer(b"".join(plain), np.uint8).reshape(len(plain), RECORD).copy()).cuda()
    for n in args.records:
        pick = torch.arange(n, device="cuda") % args.unique
        src_d, len_d = rows_of(with_dict, pick)
        src_p, len_p = rows_of(without, pick)
        want = plain_dev[pick]
        out = torch.empty((n, RECORD), dtype=torch.uint8, device="cuda")
        res = torch.empty(n, dtype=torch.int32, device="cuda")

        def dict_call(lib, src, lens, dict_len):
            b, keep = batch._make_batch(src, lens, out, RECORD, res)
            _lib.check(lib.lz4hip_decode_batch_dict_device(C.byref(b), d_dev.data_ptr() if dict_len else None, dict_len, 1, batch._stream()))

        def plain_wave():
            with _lib.tuning(decoder="wave"):
                batch.decode(src_p, len_p, out, RECORD, result=res)

        fns = {"dict": lambda: dict_call(L, src_d, len_d, dic.size), "plain_wave": plain_wave, "dict_len_0": lambda: dict_call(L, src_p, len_p, 0)}
        if variant is not None:
            fns["dict_no_preload"] = lambda: dict_call(variant, src_d, len_d, dic.size)
        for name, fn in fns.items():                                   # every decode against the source
            out.zero_()
            fn()
            torch.cuda.synchronize()
            assert torch.equal(res, len_d if name.startswith("dict") and name != "dict_len_0" else len_p) and torch.equal(out, want), name
        ms = event_ms(fns)
        row = {"ms": ms, "GB_per_s_out": {k: n * RECORD / v / 1e6 for k, v in ms.items()},
               "dict_over_plain_wave": ms["dict"] / ms["plain_wave"], "dict_over_dict_len_0": ms["dict"] / ms["dict_len_0"]}
        if variant is not None:
            row["dict_over_dict_no_preload"] = ms["dict"] / ms["dict_no_preload"]
        report["batches"][str(n)] = row
        print(n, json.dumps(row), flush=True)
    if not args.skip_emulator:
        sample = with_dict[:args.emu_sample]
        report["emulator_path_shares"] = {"with_preload": emulator_shares(sample, dic, True), "without_preload": emulator_shares(sample, dic, False),
                                          "sample_records": len(sample)}
        print(json.dumps(report["emulator_path_shares"]), flush=True)
    if args.parent_lib:
        report["plain_decode_parent_vs_new"] = parent_vs_new(typed(args.parent_lib), L)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


def parent_vs_new(parent, new):
    """lz4hip_decode_batch_device (default dispatch) on the bench's D2 and D3 at 4 096 and 65 536 blocks of 64 KiB: the parent's build and
    this one take turns; each appears twice, so the first pair of columns is the parent's own run-to-run spread"""
    out = {}
    for dist in (2, 3):
        for n in (4096, 65536):
            raw = batch.synth(dist, 4242, 0, n)
            comp = torch.empty((n, batch.BOUND_STRIDE), dtype=torch.uint8, device="cuda")
            clen = batch.encode(raw, batch.BLOCK, comp, batch.BOUND)
            back = torch.empty_like(raw)
            res = torch.empty(n, dtype=torch.int32, device="cuda")

            def call(lib):
                b, keep = batch._make_batch(comp, clen, back, batch.BLOCK, res)
                _lib.check(lib.lz4hip_decode_batch_device(C.byref(b), 1, batch._stream()))
            for lib in (parent, new):
                back.zero_()
                call(lib)
                torch.cuda.synchronize()
                assert torch.equal(res, clen) and torch.equal(back, raw)
            ms = event_ms({"parent_a": lambda: call(parent), "new_a": lambda: call(new), "parent_b": lambda: call(parent), "new_b": lambda: call(new)})
            spread = abs(ms["parent_a"] - ms["parent_b"]) / min(ms["parent_a"], ms["parent_b"])
            ratio = min(ms["new_a"], ms["new_b"]) / min(ms["parent_a"], ms["parent_b"])
            out["D%d_%d" % (dist, n)] = {"ms": ms, "parent_spread": spread, "new_over_parent_best": ratio}
            print("D%d %d" % (dist, n), json.dumps(out["D%d_%d" % (dist, n)]), flush=True)
            del raw, comp, back
    return out


if __name__ == "__main__":
    main()
