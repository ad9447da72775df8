"""Writes tests/golden/dict_blocks.json: 40 records of at most 4 KiB -- JSON-like text, tests/dict_cases.py fixture_record -- each
compressed on its own against ONE dictionary (fixture_dictionary: 64 KiB made from a seed, not stored) by liblz4's LZ4_loadDict +
LZ4_compress_fast_continue, with their plain text.  The committed file was written with liblz4 1.9.3 (LZ4_versionNumber 10903); every
block is checked with LZ4_decompress_safe_usingDict before it is written.

    python tests/golden/make_dict_golden.py
"""
import base64
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dict_cases as cases  # noqa: E402

SIZES = [4096] * 12 + [4095, 4000, 3333, 3000, 2500, 2048, 2047, 1500, 1024, 1000, 777, 512, 400, 300, 256, 200, 150, 128, 100, 90, 80, 70, 64, 50, 40, 33, 20, 13]


def main():
    L = C.CDLL(ctypes.util.find_library("lz4"))
    L.LZ4_createStream.restype = C.c_void_p
    L.LZ4_freeStream.argtypes = [C.c_void_p]
    L.LZ4_loadDict.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    dic = cases.fixture_dictionary().tobytes()
    records = []
    for k, size in enumerate(SIZES):
        plain = cases.fixture_record(cases.FIXTURE_SEED, k, size)
        stream = L.LZ4_createStream()
        assert L.LZ4_loadDict(stream, dic, len(dic)) == min(len(dic), 65536)
        cap = L.LZ4_compressBound(size)
        out = C.create_string_buffer(cap)
        n = L.LZ4_compress_fast_continue(stream, plain, out, size, cap, 1)
        L.LZ4_freeStream(stream)
        assert n > 0
        block = out.raw[:n]
        r, back = cases.using_dict(cases.liblz4(), block, size, dic)
        assert r == size and back == plain
        records.append({"plain": base64.b64encode(plain).decode(), "block": base64.b64encode(block).decode()})
    j = {"liblz4": L.LZ4_versionNumber(), "dictionary": {"seed": cases.FIXTURE_SEED, "length": cases.FIXTURE_DICT_LEN, "sha256": hashlib.sha256(dic).hexdigest()},
         "records": records}
    with open(cases.FIXTURE, "w") as fh:
        json.dump(j, fh, indent=0)
        fh.write("\n")
    plain_bytes = sum(SIZES)
    print(len(records), "records,", plain_bytes, "bytes ->", sum(len(base64.b64decode(r["block"])) for r in records), "bytes; file", os.path.getsize(cases.FIXTURE))


if __name__ == "__main__":
    main()
