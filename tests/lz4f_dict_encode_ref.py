"""The twin of the frame encode with a dictionary (lz4hip_lz4f_encode_dict_*, include/lz4hip.h): the frame writer of tests/lz4f_ref.py
with the dictionary encode's twin (tests/dict_encode_ref.py) as its block encoder -- independent blocks, every one against the same
dictionary with one byte less of room than it is long, a result of 0 stored raw; the ID, when it is not 0, in the descriptor.  Nothing
here is shared with the code under test.  Also the sources and dictionaries the emulator and GPU tests of that call are made of."""
import functools
import random

import numpy as np

import dict_encode_ref
import lz4f_ref as ref

DICT_LENGTHS = (1, 13, 4095, 4097, 65535, 70000)
SOURCE_LENGTHS = (0, 1, 12, 13, 300, 4096, 65536, 65537, 150000)
DICT_IDS = (0, 7, 0xFFFFFFFF)
BIG = 300000                                                            # at block id 5: blocks above 64 KiB


@functools.lru_cache(maxsize=None)
def write_frame_dict(src, dictionary, dict_id=0, block_id=4, flags=0):
    """-> (frame, [per block: the encoder's result (0: stored raw)]); dictionary == b"" is NOT the plain fast encoder's frame (that
    encoder has a 64 KiB variant with bytes of its own): a call without a dictionary is compared with the plain call"""
    src, dictionary = bytes(src), bytes(dictionary)
    out = [ref.descriptor(block_id, flags, len(src), dict_id=dict_id if dict_id and dictionary else None)]
    rets = []
    for block in ref.cut(src, block_id):
        ret, comp = dict_encode_ref.encode(block, dictionary, cap=len(block) - 1)
        rets.append(ret)
        stored = comp if ret else block
        out.append(ref.le32(len(stored) | (0 if ret else 0x80000000)) + stored)
        if flags & ref.F_BLOCK_CHECKSUM:
            out.append(ref.le32(ref.xxh32(stored)))
    out.append(ref.le32(0))
    if flags & ref.F_CONTENT_CHECKSUM:
        out.append(ref.le32(ref.xxh32(src)))
    return b"".join(out), rets


def raw_frame_bytes(n, block_id=4, flags=0, dict_id=0):
    """the size of the frame of n bytes with every block stored raw"""
    blocks = (n + ref.block_bytes(block_id) - 1) // ref.block_bytes(block_id)
    return (len(ref.descriptor(block_id, flags, n, dict_id=dict_id or None)) + n + blocks * (4 + (4 if flags & ref.F_BLOCK_CHECKSUM else 0)) + 4 +
            (4 if flags & ref.F_CONTENT_CHECKSUM else 0))


@functools.lru_cache(maxsize=None)
def dictionary(n):
    """n bytes of text-like records: 16-byte words out of a small alphabet, so that sources find matches everywhere in it"""
    rng = random.Random(1000 + n)
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(3, 17))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def source(n, dict_len=4097):
    """n bytes: pieces of the dictionary (from its end, which every dictionary length keeps in reach), noise, and repeats of the
    source's own bytes"""
    d = dictionary(dict_len)
    rng = random.Random(7 * n + 1)
    out = bytearray()
    while len(out) < n:
        kind = rng.randrange(8)
        k = rng.randrange(4, 200)
        if kind < 5 and len(d) >= 4:
            at = rng.randrange(max(len(d) - 60000, 0), len(d))
            out += d[at:at + k]
        elif kind == 5 and len(out) > 8:
            back = rng.randrange(1, min(len(out), 65000))
            out += out[-back:][:k]
        else:
            out += bytes(rng.randrange(256) for _ in range(k % 23 + 1))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def only_with_the_dictionary():
    """(dictionary, source): 8 192 random bytes and 200 of them from the middle -- compressible against the dictionary alone"""
    rng = random.Random(5)
    d = bytes(rng.randrange(256) for _ in range(8192))
    return d, d[-5000:-4800]


def noise(n, seed=11):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
