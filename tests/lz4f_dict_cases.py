"""TEST INFRASTRUCTURE for the tests of LZ4 frames with a dictionary -- tests/test_simt_lz4f_dict.py and tests/test_gpu_lz4f_dict.py:
the dictionaries, frames and batches the tests are made of.  (The harness is tests/lz4f_cases.py's, on its DICT path: every block runs
the real wavefront decoder under the emulator, the rounds' rows decode_dict_kernel, the linked rows the dictionary form of the ordered
decode.)"""
import base64
import functools
import json
import os

import lz4f_built as built
import lz4f_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_dict_frames.json")
GOLDEN_DICT_SEED, GOLDEN_DICT_BYTES, GOLDEN_DICT_ID = 4242, 20000, 0x0D1C7105


# ---- dictionaries, frames and batches ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dictionary(n):
    return built.dictionary(n)


@functools.lru_cache(maxsize=None)
def hand_built(n, dict_id=None):
    return built.hand_built_dict(dictionary(n), dict_id)


def hand_built_params():
    """(dictionary length, case name) for every case that length allows"""
    return [(n, name) for n in built.DICT_LENGTHS for name in sorted(hand_built(n))]


@functools.lru_cache(maxsize=None)
def golden_dictionary():
    return built.dictionary(GOLDEN_DICT_BYTES, GOLDEN_DICT_SEED)


def golden_source(n):
    """what the golden frames hold: pieces of the dictionary, a little noise, and repeats of the source's own bytes up to 60 000 back (a 32-bit
    LCG picks them: the same bytes wherever this runs)"""
    d = golden_dictionary()
    out, state = bytearray(), [(n * 2654435761 + 12345) & 0xFFFFFFFF]

    def pick():
        state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
        return state[0] >> 8

    while len(out) < n:
        kind, k = pick() % 12, 16 + pick() % 240
        if kind:
            at = pick() % (len(d) - 256)
            out += d[at:at + k]
        else:
            out += built.noise(8 + k % 17, pick() & 0xFFFF)
        if len(out) > 200 and pick() % 4 == 0:
            back = 1 + pick() % min(len(out) - 1, 60000)
            out += out[-back:][:k]
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def golden():
    """the frames liblz4 wrote with LZ4F_compressFrame_usingCDict (tests/golden/lz4f_dict_frames.json), in name order
    -> (names, records, frames, sources)"""
    with open(GOLDEN) as f:
        recs = json.load(f)["frames"]
    names = sorted(recs)
    return names, [recs[k] for k in names], [base64.b64decode(recs[k]["frame"]) for k in names], [golden_source(recs[k]["bytes"]) for k in names]


MIXED_DICT = 4097


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """dictionary independent, dictionary linked (three blocks, the middle one raw), plain independent, skippable, a frame with another
    dictionary ID -> (frames, dictionary, the call's dict_id, index of the linked item)"""
    with_id, no_id = hand_built(MIXED_DICT, 7), hand_built(MIXED_DICT)
    other = built.frame_of([(b"0123456789", True)], linked=False, dict_id=8)
    frames = (with_id["i_into_the_block"][0], with_id["l_across_a_raw_block"][0], no_id["i_first_byte"][0], ref.skippable(b"between the frames", 3), other)
    return frames, dictionary(MIXED_DICT), 7, 1
