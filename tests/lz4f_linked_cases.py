"""TEST INFRASTRUCTURE for the tests of LZ4 frames with linked blocks -- tests/test_simt_lz4f_linked.py and
tests/test_gpu_lz4f_linked.py: the frames and batches the tests are made of.  (The harness is tests/lz4f_cases.py's, on its LINKED
path: the linked rows run the real wavefront decoder under the emulator, the independent rows keep the stand-in codec.)"""
import base64
import functools
import json
import os

import lz4f_built as built
import lz4f_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_linked_frames.json")


@functools.lru_cache(maxsize=None)
def golden(oracle):
    """the linked frames liblz4 wrote (tests/golden/lz4f_linked_frames.json), in name order -> (names, records, frames, sources)"""
    with open(GOLDEN) as f:
        recs = json.load(f)["frames"]
    names = sorted(recs)
    frames = [base64.b64decode(recs[k]["frame"]) for k in names]
    srcs = [ref.golden_source(oracle, recs[k]["source"], recs[k]["bytes"]) for k in names]
    return names, [recs[k] for k in names], frames, srcs


@functools.lru_cache(maxsize=None)
def hand_built():
    return built.hand_built_linked()


@functools.lru_cache(maxsize=None)
def mixed_batch(oracle):
    """independent one-block, linked two-block, skippable, linked three-block with a raw middle block, independent two-block, empty
    frame, a linked frame with a dictionary ID -> (frames, index of the linked two-block item)"""
    cases = hand_built()
    d3 = ref.golden_source(oracle, "d3", 70000)
    dict_frame = built.frame_of([(b"0123456789", True)], linked=True, dict_id=7)
    frames = [ref.write_frame(oracle, d3[:3000], 4, False, 7)[0], cases["d_run_fill"][0], ref.skippable(b"between the frames", 3),
              cases["c_across_a_raw_block"][0], ref.write_frame(oracle, d3, 4, True, 3)[0], ref.write_frame(oracle, b"", 4, False, 0)[0], dict_frame]
    return tuple(frames), 1
