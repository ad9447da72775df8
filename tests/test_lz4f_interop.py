"""CPU-only: the LZ4 frame path against the format library.  The frames of tests/golden/lz4f_frames.json were written by liblz4's
LZ4F_compressFrame (tests/golden/make_lz4f_golden.py) and are read here by the test-side twin (tests/lz4f_ref.py) and by the emulator
path (the library's kernels and sequences, tests/simt/emu_lz4f.inc); these tests never skip.  Where liblz4 is installed (found with
ctypes.util.find_library; nothing is downloaded) fresh frames at levels 0 and 9 and every block size id go the same way, the emulator
path's frames go through LZ4F_decompress, which must consume every byte, and the descriptors are compared; those tests, and only those,
skip where the library is absent."""
import base64
import functools
import json
import os

import pytest

import lz4f_lib
import lz4f_ref as ref
from lz4f_cases import PLAIN, check_frame, emu_encode, mixed, sample
from lz4net_amd import lz4_frame

check_decode = functools.partial(check_frame, PLAIN, slot=0, max_blocks=8)   # the plain one-frame call, a table of 8 rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_frames.json")
with open(GOLDEN) as _f:
    FRAMES = json.load(_f)["frames"]
needs_liblz4 = pytest.mark.skipif(lz4f_lib.load() is None, reason="liblz4 >= 1.8.0 is not installed")


def options(rec):
    return (ref.F_BLOCK_CHECKSUM if rec["block_checksum"] else 0) | (ref.F_CONTENT_CHECKSUM if rec["content_checksum"] else 0) | \
        (ref.F_CONTENT_SIZE if rec["content_size"] else 0)


def test_the_fixture_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 137 * 1024
    assert {"empty", "one_byte", "one_block_hc", "one_block_and_a_byte", "id5", "id6", "id7_hc", "all_options", "linked",
            "behind_a_skippable_frame"} <= set(FRAMES)
    assert [FRAMES[k]["block_id"] for k in ("id5", "id6", "id7_hc")] == [5, 6, 7]


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_golden_frames_decode_through_the_twin_and_the_emulator_path(oracle, name):
    rec = FRAMES[name]
    frame = base64.b64decode(rec["frame"])
    src = ref.golden_source(oracle, rec["source"], rec["bytes"])
    if rec["skippable_bytes"]:
        info, out = check_decode(oracle, frame)
        assert info["kind"] == 1 and info["error"] == ref.OK and info["frame_bytes"] == 8 + rec["skippable_bytes"] and out == b""
        frame = frame[info["frame_bytes"]:]
    head = lz4_frame.parse_header(frame[:19])
    assert head["block_max"] == ref.block_bytes(rec["block_id"]) and head["independent"] == (not rec["linked"])
    assert (head["block_checksum"], head["content_checksum"]) == (rec["block_checksum"], rec["content_checksum"])
    assert head["content_size"] == (rec["bytes"] if rec["content_size"] and rec["bytes"] else None)
    for slot, rounds in ((0, 0), (head["block_max"], 2)):
        info, out = check_decode(oracle, frame, slot=slot, round_blocks=rounds)
        if rec["linked"]:
            assert frame[4] == 0x5C and info["error"] == ref.UNSUPPORTED_LINKED and out == b""
        else:
            assert info["error"] == ref.OK and out == src and info["frame_bytes"] == len(frame)
            assert info["checks"] == (ref.VERIFIED if rec["block_checksum"] else 0) | ((ref.VERIFIED if rec["content_checksum"] else 0) << 2)


def test_our_descriptors_equal_the_fixture_s(oracle):
    for name, rec in FRAMES.items():
        if rec["linked"] or rec["skippable_bytes"]:
            continue
        golden = base64.b64decode(rec["frame"])
        want = lz4_frame.parse_header(golden[:19])["header_bytes"]
        assert ref.descriptor(rec["block_id"], options(rec), rec["bytes"]) == golden[:want], name
    rec = FRAMES["all_options"]
    ours = emu_encode(oracle, ref.golden_source(oracle, rec["source"], rec["bytes"]), rec["block_id"], False, options(rec))
    assert ours[:15] == base64.b64decode(rec["frame"])[:15]
    assert emu_encode(oracle, b"", 4, False, 0)[:7] == base64.b64decode(FRAMES["empty"]["frame"])[:7]


# ---- with the format library ----------------------------------------------------------------------------------------------------------
@needs_liblz4
@pytest.mark.parametrize("level", [0, 9])
@pytest.mark.parametrize("block_id", [4, 5, 6, 7])
def test_liblz4_frames_decode_through_the_twin_and_the_emulator_path(oracle, level, block_id):
    src = mixed(oracle) + sample(oracle, 3, 70000)
    for bc, cc, cs in ((False, False, False), (True, True, True)):
        frame = lz4f_lib.compress_frame(src, block_id, level, bc, cc, cs)
        info, out = check_decode(oracle, frame, slot=ref.block_bytes(block_id), max_blocks=7)
        assert info["error"] == ref.OK and out == src and info["frame_bytes"] == len(frame)
        frame = lz4f_lib.compress_frame_stream(src, block_id, level, bc, cc, cs)                  # (the id as given)
        info, out = check_decode(oracle, frame, slot=ref.block_bytes(block_id), max_blocks=7)
        assert info["error"] == ref.OK and out == src and info["block_max"] == ref.block_bytes(block_id)
    for small in (b"", b"x", sample(oracle, 2, 12)):
        frame = lz4f_lib.compress_frame(small, block_id, level, True, True, True)
        info, out = check_decode(oracle, frame)
        assert info["error"] == ref.OK and out == small


@needs_liblz4
@pytest.mark.parametrize("block_id", [4, 5, 6, 7])
@pytest.mark.parametrize("hc", [False, True])
def test_liblz4_reads_the_emulator_path_s_frames(oracle, block_id, hc):
    src = mixed(oracle) + sample(oracle, 3, 70000)
    for flags in ((0, 7) if hc else range(8)):
        frame = emu_encode(oracle, src, block_id, hc, flags)
        got, used, err = lz4f_lib.decompress(frame, len(src))
        assert err is None and got == src and used == len(frame), (flags, err, used, len(frame))
        theirs = lz4f_lib.compress_frame_stream(src, block_id, 0, bool(flags & 1), bool(flags & 2), bool(flags & 4))
        n = 15 if flags & 4 else 7
        assert frame[:n] == theirs[:n], "the descriptor bytes must equal liblz4's for the same options"
    for small in (b"", b"x", sample(oracle, 2, 12)):
        frame = emu_encode(oracle, small, block_id, hc, 7)
        got, used, err = lz4f_lib.decompress(frame, len(small))
        assert err is None and got == small and used == len(frame)


@needs_liblz4
def test_liblz4_and_the_twin_agree_on_broken_frames(oracle):
    """the outcomes the twin models are errors to the format library too"""
    src = mixed(oracle)
    frame = ref.write_frame(oracle, src, 4, False, 7)[0]
    for bad in (frame[:-1], frame[:70000], bytes([frame[0] ^ 1]) + frame[1:], frame[:14] + bytes([frame[14] ^ 1]) + frame[15:],
                frame[:-1] + bytes([frame[-1] ^ 1]), frame[:30] + bytes([frame[30] ^ 0xFF]) + frame[31:]):
        assert ref.read_frame(oracle, bad)[0]["error"] != ref.OK
        assert lz4f_lib.decompress(bad, len(src))[2] is not None
    linked = lz4f_lib.compress_frame(src, 4, 0, True, True, True, linked=True)
    assert linked[4] == 0x5C and ref.read_frame(oracle, linked)[0]["error"] == ref.UNSUPPORTED_LINKED
