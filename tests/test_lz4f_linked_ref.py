"""CPU-only: the twin (tests/lz4f_ref.py) on frames with linked blocks, against the format library.  The frames of
tests/golden/lz4f_linked_frames.json were written by liblz4 with linked blocks (tests/golden/make_lz4f_linked_golden.py); the twin
reads each to its source, and refuses none.  Where liblz4 is installed (found with ctypes.util.find_library; nothing is downloaded)
LZ4F_decompress and the twin agree on every hand-built frame: the same bytes, the same frames refused; that test, and only that one,
skips where the library is absent."""
import os

import pytest

import lz4f_built as built
import lz4f_lib
import lz4f_ref as ref
from lz4f_linked_cases import GOLDEN, golden, hand_built
from lz4net_amd import _lib


def test_the_flag_s_value():
    assert _lib.LZ4F_ACCEPT_LINKED == ref.ACCEPT_LINKED == 8


def test_the_fixture_is_small_and_linked(oracle):
    assert os.path.getsize(GOLDEN) < 137 * 1024
    names, recs, frames, _ = golden(oracle)
    assert len(names) >= 5 and all(not f[4] & 0x20 and not f[4] & 0x01 for f in frames)
    assert any(r["block_id"] == 5 for r in recs) and any(r["level"] == 9 for r in recs) and any(r["block_checksum"] for r in recs)
    assert any(r["block_checksum"] and r["content_checksum"] and r["content_size"] for r in recs)
    assert all(r["bytes"] > ref.block_bytes(r["block_id"]) for r in recs), "every frame has a block that can reach into another"


def test_the_twin_reads_every_golden_frame_to_its_source(oracle):
    names, recs, frames, srcs = golden(oracle)
    reach = 0
    for name, rec, frame, src in zip(names, recs, frames, srcs):
        assert ref.read_frame(oracle, frame)[0]["error"] == ref.UNSUPPORTED_LINKED, name
        info, out, unspecified, rows = ref.read_frame(oracle, frame, accept_linked=True)
        assert info["error"] == ref.OK and out == src and not unspecified and info["frame_bytes"] == len(frame), name
        assert info["decoded_bytes"] == info["good_bytes"] == len(src) and info["blocks"] == len(rows) >= 2
        assert info["checks"] == (ref.VERIFIED if rec["block_checksum"] else 0) | ((ref.VERIFIED if rec["content_checksum"] else 0) << 2)
        reach += any(ref.size_block(frame[at:at + size], 0) < 0 < ref.size_block(frame[at:at + size]) for at, size, *_ in rows[1:])
    assert reach >= 3, "frames in which a block does not stand alone: its matches reach into the blocks before it"


def test_the_twin_s_block_decoder_knows_its_history():
    tail = bytes(range(12))
    block = built.sequence(b"", 3, 8) + built.sequence(tail)
    assert ref.size_block(block) == 20 and ref.size_block(block, 2) < 0
    assert ref.decode_block(block, 20, b"abc") == (20, b"abcabcab" + tail)
    assert ref.decode_block(block, 20, b"bc")[0] < 0, "a match that starts before the history"
    assert ref.decode_block(block, 19, b"abc")[0] < 0 and ref.decode_block(block, 21, b"abc")[0] == 20


def test_the_hand_built_frames_are_what_they_claim(oracle):
    cases = hand_built()
    assert {"a_first_byte", "a_before_the_frame", "b_offset_65535", "c_across_a_raw_block", "d_run_fill", "e_short_sequences", "f_bad_checksum"} <= set(cases)
    for name, (frame, content, bad) in cases.items():
        info, out, unspecified, rows = ref.read_frame(oracle, frame, accept_linked=True)
        if content is not None:
            assert info["error"] == ref.OK and out == content and not unspecified, name
            continue
        at = rows[bad][0] - 4
        assert info["error"] == (ref.BLOCK_CHECKSUM if name.startswith("f_") else ref.CORRUPT_BLOCK) and info["error_offset"] == at, name
    info, out, unspecified, _ = ref.read_frame(oracle, cases["a_before_the_frame"][0], accept_linked=True)
    assert (info["good_bytes"], info["decoded_bytes"], len(out), unspecified) == (1000, 1032, 1000, True), "the refused block keeps its place"
    info, out, unspecified, _ = ref.read_frame(oracle, cases["f_bad_checksum"][0], accept_linked=True)
    assert (info["good_bytes"], info["decoded_bytes"], len(out), unspecified) == (120, 120, 120, False), "blocks 2 and 3 take no bytes"
    # the clip of a linked item is at a block boundary
    frame, content, _ = cases["c_across_a_raw_block"]
    info, out, unspecified, _ = ref.read_frame(oracle, frame, room=65540, accept_linked=True)
    assert info["decoded_bytes"] == len(content) and out == content[:65536] and not unspecified


@pytest.mark.skipif(lz4f_lib.load() is None, reason="liblz4 >= 1.8.0 is not installed")
def test_liblz4_and_the_twin_agree_on_every_hand_built_frame(oracle):
    for name, (frame, content, bad) in hand_built().items():
        got, used, err = lz4f_lib.decompress(frame, 200000)
        info, out, _, _ = ref.read_frame(oracle, frame, accept_linked=True)
        assert (err is None) == (info["error"] == ref.OK) == (content is not None), (name, err, info["error"])
        if content is not None:
            assert got == out == content and used == len(frame) == info["frame_bytes"], name
