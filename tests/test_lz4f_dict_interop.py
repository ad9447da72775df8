"""CPU-only: LZ4 frames with a dictionary against the format library.  The frames of tests/golden/lz4f_dict_frames.json were written by
liblz4's LZ4F_compressFrame_usingCDict (tests/golden/make_lz4f_dict_golden.py) and are read by the emulator path in
tests/test_simt_lz4f_dict.py; that test never skips.  Here, where liblz4 is installed (found with ctypes.util.find_library; nothing is
downloaded), the same 24 shapes and a 150 000-byte source are written FRESH -- 32 combinations -- and go through the twin and the
emulator path (the library's kernels and sequences, tests/simt/emu_lz4f_dict.inc); these tests, and only these, skip where the library
or its dictionary calls are absent."""
import functools
import os

import pytest

import lz4f_dict_lib
import lz4f_ref as ref
from lz4f_cases import DICT, check_frame
from lz4f_dict_cases import GOLDEN, GOLDEN_DICT_ID, golden, golden_dictionary, golden_source
from lz4net_amd import lz4_frame

check_frame = functools.partial(check_frame, DICT, None, accept=True)

needs_liblz4 = pytest.mark.skipif(lz4f_dict_lib.load() is None, reason="liblz4 >= 1.8.0 with LZ4F_compressFrame_usingCDict is not installed")


def test_the_fixture_is_small_and_complete():
    names, recs, frames, srcs = golden()
    assert os.path.getsize(GOLDEN) < 108 * 1024 and len(names) == 24
    assert {(r["bytes"], r["linked"], r["level"], r["dict_id"] is not None) for r in recs} == \
        {(n, linked, level, with_id) for n in (300, 4096, 70000) for linked in (False, True) for level in (0, 9) for with_id in (False, True)}
    for rec, frame in zip(recs, frames):
        head = lz4_frame.parse_header(frame[:19])
        assert head["dict_id"] == rec["dict_id"] and head["independent"] == (not rec["linked"] or rec["bytes"] < 65536)


@needs_liblz4
@pytest.mark.parametrize("with_id", [True, False])
@pytest.mark.parametrize("level", [0, 9])
@pytest.mark.parametrize("linked", [False, True])
@pytest.mark.parametrize("n", [300, 4096, 70000, 150000])
def test_fresh_frames_decode_to_their_sources(n, linked, level, with_id):
    d, src = golden_dictionary(), golden_source(n)
    frame = lz4f_dict_lib.compress_frame(src, d, GOLDEN_DICT_ID if with_id else 0, level, linked, content_checksum=True, content_size=True)
    assert bool(frame[4] & 0x01) == with_id and (n < 65536 or bool(frame[4] & 0x20) != linked)
    assert lz4f_dict_lib.decompress(frame, d, n) == (src, None)
    got, out = check_frame(frame, d, GOLDEN_DICT_ID)
    assert got["error"] == ref.OK and out == src and got["content_size"] == n and got["checks"] >> 2 == ref.VERIFIED
    got, out = check_frame(frame, d[:-1], 0)                           # another dictionary: the content checksum, or a block, says so
    assert got["error"] != ref.OK or out != src
