"""Writes tests/golden/lz4f_linked_frames.json: LZ4 frames with LINKED blocks (FLG.5 clear) written by the local format library
(liblz4's LZ4F_compressFrame and, for the block size id that call lowers, LZ4F_compressBegin / Update / End; through
tests/lz4f_lib.py), base64, with their options.  Run by hand where liblz4 is installed; fetches nothing.  The sources are not stored:
tests/lz4f_ref.py's golden_source() restates them (a formula, and the oracle's D2 / D3 generators)."""
import base64
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lz4f_lib  # noqa: E402
import lz4f_ref as ref  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

OUT = os.path.join(HERE, "lz4f_linked_frames.json")

# name: (source kind, source bytes, block size id, level, block checksum, content checksum, content size)
CASES = {
    "formula_two_blocks": ("formula", 70000, 4, 0, False, False, False),
    "d3_three_blocks_all_options": ("d3", 131077, 4, 0, True, True, True),
    "d2_two_blocks_hc": ("d2", 65600, 4, 9, False, False, False),
    "formula_id5_streamed": ("formula", 270000, 5, 0, False, True, False),   # (through the streaming calls: LZ4F_compressFrame lowers the id)
    "formula_block_checksums": ("formula", 70000, 4, 0, True, False, False),
}


def main():
    assert lz4f_lib.load() is not None, "liblz4 >= 1.8.0 is needed to write the fixture"
    oracle = Oracle()
    frames = {}
    for name, (kind, n, bid, level, bc, cc, cs) in CASES.items():
        src = ref.golden_source(oracle, kind, n)
        frame = (lz4f_lib.compress_frame if bid == 4 else lz4f_lib.compress_frame_stream)(src, bid, level, bc, cc, cs, True)
        assert not frame[4] & 0x20, "the frame's blocks are linked"
        frames[name] = {"source": kind, "bytes": n, "block_id": bid, "level": level, "block_checksum": bc, "content_checksum": cc,
                        "content_size": cs, "linked": True, "frame": base64.b64encode(frame).decode()}
    with open(OUT, "w") as f:
        json.dump({"writer": "liblz4 %d" % lz4f_lib.load().LZ4_versionNumber(), "frames": frames}, f, indent=1)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
