"""Writes tests/golden/lz4f_frames.json: LZ4 frames written by the local format library (liblz4's LZ4F_compressFrame and, for the
block size ids that call lowers, LZ4F_compressBegin / Update / End; through tests/lz4f_lib.py), base64, with their options.  Run by hand where liblz4 is installed; fetches nothing.  The sources are not stored:
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

OUT = os.path.join(HERE, "lz4f_frames.json")

# name: (source kind, source bytes, block size id, level, block checksum, content checksum, content size, linked, skippable bytes in front)
CASES = {
    "empty": ("formula", 0, 4, 0, False, False, False, False, 0),
    "one_byte": ("formula", 1, 4, 0, False, False, False, False, 0),
    "one_block_hc": ("d3", 65536, 4, 9, False, False, False, False, 0),
    "one_block_and_a_byte": ("d3", 65537, 4, 0, False, False, True, False, 0),
    "id5": ("d3", 20000, 5, 0, False, True, False, False, 0),                # (ids 5-7 through the streaming calls: LZ4F_compressFrame lowers the id)
    "id6": ("formula", 5000, 6, 0, True, False, False, False, 0),
    "id7_hc": ("d2", 3000, 7, 9, False, False, True, False, 0),
    "all_options": ("d2", 3000, 4, 0, True, True, True, False, 0),
    "linked": ("d3", 65537, 4, 0, True, True, True, True, 0),
    "behind_a_skippable_frame": ("formula", 1000, 4, 0, False, True, False, False, 11),
}


def main():
    assert lz4f_lib.load() is not None, "liblz4 >= 1.8.0 is needed to write the fixture"
    oracle = Oracle()
    frames = {}
    for name, (kind, n, bid, level, bc, cc, cs, linked, skip) in CASES.items():
        src = ref.golden_source(oracle, kind, n)
        frame = (lz4f_lib.compress_frame if bid == 4 else lz4f_lib.compress_frame_stream)(src, bid, level, bc, cc, cs, linked)
        if skip:
            frame = ref.skippable(bytes(range(skip)), 7) + frame
        frames[name] = {"source": kind, "bytes": n, "block_id": bid, "level": level, "block_checksum": bc, "content_checksum": cc,
                        "content_size": cs, "linked": linked, "skippable_bytes": skip, "frame": base64.b64encode(frame).decode()}
    with open(OUT, "w") as f:
        json.dump({"writer": "liblz4 %d" % lz4f_lib.load().LZ4_versionNumber(), "frames": frames}, f, indent=1)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
