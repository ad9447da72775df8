"""Writes tests/golden/lz4f_dict_frames.json: LZ4 frames written WITH A DICTIONARY by the local format library (liblz4's
LZ4F_createCDict / LZ4F_compressFrame_usingCDict, through tests/lz4f_dict_lib.py), base64, with their options: 300, 4 096 and 70 000
bytes x independent / linked x level 0 / 9 x with and without a dictionary ID.  Every frame is read back with
LZ4F_decompress_usingDict before it is written, and must NOT read back without the dictionary.  Run by hand where liblz4 is installed;
fetches nothing.  Neither the dictionary nor the sources are stored: tests/lz4f_dict_cases.py restates them from a seed
(golden_dictionary, golden_source)."""
import base64
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "simt"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lz4f_dict_lib  # noqa: E402
import lz4f_lib  # noqa: E402
from lz4f_dict_cases import GOLDEN_DICT_ID, golden_dictionary, golden_source  # noqa: E402

OUT = os.path.join(HERE, "lz4f_dict_frames.json")
SIZES, LEVELS = (300, 4096, 70000), (0, 9)


def main():
    assert lz4f_dict_lib.load() is not None, "liblz4 >= 1.8.0 with the dictionary calls is needed to write the fixture"
    d = golden_dictionary()
    frames = {}
    for n in SIZES:
        src = golden_source(n)
        for linked in (False, True):
            for level in LEVELS:
                for with_id in (True, False):
                    frame = lz4f_dict_lib.compress_frame(src, d, GOLDEN_DICT_ID if with_id else 0, level, linked)
                    assert bool(frame[4] & 0x01) == with_id
                    assert n < 65536 or bool(frame[4] & 0x20) != linked, "above one block the mode is the one asked for"
                    back, err = lz4f_dict_lib.decompress(frame, d, n)
                    assert err is None and back == src, (n, linked, level, with_id, err)
                    plain, _, err = lz4f_lib.decompress(frame, n)
                    assert err is not None or plain != src, "the frame does not need its dictionary"
                    name = "%05d_%s_l%d_%s" % (n, "linked" if linked else "independent", level, "id" if with_id else "noid")
                    frames[name] = {"bytes": n, "linked": linked, "level": level, "dict_id": GOLDEN_DICT_ID if with_id else None,
                                    "frame": base64.b64encode(frame).decode()}
    with open(OUT, "w") as f:
        json.dump({"writer": "liblz4 %d" % lz4f_lib.load().LZ4_versionNumber(), "frames": frames}, f, indent=1)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
