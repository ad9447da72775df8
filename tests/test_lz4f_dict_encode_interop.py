"""CPU-only: the frames the dictionary encode writes (lz4hip_lz4f_encode_dict_*, here the emulator path of
tests/test_simt_lz4f_dict_encode.py: the library's kernels and sequences) against the format library.  Where liblz4 is installed (found
with ctypes.util.find_library; nothing is downloaded) LZ4F_decompress_usingDict reads the frames back to their sources, and the sizes
of the frames of the repository's golden dictionary and sources are printed next to what LZ4F_compressFrame_usingCDict (level 0,
independent blocks) writes for the same input -- a measurement (DESIGN.md 7 records it), no bound: the parse is another one.  These
tests skip where the library or its dictionary calls are absent."""
import pytest

import lz4f_dict_encode_ref as twin
import lz4f_dict_lib
import lz4f_ref as ref
from lz4f_dict_cases import GOLDEN_DICT_ID, golden_dictionary, golden_source
from lz4f_dict_encode_lib import encode_batch, encode_one

pytestmark = pytest.mark.skipif(lz4f_dict_lib.load() is None, reason="liblz4 >= 1.8.0 with LZ4F_compressFrame_usingCDict is not installed")


@pytest.mark.parametrize("n,odd", [(13, 1), (4097, 0), (70000, 1)])
def test_the_format_library_reads_the_frames_back(n, odd):
    d = twin.dictionary(n)
    for k, size in enumerate(twin.SOURCE_LENGTHS):
        src = twin.source(size, n)
        frame, _ = encode_one(src, d, twin.DICT_IDS[k % 3], flags=k % 8, odd=odd, host=bool(k & 1))
        assert lz4f_dict_lib.decompress(frame, d, size) == (src, None), size
    src = twin.source(twin.BIG, 70000)
    frame, _ = encode_one(src, d, 7, block_id=5, flags=7, odd=odd)
    assert lz4f_dict_lib.decompress(frame, d, twin.BIG) == (src, None)


def test_the_format_library_reads_a_batch_back():
    d = twin.dictionary(4097)
    items = [twin.source(size) for size in twin.SOURCE_LENGTHS] + [b"", twin.noise(200)]
    ends, got, _ = encode_batch(b"".join(items), [0] + [sum(len(i) for i in items[:k + 1]) for k in range(len(items))], d, 7, flags=7, wpg=5)
    for i, item in enumerate(items):
        assert lz4f_dict_lib.decompress(got[ends[i]:ends[i + 1]], d, len(item)) == (item, None), i


def test_sizes_next_to_the_format_librarys():
    d = golden_dictionary()
    for n in (300, 4096, 70000):
        src = golden_source(n)
        ours, _ = encode_one(src, d, GOLDEN_DICT_ID, flags=ref.F_CONTENT_SIZE)
        theirs = lz4f_dict_lib.compress_frame(src, d, GOLDEN_DICT_ID, 0, False, content_size=True)
        assert lz4f_dict_lib.decompress(ours, d, n) == (src, None) and lz4f_dict_lib.decompress(theirs, d, n) == (src, None)
        print("golden source of %d bytes: this encoder %d bytes, LZ4F_compressFrame_usingCDict %d bytes, ratio %.3f" % (n, len(ours), len(theirs), len(ours) / len(theirs)))
        assert len(ours) <= twin.raw_frame_bytes(n, 4, ref.F_CONTENT_SIZE, GOLDEN_DICT_ID)
