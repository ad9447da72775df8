"""Legacy LZ4 CLI frame (original/lz4demo.c:84-87,166-317) and batched Wrap/Unwrap (src/LZ4/LZ4Codec.cs:471-599).
CPU: header walk against a frame written by the reference's own CLI (oracle/_ref/lz4demo).  GPU: frames written by
the product are byte-identical to the CLI's and decode with it; frames written by the CLI decode with the product.
What the CLI wrote and read is recorded in tests/golden/ref_records.json (tests/golden/make_golden.py): its frames are
the frame header plus LZ4_compress / LZ4_compressHC of the input, rebuilt here and checked against the recorded digest."""
import numpy as np
import pytest

import ref_records as rr
from lz4net_amd import legacy_frame as lf

FRAMES = rr.load()["frames"]


def _cli_frame(oracle, data, dist, hc):
    """The frame the reference CLI wrote for `data` (magic, then a length-prefixed LZ4 block per 8 MiB chunk), rebuilt
    from the oracle's bytes; only returned when it is the CLI's byte for byte (length and digest as recorded)."""
    rec = FRAMES[rr.frame_key(len(data), dist, hc)]
    a = np.frombuffer(data, np.uint8)
    frame = bytearray((0x184C2102).to_bytes(4, "little"))
    for i in range(0, len(data), lf.CHUNK_SIZE):
        c = oracle.compress(a[i:i + lf.CHUNK_SIZE], hc=hc)
        frame += len(c).to_bytes(4, "little") + bytes(c)
    frame = bytes(frame)
    assert (len(frame), rr.sha(frame)) == (rec["len"], rec["sha"]), "the rebuilt frame is not the reference CLI's"
    return frame, rec


def test_parse_cli_frames(oracle):
    n, dist, hc = rr.FRAME_PARSE_CASE
    data = rr.frame_sample(oracle, n, dist)
    frame, _ = _cli_frame(oracle, data, dist, hc)
    assert frame[:4] == bytes([0x02, 0x21, 0x4C, 0x18])
    chunks = lf.parse_frame(frame)
    assert len(chunks) == 1 and chunks[0] == (8, len(frame) - 8)
    assert int.from_bytes(frame[4:8], "little") == len(frame) - 8
    # the payload is exactly LZ4_compress of the whole input (one chunk < 8 MiB)
    ret, out = oracle.compress_raw(np.frombuffer(data, np.uint8), lf._bound(len(data)))
    assert ret == len(frame) - 8 and bytes(out[:ret]) == frame[8:]
    # appended frames: the second magic is skipped like lz4demo.c:289-290 does
    both = lf.parse_frame(frame + frame)
    assert both == [(8, len(frame) - 8), (len(frame) + 8, len(frame) - 8)]
    assert lf.parse_frame(frame[:4]) == []
    with pytest.raises(lf.ArgumentException):
        lf.parse_frame(b"\x00\x00\x00\x00" + frame[4:])
    with pytest.raises(lf.ArgumentException):
        lf.parse_frame(frame[:-1])
    with pytest.raises(lf.ArgumentException):
        lf.parse_frame(frame + b"\x01\x02")


def test_bound_matches_reference_macro():
    for n in (0, 1, 254, 255, 256, 65536, 8 << 20):
        assert lf._bound(n) == n + n // 255 + 16                   # original/lz4.h:85-86


@pytest.mark.gpu
@pytest.mark.parametrize("hc", [False, True])
def test_frame_interop_with_reference_cli(oracle, hc):
    for n_bytes, dist, _ in [c for c in rr.FRAME_INTEROP_CASES if c[2] == hc]:
        data = rr.frame_sample(oracle, n_bytes, dist)
        ours = lf.compress_frame(data, high_compression=hc)
        theirs, rec = _cli_frame(oracle, data, dist, hc)
        assert ours == theirs, "frame differs from the reference CLI's at %d bytes" % n_bytes
        # their reader on our frame: the CLI's -d on this very byte string
        assert rec["cli_decode_rc"] == 0 and rec["cli_decode_sha"] == rr.sha(data)
        assert lf.decompress_frame(theirs) == data                  # our reader on their frame
        assert lf.decompress_frame(ours + ours) == data + data      # appended frames


@pytest.mark.gpu
def test_frame_small_chunks_roundtrip(oracle):
    data = rr.frame_sample(oracle, 500000, 2)
    for chunk in (4096, 65536, 100000):
        frame = lf.compress_frame(data, chunk_size=chunk)
        assert len(lf.parse_frame(frame)) == (len(data) + chunk - 1) // chunk
        assert lf.decompress_frame(frame, chunk_size=chunk) == data
    assert lf.compress_frame(b"") == (0x184C2102).to_bytes(4, "little")
    assert lf.decompress_frame(lf.compress_frame(b"")) == b""
    with pytest.raises(lf.ArgumentException):                       # corrupted payload -> negative decoder result
        bad = bytearray(lf.compress_frame(data[:70000]))
        bad[8] = 0xFF; bad[9] = 0xFF; bad[10] = 0xFF
        lf.decompress_frame(bytes(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("hc", [False, True])
def test_wrap_many_equals_wrap(oracle, hc):
    from lz4net_amd.codec import LZ4Codec
    rng = np.random.default_rng(5)
    msgs = [b"", b"a", bytes(100), rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
            rr.frame_sample(oracle, 20000, 2), rr.frame_sample(oracle, 65536, 3), b"Lorem ipsum dolor sit amet, " * 40]
    many = LZ4Codec.WrapMany(msgs, high_compression=hc)
    single = [(LZ4Codec.WrapHC if hc else LZ4Codec.Wrap)(m) for m in msgs]
    assert many == single
    assert LZ4Codec.UnwrapMany(many) == msgs
    assert [LZ4Codec.Unwrap(w) for w in many] == msgs
