"""GPU: the xxHash32 row kernel and whole LZ4 frames (magic 0x184D2204) encoded and decoded on the device in one call (lz4hip_xxh32_rows_device
and lz4hip_lz4f_* of include/lz4hip.h): the checksum's row set against a from-the-spec xxh32, the frames liblz4 wrote
(tests/golden/lz4f_frames.json), round trips through the device calls and the host calls with our frames parsed by the test-side twin
(tests/lz4f_ref.py) and compared byte for byte with the emulator path's, every outcome once, and one large frame.  The broken inputs
only have bytes flipped or cut: the kernels answer with statuses."""
import base64
import json
import os

import numpy as np
import pytest

import lz4f_ref as ref
from gpu_helpers import dev, host
from lz4f_cases import LENGTHS, emu_encode, flip, mixed, sample
from lz4f_gpu import frame_call
from lz4net_amd import batch, lz4_frame as lz
from lz4net_amd.codec import ArgumentException

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_frames.json")) as _f:
    FRAMES = json.load(_f)["frames"]


def hashes(rows, lead=0, seed=0):
    """rows laid end to end from byte `lead` of a device buffer whose last row ends where the allocation's bytes end"""
    import torch
    blob = bytes(lead) + b"".join(rows)
    off = np.cumsum([lead] + [len(r) for r in rows])[:-1].astype(np.int64)
    ln = np.array([len(r) for r in rows], np.int32)
    data = dev(blob) if blob else torch.empty(0, dtype=torch.uint8, device="cuda")
    sums = lz.xxh32_rows_device(data, torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda(), seed)
    return [int(x) for x in sums.cpu().numpy().view(np.uint32)]


def test_xxh32_known_answers_and_the_row_set():
    cases = [(b"", 0x02CC5D05), (b"abc", 0x32D153FF), (b"hello frame " * 40, 0x408E9E1A)]
    assert hashes([d for d, _ in cases]) == [w for _, w in cases]
    assert hashes([b"abc"], seed=7) == [ref.xxh32(b"abc", 7)]
    for lead in (0, 1, 2, 3, 13, 14, 15, 16):
        rng = np.random.default_rng(lead)
        rows = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENGTHS]
        assert hashes(rows, lead) == [ref.xxh32(r) for r in rows], lead


@pytest.mark.parametrize("n", [1, 16, 17, 33, 1000])
def test_xxh32_row_counts(n):
    rng = np.random.default_rng(n)
    rows = [rng.integers(0, 256, int(rng.choice(LENGTHS)), dtype=np.uint8).tobytes() for _ in range(n)]
    assert hashes(rows, 1) == [ref.xxh32(r) for r in rows]


def test_xxh32_sixteen_lengths_in_one_wavefront_and_a_long_row():
    lens = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 500, 511, 512, 513, 64 * 8 * 5 + 77)
    rng = np.random.default_rng(16)
    rows = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    assert hashes(rows, 3) == [ref.xxh32(r) for r in rows]
    big = rng.integers(0, 256, 300001, dtype=np.uint8).tobytes()
    assert hashes([big, b"x", big[:70000]]) == [ref.xxh32(big), ref.xxh32(b"x"), ref.xxh32(big[:70000])]


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_golden_frames_decode_to_their_sources(oracle, name):
    rec = FRAMES[name]
    frame = base64.b64decode(rec["frame"])
    src = ref.golden_source(oracle, rec["source"], rec["bytes"])
    if rec["linked"]:
        for call in (lambda: lz.decompress_frame_device(dev(frame)), lambda: lz.decompress_frame_host(frame)):
            with pytest.raises(ArgumentException, match="linked blocks"):
                call()
        return
    for verify in (True, False):
        assert host(lz.decompress_frame_device(dev(frame), verify=verify)) == src
    assert host(lz.decompress_frame_device(dev(frame), round_blocks=1)) == src
    assert lz.decompress_frame_host(frame) == src
    assert host(lz.decompress_frame_device(dev(frame + frame))) == src + src, "appended frames"


@pytest.mark.parametrize("flags", range(8))
def test_round_trips_every_flag_combination(oracle, flags):
    opts = dict(block_checksum=bool(flags & 1), content_checksum=bool(flags & 2), content_size=bool(flags & 4))
    for n in (0, 1, 65537):
        src = sample(oracle, 2, n)
        frame = host(lz.compress_frame_device(dev(src), **opts))
        assert frame == ref.write_frame(oracle, src, 4, False, flags)[0], (n, "not the twin writer's frame")
        info, out, _, _ = ref.read_frame(oracle, frame)
        assert info["error"] == ref.OK and out == src and info["frame_bytes"] == len(frame)
        assert host(lz.decompress_frame_device(dev(frame))) == src
        assert lz.compress_frame_host(src, **opts) == frame and lz.decompress_frame_host(frame) == src


@pytest.mark.parametrize("n", [65535, 65536, 3 * 65536 + 5])
def test_round_trips_source_lengths(oracle, n):
    src = sample(oracle, 3, n)
    for flags in (0, 7):
        frame = host(lz.compress_frame_device(dev(src), block_checksum=bool(flags & 1), content_checksum=bool(flags & 2), content_size=bool(flags & 4)))
        assert frame == ref.write_frame(oracle, src, 4, False, flags)[0]
        assert host(lz.decompress_frame_device(dev(frame), round_blocks=2)) == src
        assert lz.compress_frame_host(src, block_checksum=bool(flags & 1), content_checksum=bool(flags & 2), content_size=bool(flags & 4)) == frame
        assert lz.decompress_frame_host(frame) == src


@pytest.mark.parametrize("block_size", [65536, 262144, 1048576, 4194304])
def test_block_sizes_mixed_blocks_and_the_emulator_path_s_bytes(oracle, block_size):
    src = mixed(oracle)
    hc = block_size == 262144
    frame = host(lz.compress_frame_device(dev(src), block_size=block_size, high_compression=hc, block_checksum=True, content_checksum=True))
    assert frame == emu_encode(oracle, src, lz.BLOCK_SIZES[block_size], hc, 7), "our frames equal the emulator path's byte for byte"
    assert lz.parse_header(frame)["block_max"] == block_size
    assert host(lz.decompress_frame_device(dev(frame))) == src and lz.decompress_frame_host(frame) == src


def check_against_twin(oracle, frame, slot=0, max_blocks=8, round_blocks=0, flags=3, dst_cap=None, room=1 << 19):
    """lz4hip_lz4f_decode_device against the twin: the record field by field, the bytes, and the 0xA7 fill behind them and past dst_cap"""
    got, dst = frame_call(frame, slot, flags, room if dst_cap is None else dst_cap, max_blocks, round_blocks)
    want, out, _, _ = ref.read_frame(oracle, frame, slot or 4 << 20, max_blocks, flags, dst_cap)
    assert got == want, {f: (got[f], want[f]) for f in got if got[f] != want[f]}
    raw = dst.tobytes()
    assert raw[:len(out)] == out and raw[len(out):] == b"\xA7" * (len(raw) - len(out))
    return want


def test_every_outcome_once(oracle):
    src = mixed(oracle)
    frame, rets, _ = ref.write_frame(oracle, src, 4, False, 7)
    at1 = 15 + 4 + 65536 + 4                                           # block 1's size field (block 0 is stored raw)
    assert rets[0] == 0 and rets[1] > 0
    expect = lambda f, **kw: check_against_twin(oracle, f, **kw)["error"]
    assert expect(frame) == ref.OK
    assert expect(b"abc") == ref.BAD_MAGIC and expect(flip(frame, 1)) == ref.BAD_MAGIC
    assert expect(flip(frame, 4, 0x80)) == ref.BAD_HEADER
    assert expect(flip(frame, 14)) == ref.HEADER_CHECKSUM
    assert expect(ref.descriptor(4, 3, len(src), linked=True) + frame[15:]) == ref.UNSUPPORTED_LINKED
    assert expect(ref.descriptor(4, 7, len(src), dict_id=5) + frame[15:]) == ref.UNSUPPORTED_DICT
    assert expect(ref.write_frame(oracle, src[:70000], 6, False, 0)[0], slot=65536) == ref.SLOT_TOO_SMALL
    assert expect(frame[:at1 + 2]) == ref.TRUNCATED and expect(frame[:at1 + 100]) == ref.TRUNCATED and expect(frame[:-2]) == ref.TRUNCATED
    assert expect(frame[:at1] + ref.le32(65537) + frame[at1 + 4:]) == ref.BAD_BLOCK_SIZE
    assert expect(flip(frame, at1 + 13, 0xFF)) == ref.BLOCK_CHECKSUM
    assert expect(flip(frame, at1 + 13, 0xFF), flags=2) == ref.CORRUPT_BLOCK
    wrong_size = bytearray(flip(frame, 6))
    wrong_size[14] = (ref.xxh32(bytes(wrong_size[4:14])) >> 8) & 0xFF
    assert expect(bytes(wrong_size)) == ref.CONTENT_SIZE
    assert expect(flip(frame, len(frame) - 1)) == ref.CONTENT_CHECKSUM
    assert expect(frame, max_blocks=4) == ref.TABLE_FULL
    # precedence with two faults in one frame; clipping; a skippable frame
    two = flip(flip(frame, at1 + 13, 0xFF), len(frame) - 1)
    assert expect(two, round_blocks=2) == ref.BLOCK_CHECKSUM
    for cap in (0, 2 * 65536, 2 * 65536 - 1):
        assert expect(frame, dst_cap=cap, round_blocks=2) == ref.OK
    assert check_against_twin(oracle, ref.skippable(b"meta", 2) + frame)["kind"] == 1
    with pytest.raises(ArgumentException, match="block checksum"):
        lz.decompress_frame_device(dev(flip(frame, at1 + 13, 0xFF)))
    with pytest.raises(ArgumentException, match="content checksum"):
        lz.decompress_frame_host(flip(frame, len(frame) - 1))
    assert host(lz.decompress_frame_device(dev(flip(frame, len(frame) - 1)), verify=False)) == src


def test_64_mib_round_trip_with_both_checksums():
    """1024 rows of the checksum kernel in one launch, and one row of 64 MiB"""
    import torch
    raw = batch.synth(2, 77, 0, 1024).reshape(-1)
    frame = lz.compress_frame_device(raw, block_checksum=True, content_checksum=True)
    head = lz.parse_header(host(frame[:19]))
    assert head["content_size"] == raw.numel() and head["block_checksum"] and head["content_checksum"]
    back = lz.decompress_frame_device(frame)
    assert back.numel() == raw.numel() and bool(torch.equal(back, raw))
    # the block checksums and the content checksum are what a reader computes: flip one byte of the last block's data
    bad = frame.clone()
    bad[frame.numel() - 100] ^= 0x10
    with pytest.raises(ArgumentException, match="block checksum"):
        lz.decompress_frame_device(bad)
    want = ref.xxh32(host(raw[:65536]))
    got = lz.xxh32_rows_device(raw, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 65536, dtype=torch.int32, device="cuda"))
    assert int(got.cpu().numpy().view(np.uint32)[0]) == want
