"""GPU: LZ4 frames with linked blocks decoded on the device (LZ4HIP_LZ4F_ACCEPT_LINKED on the lz4hip_lz4f_decode_* and
lz4hip_lz4f_batch_decode_* calls of include/lz4hip.h, accept_linked=True on the Python calls of lz4net_amd/lz4_frame.py), with the real
block codecs, against the twin tests/lz4f_ref.py field by field: the hand-built frames, the frames liblz4 wrote, the mixed batch
of tests/test_simt_lz4f_linked.py, and one batch in which many wavefronts run the ordered decode at once.  Every output buffer is
filled with 0xA7 first, and what the call was not to write is still 0xA7 afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest

import lz4f_built as built
import lz4f_cases as cases
import lz4f_ref as ref
from gpu_helpers import dev, host, i64
from lz4f_cases import ACCEPT, INFO_FIELDS, check_image, check_records, offsets_of, records_of
from lz4f_gpu import FILL, PAD, batch_call, check_batch, frame_call
from lz4f_linked_cases import golden, hand_built, mixed_batch
from lz4net_amd import _lib, lz4_frame as lz
from lz4net_amd.codec import ArgumentException

pytestmark = pytest.mark.gpu

expect = functools.partial(cases.expect, accept=True)                 # what the twin says of a batch decoded with the flag


@pytest.mark.parametrize("name", sorted(hand_built()))
def test_hand_built_frames_alone_and_behind_another_item(oracle, name):
    frame, content, bad = hand_built()[name]
    recs, _ = check_batch(oracle, [frame])
    assert (recs[0]["error"] == ref.OK) == (content is not None)
    recs, got = check_batch(oracle, [built.front_item(), frame, built.front_item()], round_blocks=2)
    assert recs[0]["error"] == recs[2]["error"] == ref.OK and got["first_error"] == (-1 if content is not None else 1)


@pytest.mark.parametrize("round_blocks", [0, 2])
def test_golden_frames_as_one_batch(oracle, round_blocks):
    names, _, frames, srcs = golden(oracle)
    recs, got = check_batch(oracle, frames, slot=262144, round_blocks=round_blocks)
    assert got["error"] == ref.OK and got["decoded_bytes"] == sum(len(s) for s in srcs)


@pytest.mark.parametrize("round_blocks", [0, 2])
def test_mixed_batch_whole_and_clipped(oracle, round_blocks):
    frames, two = mixed_batch(oracle)
    _, _, _, ends, total = expect(oracle, list(frames), 65536, 3)
    for cap in (total, 0, int(ends[two]) + 50 + 500):                  # ... inside the second block of the linked two-block item
        recs, got = check_batch(oracle, frames, round_blocks=round_blocks, dst_cap=cap)
        assert [r["error"] for r in recs] == [0, 0, 0, 0, 0, 0, ref.UNSUPPORTED_DICT] and got["first_error"] == 6


def test_the_one_frame_call_and_the_python_calls_on_every_golden_frame(oracle):
    names, golden_recs, frames, srcs = golden(oracle)
    for rec, frame, src in zip(golden_recs, frames, srcs):
        slot = ref.block_bytes(rec["block_id"])
        want, out, unspecified, _ = ref.read_frame(oracle, frame, slot, accept_linked=True)
        got, dst = frame_call(frame, slot, 3 | ACCEPT, len(src))
        assert got == want, {f: (got[f], want[f]) for f in INFO_FIELDS if got[f] != want[f]}
        check_image(dst, [(out, unspecified)], [0, len(src)], len(src), FILL)
        assert out == src
        assert host(lz.decompress_frame_device(dev(frame), accept_linked=True)) == src
        assert lz.decompress_frame_host(frame, accept_linked=True) == src
    data, off = lz.decompress_frames_device(dev(b"".join(frames)), i64(offsets_of(frames)), slot_bytes=262144, accept_linked=True)
    assert host(data) == b"".join(srcs) and list(off.cpu().numpy()) == list(offsets_of(srcs))


def test_many_wavefronts_run_the_ordered_decode_at_once(oracle):
    """256 copies of the golden two-block frame interleaved with 256 independent frames of 3 000 bytes"""
    names, _, frames, srcs = golden(oracle)
    linked, linked_src = frames[names.index("formula_two_blocks")], srcs[names.index("formula_two_blocks")]
    d3 = ref.golden_source(oracle, "d3", 65536)
    small_src = [d3[37 * k:37 * k + 3000] for k in range(256)]
    small = [ref.write_frame(oracle, s, 4, False, 7)[0] for s in small_src]
    items = [f for pair in zip([linked] * 256, small) for f in pair]
    want = [s for pair in zip([linked_src] * 256, small_src) for s in pair]
    data, off = lz.decompress_frames_device(dev(b"".join(items)), i64(offsets_of(items)), max_blocks=768, accept_linked=True)
    got, ends = host(data), off.cpu().numpy()
    assert list(ends) == list(offsets_of(want))
    for i, w in enumerate(want):
        assert got[ends[i]:ends[i + 1]] == w, i


def test_the_host_calls_on_the_mixed_batch(oracle):
    frames, _ = mixed_batch(oracle)
    frames = list(frames)
    recs, outs, _, ends, total = expect(oracle, frames, 65536, 3)
    blob, off = np.frombuffer(b"".join(frames), np.uint8), offsets_of(frames)
    dst = np.full(total + PAD, FILL, np.uint8)
    dst_off = np.zeros(len(frames) + 1, np.int64)
    items, info = (_lib.Lz4fInfo * len(frames))(), _lib.Lz4fBatchInfo()
    rc = _lib.lib().lz4hip_lz4f_batch_decode_host(blob.ctypes.data, blob.size, off.ctypes.data, len(frames), 3 | ACCEPT, dst.ctypes.data, total,
                                                  dst_off.ctypes.data, items, C.byref(info))
    assert rc == ref.UNSUPPORTED_DICT and info.first_error == 6 and list(dst_off) == list(ends)
    check_records(records_of(bytes(items), len(frames)), recs)
    check_image(dst, outs, ends, total, FILL)
    good = frames[:6]
    data, off = lz.decompress_frames_host(b"".join(good), offsets_of(good), accept_linked=True)
    assert data.tobytes() == b"".join(out for out, _ in outs[:6]) and list(off) == list(ends[:7])


def test_without_the_flag_a_linked_frame_is_still_refused(oracle):
    frame = golden(oracle)[2][0]
    got, dst = frame_call(frame, 262144, 3, 1 << 17)
    assert got["error"] == ref.UNSUPPORTED_LINKED and got["decoded_bytes"] == 0 and (dst == FILL).all()
    got, recs, off, dst, written = batch_call([built.front_item(), frame], flags=3, cap=4096)
    assert got["error"] == ref.UNSUPPORTED_LINKED and got["first_error"] == 1 and list(off) == [0, 37, 37]
    assert dst[:37].tobytes() == built.FRONT and (dst[37:] == FILL).all()
    with pytest.raises(ArgumentException, match="frames with linked blocks are not supported"):
        lz.decompress_frame_device(dev(frame))
    with pytest.raises(ArgumentException, match="frames with linked blocks are not supported"):
        lz.decompress_frames_host(frame, offsets_of([frame]))
