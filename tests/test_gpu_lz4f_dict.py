"""GPU: LZ4 frames with a dictionary decoded on the device (lz4hip_lz4f_decode_dict_* and lz4hip_lz4f_batch_decode_dict_* of
include/lz4hip.h, dictionary=... on the Python calls of lz4net_amd/lz4_frame.py), with the real block decoders, against the twin
tests/lz4f_ref.py field by field: the hand-built frames, the frames liblz4 wrote with LZ4F_compressFrame_usingCDict, the mixed
batch of tests/test_simt_lz4f_dict.py, and one batch in which many wavefronts run the ordered decode at once.  Every output buffer is
filled with 0xA7 first and starts at the very start of its allocation, and what the call was not to write is still 0xA7 afterwards; the
dictionary lies between guard bytes, at an even or an odd address."""
import ctypes as C
import functools

import numpy as np
import pytest

import lz4f_built as built
import lz4f_cases as cases
import lz4f_gpu as gpu
import lz4f_ref as ref
from gpu_helpers import dev, host, i64
from lz4f_cases import ACCEPT, INFO_FIELDS, check_image, offsets_of
from lz4f_dict_cases import GOLDEN_DICT_ID, dictionary, golden, golden_dictionary, hand_built, mixed_batch
from lz4f_gpu import FILL, PAD, DeviceDict, batch_call, frame_call
from lz4net_amd import _lib, lz4_frame as lz
from lz4net_amd.codec import ArgumentException

pytestmark = pytest.mark.gpu

check_batch = functools.partial(gpu.check_batch, None)                # the _dict_ call: no codec, every block is the twin's own to decode


@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("n", built.DICT_LENGTHS)
def test_hand_built_frames_through_the_batch_call(n, odd):
    """every case the dictionary's length allows, each once as item 0 (at the very start of the output's allocation), then all as one batch"""
    cases, d = hand_built(n), dictionary(n)
    names = sorted(cases)
    for name in names:
        frame, content, bad = cases[name]
        recs, _ = check_batch([frame], d, odd=odd, round_blocks=2 * odd)
        assert (recs[0]["error"] == ref.OK) == (content is not None), name
        if content is None:
            assert recs[0]["error"] == ref.CORRUPT_BLOCK and recs[0]["good_bytes"] == (1000 if name.startswith("l") else 100), name
    recs, got = check_batch([built.front_item()] + [cases[k][0] for k in names] + [built.front_item()], d, odd=odd, round_blocks=3)
    assert [r["error"] == ref.OK for r in recs[1:-1]] == [cases[k][1] is not None for k in names] and recs[0]["error"] == recs[-1]["error"] == ref.OK


@pytest.mark.parametrize("dict_id,frame_id,error", [(7, 7, ref.OK), (7, 8, ref.DICT_ID_MISMATCH), (0, 8, ref.OK), (7, None, ref.OK)])
def test_the_dictionary_id(dict_id, frame_id, error):
    d = dictionary(13)
    frames = [hand_built(13, frame_id)[name][0] for name in ("i_into_the_block", "l_run_fill")]
    frames.append(built.frame_of([(b"0123456789", True)], linked=False, flags=ref.F_CONTENT_SIZE, content=b"0123456789", dict_id=frame_id))
    recs, _ = check_batch(frames, d, dict_id)
    assert [r["error"] for r in recs] == [error] * 3
    if error:
        assert [r["error_offset"] for r in recs] == [6, 6, 14] and all(r["blocks"] == 0 for r in recs)


@pytest.mark.parametrize("round_blocks", [0, 2])
def test_golden_frames_as_one_batch(round_blocks):
    names, _, frames, srcs = golden()
    recs, got = check_batch(frames, golden_dictionary(), GOLDEN_DICT_ID, round_blocks=round_blocks, odd=round_blocks & 1)
    assert got["error"] == ref.OK and got["decoded_bytes"] == sum(len(s) for s in srcs)


@pytest.mark.parametrize("round_blocks", [0, 2])
def test_mixed_batch_whole_and_clipped(round_blocks):
    frames, d, dict_id, linked = mixed_batch()
    _, _, _, ends, total = cases.expect(None, list(frames), 65536, 3, accept=True, dictionary=d, dict_id=dict_id)
    for cap in (total, 0, int(ends[linked]) + 10 + 30, int(ends[linked]) + 10 + 54):   # ... inside, and at the end of, the linked item's second block
        recs, got = check_batch(frames, d, dict_id, round_blocks=round_blocks, dst_cap=cap, odd=1)
        assert [r["error"] for r in recs] == [0, 0, 0, 0, ref.DICT_ID_MISMATCH] and got["first_error"] == 4


def test_the_one_frame_call_the_host_calls_and_the_python_calls_on_every_golden_frame():
    names, golden_recs, frames, srcs = golden()
    d = golden_dictionary()
    dd = DeviceDict(d, 1)
    for rec, frame, src in zip(golden_recs, frames, srcs):
        want, out, unspecified, _ = ref.read_frame(None, frame, 65536, accept_linked=True, dictionary=d, dict_id=GOLDEN_DICT_ID)
        got, dst = frame_call(frame, 65536, 3 | ACCEPT, len(src), dd=dd, dict_id=GOLDEN_DICT_ID)
        assert got == want, {f: (got[f], want[f]) for f in INFO_FIELDS if got[f] != want[f]}
        check_image(dst, [(out, unspecified)], [0, len(src)], len(src), FILL)
        assert out == src
        assert host(lz.decompress_frame_device(dev(frame), accept_linked=True, dictionary=dd.tensor, dict_id=GOLDEN_DICT_ID)) == src
        assert lz.decompress_frame_host(frame, accept_linked=True, dictionary=d) == src
        info, buf = _lib.Lz4fInfo(), np.full(len(src) + PAD, FILL, np.uint8)
        dh = np.frombuffer(d, np.uint8)
        assert _lib.lib().lz4hip_lz4f_decode_dict_host(frame, len(frame), dh.ctypes.data, dh.size, 0, 3 | ACCEPT, buf.ctypes.data, len(src), C.byref(info)) == 0
        assert buf[:len(src)].tobytes() == src and (buf[len(src):] == FILL).all() and info.decoded_bytes == len(src)
    assert dd.intact()
    data, off = lz.decompress_frames_device(dev(b"".join(frames)), i64(offsets_of(frames)), accept_linked=True, dictionary=dd.tensor, dict_id=GOLDEN_DICT_ID)
    assert host(data) == b"".join(srcs) and list(off.cpu().numpy()) == list(offsets_of(srcs))
    data, off = lz.decompress_frames_host(b"".join(frames), offsets_of(frames), accept_linked=True, dictionary=d, dict_id=GOLDEN_DICT_ID)
    assert data.tobytes() == b"".join(srcs) and list(off) == list(offsets_of(srcs))
    with pytest.raises(ArgumentException, match="dictionary ID is not the one"):
        lz.decompress_frames_host(b"".join(frames), offsets_of(frames), accept_linked=True, dictionary=d, dict_id=GOLDEN_DICT_ID + 1)
    with pytest.raises(ArgumentException, match="dictionary ID is not the one"):
        lz.decompress_frame_device(dev(frames[0]), accept_linked=True, dictionary=dd.tensor, dict_id=GOLDEN_DICT_ID + 1)


def test_many_wavefronts_run_the_ordered_decode_at_once():
    """300 small linked items out of one dictionary, every third one behind an independent item: several workgroups of the ordered decode"""
    d = dictionary(4097)
    cases = hand_built(4097, 7)
    kinds = [cases[k] for k in ("l_across_a_raw_block", "l_short_sequences", "l_run_fill", "l_behind_a_raw_block")]
    items, want = [], []
    for k in range(300):
        frame, content, _ = kinds[k % 4]
        if k % 3 == 0:
            items.append(cases["i_into_the_block"][0])
            want.append(cases["i_into_the_block"][1])
        items.append(frame)
        want.append(content)
    dd = DeviceDict(d, 1)
    data, off = lz.decompress_frames_device(dev(b"".join(items)), i64(offsets_of(items)), max_blocks=1024, accept_linked=True, dictionary=dd.tensor, dict_id=7)
    got, ends = host(data), off.cpu().numpy()
    assert list(ends) == list(offsets_of(want)) and dd.intact()
    for i, w in enumerate(want):
        assert got[ends[i]:ends[i + 1]] == w, i


def test_without_a_dictionary_the_call_is_the_plain_call():
    frames, d, _, _ = mixed_batch()
    frames = [built.front_item()] + list(frames)
    for flags in (3, 3 | ACCEPT):
        plain = batch_call(frames, max_blocks=16, round_blocks=2, flags=flags, cap=4096)
        none = batch_call(frames, max_blocks=16, round_blocks=2, flags=flags, cap=4096, dict_id=99, dict_call=True)
        assert plain[:2] == none[:2] and list(plain[2]) == list(none[2]) and (plain[3] == none[3]).all() and plain[4] == none[4]
        assert plain[1][1]["error"] == ref.UNSUPPORTED_DICT
    got, dst = frame_call(frames[1], 65536, 3, 64, dict_id=5, dict_call=True)
    assert got["error"] == ref.UNSUPPORTED_DICT and got["error_offset"] == 4 and (dst == FILL).all()
    L = _lib.lib()
    info = _lib.Lz4fInfo()
    assert L.lz4hip_lz4f_decode_dict_host(frames[1], len(frames[1]), None, 0, 5, 3, None, 0, C.byref(info)) == ref.UNSUPPORTED_DICT
    assert L.lz4hip_lz4f_decode_dict_host(frames[1], len(frames[1]), None, 5, 0, 3, None, 0, C.byref(info)) == _lib.E_ARGUMENT
    assert L.lz4hip_lz4f_decode_dict_host(frames[1], len(frames[1]), frames[1], -1, 0, 3, None, 0, C.byref(info)) == _lib.E_ARGUMENT


def test_the_existing_calls_still_refuse_a_frame_with_a_dictionary_id():
    frames, d, _, _ = mixed_batch()
    got, recs, off, dst, written = batch_call([built.front_item(), frames[0]], flags=3 | ACCEPT, cap=4096)
    assert got["error"] == ref.UNSUPPORTED_DICT and got["first_error"] == 1 and list(off) == [0, 37, 37]
    assert dst[:37].tobytes() == built.FRONT and (dst[37:] == FILL).all()
    with pytest.raises(ArgumentException, match="frames with a dictionary ID are not supported"):
        lz.decompress_frame_device(dev(frames[0]))
    with pytest.raises(ArgumentException, match="frames with a dictionary ID are not supported"):
        lz.decompress_frames_host(frames[0], offsets_of([frames[0]]), accept_linked=True)
    with pytest.raises(ArgumentException, match="frames with a dictionary ID are not supported"):
        lz.decompress_frame_host(frames[0], dictionary=b"")


def test_the_dispatch_counters_move_the_wavefront_mapping_only():
    """a batch large enough for the lane mapping in the plain call: with a dictionary every round is the wavefront mapping's"""
    d = dictionary(4097)
    frame = hand_built(4097, 7)["i_into_the_block"][0]
    items = [frame] * 3000                                             # 6 000 rows
    dd = DeviceDict(d)
    before = _lib.dispatch_counts()
    data, off = lz.decompress_frames_device(dev(b"".join(items)), i64(offsets_of(items)), max_blocks=6000, dictionary=dd.tensor, dict_id=7)
    after = _lib.dispatch_counts()
    moved = [k for k in range(_lib.K_COUNT) if after[k] != before[k]]
    assert moved == [_lib.K_DECODE_WAVE] and after[_lib.K_DECODE_WAVE] == before[_lib.K_DECODE_WAVE] + 1
    content = hand_built(4097, 7)["i_into_the_block"][1]
    assert host(data) == content * 3000
