"""GPU: many LZ4 frames encoded and decoded on the device in one call (lz4hip_lz4f_batch_* of include/lz4hip.h and the Python calls of
lz4net_amd/lz4_frame.py over them), with the real block codecs.  The reference is the one-frame path of the same library: batch encode
byte for byte against compress_frame_device of every item alone, batch decode field by field against lz4hip_lz4f_decode_device on
every item alone, at the small shapes of tests/test_simt_lz4f_batch.py; then the frames liblz4 wrote as one batch, 4 100 tiny items and
one round trip of 1 024 items of 64 KiB.  The broken inputs only have bytes flipped or cut: the kernels answer with statuses."""
import ctypes as C
import types

import numpy as np
import pytest

import lz4f_gpu as gpu
import lz4f_ref as ref
from gpu_helpers import dev, host, i64, s0
from lz4f_batch_cases import golden_batch, outcome_items, sources, tiny_items
from lz4f_cases import INFO_FIELDS, offsets_of, sample
from lz4f_gpu import dev_bytes
from lz4net_amd import _lib, batch, lz4_frame as lz
from lz4net_amd.codec import ArgumentException

pytestmark = pytest.mark.gpu

E_ARGUMENT = _lib.E_ARGUMENT


def options(flags):
    return dict(block_checksum=bool(flags & 1), content_checksum=bool(flags & 2), content_size=bool(flags & 4))


def encode_call(src, off, block_id=4, mode=0, flags=0):
    """lz4hip_lz4f_batch_encode_device -> (bytes, dst_off); asserts nothing past the bound was written"""
    import torch
    L = _lib.lib()
    n = len(off) - 1
    t, o = dev_bytes(src), i64(off)
    bound = L.lz4hip_lz4f_batch_bound(n, len(src), block_id, flags)
    out = torch.full((bound + 64,), 0xA7, dtype=torch.uint8, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(max(L.lz4hip_lz4f_batch_encode_scratch_bytes(n, len(src), block_id), 1), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_lz4f_batch_encode_device(t.data_ptr(), len(src), o.data_ptr(), n, block_id, mode, flags, out.data_ptr(), bound, out_off.data_ptr(),
                                             scratch.data_ptr(), scratch.numel(), s0()) == 0
    got_off = out_off.cpu().numpy()
    raw = host(out)
    assert raw[int(got_off[n]):] == b"\xA7" * (len(raw) - int(got_off[n])), "bytes past the last frame were written"
    return raw[:int(got_off[n])], got_off


def item_alone(frame, slot, flags=3, max_blocks=8):
    """lz4hip_lz4f_decode_device on one item alone, with a table and a dst_cap that hold it -> (record as a dict, its bytes)"""
    info, dst = gpu.frame_call(frame, slot, flags, 1 << 19, max_blocks)
    assert info["error"] != ref.TABLE_FULL and info["decoded_bytes"] <= 1 << 19
    return info, dst[:info["decoded_bytes"]].tobytes()


def decode_call(blob, off, slot=65536, max_blocks=64, round_blocks=0, flags=3, dst_cap=None, room=1 << 21):
    """lz4hip_lz4f_batch_decode_device -> (records as dicts, batch record, dst_off, written_items, the first dst_cap bytes of the
    output); asserts that the 0xA7 fill past dst_cap is intact"""
    cap = room if dst_cap is None else dst_cap
    info, recs, dst_off, dst, written = gpu.batch_call(blob, slot, max_blocks, round_blocks, flags, cap, off=off)
    raw = dst.tobytes()
    assert raw[cap:] == b"\xA7" * gpu.PAD, "bytes past dst_cap were written"
    return recs, types.SimpleNamespace(**info), dst_off, written, raw[:cap]


def check_against_one_frame_calls(items, slot=65536, one_frame_blocks=8, **kw):
    """every item's record and bytes are those of the one-frame call on it; the batch record is the lowest failing item's"""
    blob, off = b"".join(items), offsets_of(items)
    recs, info, dst_off, written, raw = decode_call(blob, off, slot=slot, **kw)
    flags, cap = kw.get("flags", 3), len(raw)                        # (dst_cap, or the room the call was given)
    outs = []
    for i, item in enumerate(items):
        want, out = item_alone(item, slot, flags, one_frame_blocks)
        if dst_off[i + 1] > cap and (want["checks"] >> 2) == ref.VERIFIED:      # not wholly written: present but not checked
            want = dict(want, checks=(want["checks"] & 3) | ref.SKIPPED << 2)
            if want["error"] == ref.CONTENT_CHECKSUM:
                want.update(error=ref.OK, error_offset=-1)
        assert recs[i] == want, (i, {f: (recs[i][f], want[f]) for f in INFO_FIELDS if recs[i][f] != want[f]})
        outs.append(out)
    assert list(dst_off) == list(offsets_of(outs))
    content = b"".join(outs)
    upto = min(cap, len(content))
    assert raw[:upto] == content[:upto] and raw[upto:] == b"\xA7" * (len(raw) - upto), "nothing outside [0, min(decoded_bytes, dst_cap)) is written"
    assert written == sum(1 for e in dst_off[1:] if e <= cap)
    bad = [i for i, r in enumerate(recs) if r["error"] != ref.OK]
    assert (info.items, info.decoded_bytes, info.blocks) == (len(items), len(content), sum(r["blocks"] for r in recs))
    assert info.first_error == (bad[0] if bad else -1) and info.error == (recs[bad[0]]["error"] if bad else 0)
    assert info.error_offset == (recs[bad[0]]["error_offset"] if bad else -1)
    return recs, outs, info


# ---- 1. encode identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", range(8))
def test_encode_is_compress_frame_device_of_every_item(oracle, flags):
    items = sources(oracle)
    t, off = dev(b"".join(items)), i64(offsets_of(items))
    for block_size, hc in ((65536, False), (65536, True), (262144, False), (262144, True)):
        frames, frame_off = lz.compress_frames_device(t, off, block_size=block_size, high_compression=hc, **options(flags))
        alone = [host(lz.compress_frame_device(dev_bytes(it), block_size=block_size, high_compression=hc, **options(flags))) for it in items]
        assert list(frame_off.cpu().numpy()) == list(offsets_of(alone))
        got = host(frames)
        assert got == b"".join(alone), (block_size, hc, "not the frames of the items alone")
        if block_size == 65536 and not hc:
            assert alone[0] == ref.write_frame(oracle, b"", 4, False, flags)[0] and alone[5] == ref.write_frame(oracle, items[5], 4, False, flags)[0]
            staged, staged_off = lz.compress_frames_host(np.frombuffer(b"".join(items), np.uint8), offsets_of(items), **options(flags))
            assert staged.tobytes() == got and list(staged_off) == list(offsets_of(alone))


def test_encode_an_item_with_decreasing_offsets_takes_no_bytes(oracle):
    items = sources(oracle)
    src, off = b"".join(items), list(offsets_of(items))
    off.insert(5, off[4] - 5)
    got, got_off = encode_call(src, off, flags=7)
    alone = [host(lz.compress_frame_device(dev_bytes(it), block_checksum=True, content_checksum=True)) for it in items[:4]]
    assert got_off[4] == got_off[5] and got[:got_off[4]] == b"".join(alone)
    with pytest.raises(ArgumentException, match="offsets are invalid"):
        lz.compress_frames_device(dev(src), i64(off))


# ---- 2. decode identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 7])
def test_decode_is_the_one_frame_decode_of_every_item(oracle, flags):
    items = sources(oracle)
    blob, off = encode_call(b"".join(items), offsets_of(items), flags=flags)
    frames = [blob[a:b] for a, b in zip(off[:-1], off[1:])]
    for verify in (3, 0):
        recs, outs, info = check_against_one_frame_calls(frames, flags=verify, max_blocks=11)
        assert outs == items and info.error == 0 and info.blocks == 10
    data, data_off = lz.decompress_frames_device(dev(blob), i64(off))
    assert host(data) == b"".join(items) and list(data_off.cpu().numpy()) == list(offsets_of(items))
    data, data_off = lz.decompress_frames_host(np.frombuffer(blob, np.uint8), off)
    assert data.tobytes() == b"".join(items) and list(data_off) == list(offsets_of(items))


# ---- 3. every outcome once, all in one batch --------------------------------------------------------------------------------------------
def test_every_outcome_in_one_batch(oracle):
    good, src, faults = outcome_items(oracle)
    items = [good]
    for _, bad, _ in faults:
        items += [bad, good]
    recs, outs, info = check_against_one_frame_calls(items, max_blocks=5 * len(items), round_blocks=3, room=1 << 23)
    assert [r["error"] for r in recs] == [ref.OK] + [c for _, _, code in faults for c in (code, ref.OK)]
    assert info.first_error == 1 and info.error == ref.BAD_MAGIC
    assert all(outs[k] == src for k in range(0, len(items), 2)), "a failing item never disturbs another item's bytes"
    names = [name for name, _, _ in faults]
    recs, _, _ = check_against_one_frame_calls(items, max_blocks=5 * len(items), flags=2, room=1 << 23)
    assert recs[2 * names.index("block_sum") + 1]["error"] == ref.CORRUPT_BLOCK
    # the Python fronts raise the first failing item's exception
    blob, off = b"".join(items[2:]), offsets_of(items[2:])
    with pytest.raises(ArgumentException, match="unknown magic") as e:
        lz.decompress_frames_device(dev(blob), i64(off))
    assert e.value.item == 1 and e.value.status == ref.BAD_MAGIC
    with pytest.raises(ArgumentException, match="unknown magic") as e:
        lz.decompress_frames_host(np.frombuffer(blob, np.uint8), off)
    assert e.value.item == 1
    off = list(offsets_of(items[:3]))
    off[1] += len(items[1]) + 1
    recs, info, dst_off, _, _ = decode_call(b"".join(items[:3]), off)
    assert recs[1]["error"] == E_ARGUMENT and dst_off[1] == dst_off[2] and info.first_error == 1 and info.error == E_ARGUMENT


# ---- 4. table, rounds, slots and clipping -------------------------------------------------------------------------------------------------
def mixed_frames(oracle):
    items = sources(oracle)
    a, ao = encode_call(b"".join(items), offsets_of(items), 4, 0, 7)
    b, bo = encode_call(b"".join(items[3:]), offsets_of(items[3:]), 5, 1, 3)
    return [a[x:y] for x, y in zip(ao[:-1], ao[1:])] + [b[x:y] for x, y in zip(bo[:-1], bo[1:])], items + items[3:]


def test_table_rounds_slots_and_clipping(oracle):
    frames, items = mixed_frames(oracle)
    recs, outs, info = check_against_one_frame_calls(frames, slot=262144, max_blocks=14)
    assert outs == items and info.blocks == 14 and info.error == 0
    recs, info, dst_off, written, raw = decode_call(b"".join(frames), offsets_of(frames), slot=262144, max_blocks=13)
    assert info.error == ref.TABLE_FULL and info.blocks == 14 and raw == b"\xA7" * len(raw) and written == 0, "the count needed; dst untouched"
    for round_blocks in (1, 2):
        _, outs, _ = check_against_one_frame_calls(frames, slot=262144, max_blocks=17, round_blocks=round_blocks)
        assert outs == items
    big = encode_call(items[5], [0, len(items[5])], 6, 0, 7)[0]
    recs, outs, info = check_against_one_frame_calls(frames[:3] + [big] + frames[3:], slot=262144, max_blocks=14)
    assert [r["error"] for r in recs] == [0] * 3 + [ref.SLOT_TOO_SMALL] + [0] * 8 and info.first_error == 3
    ends = offsets_of(items)
    for cap in (0, int(ends[5]), int(ends[5]) - 1, int(ends[6]) + 70000):
        recs, _, info = check_against_one_frame_calls(frames, slot=262144, max_blocks=14, round_blocks=2, dst_cap=cap)
        assert info.decoded_bytes == ends[-1] and [(r["checks"] >> 2) == ref.VERIFIED for r in recs] == [e <= cap for e in ends[1:]]


# ---- 6. other formats of item ------------------------------------------------------------------------------------------------------------
def test_skippable_trailing_bytes_empty_item_and_no_item(oracle):
    src = sample(oracle, 3, 70000)
    frame = host(lz.compress_frame_device(dev(src), block_checksum=True, content_checksum=True))
    items = [frame, ref.skippable(b"user data", 3), frame + frame[:40], b"", frame]
    recs, outs, info = check_against_one_frame_calls(items)
    assert [r["error"] for r in recs] == [0, 0, 0, ref.BAD_MAGIC, 0] and recs[1]["kind"] == 1 and recs[2]["frame_bytes"] == len(frame)
    assert outs == [src, b"", src, b"", src]
    recs, info, dst_off, written, raw = decode_call(b"", [0])
    assert (info.items, info.blocks, info.decoded_bytes, info.first_error, info.error) == (0, 0, 0, -1, 0) and list(dst_off) == [0] and written == 0
    import torch
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    frames, frame_off = lz.compress_frames_device(empty, i64([0]))
    assert frames.numel() == 0 and frame_off.tolist() == [0]
    data, data_off = lz.decompress_frames_device(empty, i64([0]))
    assert data.numel() == 0 and data_off.tolist() == [0]
    frames, frame_off = lz.compress_frames_device(empty, i64([0, 0, 0]), content_checksum=True)
    assert host(frames) == ref.write_frame(oracle, b"", 4, False, 6)[0] * 2


# ---- the format library's frames, tiny items, a large batch -------------------------------------------------------------------------------
def test_golden_frames_as_one_batch(oracle):
    names, recs_json, frames, srcs = golden_batch(oracle)
    recs, outs, info = check_against_one_frame_calls(frames, slot=0, one_frame_blocks=16, max_blocks=24, round_blocks=4, room=1 << 23)
    for name, j, r, out, src in zip(names, recs_json, recs, outs, srcs):
        if j["linked"]:
            assert r["error"] == ref.UNSUPPORTED_LINKED and out == b"", name
        elif j["skippable_bytes"]:
            assert r["kind"] == 1 and r["error"] == 0 and out == b"", name
        else:
            assert r["error"] == 0 and out == src, name
    assert info.first_error == names.index("linked") and info.error == ref.UNSUPPORTED_LINKED


def test_4100_tiny_items():
    import torch
    items = tiny_items()
    src, off = b"".join(items), offsets_of(items)
    frames, frame_off = lz.compress_frames_device(dev(src), i64(off), block_checksum=True, content_checksum=True)
    f, fo = host(frames), frame_off.cpu().numpy()
    for i in (0, 1, 4095, 4096, 4099):
        want, out = item_alone(f[fo[i]:fo[i + 1]], 65536)
        assert want["error"] == 0 and out == items[i] and want["checks"] == 5
    data, data_off = lz.decompress_frames_device(frames, frame_off, max_blocks=len(items))
    assert host(data) == src and bool(torch.equal(data_off.cpu(), torch.from_numpy(off)))
    recs, info, dst_off, written, raw = decode_call(f, fo, max_blocks=len(items) + 3, round_blocks=4099, room=len(src))
    assert info.error == 0 and info.blocks == len(items) and written == len(items) and raw == src
    bad = bytearray(f)
    bad[fo[4097] + 15 + 4] ^= 0xFF
    recs, info, _, _, _ = decode_call(bytes(bad), fo, max_blocks=len(items), room=len(src))
    assert [i for i, r in enumerate(recs) if r["error"]] == [4097] and info.first_error == 4097 and info.error == ref.BLOCK_CHECKSUM


def test_1024_items_of_64_kib_round_trip_and_one_flipped_byte():
    import torch
    raw = batch.synth(2, 77, 0, 1024).reshape(-1)
    off = torch.arange(1025, dtype=torch.int64, device="cuda") * 65536
    frames, frame_off = lz.compress_frames_device(raw, off, block_checksum=True, content_checksum=True)
    assert int(frame_off[1024]) == frames.numel() < raw.numel()
    back, back_off = lz.decompress_frames_device(frames, frame_off, max_blocks=1024)
    assert back.numel() == raw.numel() and bool(torch.equal(back, raw)) and bool(torch.equal(back_off, off))
    bad = frames.clone()
    bad[int(frame_off[1000]) + 15 + 4 + 100] ^= 0x10                   # a byte of item 1000's only block
    with pytest.raises(ArgumentException, match="block checksum") as e:
        lz.decompress_frames_device(bad, frame_off, max_blocks=1024)
    assert e.value.item == 1000 and e.value.status == ref.BLOCK_CHECKSUM
    L = _lib.lib()
    need = L.lz4hip_lz4f_batch_decode_scratch_bytes(1024, 65536, 1024, 0)
    scratch, out = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.empty(raw.numel(), dtype=torch.uint8, device="cuda")
    out_off, recs_dev = torch.zeros(1025, dtype=torch.int64, device="cuda"), torch.zeros(C.sizeof(_lib.Lz4fInfo) * 1024, dtype=torch.uint8, device="cuda")
    info_dev, written = torch.zeros(C.sizeof(_lib.Lz4fBatchInfo), dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.lz4hip_lz4f_batch_decode_device(bad.data_ptr(), bad.numel(), frame_off.data_ptr(), 1024, 65536, 1024, 0, 3, scratch.data_ptr(), need, out.data_ptr(),
                                             out.numel(), out_off.data_ptr(), recs_dev.data_ptr(), info_dev.data_ptr(), written.data_ptr(), s0()) == 0
    recs = (_lib.Lz4fInfo * 1024).from_buffer_copy(host(recs_dev))
    assert [i for i, r in enumerate(recs) if r.error] == [1000] and recs[1000].error == ref.BLOCK_CHECKSUM, "item 1000 and no other"
