"""TEST INFRASTRUCTURE for the tests of batches of LZ4 frames -- tests/test_simt_lz4f_batch.py and tests/test_gpu_lz4f_batch.py: the
batches the tests are made of, and the emulator's batch encode checked against the one-frame path: lz4f_cases.emu_encode of every item
alone.  (The decode harness is tests/lz4f_cases.py's, against the twin tests/lz4f_ref.py on every item alone.)"""
import ctypes as C
import functools
import os

import numpy as np

import lz4f_ref as ref
from emu_lib import GUARD, Guarded, u8
from lz4f_cases import BatchRun, emu, emu_encode, flip, mixed, offsets_of, sample, spans

ITEM_LENGTHS = (0, 1, 13, 65535, 65536, 65537, 3 * 65536 + 5)


# ---- batches -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sources(oracle):
    return tuple(sample(oracle, 2 + (k & 1), n) for k, n in enumerate(ITEM_LENGTHS))


def sources(oracle):
    """items of 0, 1, 13, 65535, 65536, 65537 and 3 * 65536 + 5 bytes, D2 and D3 in turn"""
    return list(_sources(oracle))


@functools.lru_cache(maxsize=None)
def _frame_alone(oracle, item, block_id, hc, flags):
    return emu_encode(oracle, item, block_id, hc, flags)


def frames_alone(oracle, items, block_id=4, hc=False, flags=0):
    """what the one-frame emulator path writes for every item alone (checked there against the twin writer); b"" for a bad item"""
    return [b"" if it is None else _frame_alone(oracle, it, block_id, hc, flags) for it in items]


def golden_batch(oracle):
    """the frames liblz4 wrote (tests/golden/lz4f_frames.json), in name order -> (names, records, frames, sources)"""
    import base64
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4f_frames.json")) as f:
        recs = json.load(f)["frames"]
    names = sorted(recs)
    frames = [base64.b64decode(recs[k]["frame"]) for k in names]
    srcs = [ref.golden_source(oracle, recs[k]["source"], recs[k]["bytes"]) for k in names]
    return names, [recs[k] for k in names], frames, srcs


def tiny_items(count=4100):
    """one-block items of 1 .. 40 bytes"""
    rng = np.random.default_rng(count)
    return [bytes(rng.integers(0, 4, int(n), dtype=np.uint8)) for n in rng.integers(1, 41, count)]


# ---- the emulator path against the one-frame path -----------------------------------------------------------------------------------
def emu_encode_batch(oracle, src, off, block_id=4, hc=False, flags=0, grid=0, host=False, want=None):
    """the emulator path's batch of frames for the items src[off[i], off[i + 1]) -> (bytes, dst_off); asserts that it is `want`
    (default: the concatenation of the twin writer's frames) with the prefix sums as offsets, and that nothing else was written"""
    src, off = bytes(src), np.ascontiguousarray(off, np.int64)
    L, n, bid = emu(), len(off) - 1, block_id or 4
    items = spans(src, off)
    written = [(None, [], []) if it is None else ref.write_frame(oracle, it, bid, hc, flags) for it in items]
    if want is None:
        want = [w[0] or b"" for w in written]
    rets, blob, at, lens, where = [], b"", [], [], []
    for i, (it, (_, r, d)) in enumerate(zip(items, written)):
        for j, (ret, data) in enumerate(zip(r, d)):
            rets.append(ret)
            at.append(len(blob))
            blob += data
            lens.append(min(len(it) - j * ref.block_bytes(bid), ref.block_bytes(bid)))
            where.append(int(off[i]) + j * ref.block_bytes(bid))
    arrs = [np.array(rets + [0], np.int32), u8(blob + b"\0"), np.array(at + [0], np.int64), np.array(lens + [0], np.int32), np.array(where + [0], np.int64)]
    run = BatchRun(enc_results=arrs[0].ctypes.data, enc_bytes=arrs[1].ctypes.data, enc_at=arrs[2].ctypes.data, enc_len=arrs[3].ctypes.data,
                 enc_src=arrs[4].ctypes.data, enc_rows=len(rets), grid=grid)
    bound = L.emu_lz4f_batch_bound(n, len(src), block_id, flags)
    assert bound >= sum(len(w) for w in want)
    a = Guarded(len(src))
    a.a[:] = u8(src)
    dst, dst_off = Guarded(bound), Guarded(8 * (n + 1))
    if host:
        rc = L.emu_lz4f_batch_encode_host(a.ptr, len(src), off.ctypes.data, n, block_id, int(hc), flags, dst.ptr, bound, dst_off.ptr, C.byref(run))
        assert run.intact == 1 and (n == 0 or (run.reserves == 1 and run.moves == 1 and run.syncs >= 1)), "one staged image"
    else:
        scratch = Guarded(L.emu_lz4f_batch_encode_scratch_bytes(n, len(src), block_id))
        rc = L.emu_lz4f_batch_encode(a.ptr, len(src), off.ctypes.data, n, block_id, int(hc), flags, dst.ptr, bound, dst_off.ptr, scratch.ptr, scratch.n,
                                     C.byref(run))
        assert scratch.intact()
    assert rc == 0, run.error
    assert dst.intact() and dst_off.intact() and a.intact()
    assert run.shape_errors == 0, "the block encoder was not handed every block once, at its source position, with its length - 1 of room"
    got_off = dst_off.a.view(np.int64)
    assert list(got_off) == list(offsets_of(want)), "dst_off are the prefix sums of the frames' lengths"
    total = int(got_off[n])
    got = dst.a[:total].tobytes()
    assert (dst.a[total:] == GUARD).all(), "bytes past the last frame's end were written"
    for i, w in enumerate(want):
        assert got[got_off[i]:got_off[i + 1]] == w, (i, "not the frame of the item alone")
    return got, got_off.copy()


# ---- every fault of test_gpu_lz4f.test_every_outcome_once, as items ------------------------------------------------------------------
def outcome_items(oracle):
    """-> (good frame, its source, [(name, broken frame, expected error at slot 65536)]); the last two hold two faults each"""
    src = mixed(oracle)
    frame, rets, _ = ref.write_frame(oracle, src, 4, False, 7)
    at1 = 15 + 4 + 65536 + 4                                           # block 1's size field (block 0 is stored raw)
    assert rets[0] == 0 and rets[1] > 0
    wrong_size = bytearray(flip(frame, 6))
    wrong_size[14] = (ref.xxh32(bytes(wrong_size[4:14])) >> 8) & 0xFF
    faults = [
        ("short", b"abc", ref.BAD_MAGIC), ("magic", flip(frame, 1), ref.BAD_MAGIC), ("version", flip(frame, 4, 0x80), ref.BAD_HEADER),
        ("hc", flip(frame, 14), ref.HEADER_CHECKSUM), ("linked", ref.descriptor(4, 3, len(src), linked=True) + frame[15:], ref.UNSUPPORTED_LINKED),
        ("dict", ref.descriptor(4, 7, len(src), dict_id=5) + frame[15:], ref.UNSUPPORTED_DICT),
        ("slot", ref.write_frame(oracle, src[:70000], 6, False, 0)[0], ref.SLOT_TOO_SMALL),
        ("cut_field", frame[:at1 + 2], ref.TRUNCATED), ("cut_data", frame[:at1 + 100], ref.TRUNCATED), ("cut_end", frame[:-2], ref.TRUNCATED),
        ("block_size", frame[:at1] + ref.le32(65537) + frame[at1 + 4:], ref.BAD_BLOCK_SIZE),
        ("block_sum", flip(frame, at1 + 13, 0xFF), ref.BLOCK_CHECKSUM), ("content_size", bytes(wrong_size), ref.CONTENT_SIZE),
        ("content_sum", flip(frame, len(frame) - 1), ref.CONTENT_CHECKSUM),
        ("sum_and_content", flip(flip(frame, at1 + 13, 0xFF), len(frame) - 1), ref.BLOCK_CHECKSUM),
        ("sum_and_cut", flip(frame, at1 + 13, 0xFF)[:-2], ref.BLOCK_CHECKSUM),
    ]
    return frame, src, faults
