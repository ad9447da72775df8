"""CPU-only: the encode of LZ4 frames with a dictionary (lz4hip_lz4f_encode_dict_* and lz4hip_lz4f_batch_encode_dict_*: the dictionary
forms of lz4hip_framing.hpp's encode sequences) under the SIMT emulator, byte for byte against the twin tests/lz4f_dict_encode_ref.py in
guarded buffers.  The sequences, the head kernels and the pack are the library's own, and every block runs the real encoders:
encode_dict_prime_kernel and encode_dict_kernel<1> / <5>, or encode_fast_kernel for a call without a dictionary.  Every frame is then
decoded by the emulator's dictionary decode (tests/lz4f_cases.py, its DICT path in the framing library)."""
import ctypes as C

import numpy as np
import pytest

import lz4f_cases as cases
import lz4f_dict_encode_ref as twin
import lz4f_ref as ref
from emu_lib import E_ARGUMENT, Guarded
from lz4f_cases import PlacedDict, offsets_of
from lz4f_dict_encode_lib import FILL, EncRun, emu, encode_batch, encode_one, placed

SMALL = tuple(n for n in twin.SOURCE_LENGTHS if n <= 4096)


def check_decodes(frame, src, d, dict_id, block_id=4):
    """the emulator's decode of the framing library: with the right dictionary the source; with another ID a mismatch at the ID field;
    through the plain decode UNSUPPORTED_DICT when an ID was written"""
    slot, rows = ref.block_bytes(block_id), max(len(ref.cut(src, block_id)), 1)
    rec, out, _ = cases.run_frame(cases.DICT, frame, (), d, dict_id, slot, rows, 0, 3, len(src))
    assert rec["error"] == ref.OK and out.tobytes() == src
    if dict_id and d:
        sized = frame[4] & 0x08
        rec, _, _ = cases.run_frame(cases.DICT, frame, (), d, (dict_id + 1) & 0xFFFFFFFF or 1, slot, rows, 0, 3, len(src))
        assert rec["error"] == ref.DICT_ID_MISMATCH and rec["error_offset"] == (14 if sized else 6)
        rec, _, _ = cases.run_frame(cases.DICT_PLAIN, frame, (), b"", 0, slot, rows, 0, 3, len(src))
        assert rec["error"] == ref.UNSUPPORTED_DICT


def check_one(src, d, dict_id=0, block_id=4, flags=0, odd=0, host=False, wpg=1, grid=0, decode=True):
    want, rets = twin.write_frame_dict(src, d, dict_id, block_id, flags)
    got, run = encode_one(src, d, dict_id, block_id, flags, odd, host, wpg, grid)
    assert got == want, (len(got), len(want), rets)
    assert (run.plain_calls, run.dict_calls, run.primes, run.primes_before_dict) == ((0, 1, 1, 1) if src else (0, 0, 0, 0))
    if host:
        assert (run.dict_uploads, run.dict_bytes, run.dict_first_byte, run.uploads_before_dict) == (1, min(len(d), 65535), len(d) - min(len(d), 65535), 0)
    if decode:
        check_decodes(got, src, d, dict_id, block_id)
    return got


# ---- byte equality with the twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("n", twin.DICT_LENGTHS)
def test_small_sources_against_every_dictionary(n, odd):
    d = twin.dictionary(n)
    for k, size in enumerate(SMALL):
        check_one(twin.source(size, n), d, twin.DICT_IDS[(k + odd) % 3], odd=odd, host=bool((k + odd) & 1), wpg=1 if k & 2 else 5)


@pytest.mark.parametrize("size,n,odd,host", [(65536, 13, 1, False), (65537, 4097, 0, True), (65537, 70000, 1, False), (150000, 65535, 1, False),
                                             (150000, 4095, 0, True), (65536, 1, 0, True)])
def test_sources_of_several_blocks(size, n, odd, host):
    check_one(twin.source(size, n), twin.dictionary(n), 7, odd=odd, host=host, wpg=5 if host else 1)


def test_a_block_above_64_kib_against_a_dictionary():
    src, d = twin.source(twin.BIG, 70000), twin.dictionary(70000)
    frame = check_one(src, d, 0xFFFFFFFF, block_id=5, flags=ref.F_CONTENT_SIZE, odd=1)
    assert frame[5] == 0x50 and len(ref.cut(src, 5)) == 2


@pytest.mark.parametrize("flags", range(8))
def test_every_combination_of_the_flags(flags):
    d = twin.dictionary(4097)
    for size, dict_id, host in ((300, 7, False), (300, 0, True), (65537, 0xFFFFFFFF, False)):
        check_one(twin.source(size), d, dict_id, flags=flags, odd=flags & 1, host=host, grid=(0, 1, 3)[flags % 3])


@pytest.mark.parametrize("dict_id", twin.DICT_IDS)
def test_the_dictionary_id_in_the_descriptor(dict_id):
    d, src = twin.dictionary(13), twin.source(300, 13)
    for flags, head in ((0, 7), (ref.F_CONTENT_SIZE, 15)):
        frame = check_one(src, d, dict_id, flags=flags)
        assert (frame[4] & 1) == (1 if dict_id else 0)
        at = head - 1 + (4 if dict_id else 0)
        assert frame[at] == (ref.xxh32(frame[4:at]) >> 8) & 0xFF and (not dict_id or frame[at - 4:at] == ref.le32(dict_id))
        L = emu()
        assert L.emu_lz4f_dict_bound(300, 4, flags, 13, dict_id) == L.emu_lz4f_plain_bound(300, 4, flags) + (4 if dict_id else 0)
    assert check_one(b"", d, dict_id, flags=ref.F_CONTENT_SIZE)[4] & 0x08 == 0, "an empty source carries no content size"


# ---- the test that cannot pass without the feature ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_a_source_that_only_the_dictionary_compresses(host):
    d, src = twin.only_with_the_dictionary()
    want, rets = twin.write_frame_dict(src, d)
    assert rets == [10] and want[7:11] == ref.le32(10), "the twin: one block of 10 bytes, stored compressed"
    with_dict = check_one(src, d, host=host)
    without, run = encode_one(src, b"", host=host)
    assert run.primes == 0 and without[7:11] == ref.le32(200 | 0x80000000) and without[11:211] == src, "without a dictionary: stored raw"
    assert with_dict[:7] == without[:7] and with_dict[-4:] == without[-4:] == ref.le32(0)
    assert len(with_dict) == 7 + 4 + 10 + 4 and len(without) == 7 + 4 + 200 + 4


# ---- a batch -------------------------------------------------------------------------------------------------------------------------------
def mixed_items(n):
    return [twin.source(size, n) for size in twin.SOURCE_LENGTHS] + [b"", twin.noise(200)]


@pytest.mark.parametrize("n,odd,wpg,grid", [(4097, 1, 5, 0), (70000, 0, 1, 3), (13, 1, 5, 1)])
def test_a_mixed_batch_is_the_concatenation_of_the_one_frame_results(n, odd, wpg, grid):
    """one item of every source length, an empty one, one with decreasing offsets (it takes no bytes) and 200 random bytes (stored raw even with
    the dictionary)"""
    d, items = twin.dictionary(n), mixed_items(n)
    flags = ref.F_CONTENT_SIZE | ref.F_BLOCK_CHECKSUM
    src, off = b"".join(items), list(offsets_of(items))
    off = off[:4] + [off[4], off[3]] + off[4:]                            # a sixth item [off[4], off[3]): its offsets decrease
    spans = [src[a:b] if a <= b else None for a, b in zip(off[:-1], off[1:])]
    frames = [b"" if s is None else twin.write_frame_dict(s, d, 7, 4, flags)[0] for s in spans]
    assert twin.write_frame_dict(items[-1], d, 7, 4, flags)[1] == [0]
    ends, got, run = encode_batch(src, off, d, 7, 4, flags, odd=odd, wpg=wpg, grid=grid)
    assert list(ends) == list(offsets_of(frames)) and got == b"".join(frames)
    assert (run.plain_calls, run.dict_calls, run.primes, run.primes_before_dict) == (0, 1, 1, 1)
    for s, f in zip(spans, frames):
        if s is not None and len(s) <= 4096:
            assert encode_one(s, d, 7, 4, flags, odd=odd)[0] == f
            check_decodes(f, s, d, 7)


def test_the_host_batch():
    d, items = twin.dictionary(70000), mixed_items(70000)[:7] + [b"", twin.noise(200)]
    frames = [twin.write_frame_dict(s, d, 0xFFFFFFFF, 4, ref.F_CONTENT_CHECKSUM)[0] for s in items]
    ends, got, run = encode_batch(b"".join(items), offsets_of(items), d, 0xFFFFFFFF, 4, ref.F_CONTENT_CHECKSUM, odd=1, host=True, wpg=5)
    assert list(ends) == list(offsets_of(frames)) and got == b"".join(frames)
    assert (run.dict_uploads, run.dict_bytes, run.dict_first_byte, run.uploads_before_dict, run.primes, run.dict_calls) == (1, 65535, 70000 - 65535, 0, 1, 1)
    assert run.moves == 1, "one image"
    L = emu()
    run, dst, dst_off = EncRun(), Guarded(64, FILL), Guarded(16)
    bad = np.array([5, 3], np.int64)
    assert L.emu_lz4f_batch_encode_dict_host(items[4], 300, bad.ctypes.data, 1, d, len(d), 7, 4, 0, dst.ptr, 10000, dst_off.ptr, C.byref(run)) == E_ARGUMENT
    assert b"offsets decrease" in run.error and run.dict_uploads == 0 and run.reserves == 0 and (dst.a == FILL).all()


# ---- call-level checks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 65535, 70000])
def test_the_host_call_uploads_the_reachable_tail_once_and_primes_once(n):
    d = twin.dictionary(n)
    for size in (300, 65537):
        got, run = encode_one(twin.source(size, n), d, 7, odd=1, host=True)
        assert (run.dict_uploads, run.dict_bytes, run.dict_first_byte, run.uploads_before_dict) == (1, min(n, 65535), n - min(n, 65535), 0)
        assert (run.primes, run.dict_calls, run.plain_calls, run.moves) == (1, 1, 0, 1)
        assert got == twin.write_frame_dict(twin.source(size, n), d, 7)[0]


@pytest.mark.parametrize("flags", [0, 7])
def test_without_a_dictionary_the_call_is_the_plain_call(flags):
    L = emu()
    for size in (0, 13, 300, 65537):
        src = twin.source(size)
        plain, _ = encode_one(src, b"", block_id=4, flags=flags, plain=True)
        for host in (False, True):
            got, run = encode_one(src, b"", 99, flags=flags, host=host)
            assert got == plain and (run.primes, run.dict_calls, run.dict_uploads) == (0, 0, 0) and run.plain_calls == (1 if size else 0)
        assert L.emu_lz4f_dict_bound(size, 4, flags, 0, 99) == L.emu_lz4f_plain_bound(size, 4, flags)
        assert L.emu_lz4f_encode_dict_scratch_bytes(size, 4, 0) == L.emu_lz4f_plain_encode_scratch_bytes(size, 4)
        assert L.emu_lz4f_encode_dict_scratch_bytes(size, 4, 5) >= L.emu_lz4f_plain_encode_scratch_bytes(size, 4) + 16384 + 24
    items = mixed_items(4097)[:8] + [b""]
    src, off = b"".join(items), offsets_of(items)
    plain = encode_batch(src, off, b"", flags=flags, plain=True)
    for host in (False, True):
        ends, got, run = encode_batch(src, off, b"", 99, flags=flags, host=host)
        assert list(ends) == list(plain[0]) and got == plain[1] and (run.primes, run.dict_calls, run.dict_uploads, run.plain_calls) == (0, 0, 0, 1)
    n = len(items)
    assert L.emu_lz4f_batch_dict_bound(n, len(src), 4, flags, 0, 99) == L.emu_lz4f_plain_batch_bound(n, len(src), 4, flags)
    assert L.emu_lz4f_batch_encode_dict_scratch_bytes(n, len(src), 4, 0) == L.emu_lz4f_plain_batch_encode_scratch_bytes(n, len(src), 4)
    assert L.emu_lz4f_batch_dict_bound(n, len(src), 4, flags, 13, 7) == L.emu_lz4f_plain_batch_bound(n, len(src), 4, flags) + 4 * n
    assert L.emu_lz4f_batch_dict_bound(n, len(src), 4, flags, 13, 0) == L.emu_lz4f_plain_batch_bound(n, len(src), 4, flags)


def test_every_argument_error_leaves_the_output_untouched():
    L = emu()
    src, d = twin.source(300), twin.dictionary(13)
    a, pd = placed(src), PlacedDict(d, 1)
    bound, need = L.emu_lz4f_dict_bound(300, 4, 7, 13, 7), L.emu_lz4f_encode_dict_scratch_bytes(300, 4, 13)
    bbound, bneed = L.emu_lz4f_batch_dict_bound(1, 300, 4, 7, 13, 7), L.emu_lz4f_batch_encode_dict_scratch_bytes(1, 300, 4, 13)
    off = np.array([0, 300], np.int64)
    # (dict, dict_len, block id, flags, dst_cap short by, scratch short by, the text)
    errors = [(pd.ptr, -1, 4, 7, 0, 0, b"dict_len < 0"), (None, 13, 4, 7, 0, 0, b"dict is NULL"), (pd.ptr, 13, 4, 8, 0, 0, b"unknown flag"),
              (pd.ptr, 13, 3, 7, 0, 0, b"block_size_id"), (pd.ptr, 13, 8, 7, 0, 0, b"block_size_id"), (pd.ptr, 13, 4, 7, 1, 0, b"dst_cap <"),
              (pd.ptr, 13, 4, 7, 0, 1, b"scratch_bytes <")]
    for dict_ptr, dict_len, bid, flags, short_dst, short_scratch, text in errors:
        dst, out_len, dst_off, scratch = Guarded(bbound, FILL), Guarded(8, FILL), Guarded(16, FILL), Guarded(max(need, bneed), FILL)
        run = EncRun()
        assert L.emu_lz4f_encode_dict(a.ptr, 300, dict_ptr, dict_len, 7, bid, flags, dst.ptr, bound - short_dst, out_len.ptr, scratch.ptr, need - short_scratch,
                                      C.byref(run)) == E_ARGUMENT
        assert text in run.error, run.error
        assert L.emu_lz4f_batch_encode_dict(a.ptr, 300, off.ctypes.data, 1, dict_ptr, dict_len, 7, bid, flags, dst.ptr, bbound - short_dst, dst_off.ptr, scratch.ptr,
                                            bneed - short_scratch, C.byref(run)) == E_ARGUMENT
        assert text in run.error, run.error
        if not short_scratch:
            assert L.emu_lz4f_encode_dict_host(a.ptr, 300, dict_ptr, dict_len, 7, bid, flags, dst.ptr, bound - short_dst, out_len.ptr, C.byref(run)) == E_ARGUMENT
            assert (text in run.error or b"flags known" in run.error) and run.dict_uploads == 0 and run.reserves == 0, run.error
            assert L.emu_lz4f_batch_encode_dict_host(a.ptr, 300, off.ctypes.data, 1, dict_ptr, dict_len, 7, bid, flags, dst.ptr, bbound - short_dst, dst_off.ptr,
                                                     C.byref(run)) == E_ARGUMENT
            assert (text in run.error or b"flags known" in run.error) and run.dict_uploads == 0 and run.reserves == 0, run.error
        assert run.primes == 0 and run.dict_calls == 0 and run.plain_calls == 0
        for g in (dst, out_len, dst_off, scratch):
            assert (g.a == FILL).all() and g.intact()
    assert L.emu_lz4f_dict_bound(300, 4, 0, -1, 0) == E_ARGUMENT and L.emu_lz4f_dict_bound(300, 4, 8, 13, 0) == E_ARGUMENT
    assert L.emu_lz4f_dict_bound(300, 3, 0, 13, 0) == E_ARGUMENT and L.emu_lz4f_batch_dict_bound(1, 300, 4, 0, -1, 0) == E_ARGUMENT
