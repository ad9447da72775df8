"""CPU-only: the xxHash32 row kernel and the LZ4 frame path (lz4net_amd/csrc/lz4hip_lz4f.hpp and its host code in lz4hip_framing.hpp)
under the SIMT emulator (tests/simt/emu_lz4f.inc): the real kernels, the library's fronts, launch sequences and host-pointer calls, with
the block codec replaced by results and bytes computed here with the oracle.  The reference is the test-side twin tests/lz4f_ref.py: a
from-the-spec xxh32, a frame writer and a frame reader over the oracle's block codec."""
import ctypes as C
import functools
import mmap

import numpy as np
import pytest

import lz4f_ref as ref
from emu_lib import E_ARGUMENT, Guarded, P as _P, u8
from lz4f_cases import LENGTHS, PLAIN, FrameRun as EmuRun, check_frame, emu, emu_encode, flip, mixed, sample
from lz4net_amd._lib import Lz4fInfo

check_decode = functools.partial(check_frame, PLAIN, slot=0, max_blocks=8)   # the plain one-frame call, a table of 8 rows


# ---- xxHash32 -------------------------------------------------------------------------------------------------------------------
def run_rows(rows, lead=0, grid=0, seed=0):
    """rows of bytes laid end to end from byte `lead` of a guarded buffer, explicit offsets and lengths -> the kernel's sums"""
    total = lead + sum(len(r) for r in rows)
    buf = Guarded(total, 0)
    off, at = [], lead
    for r in rows:
        buf.a[at:at + len(r)] = u8(r)
        off.append(at)
        at += len(r)
    off = np.array(off, np.int64)
    ln = np.array([len(r) for r in rows], np.int32)
    sums = Guarded(4 * len(rows))
    assert emu().emu_xxh32_rows(buf.ptr, off.ctypes.data, 0, ln.ctypes.data, 0, seed, sums.ptr, len(rows), grid) == 0
    assert sums.intact() and buf.intact()
    return [int(x) for x in sums.a.view(np.uint32)]


def test_xxh32_known_answers():
    cases = [(b"", 0x02CC5D05), (b"abc", 0x32D153FF), (b"hello frame " * 40, 0x408E9E1A)]
    for data, want in cases:
        assert ref.xxh32(data) == want
        a = u8(data + b"\0")
        assert emu().emu_xxh32_serial(a.ctypes.data, len(data), 0) == want
    assert run_rows([d for d, _ in cases]) == [w for _, w in cases]
    assert run_rows([b"abc"], seed=7) == [ref.xxh32(b"abc", 7)]


@pytest.mark.parametrize("lead", [0, 1, 2, 3, 13, 14, 15, 16])
def test_xxh32_rows_every_length_at_every_offset(lead):
    rng = np.random.default_rng(lead)
    rows = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENGTHS]
    assert run_rows(rows, lead) == [ref.xxh32(r) for r in rows]


@pytest.mark.parametrize("n,grid", [(1, 0), (16, 0), (17, 0), (33, 0), (33, 1), (200, 3), (200, 0)])
def test_xxh32_row_counts(n, grid):
    """a full wavefront, one quad over, a partly filled third; more rows than a forced grid holds in one pass"""
    rng = np.random.default_rng(n)
    rows = [rng.integers(0, 256, int(rng.choice(LENGTHS)), dtype=np.uint8).tobytes() for _ in range(n)]
    assert run_rows(rows, 1, grid) == [ref.xxh32(r) for r in rows]


def test_xxh32_sixteen_rows_of_sixteen_lengths():
    lens = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 500, 511, 512, 513, 1025)
    rng = np.random.default_rng(16)
    rows = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    assert run_rows(rows, 3) == [ref.xxh32(r) for r in rows]
    # a row much longer than its neighbours: the quads that are done idle through many rounds
    rows[5] = rng.integers(0, 256, 64 * 8 * 5 + 77, dtype=np.uint8).tobytes()
    assert run_rows(rows, 3) == [ref.xxh32(r) for r in rows]


@pytest.mark.parametrize("n", [1, 15, 16, 63, 64, 65, 511, 512, 1025])
def test_xxh32_reads_nothing_outside_the_row(n):
    """the row ends (and, a second time, starts) at the edge of its mapping, next to a page nobody may touch"""
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [_P, C.c_size_t, C.c_int]
    page = mmap.PAGESIZE
    m = mmap.mmap(-1, 3 * page)
    anchor = C.c_char.from_buffer(m)
    base = C.addressof(anchor)
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    try:
        m[2 * page - n:2 * page] = data
        m[page:page + n] = data
        assert libc.mprotect(base + 2 * page, page, 0) == 0 and libc.mprotect(base, page, 0) == 0
        off = np.array([2 * page - n, page], np.int64)
        ln = np.array([n, n], np.int32)
        sums = Guarded(8)
        assert emu().emu_xxh32_rows(base, off.ctypes.data, 0, ln.ctypes.data, 0, 0, sums.ptr, 2, 0) == 0
        assert sums.intact() and [int(x) for x in sums.a.view(np.uint32)] == [ref.xxh32(data)] * 2
    finally:
        libc.mprotect(base, page, mmap.PROT_READ | mmap.PROT_WRITE)
        libc.mprotect(base + 2 * page, page, mmap.PROT_READ | mmap.PROT_WRITE)
        del anchor
        m.close()


def test_xxh32_strided_rows_and_arguments():
    a = np.random.default_rng(3).integers(0, 256, (5, 100), dtype=np.uint8)
    sums = np.zeros(5, np.uint32)
    assert emu().emu_xxh32_rows(a.ctypes.data, None, 100, None, 70, 0, sums.ctypes.data, 5, 0) == 0
    assert [int(s) for s in sums] == [ref.xxh32(a[i, :70].tobytes()) for i in range(5)]
    assert emu().emu_xxh32_rows(a.ctypes.data, None, 100, None, 70, 0, sums.ctypes.data, -1, 0) == E_ARGUMENT
    assert emu().emu_xxh32_rows(a.ctypes.data, None, 100, None, 70, 0, None, 5, 0) == E_ARGUMENT
    assert emu().emu_xxh32_rows(None, None, 100, None, 70, 0, sums.ctypes.data, 5, 0) == E_ARGUMENT
    assert emu().emu_xxh32_rows(None, None, 0, None, 0, 0, sums.ctypes.data, 0, 0) == 0


# ---- encode ---------------------------------------------------------------------------------------------------------------------
def test_known_descriptors(oracle):
    assert emu_encode(oracle, b"")[:7] == bytes.fromhex("04224D18604082")
    f = emu_encode(oracle, b"hello frame " * 40, flags=7)
    assert f[:15] == bytes.fromhex("04224D187C40E0010000000000001D") and f[-4:] == ref.le32(0x408E9E1A)
    # an empty source: a descriptor WITHOUT the content size (0 means "unknown" to the format library), the EndMark, the content checksum
    hc = (ref.xxh32(bytes([0x74, 0x40])) >> 8) & 0xFF
    assert emu_encode(oracle, b"", flags=7) == bytes.fromhex("04224D187440") + bytes([hc]) + bytes(4) + ref.le32(0x02CC5D05)


@pytest.mark.parametrize("flags", range(8))
@pytest.mark.parametrize("n", [0, 1, 65537])
def test_encode_every_flag_combination(oracle, flags, n):
    emu_encode(oracle, sample(oracle, 2, n), flags=flags)


@pytest.mark.parametrize("flags", [0, 7])
@pytest.mark.parametrize("n", [65535, 65536, 3 * 65536 + 5])
def test_encode_source_lengths(oracle, flags, n):
    emu_encode(oracle, sample(oracle, 3, n), flags=flags)


@pytest.mark.parametrize("block_id", [0, 4, 5, 6, 7])
def test_encode_block_size_ids_and_mixed_blocks(oracle, block_id):
    src = mixed(oracle)
    frame = emu_encode(oracle, src, block_id=block_id, flags=7)
    assert frame[5] == (block_id or 4) << 4
    if block_id in (0, 4):
        fields = [int.from_bytes(frame[at - 4:at], "little") >> 31 for at, *_ in ref.read_frame(oracle, frame)[3]]
        assert fields == [1, 0, 0, 0, 1], "raw and compressed blocks were to mix"


@pytest.mark.parametrize("grid", [1, 3])
def test_encode_forced_grids_hc_and_host(oracle, grid):
    src = mixed(oracle)
    emu_encode(oracle, src, flags=3, grid=grid)
    emu_encode(oracle, src[65536:65536 + 70000], hc=True, flags=1, grid=grid)
    emu_encode(oracle, src, flags=7, grid=grid, host=True)


def test_encode_arguments():
    L = emu()
    assert L.emu_lz4f_bound(10, 3, 0) == E_ARGUMENT and L.emu_lz4f_bound(10, 8, 0) == E_ARGUMENT and L.emu_lz4f_bound(10, 4, 8) == E_ARGUMENT
    assert L.emu_lz4f_bound(0, 0, 7) == 7 + 4 + 4 and L.emu_lz4f_bound(1, 4, 7) == 15 + 1 + 8 + 4 + 4
    a, out_len = np.zeros(64, np.uint8), np.zeros(1, np.int64)
    dst, scratch = np.zeros(256, np.uint8), np.zeros(1 << 16, np.uint8)
    run = EmuRun()
    ok = [a.ctypes.data, 10, 4, 0, 0, dst.ctypes.data, 256, out_len.ctypes.data, scratch.ctypes.data, scratch.size]
    for at, bad in ((1, -1), (2, 3), (3, 2), (4, 8), (5, None), (6, 10), (7, None), (8, None), (9, 16), (0, None)):
        args = list(ok)
        args[at] = bad
        assert L.emu_lz4f_encode(*args, C.byref(run)) == E_ARGUMENT, at


# ---- decode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", range(8))
def test_decode_every_flag_combination(oracle, flags):
    src = mixed(oracle)
    frame = ref.write_frame(oracle, src, 4, False, flags)[0]
    for verify in (3, 0):
        info, out = check_decode(oracle, frame, slot=65536, verify=verify)
        assert info["error"] == ref.OK and out == src and info["frame_bytes"] == len(frame)
    want_checks = ((ref.VERIFIED if flags & 1 else ref.ABSENT) | (ref.VERIFIED if flags & 2 else ref.ABSENT) << 2)
    assert check_decode(oracle, frame, slot=65536, verify=3)[0]["checks"] == want_checks


@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 65537, 3 * 65536 + 5])
@pytest.mark.parametrize("round_blocks", [0, 2])
def test_decode_source_lengths_and_rounds(oracle, n, round_blocks):
    src = sample(oracle, 2, n)
    frame = ref.write_frame(oracle, src, 4, False, 7)[0]
    info, out = check_decode(oracle, frame, max_blocks=5, round_blocks=round_blocks)
    assert info["error"] == ref.OK and out == src


@pytest.mark.parametrize("block_id", [4, 5, 6, 7])
def test_decode_block_size_ids(oracle, block_id):
    src = mixed(oracle)
    frame = ref.write_frame(oracle, src, block_id, block_id == 5, 3)[0]
    info, out = check_decode(oracle, frame, slot=ref.block_bytes(block_id), max_blocks=6, grid=(0, 1, 3, 0)[block_id - 4])
    assert info["error"] == ref.OK and out == src and info["block_max"] == ref.block_bytes(block_id)
    check_decode(oracle, frame, slot=0, max_blocks=6)
    if block_id > 4:
        info, out = check_decode(oracle, frame, slot=65536, max_blocks=6)
        assert info["error"] == ref.SLOT_TOO_SMALL and info["block_max"] == ref.block_bytes(block_id) and out == b""


def test_decode_clipping_and_table(oracle):
    src = mixed(oracle)
    frame = ref.write_frame(oracle, src, 4, False, 7)[0]
    for cap in (0, 2 * 65536, 2 * 65536 - 1, len(src) - 1):
        info, out = check_decode(oracle, frame, dst_cap=cap, round_blocks=2)
        assert out == src[:cap] and info["decoded_bytes"] == len(src) and info["error"] == ref.OK
        assert (info["checks"] >> 2) == ref.SKIPPED, "the content checksum runs only when everything was written"
    info, out = check_decode(oracle, frame, max_blocks=4)
    assert info["error"] == ref.TABLE_FULL and info["blocks"] == 5
    check_decode(oracle, frame, max_blocks=5)
    check_decode(oracle, frame, max_blocks=1, dst_cap=0)


def rehash(frame):
    """the descriptor's HC byte made right again"""
    flg = frame[4]
    dlen = 3 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
    b = bytearray(frame)
    b[4 + dlen - 1] = (ref.xxh32(frame[4:4 + dlen - 1]) >> 8) & 0xFF
    return bytes(b)


def test_decode_descriptor_outcomes(oracle):
    src = sample(oracle, 2, 70000)
    frame = ref.write_frame(oracle, src, 4, False, 7)[0]
    expect = lambda f, code, **kw: check_decode(oracle, f, **kw)[0]["error"] == code
    assert expect(b"", ref.BAD_MAGIC) and expect(frame[:3], ref.BAD_MAGIC) and expect(flip(frame, 0), ref.BAD_MAGIC)
    assert expect(frame[:4], ref.TRUNCATED) and expect(frame[:6], ref.TRUNCATED) and expect(frame[:14], ref.TRUNCATED)
    # each header bit wrong in turn, HC left as it was and HC made right
    for at, bit in [(4, 1 << b) for b in range(8)] + [(5, 1 << b) for b in range(8)]:
        info = check_decode(oracle, flip(frame, at, bit))[0]
        assert info["error"] != ref.OK, (at, bit)
        fixed = rehash(flip(frame, at, bit))
        want = ref.read_frame(oracle, fixed)[0]["error"]
        assert check_decode(oracle, fixed)[0]["error"] == want
        if (at, bit) in ((4, 0x80), (4, 0x40), (4, 0x02), (5, 0x80), (5, 0x01), (5, 0x02), (5, 0x04), (5, 0x08), (5, 0x40)):
            assert want == ref.BAD_HEADER, (at, bit)
    assert expect(flip(frame, 14), ref.HEADER_CHECKSUM)
    assert expect(flip(frame, 8), ref.HEADER_CHECKSUM)
    assert expect(rehash(flip(frame, 5, 0x70)), ref.BAD_HEADER)            # block size id 3
    linked = ref.descriptor(4, 3, len(src), linked=True) + frame[15:]
    assert linked[4] == 0x54 and expect(linked, ref.UNSUPPORTED_LINKED)
    assert ref.descriptor(4, 7, 480, linked=True)[4] == 0x5C
    with_dict = ref.descriptor(4, 7, len(src), dict_id=77) + frame[15:]
    assert expect(with_dict, ref.UNSUPPORTED_DICT)
    big = ref.write_frame(oracle, src, 6, False, 0)[0]
    assert expect(big, ref.SLOT_TOO_SMALL, slot=262144) and expect(big, ref.OK, slot=1048576)


def test_decode_block_outcomes(oracle):
    src = mixed(oracle)
    for flags in (7, 6):
        frame, rets, datas = ref.write_frame(oracle, src, 4, False, flags)
        sums = 4 if flags & 1 else 0
        at = [15]
        for r, d in zip(rets, datas):
            at.append(at[-1] + 4 + (r or 65536 if len(at) < 5 else r or 5) + sums)
        assert frame[at[5]:at[5] + 4] == bytes(4), "the EndMark"
        expect = lambda f, code, **kw: check_decode(oracle, f, **kw)[0]
        # a size field above the maximum -- tested before the truncation rule
        too_big = frame[:at[2]] + ref.le32(65537) + frame[at[2] + 4:]
        info = expect(too_big, 0)
        assert info["error"] == ref.BAD_BLOCK_SIZE and info["error_offset"] == at[2] and info["blocks"] == 2
        assert expect(frame[:at[2]] + ref.le32(0x7FFFFFFF), 0)["error"] == ref.BAD_BLOCK_SIZE
        # truncation inside a size field, inside data, inside a block checksum, before the EndMark, inside the content checksum
        for cut, off in ((at[1] + 2, at[1]), (at[1] + 100, at[1]), (at[2] - 2, at[1]), (at[5], at[5]), (len(frame) - 1, len(frame) - 4)):
            info = expect(frame[:cut], 0)
            assert info["error"] == ref.TRUNCATED and info["error_offset"] == off, (cut, info)
        # a flipped payload byte: of a compressed block, of a raw block
        info = expect(flip(frame, at[1] + 4 + 9, 0xFF), 0)
        assert info["error"] == (ref.BLOCK_CHECKSUM if sums else ref.CORRUPT_BLOCK) and info["error_offset"] == at[1] and info["good_bytes"] == 65536
        assert info["decoded_bytes"] == len(src) - 65536, "a bad block takes 0 bytes and its neighbours pack around it"
        info = expect(flip(frame, at[0] + 4 + 9), 0)
        assert info["error"] == (ref.BLOCK_CHECKSUM if sums else ref.CONTENT_CHECKSUM)
        # ... and unverified
        info = expect(flip(frame, at[1] + 4 + 9, 0xFF), 0, verify=0)
        assert info["error"] == ref.CORRUPT_BLOCK
        assert expect(flip(frame, at[0] + 4 + 9), 0, verify=0)["error"] == ref.OK
        assert expect(flip(frame, at[0] + 4 + 9), 0, verify=1)["error"] == (ref.BLOCK_CHECKSUM if sums else ref.OK)
        # a wrong content size, a wrong content checksum
        wrong = rehash(flip(frame, 6))
        assert expect(wrong, 0)["error"] == ref.CONTENT_SIZE
        assert expect(flip(frame, len(frame) - 1), 0)["error"] == ref.CONTENT_CHECKSUM
        assert expect(flip(frame, len(frame) - 1), 0, verify=1)["error"] == ref.OK
        # precedence: the lowest bad block over a later one and over the walk's error; a full table over everything; the content size
        # over the content checksum
        two = flip(flip(frame, at[1] + 4 + 9, 0xFF), at[3] + 4 + 9, 0xFF)
        info = expect(two, 0, round_blocks=2)
        assert info["error_offset"] == at[1] and (not sums or info["decoded_bytes"] == len(src) - 2 * 65536)
        info = expect(two[:at[4] + 2], 0)
        assert info["error"] != ref.TRUNCATED and info["error_offset"] == at[1]
        assert expect(two[:at[4] + 2], 0, max_blocks=3)["error"] == ref.TABLE_FULL
        assert expect(flip(wrong, len(frame) - 1), 0)["error"] == ref.CONTENT_SIZE
    # a block that decodes to more than the frame's own maximum is a bad block even when it fits the slot
    long_block = oracle.compress(np.zeros(65537, np.uint8))
    frame = ref.descriptor(4, 0, 0) + ref.le32(len(long_block)) + bytes(long_block) + bytes(4)
    info, out = check_decode(oracle, frame, slot=262144)
    assert info["error"] == ref.CORRUPT_BLOCK and out == b""


def test_decode_skippable_and_appended_frames(oracle):
    src = sample(oracle, 3, 70000)
    frame = ref.write_frame(oracle, src, 4, False, 7)[0]
    skip = ref.skippable(b"user data", 3)
    info, out = check_decode(oracle, skip + frame)
    assert info["kind"] == 1 and info["frame_bytes"] == len(skip) and info["error"] == ref.OK and out == b""
    assert check_decode(oracle, skip[:6])[0]["error"] == ref.TRUNCATED and check_decode(oracle, skip[:-1])[0]["error"] == ref.TRUNCATED
    info, out = check_decode(oracle, frame + frame[:40])
    assert info["frame_bytes"] == len(frame) and out == src and info["error"] == ref.OK


def test_decode_arguments_and_host_call(oracle):
    L = emu()
    src = mixed(oracle)
    frame = ref.write_frame(oracle, src, 4, False, 7)[0]
    assert L.emu_lz4f_decode_scratch_bytes(65535, 4, 0) == E_ARGUMENT and L.emu_lz4f_decode_scratch_bytes(65536, 0, 0) == E_ARGUMENT
    a, dst, scratch, info, run = u8(frame), np.zeros(64, np.uint8), np.zeros(1 << 20, np.uint8), Lz4fInfo(), EmuRun()
    ok = [a.ctypes.data, a.size, 65536, 4, 0, 3, scratch.ctypes.data, scratch.size, dst.ctypes.data, 64, C.byref(info)]
    for at, bad in ((0, None), (1, -1), (2, 1000), (3, 0), (4, -1), (5, 4), (6, None), (7, 100), (8, None), (9, -1), (10, None)):
        args = list(ok)
        args[at] = bad
        assert L.emu_lz4f_decode(*args, C.byref(run)) == E_ARGUMENT, at
    # the host-pointer call: a size query, then the decode; the stand-in codec is keyed by table row
    _, _, _, rows = ref.read_frame(oracle, frame)
    n = len(frame) // 65536 + 64
    dec_results, dec_len, dec_at, blob = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), b""
    for k, (at, size, raw, badsum, res, data) in enumerate(rows):
        dec_results[k], dec_len[k], dec_at[k] = res, 0 if raw else size, len(blob)
        blob += data
    dec_bytes = u8(blob)
    run = EmuRun(dec_results=dec_results.ctypes.data, dec_len=dec_len.ctypes.data, dec_at=dec_at.ctypes.data, dec_bytes=dec_bytes.ctypes.data, dec_rows=n)
    assert L.emu_lz4f_decode_host(a.ctypes.data, a.size, 3, None, 0, C.byref(info), C.byref(run)) == E_ARGUMENT
    assert info.decoded_bytes == len(src) and run.intact == 1
    out = Guarded(len(src))
    assert L.emu_lz4f_decode_host(a.ctypes.data, a.size, 3, out.ptr, len(src), C.byref(info), C.byref(run)) == 0, run.error
    assert out.a.tobytes() == src and out.intact() and run.intact == 1 and run.shape_errors == 0 and info.checks == 5
    bad = u8(flip(frame, len(frame) - 1))
    assert L.emu_lz4f_decode_host(bad.ctypes.data, bad.size, 3, out.ptr, len(src), C.byref(info), C.byref(run)) == ref.CONTENT_CHECKSUM
