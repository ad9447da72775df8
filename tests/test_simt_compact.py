"""CPU-only: the compact decode of a block batch (lz4net_amd/csrc/lz4hip_compact.hpp and its host code in lz4hip_framing.hpp and
lz4hip_hostbatch.hpp) and the legacy frame's one-call decode on top of it, under the SIMT emulator (tests/simt/emu_compact.inc): the
real kernels, the library's fronts, launch sequences and host-pointer call, with the block decoder replaced by a stand-in keyed by
global block index that writes, into the slot and never past the block's limit, what the oracle's LZ4_uncompress_unknownOutputSize
gives for the block at that limit.  Every case runs with the library's grids and with grids forced to 1 and 3 workgroups."""
import ctypes as C
import functools

import numpy as np
import pytest

import emu_lib
import frame_cases as fc
from block_cases import SMALL, BlockCase, check_sentinels, expect_info, lengths_of, rounds_of, sentinels
from emu_lib import E_ARGUMENT, GRIDS, Guarded, I32 as _I32, I64 as _I64, P as _P, u8
from lz4net_amd._lib import Batch, CompactInfo, FrameInfo

SLOT = 70000                                    # the decoded size of the longest block: the slot width of most cases


class CompactEmuRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("results", _P), ("limits", _P), ("at", _P), ("bytes", _P), ("src", _P), ("src_at", _P), ("src_len", _P), ("n", _I64),
                ("grid", _I32), ("pad", _I32), ("calls", _I64), ("max_rows", _I64), ("shape_errors", _I64), ("counters", emu_lib.EmuCounters)]


@functools.lru_cache(maxsize=None)
def emu():
    L = emu_lib.framing()
    L.emu_compact_sizeof.restype = _I64
    assert L.emu_compact_sizeof(0) == L.emu_compact_sizeof(3) == C.sizeof(CompactInfo) and L.emu_compact_sizeof(1) == C.sizeof(CompactEmuRun)
    assert L.emu_compact_sizeof(2) == C.sizeof(Batch) and L.emu_compact_sizeof(4) == C.sizeof(fc.FrameTables) and L.emu_compact_sizeof(5) == C.sizeof(FrameInfo)
    L.emu_compact_scratch_bytes.argtypes, L.emu_compact_scratch_bytes.restype = [_I64, _I32, _I64], _I64
    L.emu_frame_compact_scratch_bytes.argtypes, L.emu_frame_compact_scratch_bytes.restype = [_I32, _I64, _I64], _I64
    L.emu_frame_compact_tables.argtypes, L.emu_frame_compact_tables.restype = [_P, _I32, _I64, _I64, _P], None
    L.emu_decode_compact.argtypes = [_P, _I64, _P, _I64, _P, _P, _P, _I64, _P, _P]
    L.emu_decode_compact_host.argtypes = [_P, _I64, _P, _I64, _P, _P, _P, _I64, _P]
    L.emu_frame_decode_compact.argtypes = [_P, _I64, _I32, _I64, _I64, _P, _I64, _P, _I64, _P, _P]
    return L


# ---- the blocks and what the reference's decoder gives for them ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def the_oracle():
    from oracle.oracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def pool():
    """{decoded length: [compressed block, ...]}: a few distinct blocks per length (length 0: the empty block and the one-byte block),
    and under "bad" blocks the decoder fails on: corrupt at the start, and cut short"""
    oracle = the_oracle()
    out = {}
    for length in SMALL + (4096, 65536, 70000):
        rows = []
        for dist in ((2, 3) if length >= 65536 else (1, 2, 3)):
            raw = oracle.gen(dist, 11, 5 + length % 7, 1, length=max(length, 1))[0, :length].copy()
            rows.append(oracle.compress(raw, hc=dist == 3))
        out[length] = rows
    out[0][0] = np.zeros(0, np.uint8)
    good = out[4096][1]
    out["bad"] = [np.concatenate([np.full(3, 0xFF, np.uint8), good[3:]]), good[:good.size - 7].copy(), out[65536][0][:300].copy()]
    return out


@functools.lru_cache(maxsize=None)
def decoded(key, which, limit):
    """(result, bytes) of LZ4_uncompress_unknownOutputSize on pool()[key][which] at `limit`"""
    comp = pool()[key][which]
    r, out = the_oracle().uncompress_unknown_raw(comp, comp.size, limit)
    return int(r), out[:max(r, 0)].copy()


class Case(BlockCase):
    """n blocks in one of the two source layouts.  bad: indices that hold a block the decoder fails on; neg: indices whose length is
    handed over negative; slot: dst_cap_all"""

    def __init__(self, n, layout, lens=None, bad=(), neg=(), slot=SLOT, pick=None):
        self.slot = slot
        lens = lengths_of(n) if lens is None else list(lens)
        self.keys = [(length, (i if pick is None else pick) % len(pool()[length])) for i, length in enumerate(lens)]
        for j, i in enumerate(sorted(bad)):
            self.keys[i] = ("bad", j % 3)
        self.comp = [pool()[key][which] for key, which in self.keys]
        self.neg = set(neg)
        src_len = [-(c.size + 1) if i in self.neg else c.size for i, c in enumerate(self.comp)]
        self.lay_out(self.comp, src_len, layout, src_len_all=0, dst_cap_all=slot)
        self.seen_len = np.maximum(self.src_len, 0)                   # what the decoder must be handed
        self.src_at = np.concatenate(([0], np.cumsum([c.size for c in self.comp], dtype=np.int64))).astype(np.int64)
        self.flat = np.concatenate(self.comp + [np.zeros(1, np.uint8)])

    def expect(self, caps=None):
        """(results, lengths, offsets, bytes per block, limits) as the contract states them"""
        res, outs, limits = np.zeros(self.n, np.int32), [], np.zeros(self.n + 1, np.int32)
        for i in range(self.n):
            limits[i] = self.slot if caps is None else max(min(int(caps[i]), self.slot), 0)
            if i in self.neg:
                res[i], out = E_ARGUMENT, np.zeros(0, np.uint8)
            else:
                res[i], out = decoded(self.keys[i][0], self.keys[i][1], int(limits[i]))
            outs.append(out)
        lens = np.maximum(res, 0)
        offs = np.concatenate(([0], np.cumsum(lens, dtype=np.int64))).astype(np.int64)
        return res, lens, offs, outs, limits

    def run_record(self, grid, caps=None):
        res, lens, offs, outs, limits = self.expect(caps)
        r = CompactEmuRun()
        # (a block whose length is negative reaches the decoder as an empty block: 0)
        self.keep = (np.append(np.where(res == E_ARGUMENT, 0, res), 0).astype(np.int32), limits, np.append(offs, 0).astype(np.int64),
                     np.concatenate(outs + [np.zeros(1, np.uint8)]))
        r.results, r.limits, r.at, r.bytes = (a.ctypes.data for a in self.keep)
        r.src, r.src_at, r.src_len, r.n, r.grid = self.flat.ctypes.data, self.src_at.ctypes.data, self.seen_len.ctypes.data, self.n, grid
        return r


def info_tuple(i):
    assert i.reserved == 0
    return (i.blocks, i.decoded_bytes, i.written_blocks, i.first_failed, i.error)


def check_outputs(case, caps, dst, dst_cap, dst_off, dlen, result, info, want_result, want_len):
    n = case.n
    res_want, len_want, off_want, outs, _ = case.expect(caps)
    total = int(off_want[n])
    check_sentinels(n, dst_off, dlen, result)
    assert (dst_off[1:n + 2] == off_want).all(), "the offsets are complete whatever dst_cap is"
    assert not want_len or (dlen[1:n + 1] == len_want).all()
    assert not want_result or (result[1:n + 1] == res_want).all()
    want = expect_info(n, res_want, off_want, dst_cap, failed=lambda r: r < 0)
    assert info_tuple(info) == want
    w = want[2]
    plain = np.concatenate([outs[i] for i in range(w)] + [np.zeros(0, np.uint8)])
    assert plain.size == off_want[w] and (dst.a[:off_want[w]] == plain).all(), "the written prefix is not the oracle's bytes"
    if w == n:
        assert (dst.a[total:] == 0xA7).all(), "bytes past the total were written"
    return want


def run(case, k=0, grid=0, dst_cap=None, caps=None, want_result=True, want_len=True, scratch_short=0):
    """decode_compact under the emulator -> (rc, dst, info, run record); checks everything the contract promises on the way"""
    n = case.n
    total = int(case.expect(caps)[2][n])
    dst_cap = total if dst_cap is None else dst_cap
    dst = Guarded(dst_cap, fill=0xA7)
    scratch = Guarded(emu().emu_compact_scratch_bytes(n, case.slot, k) - scratch_short)
    dst_off, dlen, result, info = sentinels(n, CompactInfo)
    b = case.batch(caps, result[1:] if want_result else None)
    r = case.run_record(grid, caps)
    rc = emu().emu_decode_compact(C.addressof(b), k, dst.ptr, dst_cap, dst_off.ctypes.data + 8, dlen.ctypes.data + 4 if want_len else None,
                                  scratch.ptr, scratch.n, C.addressof(info), C.addressof(r))
    assert dst.intact() and scratch.intact(), "a byte outside dst (at or past dst_cap) or outside the scratch was written"
    if rc != 0:
        return rc, dst, info, r
    assert r.shape_errors == 0, "the decoder was handed a row, a length, a limit or a descriptor that is not the batch's"
    assert (r.calls, r.max_rows) == rounds_of(n, k)
    check_outputs(case, caps, dst, dst_cap, dst_off, dlen, result, info, want_result, want_len)
    return rc, dst, info, r


# ---- parity and shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("layout", ["strided", "offsets"])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1000])
def test_parity_every_round_size(n, layout, grid):
    case = Case(n, layout)
    for k in sorted({0, 1, 64, 256, max(n - 1, 0), n, n + 1}):
        assert run(case, k, grid)[0] == 0


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", [0, 1, 64, 256, 4096, 4097, 4098])
def test_parity_across_the_scan_tile(k, grid):
    assert emu().emu_compact_sizeof(100) == 4096
    assert run(Case(4097, "offsets" if k % 2 else "strided"), k, grid)[0] == 0


@pytest.mark.parametrize("grid", GRIDS)
def test_optional_outputs(grid):
    case = Case(257, "offsets")
    assert run(case, 64, grid, want_result=False, want_len=False)[0] == 0
    assert run(case, 0, grid, want_result=False)[0] == 0


def test_uniform_length_batch():
    comp = pool()[4096][0]
    case = Case(70, "strided", lens=[4096] * 70, pick=0)
    res_want, len_want, off_want, outs, _ = case.expect()
    dst = Guarded(int(off_want[70]))
    scratch = Guarded(emu().emu_compact_scratch_bytes(70, SLOT, 64))
    dst_off = np.zeros(71, np.int64)
    info = CompactInfo()
    b = case.batch(uniform_len=comp.size)
    r = case.run_record(0)
    assert emu().emu_decode_compact(C.addressof(b), 64, dst.ptr, dst.n, dst_off.ctypes.data, None, scratch.ptr, scratch.n, C.addressof(info), C.addressof(r)) == 0
    assert r.shape_errors == 0 and (dst_off == off_want).all() and dst.intact() and scratch.intact()
    assert bytes(dst.a) == b"".join(bytes(o) for o in outs) and info_tuple(info) == (70, 70 * 4096, 70, -1, 0)


# ---- blocks that fail -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", [0, 64, 1])
def test_corrupt_blocks_take_no_bytes(k, grid):
    """corrupt blocks at index 0, at n - 1 and on both sides of the round boundaries of k = 64"""
    bad = (0, 63, 64, 127, 128, 256)
    case = Case(257, "strided", bad=bad)
    rc, dst, info, r = run(case, k, grid)
    res = case.expect()[0]
    assert rc == 0 and [i for i in range(257) if res[i] < 0] == list(bad)
    assert (info.first_failed, info.error) == (0, int(res[0])) and info.error < 0 and info.error != E_ARGUMENT
    case = Case(257, "offsets", bad=(64, 256))
    rc, dst, info, r = run(case, k, grid)
    assert (info.first_failed, info.error) == (64, int(case.expect()[0][64]))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", [0, 64])
def test_a_block_that_needs_more_than_its_limit_fails(k, grid):
    # through dst_cap_all: the slot width is 65 536 and block 2 decodes to 70 000
    case = Case(130, "strided", slot=65536)
    rc, dst, info, r = run(case, k, grid)
    res = case.expect()[0]
    assert rc == 0 and [i for i in range(130) if res[i] < 0] == [2] and info.first_failed == 2 and info.error == res[2]
    # through a per-block dst_cap: one byte short, exactly enough, above the slot width (the slot width binds), negative (no room at all)
    case = Case(130, "offsets")
    sizes = case.expect()[1]
    caps = np.full(131, SLOT + 1000, np.int32)
    for i in (1, 64, 65, 129):
        caps[i] = sizes[i] - 1
    caps[66] = sizes[66]
    caps[3] = -5
    assert sizes[3] > 0 and sizes[1] > 0 and sizes[129] > 0
    rc, dst, info, r = run(case, k, grid, caps=caps)
    res = case.expect(caps)[0]
    assert rc == 0 and [i for i in range(130) if res[i] < 0] == [1, 3, 64, 65, 129] and res[66] == sizes[66]
    assert (info.first_failed, info.error) == (1, int(res[1]))
    # an empty block succeeds with 0 also where it has no room
    case = Case(5, "strided", lens=[0, 0, 12, 0, 0])
    caps = np.array([0, -3, 12, 0, 1, 0], np.int32)
    rc, dst, info, r = run(case, k, grid, caps=caps)
    assert rc == 0 and list(case.expect(caps)[0]) == [0, 0, 12, 0, 0] and info.first_failed == -1


@pytest.mark.parametrize("grid", GRIDS)
def test_negative_length_is_an_argument_result(grid):
    case = Case(130, "offsets", neg=(70, 129))
    for k in (0, 64):
        rc, dst, info, r = run(case, k, grid)
        assert rc == 0 and (info.first_failed, info.error) == (70, E_ARGUMENT)
    case = Case(130, "strided", bad=(5,), neg=(70,))
    rc, dst, info, r = run(case, 64, grid)
    assert info.first_failed == 5 and info.error not in (0, E_ARGUMENT)


# ---- dst_cap clipping -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", [0, 64])
def test_dst_cap_clips_to_a_prefix(k, grid):
    case = Case(257, "strided", bad=(100,))
    off = case.expect()[2]
    total = int(off[257])
    caps = {0, 1, total - 1, total, total + 100}
    for blk in (1, 3, 63, 64, 65, 128, 200, 256):              # 64, 128 and 256 are round boundaries for k = 64
        caps |= {int(off[blk]) - 1, int(off[blk]), int(off[blk]) + 1}
    for dst_cap in sorted(c for c in caps if c >= 0):
        assert run(case, k, grid, dst_cap=dst_cap)[0] == 0


def test_size_query_needs_no_dst():
    case = Case(130, "offsets")
    res_want, len_want, off_want, outs, _ = case.expect()
    scratch = Guarded(emu().emu_compact_scratch_bytes(130, SLOT, 64))
    dst_off = np.zeros(131, np.int64)
    info = CompactInfo()
    b = case.batch()
    r = case.run_record(0)
    assert emu().emu_decode_compact(C.addressof(b), 64, None, 0, dst_off.ctypes.data, None, scratch.ptr, scratch.n, C.addressof(info), C.addressof(r)) == 0
    assert (dst_off == off_want).all() and info.decoded_bytes == off_want[130] and info.written_blocks == 0 and scratch.intact()
    assert r.shape_errors == 0


# ---- scratch and argument checks ------------------------------------------------------------------------------------------------------
def test_scratch_does_not_grow_past_a_round():
    f = emu().emu_compact_scratch_bytes
    assert f(0, SLOT, 0) == 0 and f(0, SLOT, 64) == 0                # 0 for an empty batch
    for k in (1, 64, 1000, 16384):
        assert len({f(n, SLOT, k) for n in (k, k + 1, 2 * k, 10 * k + 3, 1 << 22)}) == 1       # constant for every n >= K > 0
        sizes = [f(n, SLOT, k) for n in range(1, 2 * k + 2, max(k // 16, 1))]
        assert sizes == sorted(sizes) and sizes[0] > 0               # non-decreasing in n
    whole = [f(n, SLOT, 0) for n in (1, 2, 64, 65, 4096, 4097, 100000)]
    assert whole == sorted(whole)
    # the ring (a slot rounded up to 16) and three int32 tables per block of a round, the scan's tile sums, the state block, and up to
    # 256 bytes of rounding per piece
    assert f(1 << 22, SLOT, 16384) < (16384 * (SLOT + 16 + 12) + 8 * 5 + 256 * 6 + 256)
    assert f(5, 0, 0) == E_ARGUMENT and f(5, SLOT, -1) == E_ARGUMENT


def untouched(i):
    return (i.blocks, i.decoded_bytes, i.written_blocks, i.first_failed, i.error, i.reserved) == (-7,) * 6


def test_one_byte_less_scratch_is_refused():
    for k in (0, 64):
        rc, dst, info, r = run(Case(130, "strided"), k, scratch_short=1)
        assert rc == E_ARGUMENT and b"scratch_bytes" in r.error and r.calls == 0
        assert untouched(info) and (dst.a == 0xA7).all()


def test_argument_checks():
    """each check, without a device: the front refuses before anything is launched"""
    case = Case(3, "strided")
    scratch = Guarded(emu().emu_compact_scratch_bytes(3, SLOT, 0))
    dst = Guarded(1 << 18)
    dst_off = np.zeros(4, np.int64)
    info = CompactInfo()

    def call(b, k=0, dst_ptr=dst.ptr, dst_cap=dst.n, off=dst_off.ctypes.data, scratch_ptr=scratch.ptr, scratch_n=scratch.n, host=False):
        r = case.run_record(0)
        if host:
            rc = emu().emu_decode_compact_host(None if b is None else C.addressof(b), k, dst_ptr, dst_cap, off, None, C.addressof(info), -1, C.addressof(r))
            assert r.reserves == 0 or rc == 0
        else:
            rc = emu().emu_decode_compact(None if b is None else C.addressof(b), k, dst_ptr, dst_cap, off, None, scratch_ptr, scratch_n,
                                          C.addressof(info), C.addressof(r))
        assert r.calls == 0 or rc == 0
        return rc

    for host in (False, True):
        assert call(case.batch(), host=host) == 0
        assert call(None, host=host) == E_ARGUMENT
        for field, value in (("n_blocks", -1), ("dst_cap_all", 0), ("dst_cap_all", -4), ("src", None)):
            b = case.batch()
            setattr(b, field, value)
            assert call(b, host=host) == E_ARGUMENT, field
        assert call(case.batch(), k=-1, host=host) == E_ARGUMENT
        assert call(case.batch(), dst_cap=-1, host=host) == E_ARGUMENT
        assert call(case.batch(), off=None, host=host) == E_ARGUMENT
        assert call(case.batch(), dst_ptr=None, host=host) == E_ARGUMENT
        assert call(case.batch(uniform_len=-3), host=host) == E_ARGUMENT
        b = case.batch()
        b.n_blocks = 1 << 31                                       # one round of 2^31 blocks
        assert call(b, scratch_n=1 << 62, host=host) == E_ARGUMENT
    assert call(case.batch(), scratch_ptr=None) == E_ARGUMENT
    assert call(case.batch(), scratch_n=scratch.n - 1) == E_ARGUMENT
    assert dst.intact() and scratch.intact()


def test_empty_batch():
    for k in (0, 64):
        b = Batch(dst_cap_all=SLOT)
        dst_off = np.full(3, -77, np.int64)
        info = CompactInfo(-7, -7, -7, -7, -7, -7)
        r = CompactEmuRun()
        assert emu().emu_decode_compact(C.addressof(b), k, None, 0, dst_off.ctypes.data + 8, None, None, 0, C.addressof(info), C.addressof(r)) == 0
        assert list(dst_off) == [-77, 0, -77] and info_tuple(info) == (0, 0, 0, -1, 0) and r.calls == 0


# ---- the host-pointer call ------------------------------------------------------------------------------------------------------------
def run_host(case, k=0, grid=0, dst_cap=None, caps=None, want_result=True, want_len=True, pool_floor=-1):
    n = case.n
    total = int(case.expect(caps)[2][n])
    dst_cap = total if dst_cap is None else dst_cap
    dst = Guarded(dst_cap, fill=0xA7)
    dst_off, dlen, result, info = sentinels(n, CompactInfo)
    b = case.batch(caps, result[1:] if want_result else None)
    r = case.run_record(grid, caps)
    rc = emu().emu_decode_compact_host(C.addressof(b), k, dst.ptr, dst_cap, dst_off.ctypes.data + 8, dlen.ctypes.data + 4 if want_len else None,
                                       C.addressof(info), pool_floor, C.addressof(r))
    assert rc == 0, r.error
    assert dst.intact() and r.intact == 1 and r.shape_errors == 0
    check_outputs(case, caps, dst, dst_cap, dst_off, dlen, result, info, want_result, want_len)
    if n > 0:
        # the rows, their offsets and lengths (and the limits where there are any) go up once; the info comes back first, then the
        # per-block arrays, then ONE download of the payload, of min(decoded_bytes, dst_cap) bytes
        payload = min(total, dst_cap)
        assert r.reserves == 1 and r.moves == 1 and r.syncs == 2
        assert r.uploads == 3 + int(caps is not None)
        assert r.downloads == 2 + int(want_result) + int(want_len) + int(payload > 0)
        assert payload == 0 or r.last_download == payload
    return r


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("layout", ["strided", "offsets"])
def test_host_call_parity(layout, grid):
    case = Case(257, layout, bad=(64,))
    for k in (0, 64):
        run_host(case, k, grid)
    run_host(case, 64, grid, want_result=False, want_len=False, pool_floor=0)      # (the rows gathered on the row pool)
    run_host(Case(0, layout), 0, grid)
    # info is optional
    want_off, outs = case.expect()[2:4]
    dst, dst_off = Guarded(int(want_off[257])), np.zeros(258, np.int64)
    b, r = case.batch(), case.run_record(grid)
    assert emu().emu_decode_compact_host(C.addressof(b), 64, dst.ptr, dst.n, dst_off.ctypes.data, None, None, -1, C.addressof(r)) == 0
    assert (dst_off == want_off).all() and dst.intact() and bytes(dst.a) == b"".join(bytes(o) for o in outs)


def test_host_call_limits_clipping_and_negative_lengths():
    case = Case(257, "strided")
    off = case.expect()[2]
    for dst_cap in (0, 1, int(off[64]), int(off[64]) + 1, int(off[257]) - 1, int(off[257]) + 100000):
        run_host(case, 64, 0, dst_cap=dst_cap)
    caps = np.full(258, SLOT, np.int32)
    caps[64] = case.expect()[1][64] - 1
    caps[7] = -2
    run_host(case, 64, 3, caps=caps)
    run_host(Case(130, "offsets", neg=(70,)), 64, 1)


def test_host_call_image_is_not_sized_by_a_generous_dst_cap():
    case = Case(64, "strided", lens=[64] * 64)
    r = run_host(case, 0, 0, dst_cap=64 << 20)
    assert r.image_bytes < 2 * 64 * (SLOT + 16) + (1 << 20)        # the ring and at most the sum of the limits, not dst_cap


# ---- the legacy frame in one call ---------------------------------------------------------------------------------------------------------
TABLE_FULL, CORRUPT_BLOCK = fc.TABLE_FULL, fc.CORRUPT_BLOCK


def run_frame(oracle, frame, chunk, max_chunks=None, k=0, grid=0, dst_cap=None):
    """frame_decode_compact under the emulator against the reference's reader (frame_cases.reader: the size field walk, then
    LZ4_uncompress_unknownOutputSize(in, out, size, chunk) per chunk) -> (info, dst)"""
    chunks, rets, outs, offs, want = fc.reader(oracle, frame, chunk)
    m = len(chunks) + 3 if max_chunks is None else max_chunks
    rows = min(len(chunks), m)
    a = u8(frame)
    src = np.concatenate([a, np.full(64, 0xEE, np.uint8)])
    results = np.zeros(m + 1, np.int32)
    results[:rows] = rets[:rows]
    limits = np.full(m + 1, chunk, np.int32)
    lens = np.zeros(m + 1, np.int32)
    lens[:rows] = [size for _, size in chunks[:rows]]
    src_at = np.zeros(m + 1, np.int64)
    src_at[:rows] = [at for at, _ in chunks[:rows]]
    got = np.maximum(results[:m], 0)
    at = np.concatenate(([0], np.cumsum(got, dtype=np.int64))).astype(np.int64)
    plain = np.concatenate([np.frombuffer(o, np.uint8) for o in outs[:rows]] + [np.zeros(1, np.uint8)])
    total = int(at[m])
    dst_cap = total if dst_cap is None else dst_cap
    r = CompactEmuRun()
    r.results, r.limits, r.at, r.bytes = results.ctypes.data, limits.ctypes.data, at.ctypes.data, plain.ctypes.data
    r.src, r.src_at, r.src_len, r.n, r.grid = src.ctypes.data, src_at.ctypes.data, lens.ctypes.data, m, grid
    dst = Guarded(dst_cap, fill=0xA7)
    scratch = Guarded(emu().emu_frame_compact_scratch_bytes(chunk, m, k))
    info = FrameInfo(-7, -7, -7, -7, -7, -7)
    rc = emu().emu_frame_decode_compact(src.ctypes.data if a.size else None, a.size, chunk, m, k, scratch.ptr, scratch.n, dst.ptr, dst_cap,
                                        C.addressof(info), C.addressof(r))
    assert rc == 0, r.error
    assert dst.intact() and scratch.intact() and r.shape_errors == 0 and r.passes == 1
    assert (r.calls, r.max_rows) == rounds_of(m, k), "the decode runs over all max_chunks rows"
    if len(chunks) > m:
        assert fc.info_tuple(info) == (len(chunks), total, total if all(x >= 0 for x in rets[:m]) else fc.info_tuple(info)[2], chunks[m][0] - 4, TABLE_FULL)
        return info, dst
    assert fc.info_tuple(info) == want
    t = fc.FrameTables()
    emu().emu_frame_compact_tables(scratch.ptr, chunk, m, k, C.addressof(t))
    dst_off = np.ctypeslib.as_array(C.cast(t.dst_off, C.POINTER(C.c_int64)), shape=(m + 1,))
    assert (dst_off == at).all() and (dst_off[:rows + 1] == offs[:rows + 1]).all()
    w = max(i for i in range(m + 1) if at[i] <= dst_cap)
    assert (dst.a[:at[w]] == plain[:at[w]]).all(), "the written chunks are not the reader's bytes"
    if w == m:
        assert (dst.a[total:] == 0xA7).all()
    return info, dst


@pytest.mark.parametrize("grid", GRIDS)
def test_frames_equal_the_reference_reader(oracle, grid):
    for chunk, n in ((4096, 0), (4096, 4095), (4096, 3 * 4096 - 9), (17, 200 * 17 - 5), (65536, 65537)):
        frame = fc.make_frame(oracle, fc.sample(oracle, n), chunk)
        assert len(fc.walk(frame, chunk)[0]) == (n + chunk - 1) // chunk
        for k in sorted({0, 1, 2, 7} if n < 3000 or chunk > 17 else {0, 7, 64, 199, 200}):
            info, dst = run_frame(oracle, frame, chunk, k=k, grid=grid)
            assert info.error == fc.OK and bytes(dst.a) == bytes(fc.sample(oracle, n))


@pytest.mark.parametrize("grid", GRIDS)
def test_frame_header_cases(oracle, grid):
    chunk = 4096
    frame = fc.make_frame(oracle, fc.sample(oracle, 3 * chunk + 7), chunk)
    for k in (0, 2):
        for f, err in ((frame + frame, fc.OK), (fc.MAGIC + frame, fc.OK), (frame + fc.MAGIC, fc.OK),                 # appended frames
                       (frame + b"\x01\x02", fc.TRUNCATED), (frame[:-3], fc.TRUNCATED),                             # a truncated tail
                       (frame + (fc.bound(chunk) + 1).to_bytes(4, "little") + b"\x00" * 8, fc.BAD_SIZE),             # a bad size field
                       (b"\x00" + frame[1:], fc.BAD_MAGIC), (b"", fc.BAD_MAGIC), (frame[:4], fc.OK)):
            info, dst = run_frame(oracle, f, chunk, k=k, grid=grid)
            assert info.error == err, (f[:8], err)
        # dst_cap: nothing at or past it is written, the record is complete
        total = 3 * chunk + 7
        for dst_cap in (0, 1, chunk, chunk + 1, total - 1, total + 100):
            info, dst = run_frame(oracle, frame, chunk, k=k, grid=grid, dst_cap=dst_cap)
            assert (info.decoded_bytes, info.good_bytes, info.error) == (total, total, fc.OK)


@pytest.mark.parametrize("grid", GRIDS)
def test_frame_table_too_small(oracle, grid):
    chunk = 4096
    frame = fc.make_frame(oracle, fc.sample(oracle, 5 * chunk + 7), chunk)
    chunks = fc.walk(frame, chunk)[0]
    for m in (0, 1, 5):
        info, dst = run_frame(oracle, frame, chunk, max_chunks=m, k=2, grid=grid)
        assert (info.error, info.chunks, info.error_offset) == (TABLE_FULL, 6, chunks[m][0] - 4)
    info, dst = run_frame(oracle, frame, chunk, max_chunks=6, k=2, grid=grid)
    assert info.error == fc.OK


@pytest.mark.parametrize("grid", GRIDS)
def test_frame_corrupt_chunks(oracle, grid):
    """a corrupt chunk first, last and in the middle: it takes 0 bytes, its neighbours pack around it, and the lowest one is the outcome,
    ahead of the header error behind it"""
    chunk = 4096
    data = fc.sample(oracle, 9 * chunk)
    a = u8(data)
    comps = [bytes(oracle.compress(a[i * chunk:(i + 1) * chunk])) for i in range(9)]
    for bad in ((0,), (8,), (4,), (0, 4, 8)):
        parts = [b"\xFF\xFF\xFF" + c[3:] if i in bad else c for i, c in enumerate(comps)]
        frame = fc.MAGIC + b"".join(len(c).to_bytes(4, "little") + c for c in parts) + b"\x01\x02"
        for k in (0, 4, 5):
            info, dst = run_frame(oracle, frame, chunk, k=k, grid=grid)
            field = 4 + sum(4 + len(c) for c in parts[:bad[0]])
            assert fc.info_tuple(info) == (9, (9 - len(bad)) * chunk, bad[0] * chunk, field, CORRUPT_BLOCK)
            assert bytes(dst.a) == b"".join(data[i * chunk:(i + 1) * chunk] for i in range(9) if i not in bad)


@pytest.mark.parametrize("grid", GRIDS)
def test_frame_chunk_that_only_decodes_with_room(oracle, grid):
    """A chunk that walks to 10 bytes but whose first sequence ends within the last bytes of a 10-byte output: the two-call path, which
    decodes at the walked size, fails it; with chunk_size bytes of room -- the reference's reader -- it decodes.  The expected bytes are
    the oracle's at that capacity."""
    chunk = 4096
    data = fc.sample(oracle, 2 * chunk)
    a = u8(data)
    odd = bytes([0x10, 0x30, 1, 0, 0x50, 1, 2, 3, 4, 5])
    parts = [bytes(oracle.compress(a[:chunk])), odd, bytes(oracle.compress(a[chunk:]))]
    frame = fc.MAGIC + b"".join(len(c).to_bytes(4, "little") + c for c in parts)
    r, out = oracle.uncompress_unknown_raw(u8(odd), len(odd), chunk)
    assert r == 10 and oracle.uncompress_unknown_raw(u8(odd), len(odd), 10)[0] < 0
    ix = fc.Index(frame, chunk, 5, grid)
    assert ix.info.error == fc.OK and ix.decode(oracle)[1].error == CORRUPT_BLOCK, "the two-call path rejects the chunk"
    for k in (0, 2):
        info, dst = run_frame(oracle, frame, chunk, k=k, grid=grid)
        assert fc.info_tuple(info) == (3, 2 * chunk + 10, 2 * chunk + 10, -1, fc.OK)
        assert bytes(dst.a) == data[:chunk] + bytes(out[:10]) + data[chunk:]


def test_frame_argument_checks():
    L = emu()
    buf = Guarded(1 << 16)
    info = FrameInfo()
    need = L.emu_frame_compact_scratch_bytes(4096, 4, 0)
    assert 0 < L.emu_frame_compact_scratch_bytes(4096, 4, 2) < need <= buf.n
    assert L.emu_frame_compact_scratch_bytes(-1, 4, 0) == E_ARGUMENT and L.emu_frame_compact_scratch_bytes(4096, -1, 0) == E_ARGUMENT
    assert L.emu_frame_compact_scratch_bytes(4096, 4, -1) == E_ARGUMENT

    def call(src=buf.ptr, src_len=100, chunk=4096, m=4, k=0, scratch=buf.ptr, scratch_n=need, dst=buf.ptr, dst_cap=100, info_ptr=C.addressof(info)):
        r = CompactEmuRun()
        rc = L.emu_frame_decode_compact(src, src_len, chunk, m, k, scratch, scratch_n, dst, dst_cap, info_ptr, C.addressof(r))
        assert r.passes == 0 or rc == 0
        return rc

    for kw in (dict(src_len=-1), dict(m=-1), dict(k=-1), dict(dst_cap=-1), dict(info_ptr=None), dict(scratch=None), dict(src=None), dict(dst=None),
               dict(chunk=-1), dict(chunk=0x7E000001), dict(scratch_n=need - 1)):
        assert call(**kw) == E_ARGUMENT, kw
    assert buf.intact()
