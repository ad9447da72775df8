"""CPU-only: the packed encode of a block batch (lz4net_amd/csrc/lz4hip_packed.hpp and its host code in lz4hip_framing.hpp and
lz4hip_hostbatch.hpp) under the SIMT emulator (tests/simt/emu_packed.inc): the real kernels, the library's front, launch sequence and
host-pointer call, with the block encoder replaced by a stand-in keyed by global block index that hands out what the oracle's
LZ4_compress / LZ4_compressHC wrote for the block -- or 0 and junk where that does not fit the block's limit, as a limited encoder
may.  Every case runs with the library's grids and with grids forced to 1 and 3 workgroups."""
import ctypes as C
import functools

import numpy as np
import pytest

import emu_lib
from block_cases import SMALL, BlockCase, check_sentinels, expect_info, lengths_of, rounds_of, sentinels
from emu_lib import E_ARGUMENT, GRIDS, Guarded, I32 as _I32, I64 as _I64, P as _P
from lz4net_amd._lib import Batch, PackedInfo

SLOT = 70000 + 70000 // 255 + 16                # compressBound of the longest block


class PackedEmuRun(C.Structure):
    _anonymous_ = ("counters",)
    _fields_ = [("sizes", _P), ("at", _P), ("bytes", _P), ("src", _P), ("src_at", _P), ("bad_len", _P), ("n", _I64), ("grid", _I32), ("pad", _I32),
                ("calls", _I64), ("max_rows", _I64), ("shape_errors", _I64), ("counters", emu_lib.EmuCounters)]


@functools.lru_cache(maxsize=None)
def emu():
    L = emu_lib.framing()
    L.emu_packed_sizeof.restype = _I64
    assert L.emu_packed_sizeof(0) == C.sizeof(PackedInfo) and L.emu_packed_sizeof(1) == C.sizeof(PackedEmuRun)
    assert L.emu_packed_sizeof(2) == C.sizeof(Batch)
    L.emu_packed_scratch_bytes.argtypes, L.emu_packed_scratch_bytes.restype = [_I64, _I32, _I64], _I64
    L.emu_packed_copy_grid.argtypes = [_I64]
    L.emu_encode_packed.argtypes = [_P, C.c_int, _I64, _P, _I64, _P, _P, _P, _I64, _P, _P]
    L.emu_encode_packed_host.argtypes = [_P, C.c_int, _I64, _P, _I64, _P, _P, _P, _I64, _P]
    return L


# ---- the blocks and what the reference's encoders write for them ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool():
    """{length: [(source, LZ4_compress output, LZ4_compressHC output), ...]}: a few distinct blocks per length, encoded once"""
    from oracle.oracle import Oracle
    oracle = Oracle()
    out = {}
    for length in SMALL + (4096, 65536, 70000):
        rows = []
        for dist in ((2, 3) if length >= 65536 else (1, 2, 3)):
            raw = oracle.gen(dist, 11, 5 + length % 7, 1, length=max(length, 1))[0, :length].copy()
            enc = []
            for hc in (False, True):
                ret, buf = oracle.compress_raw(raw, length + length // 255 + 16, hc)
                assert 0 < ret <= length + length // 255 + 16
                enc.append(buf[:ret].copy())
            rows.append((raw, enc[0], enc[1]))
        out[length] = rows
    return out


class Case(BlockCase):
    """n blocks in one of the two source layouts, and the stand-in's tables for them"""

    def __init__(self, n, layout, hc=False, lens=None):
        self.hc = hc
        self.lens = lengths_of(n) if lens is None else list(lens)
        picks = [pool()[abs(length)][i % len(pool()[abs(length)])] for i, length in enumerate(self.lens)]
        self.raw = [p[0] for p in picks]
        self.enc = [p[2 if hc else 1] for p in picks]
        self.sizes = np.array([len(e) for e in self.enc] + [0], np.int32)
        self.at = np.concatenate(([0], np.cumsum(self.sizes[:-1], dtype=np.int64))).astype(np.int64)
        self.bytes = np.concatenate(self.enc + [np.zeros(1, np.uint8)])
        self.src_at = np.concatenate(([0], np.cumsum([r.size for r in self.raw], dtype=np.int64))).astype(np.int64)
        self.flat = np.concatenate(self.raw + [np.zeros(1, np.uint8)])
        self.lay_out(self.raw, self.lens, layout, src_len_all=70000, dst_cap_all=SLOT)
        self.bad_len = (self.src_len < 0).astype(np.uint8)      # the stand-in must see an empty block there, never the negative length

    def expect(self, caps=None):
        """(results, lengths, offsets) as the contract states them"""
        res = np.zeros(self.n, np.int32)
        for i in range(self.n):
            limit = SLOT if caps is None else max(min(int(caps[i]), SLOT), 0)
            res[i] = E_ARGUMENT if self.lens[i] < 0 else (self.sizes[i] if self.sizes[i] <= limit else 0)
        lens = np.maximum(res, 0)
        offs = np.concatenate(([0], np.cumsum(lens, dtype=np.int64))).astype(np.int64)
        return res, lens, offs

    def run_record(self, grid):
        r = PackedEmuRun()
        r.sizes, r.at, r.bytes = self.sizes.ctypes.data, self.at.ctypes.data, self.bytes.ctypes.data
        r.src, r.src_at, r.n, r.grid = self.flat.ctypes.data, self.src_at.ctypes.data, self.n, grid
        r.bad_len = self.bad_len.ctypes.data
        return r


def info_tuple(i):
    assert i.reserved == 0
    return (i.blocks, i.packed_bytes, i.written_blocks, i.first_failed, i.error)


def run(case, k=0, grid=0, dst_cap=None, caps=None, want_result=True, want_len=True, scratch_short=0):
    """encode_packed under the emulator -> (rc, dst, info, run record); checks everything the contract promises on the way"""
    n = case.n
    res_want, len_want, off_want = case.expect(caps)
    total = int(off_want[n])
    dst_cap = total if dst_cap is None else dst_cap
    dst = Guarded(dst_cap, fill=0xA7)
    scratch = Guarded(emu().emu_packed_scratch_bytes(n, SLOT, k) - scratch_short)
    dst_off, plen, result, info = sentinels(n, PackedInfo)
    b = case.batch(caps, result[1:] if want_result else None)
    r = case.run_record(grid)
    rc = emu().emu_encode_packed(C.addressof(b), int(case.hc), k, dst.ptr, dst_cap, dst_off.ctypes.data + 8, plen.ctypes.data + 4 if want_len else None,
                                 scratch.ptr, scratch.n, C.addressof(info), C.addressof(r))
    assert dst.intact() and scratch.intact(), "a byte outside dst (at or past dst_cap) or outside the scratch was written"
    check_sentinels(n, dst_off, plen, result)
    if rc != 0:
        return rc, dst, info, r
    assert r.shape_errors == 0, "the encoder was handed a row or a descriptor that is not the batch's"
    assert (r.calls, r.max_rows) == rounds_of(n, k)
    assert (dst_off[1:n + 2] == off_want).all()
    if want_len:
        assert (plen[1:n + 1] == len_want).all()
    if want_result:
        assert (result[1:n + 1] == res_want).all()
    want = expect_info(n, res_want, off_want, dst_cap, failed=lambda r: r <= 0)
    assert info_tuple(info) == want
    w = want[2]
    packed = np.concatenate([case.enc[i][:len_want[i]] for i in range(w)] + [np.zeros(0, np.uint8)])
    assert packed.size == off_want[w] and (dst.a[:off_want[w]] == packed).all(), "the written prefix is not the oracle's bytes"
    if w == n:
        assert (dst.a[total:] == 0xA7).all(), "bytes past the total were written"
    return rc, dst, info, r


# ---- parity and shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("layout", ["strided", "offsets"])
@pytest.mark.parametrize("n", [0, 1, 3, 257])
def test_parity_every_round_size(n, layout, grid):
    case = Case(n, layout)
    for k in sorted({0, 1, 64, 1000, n, n + 5}):
        assert run(case, k, grid)[0] == 0


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", [0, 1, 64, 1000, 4097, 4102])
def test_parity_across_the_scan_tile(k, grid):
    assert emu().emu_packed_sizeof(100) == 4096
    assert run(Case(4097, "offsets" if k % 2 else "strided"), k, grid)[0] == 0


@pytest.mark.parametrize("grid", GRIDS)
def test_parity_hc_and_optional_outputs(grid):
    case = Case(257, "offsets", hc=True)
    assert run(case, 64, grid, want_result=False, want_len=False)[0] == 0
    assert run(case, 0, grid, want_result=False)[0] == 0


def test_uniform_length_batch():
    case = Case(70, "strided", lens=[4096] * 70)
    b_len = 4096
    res_want, len_want, off_want = case.expect()
    dst = Guarded(int(off_want[70]))
    scratch = Guarded(emu().emu_packed_scratch_bytes(70, SLOT, 64))
    dst_off = np.zeros(71, np.int64)
    info = PackedInfo()
    b = case.batch(uniform_len=b_len)
    r = case.run_record(0)
    assert emu().emu_encode_packed(C.addressof(b), 0, 64, dst.ptr, dst.n, dst_off.ctypes.data, None, scratch.ptr, scratch.n, C.addressof(info), C.addressof(r)) == 0
    assert r.shape_errors == 0 and (dst_off == off_want).all() and dst.intact() and scratch.intact()
    assert bytes(dst.a) == b"".join(bytes(e) for e in case.enc)


# ---- per-block limits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", [0, 64, 1])
def test_blocks_that_fail_their_limit_take_no_bytes(k, grid):
    case = Case(257, "strided")
    caps = np.full(258, SLOT + 1000, np.int32)                # (above the slot width: the slot width binds)
    for i in (1, 64, 65, 130, 256):
        caps[i] = case.sizes[i] - 1                            # one byte short
    caps[66] = case.sizes[66]                                  # exactly enough
    caps[3] = -5                                               # a negative limit is no room at all
    rc, dst, info, r = run(case, k, grid, caps=caps)
    assert rc == 0 and info.first_failed == 1 and info.error == 0
    res = case.expect(caps)[0]
    assert [i for i in range(257) if res[i] == 0] == [1, 3, 64, 65, 130, 256]


@pytest.mark.parametrize("grid", GRIDS)
def test_negative_length_is_an_argument_result(grid):
    lens = lengths_of(130)
    lens[70] = -13
    lens[129] = -1
    case = Case(130, "offsets", lens=lens)
    for k in (0, 64):
        rc, dst, info, r = run(case, k, grid)
        assert rc == 0 and (info.first_failed, info.error) == (70, E_ARGUMENT)
    caps = np.full(131, SLOT, np.int32)
    caps[5] = 0
    rc, dst, info, r = run(case, 64, grid, caps=caps)
    assert (info.first_failed, info.error) == (5, 0)


# ---- dst_cap clipping -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", [0, 64])
def test_dst_cap_clips_to_a_prefix(k, grid):
    case = Case(257, "strided")
    off = case.expect()[2]
    caps = {0, int(off[257]) - 1}
    for blk in (1, 3, 63, 64, 65, 128, 200, 256, 257):         # 64, 128 and 256 are round boundaries for k = 64
        caps |= {int(off[blk]) - 1, int(off[blk]), int(off[blk]) + 1}
    for dst_cap in sorted(c for c in caps if c >= 0):
        assert run(case, k, grid, dst_cap=dst_cap)[0] == 0


def test_size_query_needs_no_dst():
    case = Case(130, "offsets")
    res_want, len_want, off_want = case.expect()
    scratch = Guarded(emu().emu_packed_scratch_bytes(130, SLOT, 64))
    dst_off = np.zeros(131, np.int64)
    info = PackedInfo()
    b = case.batch()
    r = case.run_record(0)
    assert emu().emu_encode_packed(C.addressof(b), 0, 64, None, 0, dst_off.ctypes.data, None, scratch.ptr, scratch.n, C.addressof(info), C.addressof(r)) == 0
    assert (dst_off == off_want).all() and info.packed_bytes == off_want[130] and info.written_blocks == 0 and scratch.intact()


# ---- scratch and argument checks ------------------------------------------------------------------------------------------------------
def test_scratch_does_not_grow_past_a_round():
    f = emu().emu_packed_scratch_bytes
    assert f(0, SLOT, 0) == 0 and f(0, SLOT, 64) == 0
    for k in (1, 64, 1000, 16384):
        assert len({f(n, SLOT, k) for n in (k, k + 1, 2 * k, 10 * k + 3, 1 << 22)}) == 1
        sizes = [f(n, SLOT, k) for n in range(1, 2 * k + 2, max(k // 16, 1))]
        assert sizes == sorted(sizes) and sizes[0] > 0
    whole = [f(n, SLOT, 0) for n in (1, 2, 64, 65, 4096, 4097, 100000)]
    assert whole == sorted(whole)
    # the ring (a slot rounded up to 16) and three int32 tables per block of a round (limits, lengths, results), the scan's tile sums,
    # the state block, and up to 256 bytes of rounding per piece
    assert f(1 << 22, SLOT, 16384) < (16384 * (SLOT + 16 + 12) + 8 * 5 + 256 * 6 + 256)
    assert f(5, 0, 0) == E_ARGUMENT and f(5, SLOT, -1) == E_ARGUMENT


def test_one_byte_less_scratch_is_refused():
    for k in (0, 64):
        rc, dst, info, r = run(Case(130, "strided"), k, scratch_short=1)
        assert rc == E_ARGUMENT and b"scratch_bytes" in r.error and r.calls == 0
        assert info_tuple_untouched(info) and (dst.a == 0xA7).all()


def info_tuple_untouched(i):
    return (i.blocks, i.packed_bytes, i.written_blocks, i.first_failed, i.error, i.reserved) == (-7,) * 6


def test_argument_checks():
    case = Case(3, "strided")
    scratch = Guarded(emu().emu_packed_scratch_bytes(3, SLOT, 0))
    dst = Guarded(1 << 18)
    dst_off = np.zeros(4, np.int64)
    info = PackedInfo()

    def call(b, mode=0, k=0, dst_ptr=dst.ptr, dst_cap=dst.n, off=dst_off.ctypes.data, scratch_ptr=scratch.ptr, scratch_n=scratch.n):
        r = case.run_record(0)
        rc = emu().emu_encode_packed(None if b is None else C.addressof(b), mode, k, dst_ptr, dst_cap, off, None, scratch_ptr, scratch_n,
                                     C.addressof(info), C.addressof(r))
        assert r.calls == 0 or rc == 0
        return rc

    assert call(case.batch()) == 0
    assert call(None) == E_ARGUMENT
    for field, value in (("n_blocks", -1), ("dst_cap_all", 0), ("dst_cap_all", -4), ("src", None)):
        b = case.batch()
        setattr(b, field, value)
        assert call(b) == E_ARGUMENT, field
    assert call(case.batch(), mode=2) == E_ARGUMENT and call(case.batch(), mode=-1) == E_ARGUMENT
    assert call(case.batch(), k=-1) == E_ARGUMENT
    assert call(case.batch(), dst_cap=-1) == E_ARGUMENT
    assert call(case.batch(), off=None) == E_ARGUMENT
    assert call(case.batch(), dst_ptr=None) == E_ARGUMENT
    assert call(case.batch(), scratch_ptr=None) == E_ARGUMENT
    b = case.batch(uniform_len=-3)
    assert call(b) == E_ARGUMENT
    b = case.batch()
    b.n_blocks = 1 << 31                                       # one round of 2^31 blocks
    assert call(b, scratch_n=1 << 62) == E_ARGUMENT
    assert dst.intact() and scratch.intact()


def test_empty_batch():
    for k in (0, 64):
        b = Batch(dst_cap_all=SLOT)
        dst_off = np.full(3, -77, np.int64)
        info = PackedInfo(-7, -7, -7, -7, -7, -7)
        r = PackedEmuRun()
        assert emu().emu_encode_packed(C.addressof(b), 0, k, None, 0, dst_off.ctypes.data + 8, None, None, 0, C.addressof(info), C.addressof(r)) == 0
        assert list(dst_off) == [-77, 0, -77] and info_tuple(info) == (0, 0, 0, -1, 0) and r.calls == 0


# ---- the host-pointer call ------------------------------------------------------------------------------------------------------------
def run_host(case, k=0, grid=0, dst_cap=None, caps=None, want_result=True, want_len=True, pool_floor=-1):
    n = case.n
    res_want, len_want, off_want = case.expect(caps)
    total = int(off_want[n])
    dst_cap = total if dst_cap is None else dst_cap
    dst = Guarded(dst_cap, fill=0xA7)
    dst_off, plen, result, info = sentinels(n, PackedInfo)
    b = case.batch(caps, result[1:] if want_result else None)
    r = case.run_record(grid)
    rc = emu().emu_encode_packed_host(C.addressof(b), int(case.hc), k, dst.ptr, dst_cap, dst_off.ctypes.data + 8, plen.ctypes.data + 4 if want_len else None,
                                      C.addressof(info), pool_floor, C.addressof(r))
    assert rc == 0, r.error
    assert dst.intact() and r.intact == 1 and r.shape_errors == 0
    check_sentinels(n, dst_off, plen, result)
    assert (dst_off[1:n + 2] == off_want).all()
    assert not want_len or (plen[1:n + 1] == len_want).all()
    assert not want_result or (result[1:n + 1] == res_want).all()
    want = expect_info(n, res_want, off_want, dst_cap, failed=lambda r: r <= 0)
    assert info_tuple(info) == want
    w = want[2]
    packed = np.concatenate([case.enc[i][:len_want[i]] for i in range(w)] + [np.zeros(0, np.uint8)])
    assert (dst.a[:off_want[w]] == packed).all()
    if n > 0:
        # one download of the payload, of min(packed_bytes, dst_cap) bytes, after the info and the per-block arrays
        payload = min(total, dst_cap)
        assert r.reserves == 1 and r.syncs == 2
        assert r.downloads == 2 + int(want_result) + int(want_len) + int(payload > 0)
        assert payload == 0 or r.last_download == payload
    return r


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("layout", ["strided", "offsets"])
def test_host_call_parity(layout, grid):
    case = Case(257, layout)
    for k in (0, 64):
        run_host(case, k, grid)
    run_host(case, 64, grid, want_result=False, want_len=False, pool_floor=0)      # (the rows gathered on the row pool)
    run_host(Case(0, layout), 0, grid)
    # info is optional
    want_off = case.expect()[2]
    dst, dst_off = Guarded(int(want_off[257])), np.zeros(258, np.int64)
    b, r = case.batch(), case.run_record(grid)
    assert emu().emu_encode_packed_host(C.addressof(b), 0, 64, dst.ptr, dst.n, dst_off.ctypes.data, None, None, -1, C.addressof(r)) == 0
    assert (dst_off == want_off).all() and dst.intact() and bytes(dst.a) == b"".join(bytes(e) for e in case.enc)


def test_host_call_limits_clipping_and_negative_lengths():
    case = Case(257, "strided")
    off = case.expect()[2]
    for dst_cap in (0, int(off[64]), int(off[64]) + 1, int(off[257]) - 1, int(off[257]) + 100000):
        run_host(case, 64, 0, dst_cap=dst_cap)
    caps = np.full(258, SLOT, np.int32)
    caps[64] = case.sizes[64] - 1
    run_host(case, 64, 3, caps=caps)
    lens = lengths_of(130)
    lens[70] = -13
    run_host(Case(130, "offsets", lens=lens), 64, 1)


def test_host_call_image_is_not_sized_by_a_generous_dst_cap():
    case = Case(64, "strided", lens=[64] * 64)
    r = run_host(case, 0, 0, dst_cap=64 << 20)
    assert r.image_bytes < 2 * 64 * (SLOT + 16) + (1 << 20)        # the ring and at most the sum of the limits, not dst_cap
