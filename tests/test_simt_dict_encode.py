"""Block batches encoded against a shared dictionary (encode_dict_prime_kernel, encode_dict_kernel and encode_fast_block's DICT mode:
lz4hip_encode_dict.hpp, lz4hip_encode.hpp) under the CPU SIMT emulator: the built blocks of tests/dict_encode_cases.py, dictionary by
dictionary, with 1 and with 5 wavefronts per workgroup, in one batch and one block per call, rows at offsets and rows at a stride,
byte for byte and result for result against the twin (tests/dict_encode_ref.py) -- every row, every output and the dictionary in a
place of its own between UNMAPPED pages, the page in front of the dictionary's reachable bytes included, so a read or a write outside
them ends the run -- and the emulator's DICT counters (tests/simt/emu_dict_encode.cpp) as the proof that a case reached the edge it was
built for.  Also the primed table alone, the identity of dict_len = 0 with the plain call, and the host-pointer call over EmuStage: one
upload and one priming, before anything else.  The -m gpu twin is tests/test_gpu_dict_encode.py."""
import ctypes as C
import mmap

import numpy as np
import pytest

import dict_cases
import dict_encode_cases as cases
import dict_encode_ref as ref
import emu_helpers as emu
from lz4net_amd import _lib

PAGE = mmap.PAGESIZE
_libc = C.CDLL(None, use_errno=True)
_libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]


class Arena:
    """places of the given sizes, each between two pages without access: flush against the page in front of it ("low") or against the
    page behind it ("high"); `lead` bytes of slack set the alignment of a low place.  Filled with `fill`."""

    def __init__(self, sizes, mode, fill=cases.HOLE, lead=0):
        spans = [(max(int(n), 0) + lead + PAGE - 1) // PAGE * PAGE for n in sizes]
        self.map = mmap.mmap(-1, sum(spans) + PAGE * (len(spans) + 1))
        self.view = np.frombuffer(self.map, np.uint8)
        self.base = self.view.ctypes.data
        assert self.base % PAGE == 0
        self.at, pos = [], 0
        for n, span in zip(sizes, spans):
            assert _libc.mprotect(self.base + pos, PAGE, 0) == 0
            pos += PAGE
            self.view[pos:pos + span] = fill
            self.at.append(pos + lead if mode == "low" else pos + span - int(n))
            pos += span
        assert _libc.mprotect(self.base + pos, PAGE, 0) == 0
        self.sizes = [int(n) for n in sizes]

    def put(self, i, data):
        self.view[self.at[i]:self.at[i] + len(data)] = np.frombuffer(bytes(data), np.uint8)

    def get(self, i):
        return self.view[self.at[i]:self.at[i] + self.sizes[i]]

    def offsets(self):
        return np.array(self.at, np.int64)


class DictPlace:
    """the dictionary's REACHABLE bytes between unmapped pages; the pointer the call gets is where the whole dictionary would begin,
    so the bytes no match can reach lie (low: all but `align` of them) in memory without access"""

    def __init__(self, dic, mode, align):
        reach = min(int(dic.size), cases.REACH)
        self.arena = Arena([reach], mode, fill=0x22, lead=align if mode == "low" else 0)
        self.arena.put(0, dic[dic.size - reach:])
        self.ptr = self.arena.base + self.arena.at[0] - (int(dic.size) - reach)


def _table():
    store = np.full(16384 + 256, 0x77, np.uint8)
    lead = (-store.ctypes.data) % 16 + 64
    return store, lead


def _encoder(wpg, mode, strided=False, keep=None):
    """dict_encode_cases.check's encode over the emulator; keep: a dict that receives the call's scratch (the primed table) afterwards"""
    def encode(blocks, caps, dic, align):
        n = len(blocks)
        sl, cp = np.array([len(b) for b in blocks], np.int32), np.array(caps, np.int32)
        res = np.full(n, -12345678, np.int32)
        place = DictPlace(dic, mode, align) if dic.size else None
        store, lead = _table()
        table_ptr = store.ctypes.data + lead
        if strided:
            src = np.full((n, int(sl.max()) + 7), 0x11, np.uint8)
            dst = np.full((n, int(cp.max()) + 64 + 5), cases.HOLE, np.uint8)
            for i, b in enumerate(blocks):
                src[i, :len(b)] = np.frombuffer(b, np.uint8)
            cases.emu().emu_encdict_encode(C.c_void_p(src.ctypes.data), None, C.c_int64(src.strides[0]), C.c_void_p(sl.ctypes.data), C.c_void_p(dst.ctypes.data), None,
                                           C.c_int64(dst.strides[0]), C.c_void_p(cp.ctypes.data), C.c_void_p(res.ctypes.data), C.c_int64(n), wpg,
                                           C.c_void_p(place.ptr) if place else None, C.c_int64(dic.size), C.c_void_p(table_ptr))
            outs = [dst[i, :caps[i] + 64].copy() for i in range(n)]
            assert all((dst[i, caps[i]:] == cases.HOLE).all() for i in range(n))
        else:
            sa = Arena([len(b) for b in blocks], mode, fill=0x11)
            for i, b in enumerate(blocks):
                sa.put(i, b)
            da = Arena([cap + 64 for cap in caps], mode)
            so, do = sa.offsets(), da.offsets()
            cases.emu().emu_encdict_encode(C.c_void_p(sa.base), C.c_void_p(so.ctypes.data), C.c_int64(0), C.c_void_p(sl.ctypes.data), C.c_void_p(da.base),
                                           C.c_void_p(do.ctypes.data), C.c_int64(0), C.c_void_p(cp.ctypes.data), C.c_void_p(res.ctypes.data), C.c_int64(n), wpg,
                                           C.c_void_p(place.ptr) if place else None, C.c_int64(dic.size), C.c_void_p(table_ptr))
            outs = [da.get(i).copy() for i in range(n)]
        assert (store[:lead] == 0x77).all() and (store[lead + 16384:] == 0x77).all(), "wrote outside the scratch"
        if keep is not None:
            keep["table"] = store[lead:lead + 16384].view(np.uint32).copy()
        return res, outs
    return encode


def _stats(run):
    st = (C.c_ulonglong * 16)()
    cases.emu().emu_encdict_stats(st, 1)
    run()
    cases.emu().emu_encdict_stats(st, 1)
    return list(st)


@pytest.mark.parametrize("wpg,mode,align,strided", [(1, "low", 0, False), (5, "high", 0, False), (5, "low", 1, False), (1, "low", 3, True)])
@pytest.mark.parametrize("group", cases.GROUPS, ids=cases.IDS)
def test_built_blocks_match_the_twin(oracle, group, wpg, mode, align, strided):
    cases.check(oracle, group, _encoder(wpg, mode, strided), align=align)


@pytest.mark.parametrize("group", cases.GROUPS, ids=cases.IDS)
def test_one_block_per_call(oracle, group):
    cases.check(oracle, group, _encoder(1, "high"), one_by_one=True)


@pytest.mark.parametrize("group", [g for g in cases.GROUPS if g[1] > 0], ids=[i for g, i in zip(cases.GROUPS, cases.IDS) if g[1] > 0])
def test_cases_reach_their_edges(oracle, group):
    """every case alone: the counters it names moved -- a case that does not move its counter never reached its edge -- and a block of
    fewer than 13 bytes reads nothing of the dictionary"""
    for i, c in enumerate(cases.cases(group)):
        st = _stats(lambda: cases.check(oracle, group, _encoder(1, "low"), only=[i]))
        for slot in c.moves:
            assert st[slot] > 0, (group, c.note, "counter never moved", slot, st)
        if len(c.block) < 13:
            assert sum(st) == 0, (group, c.note, st)


def test_the_three_lanes_and_both_rounds_of_the_crossing_are_there():
    notes = [c.note for c in cases.cases(("generic", 65536))]
    for rnd in (0, 1):
        for lane in (0, 31, 63):
            assert any(n.startswith("the count crosses T in round %d, lane %d " % (rnd, lane)) for n in notes), (rnd, lane)
    for dict_len in (17, 4097, 70000):
        notes = [c.note for c in cases.cases(("generic", dict_len))]
        assert sum(n.startswith("the last ") for n in notes) == (2 if dict_len == 17 else 3), dict_len
    assert any("stopped by ref > 0" in c.note for c in cases.cases(("generic", 17)))


# ---- the primed table ------------------------------------------------------------------------------------------------------------------------
def _dictionaries():
    return [dict_cases.dictionary(n) for n in cases.DICT_LENS if n] + [cases.far_dictionary(n) for n in (65535, 70000)]


@pytest.mark.parametrize("mode,align", [("low", 0), ("low", 1), ("low", 3), ("high", 0)])
def test_primed_table_is_the_twins(mode, align):
    """encode_dict_prime_kernel alone, for every dictionary length: T < 4 gives the zero table"""
    for dic in _dictionaries():
        place = DictPlace(dic, mode, align)
        store, lead = _table()
        cases.emu().emu_encdict_prime(C.c_void_p(place.ptr), C.c_int64(dic.size), C.c_void_p(store.ctypes.data + lead))
        got = store[lead:lead + 16384].view(np.uint32)
        assert np.array_equal(got, ref.primed_table(dic.tobytes())), dic.size
        assert (store[:lead] == 0x77).all() and (store[lead + 16384:] == 0x77).all()
        if dic.size < 4:
            assert not got.any()


@pytest.mark.parametrize("group", [("generic", 17), ("generic", 4097), ("generic", 70000), ("far", 65536)])
def test_a_batch_leaves_the_primed_table_as_it_was(oracle, group):
    """blocks write only their LDS copy: the scratch after a batch is the twin's table"""
    for wpg in (1, 5):
        keep = {}
        cases.check(oracle, group, _encoder(wpg, "low", keep=keep))
        assert np.array_equal(keep["table"], ref.primed_table(cases.cases(group)[0].dic.tobytes())), (group, wpg)


# ---- dict_len = 0 ----------------------------------------------------------------------------------------------------------------------------
def test_dict_len_zero_is_the_plain_call(oracle):
    """result for result and byte for byte, a NULL dictionary and a NULL scratch included, short blocks (the 64k variant) and a long one"""
    rng = np.random.default_rng(5)
    blocks = [c.block for c in cases.cases(("generic", 0))] + [bytes(rng.integers(0, 4, 65547 + 300, dtype=np.uint8))]
    caps = [c.cap for c in cases.cases(("generic", 0))] + [ref.bound(65547 + 300)]
    for wpg in (1, 5):
        want_res, want_dst = emu.encode([np.frombuffer(b, np.uint8) for b in blocks], caps, wg5=wpg == 5)
        n = len(blocks)
        sl, cp = np.array([len(b) for b in blocks], np.int32), np.array(caps, np.int32)
        src = np.zeros((n, int(sl.max()) + 16), np.uint8)
        for i, b in enumerate(blocks):
            src[i, :len(b)] = np.frombuffer(b, np.uint8)
        dst = np.full((n, int(cp.max()) + 64), cases.HOLE, np.uint8)
        res = np.full(n, -7, np.int32)
        cases.emu().emu_encdict_encode(C.c_void_p(src.ctypes.data), None, C.c_int64(src.strides[0]), C.c_void_p(sl.ctypes.data), C.c_void_p(dst.ctypes.data), None,
                                       C.c_int64(dst.strides[0]), C.c_void_p(cp.ctypes.data), C.c_void_p(res.ctypes.data), C.c_int64(n), wpg, None, C.c_int64(0), None)
        assert list(res) == list(want_res)
        for i in range(n):
            assert np.array_equal(dst[i, :max(res[i], 0)], np.asarray(want_dst[i])[:max(res[i], 0)]), (wpg, i)
            assert (dst[i, caps[i]:] == cases.HOLE).all()
    long_one = np.frombuffer(blocks[-1], np.uint8)
    assert bytes(dst[n - 1, :res[n - 1]]) == bytes(oracle.compress(long_one))          # (the generic variant)
    assert ref.encode(blocks[-1]) == (int(res[n - 1]), bytes(dst[n - 1, :res[n - 1]]))  # ... which the twin is with T = 0


# ---- the host-pointer call -------------------------------------------------------------------------------------------------------------------
class EncDictHost(C.Structure):
    _fields_ = [("uploads", C.c_int64), ("bytes", C.c_int64), ("log_at_upload", C.c_int64), ("kernels_at_upload", C.c_int64), ("first_byte_offset", C.c_int64),
                ("primes", C.c_int64), ("log_at_prime", C.c_int64), ("kernels_at_prime", C.c_int64), ("uploads_at_prime", C.c_int64), ("intact", C.c_int64),
                ("table_unchanged", C.c_int64)]


@pytest.mark.parametrize("group,slices,hint", [(("generic", 4097), 1, 0), (("generic", 70000), 3, 0), (("generic", 17), 0, 4), (("far", 70000), 2, 0)])
def test_host_call_uploads_and_primes_once(oracle, group, slices, hint):
    """lz4hip_encode_batch_dict_host's upload, priming and slice loop over EmuStage, the slices' kernels under the emulator: every case
    comes back right whatever the slices are; the stage saw ONE reserve of its images, ONE upload of the dictionary -- its reachable
    bytes, no others -- and ONE priming behind it, both before its first record and before any kernels; the slices are the plain
    encode's (those run_host_batch cuts for the same knob and hint); nothing outside the images, the copy or the table was written, and
    the table is after the call what the priming left"""
    L = cases.emu()
    assert L.emu_encdict_sizeof(0) == C.sizeof(EncDictHost) and L.emu_encdict_sizeof(1) == C.sizeof(emu.HostBatch)
    cs = cases.cases(group)
    want = cases.expected(oracle.compress_raw, group)
    n = len(cs)
    src, sl = emu.pack([np.frombuffer(c.block, np.uint8) for c in cs])
    cp = np.array([c.cap for c in cs], np.int32)
    dst = np.full((n, int(cp.max()) + 64), cases.HOLE, np.uint8)
    res = np.full(n, -12345678, np.int32)
    hb = _lib.Batch(src=src.ctypes.data, src_off=None, src_stride=src.strides[0], src_len=sl.ctypes.data, dst=dst.ctypes.data, dst_off=None,
                    dst_stride=dst.strides[0], dst_cap=cp.ctypes.data, dst_cap_all=0, src_len_all=0, result=res.ctypes.data, n_blocks=n)
    log = np.zeros((256, 8), np.int64)
    r = emu.HostBatch(slice_floor=0, slice_ceiling=-1, hinted_ceiling=-1, pool_floor=-1, fail_at=-1, slices_knob=slices, slice_hint=hint, dst_len_is_result=1,
                      log=log.ctypes.data, log_cap=256)
    d = EncDictHost()
    dic = cs[0].dic
    rc = L.emu_encdict_host(C.byref(hb), C.c_void_p(dic.ctypes.data), C.c_int64(dic.size), 5, C.byref(r), C.byref(d))
    assert rc == 0, r.error
    # the plain encode's plan for the same batch, knob and hint
    plan = np.zeros(19, np.int64)
    text = C.create_string_buffer(160)
    assert emu.hostbatch().emu_host_plan(C.byref(hb), slices, hint, C.byref(r), C.c_void_p(plan.ctypes.data), text) == 0
    assert r.violations == 0 and r.intact == 1 and d.intact == 1 and d.table_unchanged == 1 and r.reserves == 1 and r.kernel_calls == plan[6]
    kernels = [row for row in log[:r.log_n] if row[0] == 3]
    assert [int(k[2]) for k in kernels] == [int(min(plan[5], n - s * plan[5])) for s in range(int(plan[6]))]
    reach = min(dic.size, cases.REACH)
    assert d.uploads == 1 and d.bytes == reach and d.first_byte_offset == dic.size - reach
    assert d.log_at_upload == 0 and d.kernels_at_upload == 0
    assert d.primes == 1 and d.uploads_at_prime == 1 and d.log_at_prime == 0 and d.kernels_at_prime == 0
    for i in range(n):
        wr, wb = want[i]
        assert res[i] == wr, (cs[i].note, int(res[i]), wr)
        assert bytes(dst[i, :wr]) == wb, cs[i].note
        assert (dst[i, max(wr, 0):] == cases.HOLE).all(), (cs[i].note, "the caller got more than the result's bytes")


# ---- the fixture's records -------------------------------------------------------------------------------------------------------------------
def test_fixture_records_encode_to_the_twins_bytes_and_decode():
    """the plain text of tests/golden/dict_blocks.json against its dictionary: the twin's bytes, which decode by the twin decoder and by a
    live liblz4 where there is one"""
    import lz4f_ref
    dic, records, _ = dict_cases.load_fixture()
    plains = [p for p, _ in records]
    res, outs = _encoder(5, "high")(plains, [ref.bound(len(p)) for p in plains], dic, 0)
    lz4 = dict_cases.liblz4()
    for p, r, o in zip(plains, res, outs):
        assert (int(r), bytes(o[:r])) == ref.encode(p, dic.tobytes())
        assert lz4f_ref.decode_block(bytes(o[:r]), len(p), history=ref.tail_of(dic.tobytes())) == (len(p), p)
        if lz4 is not None:
            assert dict_cases.using_dict(lz4, bytes(o[:r]), len(p), dic) == (len(p), p)
