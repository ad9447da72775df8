"""Block batches decoded against a shared dictionary (decode_block's DICT mode and decode_dict_kernel of lz4hip_decode.hpp) under the CPU
SIMT emulator: the built blocks of tests/dict_cases.py, family by family, with 1 and with 4 wavefronts per workgroup, against the
spliced truth -- every row, every output and the dictionary in a place of its own between UNMAPPED pages, so a read or a write outside
them ends the run -- and the emulator's DICT counters (tests/simt/emu_dict.cpp) as the proof that a case reached the path it was built
for.  Also the sizes walk with the dictionary's length, the identity of dict_len = 0 with the plain call, and the host-pointer call over
EmuStage: one upload of the reachable bytes, before anything else.  The -m gpu twin is tests/test_gpu_dict_decode.py."""
import ctypes as C
import mmap

import numpy as np
import pytest

import dict_cases as cases
import emu_helpers as emu
from lz4net_amd import _lib

PAGE = mmap.PAGESIZE
_libc = C.CDLL(None, use_errno=True)
_libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]


class Arena:
    """places of the given sizes, each between two pages without access: flush against the page in front of it ("low": a read below
    the place faults) or against the page behind it ("high": a read or write past it faults); `lead` bytes of slack set the
    alignment of a low place.  Filled with `fill`."""

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


def _decoder(wpg, mode):
    """dict_cases.check's decode over the emulator: rows, outputs and the dictionary each between unmapped pages"""
    def decode(comps, caps, known, lens, dic, align):
        n = len(comps)
        src = Arena([len(c) for c in comps], mode, fill=0x11)
        for i, c in enumerate(comps):
            src.put(i, c)
        # an output: its capacity and 64 guard bytes behind it, the row's first byte flush against the page in front in "low"
        dst = Arena([cap + 64 for cap in caps], mode)
        dct = Arena([dic.size], mode, fill=0x22, lead=align if mode == "low" else 0)
        dct.put(0, dic)
        sl, cp = np.array(lens, np.int32), np.array(caps, np.int32)
        res = np.full(n, -12345678, np.int32)
        so, do = src.offsets(), dst.offsets()
        cases.emu().emu_dict_decode_at(int(known), C.c_void_p(src.base), C.c_void_p(so.ctypes.data), C.c_void_p(sl.ctypes.data), C.c_void_p(dst.base),
                                       C.c_void_p(do.ctypes.data), C.c_void_p(cp.ctypes.data), C.c_void_p(res.ctypes.data), C.c_int64(n), wpg,
                                       C.c_void_p(dct.base + dct.at[0]) if dic.size else None, C.c_int64(dic.size))
        return res, [dst.get(i).copy() for i in range(n)]
    return decode


def _stats(run):
    st = (C.c_ulonglong * cases.N_STATS)()
    cases.emu().emu_dict_stats(st, 1)
    run()
    cases.emu().emu_dict_stats(st, 1)
    return list(st)


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("wpg,mode,align", [(1, "low", 0), (4, "high", 0), (4, "low", 1), (1, "low", 3)])
@pytest.mark.parametrize("name", cases.NAMES)
def test_built_blocks_match_the_spliced_truth(oracle, name, wpg, mode, align, known):
    cases.check(oracle, name, known, _decoder(wpg, mode), align=align)


@pytest.mark.parametrize("name", [n for n in cases.NAMES if cases.family(n).moves])
def test_family_reaches_its_paths(oracle, name):
    """the family's counters moved, and the preload stored min(dict_len, 4 096) bytes per block"""
    f = cases.family(name)
    for known in (True, False):
        st = _stats(lambda: cases.check(oracle, name, known, _decoder(1, "low")))
        for slot in f.moves:
            assert st[slot] > 0, (name, known, "counter never moved", slot)
        assert st[cases.PRELOAD] == sum(min(c.dict_len, cases.RING) for c in f.cases), (name, known, "preload bytes")


@pytest.mark.parametrize("name", [n for n in cases.NAMES if cases.family(n).pairs])
def test_pairs_differ_in_the_declared_direction(oracle, name):
    """of two blocks on either side of an edge, decoded alone, the named counter differs in the declared direction"""
    f = cases.family(name)
    for known in (True, False):
        alone = {i: _stats(lambda: cases.check(oracle, name, known, _decoder(1, "low"), only=[i])) for a, b, _ in f.pairs for i in (a, b)}
        for a, b, slot in f.pairs:
            assert alone[a][slot] < alone[b][slot], (name, known, f.cases[a].note, f.cases[b].note, slot, alone[a][slot], alone[b][slot])


def test_after_a_long_copy_nothing_before_the_block_comes_from_the_mirror(oracle):
    """ring_from has moved, or the block's own output has passed 4 096 bytes: the sequences behind that take their dictionary bytes from
    memory -- the mirror's counters stay where they were"""
    f = cases.family("after_long_copy")
    for i, c in enumerate(f.cases):
        if c.note.startswith(("a long copy", "the dictionary behind 4 200")):
            st = _stats(lambda: cases.check(oracle, "after_long_copy", True, _decoder(1, "low"), only=[i]))
            assert st[cases.GEN_MEMORY] > 0 and st[cases.BURST_MIRROR] == st[cases.SHORT_MIRROR] == st[cases.GEN_MIRROR] == 0, (c.note, st)


def test_dict_len_zero_is_the_plain_call(oracle):
    """result for result and byte for byte, a NULL dictionary included, on valid and damaged blocks"""
    f = cases.family("identity")
    comps = [np.frombuffer(c.block, np.uint8) for c in f.cases] + [c for c, _ in cases.plain_blocks()]
    caps = [c.cap for c in f.cases] + [raw.size for _, raw in cases.plain_blocks()]
    for known in (True, False):
        for wpg in (1, 4):
            want_res, want_dst = emu.decode(comps, caps, known=known, waves_per_group=wpg)
            res, dst = _decoder(wpg, "low")(comps, caps, known, [len(c) for c in comps], np.zeros(0, np.uint8), 0)
            assert list(res) == list(want_res)
            for i in range(len(comps)):
                assert np.array_equal(dst[i], want_dst[i, :caps[i] + 64]), (known, wpg, i)


# ---- the sizes walk ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_sizes_walk_with_the_dictionary_length(oracle, name):
    """lz4hip_decoded_sizes_dict_device's sequence: a block's size is what its unknown-size decode against the dictionary produces with
    room to spare, or the walk's refusal of a source before the dictionary"""
    import lz4f_ref
    f = cases.family(name)
    L = cases.emu()
    for dict_len, idx in sorted(cases.groups(f).items()):
        rows = [np.frombuffer(f.cases[j].block, np.uint8) for j in idx]
        n = len(rows)
        src, sl = emu.pack(rows)
        res = np.full(n, -7, np.int32)
        caps, offs = np.full(n, -7, np.int32), np.full(n + 1, -7, np.int64)
        need = L.emu_dict_sizes_scratch_bytes(n)
        scratch = np.zeros(need + 64, np.uint8)
        info = _lib.SizesInfo()
        b = _lib.Batch(src=src.ctypes.data, src_off=None, src_stride=src.strides[0], src_len=sl.ctypes.data, dst=None, dst_off=None, dst_stride=0,
                       dst_cap=None, dst_cap_all=0, src_len_all=0, result=res.ctypes.data, n_blocks=n)
        err = C.create_string_buffer(160)
        rc = L.emu_dict_sizes(C.byref(b), C.c_int64(dict_len), C.c_void_p(offs.ctypes.data), C.c_void_p(caps.ctypes.data), C.c_void_p(scratch.ctypes.data),
                              C.c_int64(need), C.byref(info), 1, err)
        assert rc == 0, err.value
        want = [lz4f_ref.size_block(bytes(r), history=min(dict_len, cases.REACH)) for r in rows]
        assert list(res) == want, (name, dict_len)
        assert list(caps) == [max(w, 0) for w in want] and list(offs) == list(np.concatenate(([0], np.cumsum([max(w, 0) for w in want]))))
        for j, w in zip(idx, want):
            if f.cases[j].raw is not None:
                assert w == f.cases[j].cap
        bad = [i for i, w in enumerate(want) if w < 0]
        assert info.blocks == n and info.first_error == (bad[0] if bad else -1) and info.decoded_bytes == offs[n]
    assert L.emu_dict_sizes(None, C.c_int64(0), None, None, None, C.c_int64(0), None, 0, err) == _lib.E_ARGUMENT


# ---- the host-pointer call -------------------------------------------------------------------------------------------------------------------
class DictHost(C.Structure):
    _fields_ = [("uploads", C.c_int64), ("bytes", C.c_int64), ("log_at_upload", C.c_int64), ("kernels_at_upload", C.c_int64), ("intact", C.c_int64),
                ("first_byte_offset", C.c_int64)]


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("dict_len,slices", [(4097, 1), (70000, 3), (0, 2)])
def test_host_call_uploads_the_dictionary_once(oracle, dict_len, slices, known):
    """lz4hip_decode_batch_dict_host's upload and slice loop over EmuStage, the slices' kernels under the emulator: every case of that
    dictionary comes back right whatever the slices are; the stage saw ONE reserve of its images and ONE upload of the dictionary -- its
    reachable bytes, no others -- before its first record and before any kernels; nothing outside the images or the copy was written"""
    L = cases.emu()
    assert L.emu_dict_sizeof(0) == C.sizeof(DictHost) and L.emu_dict_sizeof(1) == C.sizeof(emu.HostBatch)
    picked = [(name, j) for name in cases.NAMES for j in cases.groups(cases.family(name)).get(dict_len, [])][:24]
    assert len(picked) >= 4
    want, outs, rows, caps = [], [], [], []
    for name, j in picked:
        f, w, o = cases.expected(oracle, name, known)
        c = f.cases[j]
        want.append(w[j]); outs.append(o[j])
        rows.append(np.frombuffer(c.block + (bytes(c.cap + 1024) if known and c.raw is None else b""), np.uint8))
        caps.append(c.cap + (0 if known else cases.EXTRA))
    n = len(rows)
    src, sl = emu.pack(rows)
    cp = np.array(caps, np.int32)
    dst = np.full((n, int(cp.max()) + 64), cases.HOLE, np.uint8)
    res = np.full(n, -12345678, np.int32)
    hb = _lib.Batch(src=src.ctypes.data, src_off=None, src_stride=src.strides[0], src_len=sl.ctypes.data, dst=dst.ctypes.data, dst_off=None,
                    dst_stride=dst.strides[0], dst_cap=cp.ctypes.data, dst_cap_all=0, src_len_all=0, result=res.ctypes.data, n_blocks=n)
    log = np.zeros((256, 8), np.int64)
    r = emu.HostBatch(slice_floor=0, slice_ceiling=-1, hinted_ceiling=-1, pool_floor=-1, fail_at=-1, slices_knob=slices, dst_len_is_result=int(not known),
                      log=log.ctypes.data, log_cap=256)
    d = DictHost()
    dic = cases.dictionary(dict_len)
    rc = L.emu_dict_host(C.byref(hb), C.c_void_p(dic.ctypes.data) if dict_len else None, C.c_int64(dict_len), int(known), 4, C.byref(r), C.byref(d))
    assert rc == 0, r.error
    assert r.violations == 0 and r.intact == 1 and d.intact == 1 and r.reserves == 1 and r.kernel_calls == -(-n // -(-n // slices))
    reach = min(dict_len, cases.REACH)
    assert d.uploads == (1 if dict_len else 0) and d.bytes == reach and d.first_byte_offset == dict_len - reach
    assert d.log_at_upload == 0 and d.kernels_at_upload == 0
    for i in range(n):
        assert res[i] == want[i], (picked[i], int(res[i]), want[i])
        if want[i] >= 0:
            m = caps[i] if known else want[i]
            assert np.array_equal(dst[i, :m], outs[i][:m]), picked[i]
        assert (dst[i, caps[i]:] == cases.HOLE).all(), (picked[i], "wrote past the block")


# ---- the fixture: what liblz4 wrote against a dictionary -------------------------------------------------------------------------------------
def test_fixture_blocks_decode_to_their_records():
    """tests/golden/dict_blocks.json (LZ4_loadDict + LZ4_compress_fast_continue) under the emulator, known and unknown size, against the
    records' plain text; the twin first, and a live liblz4 where there is one"""
    import lz4f_ref
    dic, records, header = cases.load_fixture()
    assert len(records) >= 40 and max(len(p) for p, _ in records) <= 4096 and header["dictionary"]["length"] == dic.size
    lz4 = cases.liblz4()
    for plain, block in records:
        assert lz4f_ref.decode_block(block, len(plain), history=dic.tobytes()[-cases.REACH:]) == (len(plain), plain)
        if lz4 is not None:
            assert cases.using_dict(lz4, block, len(plain), dic) == (len(plain), plain)
    comps = [np.frombuffer(b, np.uint8) for _, b in records]

    def both():
        for known, wpg, mode in ((True, 4, "high"), (False, 1, "low")):
            caps = [len(p) + (0 if known else 3) for p, _ in records]
            res, dst = _decoder(wpg, mode)(comps, caps, known, [len(c) for c in comps], dic, 0)
            assert list(res) == [len(b) if known else len(p) for p, b in records]
            for i, (p, _) in enumerate(records):
                assert bytes(dst[i][:len(p)]) == p and (dst[i][caps[i]:] == cases.HOLE).all(), (known, i)
    st = _stats(both)
    assert st[cases.BURST_MIRROR] + st[cases.SHORT_MIRROR] + st[cases.GEN_MIRROR] > 0 and st[cases.GEN_MEMORY] > 0   # (real data meets both)
