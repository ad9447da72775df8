"""The wavefront fast encoder (lz4hip_encode.hpp) under the CPU SIMT emulator over the built blocks of tests/wave_encode_cases.py, family by
family: bit-exact against the oracle with guard bytes through every emulator form of the fast encoder, with the emulator's
LZ4HIP_STAT_ENC counters as the proof that a family reached the branches it was built for and that the two blocks of a threshold pair
stand on its two sides.  Every expectation of a built block is asserted against the oracle's own parse first (wave_encode_cases.checked).
Families S, X and Z run once more with the emulator's lanes in DESCENDING order (which lane wins a store to a shared LDS address is the
hardware's choice; ascending order only ever answers "the highest"), and S and Z through the dictionary encoder against its twin
(tests/dict_encode_ref.py).  The -m gpu twin is tests/test_gpu_wave_encode_cases.py."""
import ctypes as C

import numpy as np
import pytest

import dict_encode_cases as dcases
import dict_encode_ref as ref
import emu_helpers as emu
import encoder_cases as ec
import wave_encode_cases as wc
from encoder_cases import check_bit_exact, check_limited

FORMS = [f for f in ec.EMU_FORMS if f[0].startswith("fast-")]
FORM = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
WAVE = dict()


def _encode(kwargs):
    return lambda b, c: ec.emu_encode(kwargs, b, c)


def _stats(run):
    """the counters that run() moved"""
    emu.enc_stats()
    run()
    return emu.enc_stats()


def _alone(case, kwargs=WAVE):
    """the counters of one case encoded alone (bit-exact on the way)"""
    return _stats(lambda: check_bit_exact(_encode(kwargs), [case], case[0]))


def _idle_tail(cases):
    """the cases, so many that the last workgroup of five has idle wavefronts"""
    return cases if len(cases) % 5 else cases + cases[:1]


def test_slot_names_are_the_kernels():
    assert len(emu.enc_stats()) == len(wc.SLOTS) == len(set(wc.SLOTS))
    emu.lib().emu_enc_stat_name.restype = C.c_char_p
    assert [emu.lib().emu_enc_stat_name(i).decode() for i in range(len(wc.SLOTS))] == wc.SLOTS


def test_block_counts():
    """every family is there in the 64k variant, S and X also in the generic one, and the generic blocks stay a few dozen"""
    generic = [c for n in wc.NAMES for c in wc.family(n).cases if len(c[1]) >= ec.LIMIT_64K]
    assert 10 <= len(generic) <= 48, len(generic)
    assert {c[0][0] for c in generic} == {"S", "X"}
    for n in wc.NAMES:
        assert any(len(c[1]) < ec.LIMIT_64K for c in wc.family(n).cases), n


# ---- the families ----------------------------------------------------------------------------------------------------------------------
@FORM
@pytest.mark.parametrize("name", wc.NAMES)
def test_family_bit_exact(oracle, name, form):
    cases = wc.checked(oracle, name)
    check_bit_exact(_encode(form[3]), _idle_tail(cases) if form[3] and form[3].get("wg5") else cases, (name, form[0]))


@pytest.mark.parametrize("name", wc.NAMES)
def test_family_reaches_its_branches(oracle, name):
    cases = wc.checked(oracle, name)
    kwargs = None if name == "H" else WAVE                                # (the hand-over rule runs in the first of the two launches only)
    st = _stats(lambda: check_bit_exact(_encode(kwargs), cases, name))
    wc.assert_moves(wc.family(name), st)
    for slot in wc.UNREACHED:
        assert st[wc.S[slot]] == 0, ("reached", slot)


@pytest.mark.parametrize("name", wc.NAMES)
def test_threshold_pairs_differ_as_declared(oracle, name):
    f, cases = wc.family(name), wc.checked(oracle, name)
    kwargs = None if name == "H" else WAVE
    alone = {i: _alone(cases[i], kwargs) for i in sorted({i for a, b, _ in f.pairs for i in (a, b)})}
    wc.assert_pairs(f, alone)


def test_every_slot_is_asserted_somewhere():
    moved = {s for n in wc.NAMES for s in wc.family(n).moves} | set(wc.LIMITED_MOVES) | set(wc.GENERIC_MOVES)
    assert moved >= set(wc.SLOTS) - set(wc.UNREACHED), sorted(set(wc.SLOTS) - moved - set(wc.UNREACHED))


@pytest.mark.parametrize("name", wc.DESCENDING)
def test_family_with_lanes_in_descending_order(oracle, name):
    """same bytes, same branches, whichever lane's store to a shared bucket lands last"""
    cases = wc.checked(oracle, name)
    with emu.descending_lanes():
        st = _stats(lambda: check_bit_exact(_encode(WAVE), cases, (name, "descending")))
        wc.assert_moves(wc.family(name), st)
        f = wc.family(name)
        alone = {i: _alone(cases[i]) for i in sorted({i for a, b, _ in f.pairs for i in (a, b)})}
        wc.assert_pairs(f, alone)
        check_bit_exact(_encode(dict(wg5=True)), _idle_tail(cases), (name, "descending, five per workgroup"))


def test_generic_blocks_reach_the_generic_step(oracle):
    """the generic blocks of S and X alone: the shared-bucket slots move there too"""
    cases = [c for n in ("S", "X") for c in wc.checked(oracle, n) if len(c[1]) >= ec.LIMIT_64K]
    st = _stats(lambda: check_bit_exact(_encode(WAVE), cases, "generic"))
    for slot in wc.GENERIC_MOVES:
        assert st[wc.S[slot]] > 0, ("counter never moved", slot)
    assert st[wc.S["FirstWords"]] == 0 and st[wc.S["Pos0Search"]] == 0


def test_hand_over_blocks_are_handed_over_as_built(oracle):
    f, cases = wc.family("H"), wc.checked(oracle, "H")
    res, dst, deferred = emu.encode_two_launches([c[1] for c in cases])
    assert [bool(d) for d in deferred] == f.handed_over, list(deferred)
    for i, (name, block, want, _) in enumerate(cases):
        assert res[i] == len(want) and np.array_equal(dst[i, :res[i]], want), name


# ---- family E at every capacity ---------------------------------------------------------------------------------------------------------
@FORM
def test_one_store_emit_output_limit(oracle, form):
    """every capacity from 12 below to 4 above the compressed size: the oracle's return value, its bytes, nothing behind the capacity"""
    limited = wc.limited_cases(oracle, wc.checked(oracle, "E"))
    st = _stats(lambda: check_limited(_encode(form[3]), limited, ("E limited", form[0])))
    if form[0] == "fast-wave":
        for slot in wc.LIMITED_MOVES:
            assert st[wc.S[slot]] > 0, ("counter never moved", slot)


# ---- the dictionary encoder -----------------------------------------------------------------------------------------------------------------
def _dict_stats(run):
    L = dcases.emu()
    st = (C.c_ulonglong * 16)()
    L.emu_encdict_stats(st, 1)
    emu.enc_stats(library=L)
    run()
    L.emu_encdict_stats(st, 1)
    return list(st), emu.enc_stats(library=L)


def _dict_encode(blocks, dic, wpg):
    """lz4hip_encode_batch_dict_device under the emulator over rows at a stride: (results, rows)"""
    n = len(blocks)
    sl = np.array([len(b) for b in blocks], np.int32)
    cp = np.array([ref.bound(len(b)) for b in blocks], np.int32)
    src = np.full((n, int(sl.max()) + 16), 0x11, np.uint8)
    for i, b in enumerate(blocks):
        src[i, :len(b)] = b
    dst = np.full((n, int(cp.max()) + 64), 0xA5, np.uint8)
    res = np.full(n, -12345678, np.int32)
    store = np.full(16384 + 256, 0x77, np.uint8)
    lead = (-store.ctypes.data) % 16 + 64
    dic = np.ascontiguousarray(dic)
    dcases.emu().emu_encdict_encode(C.c_void_p(src.ctypes.data), None, C.c_int64(src.strides[0]), C.c_void_p(sl.ctypes.data), C.c_void_p(dst.ctypes.data), None,
                                    C.c_int64(dst.strides[0]), C.c_void_p(cp.ctypes.data), C.c_void_p(res.ctypes.data), C.c_int64(n), wpg,
                                    C.c_void_p(dic.ctypes.data), C.c_int64(dic.size), C.c_void_p(store.ctypes.data + lead))
    assert (store[:lead] == 0x77).all() and (store[lead + 16384:] == 0x77).all(), "wrote outside the scratch"
    return res, dst


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("kind", wc.DICT_KINDS)
@pytest.mark.parametrize("name", wc.DICT)
def test_family_through_the_dictionary_encoder(oracle, name, kind, order):
    """each block against a dictionary, the twin's result and bytes; the dictionary that holds a word of every shared bucket makes the
    buckets' old entries point into it: the restore slots move next to the dictionary mode's own"""
    cases = wc.dict_cases(oracle, name)
    dic = wc.dictionary(kind, [c[1] for c in cases])
    blocks = [c[1] for c in cases]
    want = [ref.encode(b.tobytes(), dic.tobytes()) for b in blocks]

    def run():
        for wpg in (1, 5):
            wc.check_dict(lambda b: _dict_encode(b, dic, wpg), cases, want, (name, kind, wpg))
    if order == "descending":
        with emu.descending_lanes(dcases.emu()):
            dstat, st = _dict_stats(run)
    else:
        dstat, st = _dict_stats(run)
    assert dstat[dcases.BLOCKS] == 2 * len(blocks)
    for slot in ("Bucket2", "Rounds1", "CandLower") if name == "S" else ("Rounds1",):
        assert st[wc.S[slot]] > 0, ("counter never moved", slot)
    if kind == "shared-buckets":
        # every shared bucket is restored to a position inside the dictionary, but for the bucket of a block's first word (one per block at
        # the most), which the generic variant's insert of the first position has taken
        shared = sum(st[wc.S[k]] for k in ("Bucket2", "Bucket3", "Bucket4"))
        assert st[wc.S["RestoreIntoDict"]] >= shared - 2 * len(blocks) > 0 and dstat[dcases.WORD_IN_DICT] > 0, (st[wc.S["RestoreIntoDict"]], shared, dstat)
    else:
        assert dstat[dcases.CANDIDATE] == 0, dstat


# ---- the comparisons themselves ---------------------------------------------------------------------------------------------------------------
def test_comparison_helpers_refuse_a_wrong_byte(oracle):
    cases = wc.checked(oracle, "Z")[:2]

    def wrong(where):
        def encode(blocks, caps):
            res, dst = emu.encode(blocks, caps=caps)
            if where == "byte":
                dst[1, res[1] // 2] ^= 1
            elif where == "result":
                res[0] += 1
            else:
                dst[0, ec.compress_bound(len(blocks[0])) if caps is None else caps[0]] = 0
            return res, dst
        return encode
    check_bit_exact(emu.encode, cases, "right")
    limited = wc.limited_cases(oracle, cases)
    check_limited(lambda b, c: emu.encode(b, caps=c), limited, "right")
    for where in ("byte", "result", "guard"):
        with pytest.raises(AssertionError):
            check_bit_exact(wrong(where), cases, where)
        with pytest.raises(AssertionError):
            check_limited(wrong(where), limited[-2:], where)
    dic = wc.dictionary("disjoint", [c[1] for c in cases])
    want = [ref.encode(c[1].tobytes(), dic.tobytes()) for c in cases]
    wc.check_dict(lambda b: _dict_encode(b, dic, 1), cases, want, "right")
    for where in ("byte", "result"):
        def bad(b):
            res, dst = _dict_encode(b, dic, 1)
            if where == "byte":
                dst[1, 3] ^= 1
            else:
                res[0] -= 1
            return res, dst
        with pytest.raises(AssertionError):
            wc.check_dict(bad, cases, want, where)


def test_moved_counters_refuse_plain_generator_output(oracle):
    """4 KiB blocks of generator output are encoded right and do not move the counters of the families built for rare branches"""
    rows = oracle.gen(2, 77, 0, 8, length=4096)
    cases = [(f"plain {i}", r, oracle.compress(r)) for i, r in enumerate(rows)]
    st = _stats(lambda: check_bit_exact(_encode(WAVE), cases, "plain"))
    for name in ("S", "Z", "H"):
        with pytest.raises(AssertionError, match="counter never moved"):
            wc.assert_moves(wc.family(name), st)
