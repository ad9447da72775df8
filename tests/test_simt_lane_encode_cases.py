"""The fast lane encoder (lz4hip_encode_lane.hpp) under the CPU SIMT emulator over the built blocks of tests/lane_encode_cases.py, family by
family: bit-exact against the oracle with guard bytes through the two emulator forms that run the kernel (fast-lane, and the second of
fast-two-launches), with the emulator's LZ4HIP_STAT_LANE counters as the proof that a family reached the branches it was built for and
that the two blocks of a threshold pair stand on its two sides.  Every expectation of a built block is asserted against the oracle's
own parse first (lane_encode_cases.checked).  Both launches are one wavefront, and the emulator switches fibers only at cross-lane
operations, of which the kernel has none: lane 0 pulls every block of a call from the counter, in order, so a call IS one lane's
sequence of blocks, and family Q's tests are about exactly that.  The -m gpu twin is tests/test_gpu_lane_encode_cases.py."""
import ctypes as C

import pytest

import emu_helpers as emu
import encoder_cases as ec
import lane_encode_cases as lc
from encoder_cases import check_bit_exact, check_limited
from wave_encode_cases import assert_moves, assert_pairs

FORMS = [f for f in ec.EMU_FORMS if f[0] in ("fast-lane", "fast-two-launches")]
FORM = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
LANE = dict(lane=True)


def _encode(kwargs):
    return lambda b, c: ec.emu_encode(kwargs, b, c)


def _stats(run):
    """the counters that run() moved"""
    emu.lane_enc_stats()
    run()
    return emu.lane_enc_stats()


def _alone(case):
    """the counters of one case encoded alone (bit-exact on the way)"""
    return _stats(lambda: check_bit_exact(_encode(LANE), [case], case[0]))


def test_slot_names_are_the_kernels():
    assert len(emu.lane_enc_stats()) == len(lc.SLOTS) == len(set(lc.SLOTS))
    emu.lib().emu_lane_enc_stat_name.restype = C.c_char_p
    assert [emu.lib().emu_lane_enc_stat_name(i).decode() for i in range(len(lc.SLOTS))] == lc.SLOTS


def test_block_counts():
    """every family is there in the 64k variant, K, N and L also in the generic one, and the generic blocks stay a dozen"""
    generic = [c for n in lc.NAMES for c in lc.family(n).cases if len(c[1]) >= ec.LIMIT_64K]
    assert 3 <= len(generic) <= 16, len(generic)
    assert {c[0].split()[0] for c in generic} == set(lc.GENERIC) | set(lc.LARGE)
    for n in lc.NAMES:
        assert n in lc.LARGE or any(len(c[1]) < ec.LIMIT_64K for c in lc.family(n).cases), n
    assert all(len(c[1]) <= 200 for c in lc.family("Q").cases)


# ---- the families ----------------------------------------------------------------------------------------------------------------------
@FORM
@pytest.mark.parametrize("name", lc.NAMES)
def test_family_bit_exact(oracle, name, form):
    check_bit_exact(_encode(form[3]), lc.checked(oracle, name), (name, form[0]))


@pytest.mark.parametrize("name", lc.NAMES)
def test_family_reaches_its_branches(oracle, name):
    cases = lc.checked(oracle, name)
    st = _stats(lambda: check_bit_exact(_encode(LANE), cases, name))
    assert_moves(lc.family(name), st, lc.S)
    for slot in lc.UNREACHED:
        assert st[lc.S[slot]] == 0, ("reached", slot)


@pytest.mark.parametrize("name", lc.NAMES)
def test_threshold_pairs_differ_as_declared(oracle, name):
    f, cases = lc.family(name), lc.checked(oracle, name)
    alone = {i: _alone(cases[i]) for i in sorted({i for a, b, _ in f.pairs for i in (a, b)})}
    assert_pairs(f, alone, lc.S)


def test_every_slot_is_asserted_somewhere():
    moved = {s for n in lc.NAMES for s in lc.family(n).moves} | set(lc.LIMITED_MOVES) | set(lc.GENERIC_MOVES) | set(lc.R_MOVES) | {"Stamp63"}   # (Stamp63: test_one_lane_many_blocks)
    assert moved >= set(lc.SLOTS) - set(lc.UNREACHED), sorted(set(lc.SLOTS) - moved - set(lc.UNREACHED))
    assert not moved & set(lc.UNREACHED)


def test_generic_blocks_reach_the_generic_variant(oracle):
    """the generic blocks of K, N and L alone: the emit, count and copy slots move there too, and nothing of the 64k variant's table"""
    cases = [c for n in lc.GENERIC for c in lc.checked(oracle, n) if len(c[1]) >= ec.LIMIT_64K]
    st = _stats(lambda: check_bit_exact(_encode(LANE), cases, "generic"))
    for slot in lc.GENERIC_MOVES:
        assert st[lc.S[slot]] > 0, ("counter never moved", slot)
    assert st[lc.S["GenericClear"]] == len(cases)
    for slot in ("TableZeroed", "TableKept", "ZeroMissS", "OldMissS", "TagRejectS", "WordDiffersS"):
        assert st[lc.S[slot]] == 0, ("the 64k variant ran", slot)


def test_tag_field_ends(oracle):
    """family T (d), block by block: a product that differs from A's in bit 4 or 13 is rejected by the tag, twice (B against A's entry, A
    against B's), without a load; one that differs in bit 3 or 14 passes the tag and misses on the load, twice"""
    for case in lc.checked(oracle, "T"):
        site, form = case[0].split()[1], case[0].split(None, 2)[2]
        if not form.startswith("bit"):
            continue
        st = _alone(case)
        slot = "S" if site == "search" else "T"
        reject, differ = st[lc.S["TagRejectS"]] + st[lc.S["TagRejectT"]], st[lc.S["WordDiffersS"]] + st[lc.S["WordDiffersT"]]
        assert (reject, differ) == ((2, 0) if form in ("bit 4", "bit 13") else (0, 2)), (case[0], reject, differ)
        assert st[lc.S["TagReject" + slot]] + st[lc.S["WordDiffers" + slot]] >= 1, case[0]


# ---- family KS at every capacity -------------------------------------------------------------------------------------------------------------
@FORM
def test_one_store_emit_output_limit(oracle, form):
    """every capacity from 12 below to 16 above the compressed size and the full bound: the oracle's return value, its bytes, nothing behind the capacity"""
    limited = lc.limited_cases(oracle, lc.checked(oracle, "KS"))
    st = _stats(lambda: check_limited(_encode(form[3]), limited, ("KS limited", form[0])))
    if form[0] == "fast-lane":
        for slot in lc.LIMITED_MOVES:
            assert st[lc.S[slot]] > 0, ("counter never moved", slot)
        for slot in lc.UNREACHED:
            assert st[lc.S[slot]] == 0, ("reached", slot)


@FORM
def test_length_byte_refusals(oracle, form):
    """Family R at every capacity from 12 below to 16 above the compressed size: the oracle's return value -- where the reference has run
    past the capacity and returned 0 from a later test, the same 0 --, its bytes, nothing behind the capacity; each of the kernel's own
    three tests decides at one capacity at the least"""
    limited = lc.limited_cases(oracle, lc.checked(oracle, "R"))
    st = _stats(lambda: check_limited(_encode(form[3]), limited, ("R limited", form[0])))
    if form[0] == "fast-lane":
        for slot in lc.R_MOVES:
            assert st[lc.S[slot]] > 0, ("counter never moved", slot)


def test_capacity_decides_the_last_sequence(oracle):
    """One capacity per call.  The last sequence of a KS block is token, ll literals, offset, and five last literals behind their token:
    ll + 9 bytes from token_at, against the 16 the one store needs.  So for ll <= 6 (and at the zero-literal site) the sweep holds
    capacities at which the encode succeeds with that sequence plain BECAUSE OF cap, and others at which it is packed; from ll = 7 on
    every capacity that lets the block succeed lets the store in too, and a smaller one is refused by the literal check (lz4.c:663) before
    the emit is chosen -- there plain-by-cap must never be seen."""
    for case in lc.checked(oracle, "KS"):
        name, block, want, _ = case
        if lc.sweep_ll(name) is None:
            continue
        ll, zero_site = lc.sweep_ll(name)
        plain_ok = packed_ok = plain_any = 0
        for lim in lc.limited_cases(oracle, [case]):
            st = _stats(lambda: check_limited(_encode(LANE), [lim], lim[0]))
            plain = st[lc.S["ZeroPlainCap" if zero_site else "PlainCap"]]
            packed = st[lc.S["ZeroPacked"]] if zero_site else sum(st[lc.S[k]] for k in ("PackSh8To40", "PackSh48", "PackSh56", "PackSh64Up"))
            assert plain + packed <= 1, (lim[0], plain, packed)          # (the first sequence has a long literal run: plain by length)
            plain_ok += plain and lim[3] > 0
            packed_ok += packed and lim[3] > 0
            plain_any += plain
        assert packed_ok > 0, name
        assert (plain_ok > 0) == (ll <= 6) and (plain_any > 0) == (ll <= 6), (name, ll, plain_ok, plain_any)


# ---- family Q: one lane, many blocks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lc.Q_LENGTHS)
def test_one_lane_many_blocks(oracle, n):
    """n blocks of family Q through one lane: every row the oracle's, the table zeroed once per TABLE_BLOCKS blocks and not once more, a
    block under stamp 63 from n = 63 on, position 0 found out of an earlier block's entry, and the pair's second block probing the
    first's entry for its own word"""
    cases = lc.q_sequence(lc.checked(oracle, "Q"), n)
    st = _stats(lambda: check_bit_exact(_encode(LANE), cases, ("Q", n)))
    assert st[lc.S["TableZeroed"]] == -(-n // lc.TABLE_BLOCKS) and st[lc.S["TableZeroed"]] + st[lc.S["TableKept"]] == n, (n, st[:4])
    assert st[lc.S["Stamp63"]] == n // lc.TABLE_BLOCKS, (n, st[:4])
    assert st[lc.S["OldHitS"]] > 0 and st[lc.S["OldHitT"]] > 0 and st[lc.S["OldTagEqualS"]] > 0 and st[lc.S["OldTagEqualT"]] > 0
    assert st[lc.S["GenericClear"]] == 0


def test_pair_survivor_probes_the_first_blocks_entry(oracle):
    """A, then B, in one lane: both of B's words meet A's entries, tag equal, and miss"""
    cases = lc.checked(oracle, "Q")
    A, B = cases[-2], cases[-1]
    st = _stats(lambda: check_bit_exact(_encode(LANE), [A, B], "pair"))
    assert st[lc.S["OldTagEqualS"]] >= 1 and st[lc.S["OldTagEqualT"]] == 1 and st[lc.S["OldHitS"]] == 0 == st[lc.S["OldHitT"]], st
    st = _alone(B)
    assert st[lc.S["OldTagEqualS"]] == 0 == st[lc.S["OldTagEqualT"]] and st[lc.S["OldMissS"]] == 0


def test_generic_block_in_the_middle(oracle):
    """a generic block leaves raw positions in the table: the 64k block behind it zeroes the table, exactly once more"""
    q = lc.q_sequence(lc.checked(oracle, "Q"), 20)
    g = next(c for c in lc.checked(oracle, "L") if len(c[1]) >= ec.LIMIT_64K)
    base = _stats(lambda: check_bit_exact(_encode(LANE), q, "Q 20"))
    st = _stats(lambda: check_bit_exact(_encode(LANE), q[:10] + [g] + q[10:], "Q 20, a generic block in the middle"))
    assert base[lc.S["TableZeroed"]] == 1 and base[lc.S["GenericClear"]] == 0
    assert st[lc.S["TableZeroed"]] == 2 and st[lc.S["GenericClear"]] == 1 and st[lc.S["TableKept"]] == 18, st[:4]


# ---- the checks themselves ------------------------------------------------------------------------------------------------------------------------
def test_moved_counters_refuse_plain_generator_output(oracle):
    """4 KiB blocks of generator output are encoded right and do not move the counters of the families built for rare branches"""
    rows = oracle.gen(2, 77, 0, 8, length=4096)
    cases = [(f"plain {i}", r, oracle.compress(r)) for i, r in enumerate(rows)]
    st = _stats(lambda: check_bit_exact(_encode(LANE), cases, "plain"))
    for name in ("T", "Q"):
        with pytest.raises(AssertionError, match="counter never moved"):
            assert_moves(lc.family(name), st, lc.S)
