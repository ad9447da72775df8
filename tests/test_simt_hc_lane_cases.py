"""The LZ4HC lane encoder over chains with shared lengths (lz4hip_hc_lcp.hpp) and its two table builders under the CPU SIMT emulator: the
builders' table against a plain reference, entry by entry, and the built blocks of tests/hc_lane_cases.py family by family, bit-exact
against the oracle -- with the emulator's LZ4HIP_STAT_HC counters as the proof that a family reached the branch it was built for: a
block that misses its threshold fails here, on the CPU.  Every expectation of a built block is asserted against the oracle's own parse
first (hc_lane_cases.checked).  The -m gpu twin is tests/test_gpu_hc_lane_cases.py."""
import numpy as np
import pytest

import emu_helpers as emu
import encoder_cases as ec
import hc_lane_cases as hl
from encoder_cases import check_bit_exact, check_limited

LCP = dict(hc=True, lcp=True, groups=1)
CONV = dict(hc=True, lane=True, conv=True)


def _encode(kwargs):
    return lambda b, c: emu.encode(b, caps=c, **kwargs)


def _stats(run):
    """the counters that run() moved"""
    emu.hc_stats()
    run()
    return emu.hc_stats()


def _alone(case, kwargs=LCP):
    """the counters of one case encoded alone (bit-exact on the way)"""
    return _stats(lambda: check_bit_exact(_encode(kwargs), [case], case[0]))


def test_slot_names_are_the_kernels():
    assert len(emu.hc_stats()) == len(hl.SLOTS) == len(set(hl.SLOTS))


# ---- the builders' table ---------------------------------------------------------------------------------------------------------------
def test_builders_table_matches_plain_reference():
    """every entry of every block: chain and length everywhere, y where the length is below both caps, entry 0, the poison behind n - 4"""
    blocks = hl.table_blocks()
    assert {len(b) for _, b in blocks} >= set(hl.TABLE_SMALL) | set(hl.TABLE_EDGES) | {65536}
    emu.hc_stats()
    for i in range(0, len(blocks), 32):
        part = blocks[i:i + 32]
        tables = emu.hc_lcp_tables([b for _, b in part])
        for (name, block), table in zip(part, tables):
            hl.check_table(block, table, name)
    st = emu.hc_stats()
    for slot in hl.TABLE_MOVES:
        assert st[hl.S[slot]] > 0, ("counter never moved", slot)
    named = dict(blocks)
    alone = {name: _stats(lambda: emu.hc_lcp_tables([named[name]])) for a, b, _ in hl.TABLE_PAIRS for name in (a, b)}
    for a, b, slot in hl.TABLE_PAIRS:
        assert alone[a][hl.S[slot]] < alone[b][hl.S[slot]], ("pair not in the declared direction", a, b, slot, alone[a][hl.S[slot]], alone[b][hl.S[slot]])


def test_table_reference_refuses_a_wrong_entry():
    """the comparison itself: one length off by one, one chain entry, one y, one entry behind the end"""
    name, block = next(x for x in hl.table_blocks() if x[0] == "n=261 shared-lengths")
    table = emu.hc_lcp_tables([block])[0]
    hl.check_table(block, table, name)
    chain, length, y, y_valid = hl.table_reference(block)
    at = int(np.flatnonzero(y_valid[1:])[0]) + 1
    for p, delta in ((100, 1 << 16), (100, 1), (at, 1 << 24), (len(block) - 3, 1)):
        bad = table.copy()
        bad[p] += np.uint32(delta)
        with pytest.raises(AssertionError):
            hl.check_table(block, bad, name)


# ---- the families ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hl.NAMES)
def test_family_bit_exact_and_reaches_its_branches(oracle, name):
    cases = hl.checked(oracle, name)
    st = _stats(lambda: check_bit_exact(_encode(LCP), cases, name))
    hl.assert_moves(hl.family(name), st)


@pytest.mark.parametrize("name", hl.NAMES)
def test_threshold_pairs_differ_as_declared(oracle, name):
    f, cases = hl.family(name), hl.checked(oracle, name)
    alone = {i: _alone(cases[i]) for i in sorted({i for a, b, _ in f.pairs for i in (a, b)} | {a for a, _ in f.zero})}
    hl.assert_pairs(f, alone)


def test_every_slot_is_asserted_somewhere():
    moved = {s for n in hl.NAMES for s in hl.family(n).moves} | set(hl.TABLE_MOVES) | set(hl.REFUSALS)
    paired = {s for n in hl.NAMES for _, _, s in hl.family(n).pairs} | {s for _, _, s in hl.TABLE_PAIRS}
    assert moved >= set(hl.SLOTS) - set(hl.UNREACHED), sorted(set(hl.SLOTS) - moved)
    assert paired >= set(hl.TWO_SIDED), sorted(set(hl.TWO_SIDED) - paired)


@pytest.mark.parametrize("kwargs", [LCP, CONV], ids=["chains-with-shared-lengths", "large-block-lane-kernel"])
def test_parse_blocks_reach_the_branch_they_were_chosen_for(oracle, kwargs):
    """family P, block by block, for both kernels that include lz4hip_hc_parse.inc"""
    f, cases = hl.family("P"), hl.checked(oracle, "P")
    for i, slot in f.slot_of:
        assert _alone(cases[i], kwargs)[hl.S[slot]] > 0, (cases[i][0], "never reached", slot)


@pytest.mark.parametrize("kwargs", [LCP, CONV], ids=["chains-with-shared-lengths", "large-block-lane-kernel"])
def test_parse_blocks_output_limit(oracle, kwargs):
    """every capacity from 8 below to 2 above the compressed size: the oracle's return value, its bytes, nothing behind the capacity; both
    refusals of the sequence emit are reached, and the kernels' own third one, which keeps the length bytes of a long match inside the capacity"""
    limited = hl.limited_cases(oracle, hl.family("P"))
    st = _stats(lambda: check_limited(_encode(kwargs), limited, "P limited"))
    for slot in hl.REFUSALS:
        assert st[hl.S[slot]] > 0, ("counter never moved", slot)


def test_row_in_front_of_the_block_is_not_read(oracle):
    """the candidate at the block's position 3: three bytes backwards and no further, whatever the row in front ends with"""
    f = hl.family("B")
    case = hl.checked(oracle, "B")[f.start[3]]
    front = ("B row in front", f.front_row, oracle.compress(f.front_row, hc=True))
    rows = [front, case, front]
    assert len(front[1]) == max(len(r[1]) for r in rows) and front[1][-1] == f.front_byte
    st = _stats(lambda: check_bit_exact(lambda b, c: emu.encode(b, caps=c, pad=0, **LCP), rows, "row stride = the front row's length"))
    assert st[hl.S["B_StopStart"]] > 0


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_all_blocks_in_one_launch(oracle, order):
    """one wavefront, 64 lanes taking blocks from the counter: a lane meets the blocks of different families one after the other, in two
    orders -- what it keeps between blocks (the window's position, the cached probe, the repeat state) meets every shape"""
    cases = hl.everything(oracle)
    st = _stats(lambda: check_bit_exact(_encode(LCP), cases if order == "forward" else cases[::-1], order))
    for slot in hl.UNREACHED:                                             # (the branch the parse cannot take: hc_lane_cases.UNREACHED)
        assert st[hl.S[slot]] == 0, ("reached", slot)


OTHER_FORMS = [f for f in ec.EMU_FORMS if f[0] in ("hc-lane-natural-chains", "hc-wave-heads16")] + [("hc-lane-large-blocks on small blocks", True, ec.ANY, CONV)]


@pytest.mark.parametrize("form", OTHER_FORMS, ids=[f[0] for f in OTHER_FORMS])
def test_all_blocks_through_the_other_encoders(oracle, form):
    st = _stats(lambda: check_bit_exact(lambda b, c: ec.emu_encode(form[3], b, c), hl.everything(oracle), form[0]))
    for slot in hl.UNREACHED:
        assert st[hl.S[slot]] == 0, ("reached", slot)


# ---- the counters gate ----------------------------------------------------------------------------------------------------------------
GATED = [n for n in hl.NAMES if n not in hl.PLAIN_MOVES_ALL]


@pytest.mark.parametrize("name", GATED)
def test_moved_counters_refuse_plain_generator_output(oracle, name):
    """4 KiB blocks of generator output are encoded right and do not move all the counters the family names"""
    rows = oracle.gen(2, 77, 0, 8, length=4096)
    cases = [(f"plain {i}", r, oracle.compress(r, hc=True)) for i, r in enumerate(rows)]
    st = _stats(lambda: check_bit_exact(_encode(LCP), cases, "plain"))
    with pytest.raises(AssertionError, match="counter never moved"):
        hl.assert_moves(hl.family(name), st)
