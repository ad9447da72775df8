"""The predicates the lane decoder makes once per iteration and combines as lane masks (lz4hip_decode_lane4.hpp: L4_COND / L4_LANE, the class
word of the parsed-ahead sequence, the merged test against the end of the source) under the CPU SIMT emulator: the built blocks of
tests/lane_predicate_cases.py, one wavefront per family, through every form of the kernel the emulator library instantiates, against the CPU
codec -- and the emulator's counters as the proof that a family reached the branch it was built for.  The -m gpu twin is
tests/test_gpu_lane_predicates.py."""
import pytest

import lane_decode_cases as base
import lane_predicate_cases as cases
from test_simt_lane_decode_cases import _decode, _stats, assert_moves, assert_pairs
from test_simt_lane_flush_order import FORMS


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", cases.NAMES)
def test_built_blocks_match_cpu_codec(oracle, name, form, known):
    cases.check(oracle, name, known, _decode(form))


@pytest.mark.parametrize("name", cases.NAMES)
def test_family_reaches_its_branches(oracle, name):
    """the family's counters moved, and each of its pairs, its two items decoded alone, differs in the declared direction"""
    f = cases.family(name)
    st = {known: _stats(lambda: cases.check(oracle, name, known, _decode("lane"))) for known in (True, False)}
    assert_moves(f, name, st)
    alone = {(i, known): _stats(lambda: cases.check(oracle, name, known, _decode("lane"), only=[i])) for a, b, _, known in f.pairs for i in (a, b)}
    assert_pairs(f, name, alone)


def test_refills_at_both_sides_of_a_piece():
    """by the cursor model: the cursor rests at offset 31 of the window (no refill), a refill happens at 32, for the low and the high half of the
    sector, and at both for the piece that is a block's last"""
    views, crossings = cases.refill_reach(cases.family("refills"))
    assert {30, 31} <= views and max(views) <= 31
    assert {(32, half, last) for half in (False, True) for last in (False, True)} <= crossings
    assert {(33, half, True) for half in (False, True)} <= crossings


def test_offset_field_pick_stays_on_the_fast_path(oracle):
    """the eleven blocks that differ only in where the offset field lies in the view, each decoded alone, take the trap equally often: a wrong
    pick of the field's dwords is refused by the fast path's own tests and parsed again byte by byte, so the bytes alone would not show it"""
    f = cases.family("tokens")
    idx = [i for i, n in enumerate(f.names) if n.startswith("T offset field")]
    assert len(idx) == 11
    for known in (True, False):
        traps = {f.names[i]: _stats(lambda: cases.check(oracle, "tokens", known, _decode("lane"), only=[i]))[base.TRAP_TOKEN] for i in idx}
        assert len(set(traps.values())) == 1, (known, traps)
