"""The lane decoder's parser and ring logic (lz4hip_decode_lane4.hpp: T4 / T4x, T1c, T3, T5, B3 .. B5) under the CPU SIMT emulator: the built
blocks of tests/lane_decode_cases.py, family by family, through every form of the kernel the emulator library instantiates, against the CPU
codec -- and the emulator's counters (LZ4HIP_STAT, LZ4HIP_STAT_L4) as the proof that a family reached the path it was built for: a block
that misses its path fails here, on the CPU.  The -m gpu twin is tests/test_gpu_lane_decode_cases.py."""
import ctypes as C

import pytest

import emu_helpers as emu
import lane_decode_cases as cases
import wave_decode_cases as wave_cases
from test_simt_lane_flush_order import FORMS
from test_simt_lane_window import decode as window_decode


def _decode(form):
    """row i of a batch at alignment i % 64 of a 64-byte sector: where a lane's input arrives, and with it the iteration in which it flushes,
    follows from the batch alone, so the counters do too"""
    return lambda comps, caps, known: window_decode(comps, caps, known, 1, 0, **FORMS[form])


def _stats(run):
    """the counters that run() moved: LZ4HIP_STAT's 40 slots, then LZ4HIP_STAT_L4's"""
    st, l4 = (C.c_ulonglong * 40)(), (C.c_ulonglong * 32)()
    emu.lib().emu_stats(st, 1)
    emu.lib().emu_l4_stats(l4, 1)
    run()
    emu.lib().emu_stats(st, 1)
    assert emu.lib().emu_l4_stats(l4, 1) == cases.N_L4
    return list(st) + list(l4)


def family_stats(oracle, name, fam=None, form="lane"):
    """known -> the counters of the whole family (results and bytes are checked on the way)"""
    return {known: _stats(lambda: cases.check(oracle, name, known, _decode(form), fam=fam)) for known in (True, False)}


def pair_stats(oracle, name, fam=None):
    """(item, known) -> the counters of each item of a pair decoded alone"""
    f = cases.family(name) if fam is None else fam
    return {(i, known): _stats(lambda: cases.check(oracle, name, known, _decode("lane"), only=[i], fam=fam))
            for a, b, _, known in f.pairs for i in (a, b)}


def assert_moves(f, name, st):
    for known in (True, False):
        for slot in f.moves + (f.moves_known if known else f.moves_unknown):
            assert st[known][slot] > 0, (name, known, "counter never moved", slot)


def assert_pairs(f, name, alone):
    for a, b, slot, known in f.pairs:
        x, y = alone[a, known][slot], alone[b, known][slot]
        assert x < y, (name, known, "pair not in the declared direction", f.names[a], f.names[b], "slot", slot, x, y)


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", cases.NAMES)
def test_built_blocks_match_cpu_codec(oracle, name, form, known):
    cases.check(oracle, name, known, _decode(form))


@pytest.mark.parametrize("name", cases.NAMES)
def test_family_reaches_its_paths(oracle, name):
    """the family's counters moved, and each of its pairs differs in the declared direction"""
    f = cases.family(name)
    assert bool(f.pairs) == (name not in NO_PAIRS) and f.moves
    assert_moves(f, name, family_stats(oracle, name))
    assert_pairs(f, name, pair_stats(oracle, name))


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
def test_ring_room_with_fewer_records_than_units(oracle, known):
    """family M in the 'starved' build: most lanes that want to flush find no record, run their rings full and wait for room"""
    with emu.starved_flush():
        st = _stats(lambda: cases.check(oracle, "M", known, _decode("lane")))
    assert st[cases.NO_ROOM_COPY] > 0 and st[cases.NO_ROOM_PROMOTE] > 0


# Plain encoder output of the test's repetitive rows is literal runs and near and far matches of many lengths: it takes the fast path, the trap
# near the end of the source and a final run, promotes to Lit, Near and Far, doubles and wraps the ring.  It never meets a refused offset, a
# length byte of 255, a far match whose source is not flushed or a lane without room.  A family that names only counters of the first kind
# is gated by its pairs alone.
PLAIN_MOVES_ALL = ("C", "N", "D")
MOVES_GATE = [n for n in cases.NAMES if n not in PLAIN_MOVES_ALL]
NO_PAIRS = ("C", "M", "S")                                   # families of sweeps and of one long batch: gated by their counters alone
PAIRS_GATE = [n for n in cases.NAMES if n not in NO_PAIRS]


@pytest.mark.parametrize("name", MOVES_GATE)
def test_moved_counters_refuse_plain_encoder_output(oracle, name):
    """the counters gate: the family's shape filled with plain encoder output decodes right, and its named counters do not all move"""
    g = cases.plain(oracle, name)
    st = family_stats(oracle, name, g)                       # (bytes and results hold: outside the expectation below)
    with pytest.raises(AssertionError, match="counter never moved"):
        assert_moves(g, name, st)


@pytest.mark.parametrize("name", PAIRS_GATE)
def test_pairs_refuse_plain_encoder_output(oracle, name):
    """... and its pairs do not all differ in the declared direction"""
    g = cases.plain(oracle, name)
    alone = pair_stats(oracle, name, g)
    with pytest.raises(AssertionError, match="pair not in the declared direction"):
        assert_pairs(g, name, alone)


# ---- cross-runs, bytes and results only -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("wpg", [1, 4])
@pytest.mark.parametrize("name", cases.NAMES)
def test_lane_families_through_the_wavefront_decoder(oracle, name, wpg, known):
    cases.check(oracle, name, known, lambda comps, caps, k: emu.decode(comps, caps, known=k, waves_per_group=wpg))


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", wave_cases.NAMES)
def test_wave_families_through_the_lane_decoder(oracle, name, form, known):
    # (holes_keep: a refused block's finished bytes stay in the lane's ring, so such a row is compared by its result.  A family of more than
    #  130 blocks is dealt out among the forms, every fifth block to each: the emulator's time)
    n, first = len(wave_cases.family(name).items), list(FORMS).index(form)
    only = None if n <= 130 else range(first, n, len(FORMS))
    wave_cases.check(oracle, name, known, lambda comps, caps, k, lens: emu.decode(comps, caps, known=k, src_lens=lens, **FORMS[form]), only=only, holes_keep=True)
