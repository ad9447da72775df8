"""The wavefront decoder (lz4hip_decode.hpp) under the CPU SIMT emulator: the built blocks of tests/wave_decode_cases.py, family by family,
with 1 and with 4 wavefronts per workgroup, against the CPU codec -- and the emulator's LZ4HIP_STAT counters as the proof that a family
reached the path it was built for: a block that misses its path fails here, on the CPU.  The -m gpu twin is
tests/test_gpu_wave_decode_cases.py."""
import ctypes as C

import pytest

import emu_helpers as emu
import wave_decode_cases as cases


def _decode(wpg):
    return lambda comps, caps, known, lens: emu.decode(comps, caps, known=known, src_lens=lens, waves_per_group=wpg)


def _stats(run):
    """the counters that run() moved"""
    st = (C.c_ulonglong * cases.N_SLOTS)()
    emu.lib().emu_stats(st, 1)
    run()
    emu.lib().emu_stats(st, 1)
    return list(st)


def family_stats(oracle, name, fam=None):
    """known -> the counters of the whole family decoded in one batch (results and bytes are checked on the way)"""
    return {known: _stats(lambda: cases.check(oracle, name, known, _decode(1), fam=fam)) for known in (True, False)}


def pair_stats(oracle, name, fam=None):
    """(item, known) -> the counters of each item of a pair decoded alone"""
    f = cases.family(name) if fam is None else fam
    return {(i, known): _stats(lambda: cases.check(oracle, name, known, _decode(1), only=[i], fam=fam))
            for a, b, _, known in f.pairs for i in (a, b)}


def assert_moves(f, name, st):
    for known in (True, False):
        for slot in f.moves + ([] if known else f.moves_unknown):
            assert st[known][slot] > 0, (name, known, "counter never moved", slot)


def assert_pairs(f, name, alone):
    for a, b, slot, known in f.pairs:
        x, y = alone[a, known][slot], alone[b, known][slot]
        assert x < y, (name, known, "pair not in the declared direction", "items", a, b, "slot", slot, x, y)


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("wpg", [1, 4])
@pytest.mark.parametrize("name", cases.NAMES)
def test_built_streams_match_cpu_codec(oracle, name, wpg, known):
    cases.check(oracle, name, known, _decode(wpg))


@pytest.mark.parametrize("name", cases.NAMES)
def test_family_reaches_its_paths(oracle, name):
    """the family's counters moved, and each of its pairs differs in the declared direction"""
    f = cases.family(name)
    assert_moves(f, name, family_stats(oracle, name))
    assert_pairs(f, name, pair_stats(oracle, name))


# Plain encoder output is bursts of short sequences, short-path and general-path sequences near a block's end and re-bases of the
# window: it moves those counters and not the ones of a long copy, a register fill, a failed burst, or a source behind the mirror or in
# memory.  The three families that name only counters of the first kind are gated by their pairs alone.
PLAIN_MOVES_ALL = ("short_path", "short_input_edges", "window")
MOVES_GATE = [n for n in cases.NAMES if n not in PLAIN_MOVES_ALL]


@pytest.mark.parametrize("name", MOVES_GATE)
def test_moved_counters_refuse_plain_encoder_output(oracle, name):
    """the counters gate: the family's shape filled with plain encoder output decodes right, and its named counters do not all move"""
    g = cases.plain(oracle, name)
    st = family_stats(oracle, name, g)                       # (bytes and results hold: outside the expectation below)
    with pytest.raises(AssertionError, match="counter never moved"):
        assert_moves(g, name, st)


@pytest.mark.parametrize("name", cases.NAMES)
def test_pairs_refuse_plain_encoder_output(oracle, name):
    """... and its pairs do not all differ in the declared direction"""
    g = cases.plain(oracle, name)
    alone = pair_stats(oracle, name, g)
    with pytest.raises(AssertionError, match="pair not in the declared direction"):
        assert_pairs(g, name, alone)
