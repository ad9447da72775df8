"""The lane decoder's staged flush (lz4hip_decode_lane4.hpp, T2a .. T2d) under the CPU SIMT emulator: the built blocks of
tests/lane_flush_cases.py through every form of the kernel the emulator library instantiates, against the CPU codec.  The -m gpu twin is
tests/test_gpu_lane_flush_order.py."""
import pytest

import emu_helpers as emu
import lane_flush_cases as cases

# one block per lane (the default configuration), the persistent grid with one and with two wavefronts, workgroups of four wavefronts with
# dual ring stores and with wrapped rows (the wrapped-row instantiation)
FORMS = {"lane": dict(lane=59192, gen=4), "persistent-1": dict(lane=1, gen=5), "persistent-2": dict(lane=2, gen=5),
         "wg4": dict(lane=1, gen=6), "wg4-wrapped": dict(lane=2, gen=6)}


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["lengths_and_far", "near_then_far", "identical", "different_lengths"])
def test_staged_flush_matches_cpu_codec(oracle, name, form, known):
    cases.check(oracle, name, known, lambda comps, caps, k: emu.decode(comps, caps, known=k, **FORMS[form]))


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
def test_staged_flush_with_fewer_records_than_units(oracle, known):
    """the 'starved' build (four flush records per iteration): most lanes that want to flush find no record and wait"""
    with emu.starved_flush():
        cases.check(oracle, "identical", known, lambda comps, caps, k: emu.decode(comps, caps, known=k, **FORMS["lane"]))
