"""The lane decoder's input window (lz4hip_decode_lane4.hpp, T1a / T1b / B3: conditional assignments as moves under a lane mask on the device,
as selects here) under the CPU SIMT emulator: the built blocks of tests/lane_window_cases.py through every form of the kernel the emulator
library instantiates, against the CPU codec; and what those blocks reach, by the cursor model of the same file.  The -m gpu twin is
tests/test_gpu_lane_window.py."""
import ctypes as C

import numpy as np
import pytest

import emu_helpers as emu
import lane_window_cases as cases
from test_simt_lane_flush_order import FORMS

NAMES = ["skew", "refill", "cursor", "ends", "identical", "last_wave"]


def decode(comps, caps, known, step, first, lane, gen):
    """emu_helpers.decode over rows laid out at chosen alignments of a 64-byte sector"""
    raw, at, stride = cases.lay_out(comps, step, first)
    assert (raw.ctypes.data + at) % 64 == first
    sl, caps = np.array([len(c) for c in comps], np.int32), np.array(caps, np.int32)
    ds = int(caps.max()) + 64
    dst = np.full((len(comps), ds), 0xA5, np.uint8)
    res = np.full(len(comps), -12345678, np.int32)
    args = (int(known), C.c_void_p(raw.ctypes.data + at), C.c_int64(stride), emu._p(sl), emu._p(dst), C.c_int64(ds), emu._p(caps), emu._p(res), C.c_int64(len(comps)))
    if gen == 6:
        emu.lib().emu_decode_lane4_wg4(*args, 0, int(lane == 2))
    elif gen == 5:
        emu.lib().emu_decode_lane4_persistent(*args, 0, lane)
    else:
        emu.lib().emu_decode_lane4(*args, 0, lane)
    return res, dst


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_window_matches_cpu_codec(oracle, name, form, known):
    cases.check(oracle, name, known, lambda comps, caps, k, step, first: decode(comps, caps, k, step, first, **FORMS[form]))


def test_what_the_batches_reach():
    """by the cursor model: a refill at every d in 32 .. 47 for either half of the sector, the cursor at every byte 0 .. 31 of the window (dword
    index 0 .. 7, byte phase 0 .. 3: at 32 and beyond the next piece comes in first), every alignment of the source, every end of the source
    in its sector, every listed literal run and match length"""
    _, crossings = cases.reach("refill")
    assert {(d, h) for d in range(32, 48) for h in (False, True)} <= crossings
    views, _ = cases.reach("cursor")
    assert set(range(32)) <= views
    b = cases.batches()
    items, step, first = b["skew"]
    assert step == 1 and len({c.tobytes() for c, raw, _ in items if raw is not None}) == 1 and len(items) >= 64
    items, step, first = b["ends"]
    assert {(first + i * step + c.size - 1) % 64 + 1 for i, (c, raw, _) in enumerate(items[:64])} == set(range(1, 65))
    assert {(first + i * step) % 64 + c.size <= 32 for i, (c, raw, _) in enumerate(items[64:80])} == {True, False}
    items, step, first = b["identical"]
    assert step == 0 and len({c.tobytes() for c, raw, _ in items if raw is not None}) == 1
    assert len(b["last_wave"][0]) % 64 in range(1, 16)
    lits, matches = set(), set()
    for c, raw, _ in b["cursor"][0]:
        if raw is not None:
            lits.update(cases.sequence_lengths(c)[0])
            matches.update(cases.sequence_lengths(c)[1])
    assert set(cases.LITS) <= lits and set(cases.MATCHES) <= matches
