"""The built blocks of tests/encoder_cases.py -- the 65 535-byte distance limit, the length-byte boundaries, the end of a block, the output
limit around long lengths -- through every encoder form the SIMT emulator has, bit-exact against the oracle; and a fixed slice of the
encoder fuzz (tests/encoder_fuzz.py).  Every expectation of a built block is asserted against the oracle's own output first
(encoder_cases.Reference): a block that misses its rule fails before a kernel is asked.  tests/test_gpu_encoder_edges.py repeats all of
it through the C ABI."""
import numpy as np
import pytest

import emu_helpers as emu
import encoder_cases as ec
import encoder_fuzz
from encoder_cases import check_bit_exact, check_limited, fits

FORMS = ec.EMU_FORMS
FORM = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
_encode = ec.emu_encode


@FORM
def test_built_blocks_bit_exact(oracle, form):
    """Families A, B and C"""
    name, hc, sizes, kwargs = form
    ref = ec.reference(oracle, hc)
    check_bit_exact(lambda b, c: _encode(kwargs, b, c), [c for c in ref.everything() if fits(c[1], sizes)], name)


@FORM
def test_built_blocks_output_limit(oracle, form):
    """Family D: the reference's limit checks count length >> 8, not the length bytes, and refuse some capacities that would have fit"""
    name, hc, sizes, kwargs = form
    ref = ec.reference(oracle, hc)
    check_limited(lambda b, c: _encode(kwargs, b, c), [c for c in ref.limited if fits(c[1], sizes)], name)


@pytest.mark.parametrize("hc", [False, True], ids=["fast-lane", "hc-lane-large-blocks"])
def test_one_lane_generic_then_64k_then_generic(oracle, hc):
    """The distance-limit blocks in an order in which ONE lane meets a block over 64 KiB, then one below, then one over again.  Both
    launches are one wavefront (emu_helpers.encode's shape for these kernels), and the emulator switches fibers only at cross-lane
    operations, of which neither kernel has any: lane 0 pulls every block from the counter, in order.  What a lane keeps between blocks
    then meets the limit cases, and the blocks below 64 KiB start with the same P as their neighbours, so an entry that survives a
    block would be found.  Fast lane encoder: the variant changes with every block (LaneTable's epoch and clear rules).  LZ4HC: the
    batch's largest block picks 32-bit heads for all of it, so this is slab reuse alone, no change of variant."""
    ref = ec.reference(oracle, hc)
    cases = []
    for name, block, want, _ in ref.distance:
        cases.append((name, block, want))
        cut = block[:65546 if len(cases) % 4 == 1 else 3000]
        cases.append((name + " cut", cut, oracle.compress(cut, hc=hc)))
    cases.append(cases[0])
    kwargs = dict(hc=True, lane=True, conv=True) if hc else dict(lane=True)
    check_bit_exact(lambda b, c: emu.encode(b, caps=c, **kwargs), cases, "one lane")


# what the slice can afford under the emulator: all four output limits for one form, two for most, the full bound alone for the slowest
FUZZ_LIMITS = {name: (None, -1) for name, *_ in FORMS}
FUZZ_LIMITS.update({"fast-wave": (None, 0, -1, -5), "fast-two-launches": (None,), "hc-wave-heads32": (None,), "hc-lane-large-blocks": (None,)})
CPU_FUZZ_SEEDS, CPU_FUZZ_PER = 2, 6


def test_encoder_fuzz_slice(oracle, tmp_path):
    """tests/encoder_fuzz.py, ALWAYS the same seeds (7000 .. 7000 + CPU_FUZZ_SEEDS - 1, CPU_FUZZ_PER rows each), every row through every form
    that takes its size, with the full bound and with too-small output limits.  A mismatch names seed, round and block and saves the row."""
    msgs = []
    forms = encoder_fuzz.emu_forms(FUZZ_LIMITS)
    total, bad = encoder_fuzz.run(oracle, forms, 7000, CPU_FUZZ_SEEDS, CPU_FUZZ_PER, report=msgs.append, save_dir=str(tmp_path))
    print(f"encoder fuzz slice: seeds 7000..{7000 + CPU_FUZZ_SEEDS - 1}, per={CPU_FUZZ_PER}: {total} comparisons, {bad} mismatches")
    assert bad == 0, msgs[:10]
    # seed 7000 draws rows of 4594, 68682, 1048, 3894, 41 and 69296 (planted repeats) bytes, seed 7001 of 68956, 1515, 66977, 4359, 3149 and
    # 5816: four for the LZ4HC forms above 64 KiB, eight for those below, all twelve for the fast forms
    rows = {f.name: (12 if not f.hc else 4 if f.sizes == ec.LARGE else 8) for f in forms}
    assert {f.name: f.compared for f in forms} == {f.name: rows[f.name] * len(f.deltas) for f in forms}
