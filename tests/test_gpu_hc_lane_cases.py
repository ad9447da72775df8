"""-m gpu twin of tests/test_simt_hc_lane_cases.py: the built blocks of tests/hc_lane_cases.py through the C ABI, bit-exact against the
oracle with guard bytes, for the LZ4HC mappings forced in turn (and proven to have run: conftest.ForcedMapping) and with nothing
forced; for the lane mapping -- the kernel the blocks were built for -- in four shapes.  Same blocks, same expectations, asserted
against the oracle before a kernel is asked; the counters that prove reach exist only under the emulator."""
import pytest

import encoder_cases as ec
import hc_lane_cases as hl
from encoder_cases import check_bit_exact, check_limited

pytestmark = pytest.mark.gpu

FORMS = [f for f in ec.GPU_FORMS if f[0] in ("hc-wave", "hc-lane", "hc-default")]
FORM = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
LANE = next(f for f in FORMS if f[0] == "hc-lane")


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    assert "gfx950" in _lib.lib().lz4hip_codec_name().decode()
    return gpu_helpers


def _encode(gpu):
    return lambda b, c: gpu.encode(b, caps=c, hc=True)


@FORM
def test_built_blocks_bit_exact(gpu, oracle, form):
    """every family in one batch"""
    cases = hl.everything(oracle)
    assert len(cases) >= 300
    with ec.forced(form):
        check_bit_exact(_encode(gpu), cases, form[0])


def test_lane_mapping_one_block_per_call(gpu, oracle):
    with ec.forced(LANE):
        for case in hl.everything(oracle):
            check_bit_exact(_encode(gpu), [case], case[0])


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_lane_mapping_one_wavefront(gpu, oracle, order):
    """hc_groups=1: 64 lanes take every block from the counter, so a lane meets the families one after the other, in two orders"""
    from lz4net_amd import _lib
    cases = hl.everything(oracle)
    with ec.forced(LANE), _lib.tuning(hc_groups=1):
        check_bit_exact(_encode(gpu), cases if order == "forward" else cases[::-1], order)


@FORM
def test_table_blocks_end_to_end(gpu, oracle, form):
    """the blocks the builders' table is checked with under the emulator (every n in 0..20, the steps, rows and rounds, 65 536 bytes), encoded"""
    cases = [(name, block, oracle.compress(block, hc=True)) for name, block in hl.table_blocks()]
    with ec.forced(form):
        check_bit_exact(_encode(gpu), cases, form[0])


@FORM
def test_parse_blocks_output_limit(gpu, oracle, form):
    """family P at every capacity from 8 below to 2 above the compressed size"""
    limited = hl.limited_cases(oracle, hl.family("P"))
    with ec.forced(form):
        check_limited(_encode(gpu), limited, form[0])
