"""The lane decoder's parser and ring logic (lz4hip_decode_lane4.hpp: T4 / T4x, T1c, T3, T5, B3 .. B5) on the device: the built blocks of
tests/lane_decode_cases.py -- batches of 64 to 130 blocks of at most 2 KiB, every one on one side of a threshold -- through every form of the
kernel, one batch per call, against the CPU codec.  That each block reaches the path it was built for is proven where the kernel's counters
exist, under the emulator: tests/test_simt_lane_decode_cases.py."""
import pytest

import lane_decode_cases as cases
from test_gpu_lane_flush_order import FORMS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    return gpu_helpers


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", cases.NAMES)
def test_built_blocks_match_cpu_codec(gpu, oracle, name, form, known):
    from lz4net_amd import _lib
    knobs, repeat = FORMS[form]
    with _lib.tuning(decoder="lane", **knobs):
        before = _lib.dispatch_counts()
        cases.check(oracle, name, known, lambda comps, caps, k: gpu.decode(comps, caps, known=k), repeat=repeat)
        after = _lib.dispatch_counts()
    assert after[_lib.K_DECODE_LANE] > before[_lib.K_DECODE_LANE] and after[_lib.K_DECODE_WAVE] == before[_lib.K_DECODE_WAVE]
