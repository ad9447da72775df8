"""The predicates the lane decoder makes once per iteration and combines as lane masks (lz4hip_decode_lane4.hpp) on the device: the built blocks
of tests/lane_predicate_cases.py -- one wavefront of 64 blocks of at most 1 KiB per family, every block on one side of an edge -- through the
lane decoder, one block per lane and persistent, with dual and with wrapped ring stores, known and unknown size, against the CPU codec.  That
each block reaches the branch it was built for is proven where the kernel's counters exist: tests/test_simt_lane_predicates.py."""
import pytest

import lane_predicate_cases as cases

pytestmark = pytest.mark.gpu

FORMS = {"lane": dict(decoder_persist=2), "persist-1": dict(decoder_persist=1, decoder_groups=1),
         "wrapped": dict(decoder_persist=2, decoder_wrapped_stores=1), "wrapped-persist-1": dict(decoder_persist=1, decoder_groups=1, decoder_wrapped_stores=1)}


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
    with _lib.tuning(decoder="lane", **FORMS[form]):
        before = _lib.dispatch_counts()
        cases.check(oracle, name, known, lambda comps, caps, k: gpu.decode(comps, caps, known=k))
        after = _lib.dispatch_counts()
    assert after[_lib.K_DECODE_LANE] > before[_lib.K_DECODE_LANE] and after[_lib.K_DECODE_WAVE] == before[_lib.K_DECODE_WAVE]
