"""The lane decoder's staged flush (lz4hip_decode_lane4.hpp, T2a .. T2d) on the device: the built blocks of tests/lane_flush_cases.py --
batches of 64 to 130 blocks of at most 1 KiB -- through every form of the kernel, against the CPU codec.  The emulator twin is
tests/test_simt_lane_flush_order.py."""
import pytest

import lane_flush_cases as cases

pytestmark = pytest.mark.gpu

# knobs of lz4hip_tuning_set and how often the batch is repeated in the call: the persistent grid (one wavefront pulls every block), one
# block per lane, workgroups of four wavefronts (taken from four wavefronts on: the batch three times over), the wrapped-row instantiation
FORMS = {"persist-1": (dict(decoder_persist=1, decoder_groups=1), 1), "persist-2": (dict(decoder_persist=2), 1),
         "wg4": (dict(decoder_persist=0, decoder_wg4=2), 3), "wrapped": (dict(decoder_persist=2, decoder_wrapped_stores=1), 1),
         "wrapped-persist-1": (dict(decoder_persist=1, decoder_groups=1, decoder_wrapped_stores=1), 1)}


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    return gpu_helpers


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["lengths_and_far", "near_then_far", "identical", "different_lengths"])
def test_staged_flush_matches_cpu_codec(gpu, oracle, name, form, known):
    from lz4net_amd import _lib
    knobs, repeat = FORMS[form]
    with _lib.tuning(decoder="lane", **knobs):
        before = _lib.dispatch_counts()
        cases.check(oracle, name, known, lambda comps, caps, k: gpu.decode(comps, caps, known=k), repeat=repeat)
        after = _lib.dispatch_counts()
    assert after[_lib.K_DECODE_LANE] > before[_lib.K_DECODE_LANE] and after[_lib.K_DECODE_WAVE] == before[_lib.K_DECODE_WAVE]
