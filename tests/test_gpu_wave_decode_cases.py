"""The wavefront decoder (lz4hip_decode.hpp) on the device: the built blocks of tests/wave_decode_cases.py -- a few hundred blocks of at
most 12 KiB, every one on one side of a threshold of the kernel's paths -- through the C ABI with the wavefront mapping forced, as
single-block batches and as one batch of all of them (neighbouring wavefronts of a workgroup then hold different blocks), and once more
under default dispatch, against the CPU codec.  That each block reaches the path it was built for is proven where the kernel's counters
exist, under the emulator: tests/test_simt_wave_decode_cases.py."""
import numpy as np
import pytest

import wave_decode_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    return gpu_helpers


def _decode(gpu):
    return lambda comps, caps, known, lens: gpu.decode(comps, caps, known=known, src_lens=lens)


def _one_by_one(gpu):
    def decode(comps, caps, known, lens):
        rows = [gpu.decode([c], [cap], known=known, src_lens=[n]) for c, cap, n in zip(comps, caps, lens)]
        width = max(d.shape[1] for _, d in rows)
        dst = np.full((len(rows), width), 0xA5, np.uint8)
        for i, (_, d) in enumerate(rows):
            dst[i, :caps[i] + 64] = d[0, :caps[i] + 64]
        return np.array([int(r[0]) for r, _ in rows]), dst
    return decode


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("batch", ["single-block", "one-batch"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_built_streams_match_cpu_codec(gpu, oracle, name, batch, known):
    from lz4net_amd import _lib
    with _lib.tuning(decoder="wave"):
        before = _lib.dispatch_counts()
        cases.check(oracle, name, known, _one_by_one(gpu) if batch == "single-block" else _decode(gpu), holes_keep=True)
        after = _lib.dispatch_counts()
    assert after[_lib.K_DECODE_WAVE] > before[_lib.K_DECODE_WAVE] and after[_lib.K_DECODE_LANE] == before[_lib.K_DECODE_LANE]


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_built_streams_under_default_dispatch(gpu, oracle, name, known):
    """batches this small are the wavefront mapping's by the library's own rule"""
    from lz4net_amd import _lib
    before = _lib.dispatch_counts()
    cases.check(oracle, name, known, _decode(gpu), holes_keep=True)
    after = _lib.dispatch_counts()
    assert after[_lib.K_DECODE_WAVE] > before[_lib.K_DECODE_WAVE] and after[_lib.K_DECODE_LANE] == before[_lib.K_DECODE_LANE]
