"""The lane decoder's input window (lz4hip_decode_lane4.hpp, T1a / T1b / B3: conditional assignments as moves under a lane mask) on the device:
the built blocks of tests/lane_window_cases.py -- batches of 64 to 130 blocks of at most 2 KiB, each row at a chosen alignment of a 64-byte
sector -- through every form of the kernel, against the CPU codec.  The emulator twin is tests/test_simt_lane_window.py."""
import numpy as np
import pytest

import lane_window_cases as cases
from test_gpu_lane_flush_order import FORMS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    return gpu_helpers


def decode(comps, caps, known, step, first):
    """the device-pointer entry point over rows of device memory laid out at chosen alignments of a 64-byte sector"""
    import torch
    from lz4net_amd import batch
    raw, at, stride = cases.lay_out(comps, step, first)
    buf = torch.from_numpy(raw[at - first:]).cuda()                  # (the host buffer's own alignment does not travel: row 0 lies `first` bytes into the device's)
    assert buf.data_ptr() % 64 == 0
    src = buf[first:].as_strided((len(comps), stride), (stride, 1))
    assert src.data_ptr() % 64 == first
    sl = torch.tensor([len(c) for c in comps], dtype=torch.int32, device="cuda")
    cap = torch.tensor(caps, dtype=torch.int32, device="cuda")
    dst = torch.full((len(comps), max(caps) + 64), 0xA5, dtype=torch.uint8, device="cuda")
    res = batch.decode(src, sl, dst, cap, known_output_size=known)
    torch.cuda.synchronize()
    return res.cpu().numpy(), dst.cpu().numpy()


@pytest.mark.parametrize("known", [True, False], ids=["known", "unknown"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["skew", "refill", "cursor", "ends", "identical", "last_wave"])
def test_window_matches_cpu_codec(gpu, oracle, name, form, known):
    from lz4net_amd import _lib
    knobs, repeat = FORMS[form]
    with _lib.tuning(decoder="lane", **knobs):
        before = _lib.dispatch_counts()
        cases.check(oracle, name, known, decode, repeat=repeat)
        after = _lib.dispatch_counts()
    assert after[_lib.K_DECODE_LANE] > before[_lib.K_DECODE_LANE] and after[_lib.K_DECODE_WAVE] == before[_lib.K_DECODE_WAVE]
