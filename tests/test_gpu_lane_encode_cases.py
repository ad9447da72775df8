"""-m gpu twin of tests/test_simt_lane_encode_cases.py: the built blocks of tests/lane_encode_cases.py -- each at one branch of the fast lane
encoder, its expectation asserted against the oracle's own parse before a kernel is asked -- through the C ABI, all families in one
batch with the lane mapping forced (and proven to have run) and with nothing forced; families KS and R at every capacity around the
compressed size; and family Q cycled over 200 blocks per lane of a one-wavefront-per-CU grid in one call, where which lane meets which block
behind which is the hardware's choice: every row is compared on the device with its kind's expected bytes and guard bytes.  That a
block reaches the branch it was built for is proven where the kernel's counters exist, under the emulator."""
import numpy as np
import pytest

import encoder_cases as ec
import lane_encode_cases as lc
from encoder_cases import check_bit_exact, check_limited

pytestmark = pytest.mark.gpu

FORMS = [f for f in ec.GPU_FORMS if f[0] in ("fast-lane", "fast-default")]
FORM = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
LANE = next(f for f in FORMS if f[0] == "fast-lane")
BLOCKS_PER_LANE = 200                  # of a grid of one wavefront per CU: three zeroings of a lane's table on the average


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    assert "gfx950" in _lib.lib().lz4hip_codec_name().decode()
    return gpu_helpers


@FORM
def test_all_families_in_one_batch(gpu, oracle, form):
    cases = lc.everything(oracle)
    assert 400 <= len(cases) <= 800, len(cases)
    with ec.forced(form):
        check_bit_exact(lambda b, c: gpu.encode(b, caps=c), cases, form[0])


@FORM
def test_one_store_emit_output_limit(gpu, oracle, form):
    """family KS at every capacity from 12 below to 16 above the compressed size, and the full bound"""
    limited = lc.limited_cases(oracle, lc.checked(oracle, "KS"))
    with ec.forced(form):
        check_limited(lambda b, c: gpu.encode(b, caps=c), limited, form[0])


@FORM
def test_length_byte_refusals(gpu, oracle, form):
    """family R, blocks of hundreds of KiB in a batch of their own: bit-exact, and at every capacity from 12 below to 16 above the
    compressed size the oracle's return value -- the 0 the reference reaches after running past the capacity included"""
    cases = lc.checked(oracle, "R")
    with ec.forced(form):
        check_bit_exact(lambda b, c: gpu.encode(b, caps=c), cases, form[0])
        check_limited(lambda b, c: gpu.encode(b, caps=c), lc.limited_cases(oracle, cases), form[0])


def test_one_lane_many_blocks(gpu, oracle):
    """Family Q's blocks cycled over BLOCKS_PER_LANE x 64 x (number of CUs) rows, one call, the lane mapping forced with one wavefront
    per CU: every lane encodes some 200 blocks in the order the counter hands them out and zeroes its table about three times.  Each
    kind's first word is in every other kind's block, so a lane meets position-0 hits out of earlier blocks' entries all the time, and
    the pair's second block meets the first's entries wherever it follows it.  EVERY row: result, bytes, guard bytes."""
    import torch
    from lz4net_amd import _lib, batch
    cases = lc.checked(oracle, "Q")
    k = len(cases)
    src_h, sl_h = gpu.pack([c[1] for c in cases])
    cap = max(ec.compress_bound(len(c[1])) for c in cases)
    rows = BLOCKS_PER_LANE * 64 * torch.cuda.get_device_properties(0).multi_processor_count
    reps = rows // k
    assert reps * k == rows and src_h.shape[1] <= 216
    src = torch.from_numpy(src_h).cuda().repeat(reps, 1)
    sl = torch.from_numpy(sl_h).cuda().repeat(reps)
    dst = torch.full((rows, cap + 64), 0xA5, dtype=torch.uint8, device="cuda")
    with ec.forced(LANE), _lib.tuning(encoder_waves_per_cu=1):
        res = batch.encode(src, sl, dst, cap)
        torch.cuda.synchronize()
    expect = np.full((k, cap + 64), 0xA5, np.uint8)
    for i, (name, block, want, _) in enumerate(cases):
        expect[i, :len(want)] = want
    want_len = torch.tensor([len(c[2]) for c in cases], dtype=res.dtype, device="cuda")
    bad_len = (res.view(reps, k) != want_len).any(dim=0).cpu().numpy()
    bad_row = (dst.view(reps, k, cap + 64) != torch.from_numpy(expect).cuda()).any(dim=2)
    bad_bytes = bad_row.any(dim=0).cpu().numpy()
    for i, (name, *_) in enumerate(cases):
        assert not bad_len[i], (name, "a row's result is not the oracle's", torch.unique(res.view(reps, k)[:, i]).cpu().numpy()[:8])
        assert not bad_bytes[i], (name, int(bad_row[:, i].sum()), "rows differ from the oracle's bytes or wrote past them")
