"""-m gpu twin of tests/test_simt_wave_encode_cases.py: the built blocks of tests/wave_encode_cases.py -- each at one branch of the wavefront
fast encoder, its expectation asserted against the oracle's own parse before a kernel is asked -- through the C ABI with every fast
form of encoder_cases.GPU_FORMS forced in turn (and proven to have run), all families in one batch; for the wavefront mapping also one
block per call, which is the hardware's answer to which lane's store to a shared LDS address lands last; family E at every capacity
around the compressed size; families S and Z through the dictionary encode call against its twin (tests/dict_encode_ref.py); and family
H repeated to 49 152 rows in one call with nothing forced, every row compared, the lane dispatch counted.  That a block reaches the
branch it was built for is proven where the kernel's counters exist, under the emulator."""
import numpy as np
import pytest

import dict_encode_ref as ref
import encoder_cases as ec
import wave_encode_cases as wc
from encoder_cases import check_bit_exact, check_limited

pytestmark = pytest.mark.gpu

FORMS = [f for f in ec.GPU_FORMS if not f[1]]
FORM = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
WAVE = next(f for f in FORMS if f[0] == "fast-wave")
HAND_OVER_ROWS = 49152


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    assert "gfx950" in _lib.lib().lz4hip_codec_name().decode()
    return gpu_helpers


@FORM
def test_all_families_in_one_batch(gpu, oracle, form):
    cases = wc.everything(oracle)
    assert 100 <= len(cases) <= 400, len(cases)
    with ec.forced(form):
        check_bit_exact(lambda b, c: gpu.encode(b, caps=c), cases, form[0])


@pytest.mark.parametrize("name", wc.NAMES)
def test_wavefront_mapping_one_block_per_call(gpu, oracle, name):
    for case in wc.checked(oracle, name):
        with ec.forced(WAVE):
            check_bit_exact(lambda b, c: gpu.encode(b, caps=c), [case], case[0])


@FORM
def test_one_store_emit_output_limit(gpu, oracle, form):
    """family E at every capacity from 12 below to 4 above the compressed size"""
    limited = wc.limited_cases(oracle, wc.checked(oracle, "E"))
    with ec.forced(form):
        check_limited(lambda b, c: gpu.encode(b, caps=c), limited, form[0])


def _dict_encode(gpu, blocks, dic):
    import torch
    from lz4net_amd import batch
    src_h, sl_h = gpu.pack(blocks)
    caps = [ref.bound(len(b)) for b in blocks]
    src, sl = torch.from_numpy(src_h).cuda(), torch.from_numpy(sl_h).cuda()
    cp = torch.tensor(caps, dtype=torch.int32, device="cuda")
    dst = torch.full((len(blocks), max(caps) + 64), 0xA5, dtype=torch.uint8, device="cuda")
    res = batch.encode_dict(src, sl, dst, cp, torch.from_numpy(np.ascontiguousarray(dic)).cuda())
    torch.cuda.synchronize()
    return res.cpu().numpy(), dst.cpu().numpy()


@pytest.mark.parametrize("kind", wc.DICT_KINDS)
@pytest.mark.parametrize("name", wc.DICT)
def test_family_through_the_dictionary_encoder(gpu, oracle, name, kind):
    cases = wc.dict_cases(oracle, name)
    dic = wc.dictionary(kind, [c[1] for c in cases])
    want = [ref.encode(c[1].tobytes(), dic.tobytes()) for c in cases]
    wc.check_dict(lambda b: _dict_encode(gpu, b, dic), cases, want, (name, kind, "one batch"))
    for case, w in zip(cases, want):
        wc.check_dict(lambda b: _dict_encode(gpu, b, dic), [case], [w], (name, kind, "one block per call"))


def test_hand_over_batch(gpu, oracle):
    """family H's blocks repeated to 49 152 rows, one device call, nothing forced: the wavefront launch hands over the blocks built for
    it, the lane launch finishes them, every row equals its block's expectation"""
    import torch
    from lz4net_amd import _lib, batch
    cases = wc.checked(oracle, "H")
    k = len(cases)
    src_h, sl_h = gpu.pack([c[1] for c in cases])
    cap = max(ec.compress_bound(len(c[1])) for c in cases)
    reps = HAND_OVER_ROWS // k
    assert reps * k == HAND_OVER_ROWS
    src = torch.from_numpy(src_h).cuda().repeat(reps, 1)
    sl = torch.from_numpy(sl_h).cuda().repeat(reps)
    dst = torch.full((HAND_OVER_ROWS, cap + 64), 0xA5, dtype=torch.uint8, device="cuda")
    before = _lib.dispatch_counts()
    res = batch.encode(src, sl, dst, cap)
    torch.cuda.synchronize()
    after = _lib.dispatch_counts()
    assert after[_lib.K_ENCODE_WAVE] > before[_lib.K_ENCODE_WAVE] and after[_lib.K_ENCODE_LANE] > before[_lib.K_ENCODE_LANE], (before, after)
    res, out = res.cpu().numpy().reshape(reps, k), dst.cpu().numpy().reshape(reps, k, cap + 64)
    for i, (name, block, want, _) in enumerate(cases):
        assert (res[:, i] == len(want)).all(), (name, np.unique(res[:, i]))
        expect = np.full(cap + 64, 0xA5, np.uint8)
        expect[:len(want)] = want
        assert (out[:, i, :] == expect).all(), (name, "a row differs from the oracle's bytes or wrote past them")
