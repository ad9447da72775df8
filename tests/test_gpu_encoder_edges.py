"""-m gpu twins of tests/test_simt_encoder_edges.py: the built blocks of tests/encoder_cases.py (distance limit, length-byte boundaries,
end of a block, output limit around long lengths) and a fixed slice of tests/encoder_fuzz.py through the C ABI, with every
block->hardware mapping of the encoders forced in turn (and proven to have run: conftest.ForcedMapping) and once with nothing forced.
Same blocks, same expectations -- asserted against the oracle before a kernel is asked -- same comparisons."""
import pytest

import encoder_cases as ec
import encoder_fuzz
from encoder_cases import check_bit_exact, check_limited, fits

pytestmark = pytest.mark.gpu

FORMS = ec.GPU_FORMS
FORM = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
_forced, _size_classes = ec.forced, ec.gpu_size_classes


@pytest.fixture(scope="module")
def gpu():
    import gpu_helpers
    from lz4net_amd import _lib
    assert _lib.lib().lz4hip_device_count() >= 1, "no HIP device visible"
    assert "gfx950" in _lib.lib().lz4hip_codec_name().decode()
    return gpu_helpers


@FORM
def test_built_blocks_bit_exact(gpu, oracle, form):
    """Families A, B and C"""
    name, hc = form[:2]
    ref = ec.reference(oracle, hc)
    for sizes in _size_classes(hc):
        with _forced(form):
            check_bit_exact(lambda b, c: gpu.encode(b, caps=c, hc=hc), [c for c in ref.everything() if fits(c[1], sizes)], (name, sizes))


@FORM
def test_built_blocks_output_limit(gpu, oracle, form):
    """Family D: every capacity from 12 below to 4 above the compressed size"""
    name, hc = form[:2]
    ref = ec.reference(oracle, hc)
    for sizes in _size_classes(hc):
        with _forced(form):
            check_limited(lambda b, c: gpu.encode(b, caps=c, hc=hc), [c for c in ref.limited if fits(c[1], sizes)], (name, sizes))


GPU_FUZZ_SEEDS, GPU_FUZZ_PER = 1, 192


def test_encoder_fuzz_slice(gpu, oracle, tmp_path):
    """tests/encoder_fuzz.py, ALWAYS the same seeds (8000 .. 8000 + GPU_FUZZ_SEEDS - 1, GPU_FUZZ_PER rows each): every row through every form
    above, the full bound and three too-small output limits.  A mismatch names seed, round and block and saves the row; replay with
    tools/fuzz_gpu_encoders.py."""
    msgs = []
    total, bad = encoder_fuzz.run(oracle, encoder_fuzz.gpu_forms(), 8000, GPU_FUZZ_SEEDS, GPU_FUZZ_PER, report=msgs.append, save_dir=str(tmp_path))
    print(f"encoder fuzz slice: seeds 8000..{8000 + GPU_FUZZ_SEEDS - 1}, per={GPU_FUZZ_PER}: {total} comparisons, {bad} mismatches")
    assert bad == 0, msgs[:10]
    assert total == GPU_FUZZ_SEEDS * GPU_FUZZ_PER * len(FORMS) * 4, total
