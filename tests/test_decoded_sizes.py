"""The size query of a block batch (lz4hip_decoded_sizes_*) without a GPU: the real kernel (lz4net_amd/csrc/lz4hip_sizes.hpp), the
library's launch sequence and argument checks (lz4hip_framing.hpp) and its host-pointer call (lz4hip_hostbatch.hpp) under the SIMT
emulator, against what the reference's LZ4_uncompress_unknownOutputSize returns with an output limit that never binds."""
import ctypes as C

import numpy as np
import pytest

import sizes_helpers as sh
from sizes_helpers import Outputs, make_batch


def walk(blocks, groups=0):
    """every block's result under the emulator, from one call over an odd-offset layout"""
    buf, off, lens = sh.pack_offsets(blocks)
    out = Outputs(len(blocks))
    rc, text = sh.emu_sizes(make_batch(buf, off=off, lens=lens, n=len(blocks)), out, groups)
    assert rc == 0, text
    return out.result[1:-1].copy(), out


def assert_parity(blocks, groups=0):
    want = sh.reference_sizes(blocks)
    got, out = walk(blocks, groups)
    wrong = np.flatnonzero(got != want)
    assert len(wrong) == 0, [(int(i), len(blocks[i]), int(got[i]), int(want[i])) for i in wrong[:8]]
    out.check(want)
    return want


def test_window_is_what_the_corpus_was_built_for():
    assert sh.emu().emu_sizes_window() == 64


def test_parity_encoder_output(oracle):
    blocks = sh.encoder_corpus(oracle)
    assert len(blocks) == 9 * 4 * 2
    want = assert_parity(blocks)
    assert (want >= 0).all()                                           # encoder output walks to its size:
    sizes = [n for n in (0, 1, 12, 13, 64, 65535, 65536, 65547, 200000) for _ in range(8)]
    assert list(want) == sizes


def test_parity_hand_made_blocks():
    blocks = sh.hand_blocks()
    want = assert_parity(blocks)
    assert want[0] == 0 and want[1] == -4                              # `00`; the run of 255s that ends at iend fails there
    assert list(want[7:10]) == [-1, 5, -1]                            # last literals ending at iend - 1, iend, iend + 1
    assert want[10] == 10 and want[11] == -1                           # ip + ll == iend - 8 against iend - 7
    assert want[12] == -4 and want[13] == 10                           # offset == produced + 1; offset 0 is no error
    assert want[-1] == 1 << 20 and want[-2] == 1 << 20 and len(blocks[-2]) < 8192
    assert (want < 0).any() and (want > 0).any()


def test_parity_every_prefix(oracle):
    want = assert_parity(sh.prefixes(oracle))
    assert (want < 0).sum() > len(want) // 2 and (want > 0).sum() >= 2     # (a prefix that ends on a last sequence of its own walks)


def test_parity_window_edges():
    w = int(sh.emu().emu_sizes_window())
    blocks = sh.window_blocks(w)
    want = assert_parity(blocks)
    assert (want > 0).all()                                            # (every one of them is a well-formed block)
    assert min(len(b) for b in blocks) < w and max(len(b) for b in blocks) > 3 * w


def test_parity_mutation_fuzz(oracle):
    blocks = sh.fuzz_blocks(oracle)
    assert len(blocks) >= 20000 and all(16 <= len(b) <= 600 for b in blocks)
    want = assert_parity(blocks)
    share = float((want < 0).mean())
    print(f"mutation fuzz: {len(blocks)} blocks, {100 * share:.1f} % negative results (seed {sh.FUZZ_SEED})")
    assert 0.10 < share < 0.90


def test_overflowing_count_is_an_argument_error():
    # 2^31 bytes and more out of match-length bytes alone: the reference's int would wrap (no buffer to ask it with)
    n255 = (1 << 31) // 255 + 16
    block = np.concatenate([np.array([0x1F, 0x41, 1, 0], np.uint8), np.full(n255, 255, np.uint8), np.array([0x50, 1, 2, 3, 4, 5], np.uint8)])
    just_below = np.concatenate([np.array([0x1F, 0x41, 1, 0], np.uint8), np.full(1000, 255, np.uint8), np.array([0x50, 1, 2, 3, 4, 5], np.uint8)])
    got, _ = walk([block, just_below])
    assert got[0] == sh.E_ARGUMENT and got[1] == sh.reference_sizes([just_below])[0] == 1 + 19 + 255 * 1000 + 5


# ---- the launch sequence and the host call ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(oracle):
    """valid blocks and corrupt ones, with the reference's results"""
    good = [sh.compress(sh.data(oracle, 2 + k % 2, 40 + 37 * k, seed=20 + k), hc=bool(k & 1)) for k in range(12)] + [np.array([0], np.uint8), np.zeros(0, np.uint8)]
    bad = [good[3][:-2].copy(), np.array([0x10, 0x30, 2, 0, 0x50, 1, 2, 3, 4, 5], np.uint8), good[7][:11].copy()]
    g, b = sh.reference_sizes(good), sh.reference_sizes(bad)
    assert (g >= 0).all() and (b < 0).all()
    return good, g, bad, b


def layout(pool, n, failures):
    good, g, bad, b = pool
    where = {"none": [], "first": [0], "middle": [n // 2], "last": [n - 1], "all": [0, n // 2, n - 1]}[failures] if n else []
    blocks, want = [], np.zeros(n, np.int32)
    for i in range(n):
        k = (i * 7 + 3) % len(bad) if i in where else (i * 5 + 1) % len(good)
        blocks.append(bad[k] if i in where else good[k])
        want[i] = b[k] if i in where else g[k]
    return blocks, want


@pytest.mark.parametrize("failures", ["none", "first", "middle", "last", "all"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sequence_and_host_call(pool, n, failures):
    if n == 0 and failures != "none":
        return
    blocks, want = layout(pool, n, failures)
    buf, off, lens = sh.pack_offsets(blocks)                            # odd byte offsets
    for groups in (0, 1, 3):
        out = Outputs(n)
        rc, text = sh.emu_sizes(make_batch(buf, off=off, lens=lens, n=n), out, groups)
        assert rc == 0, text
        out.check(want)
    for wanted in (("dst_off",), ("dst_cap", "info"), ("result",), ("info",), ()):     # the other outputs are NULL
        out = Outputs(n, wanted)
        rc, text = sh.emu_sizes(make_batch(buf, off=off, lens=lens, n=n), out)
        assert rc == 0, text
        out.check(want)
    for wanted, pool_floor in ((("result", "dst_off", "dst_cap", "info"), -1), (("dst_off", "info"), 0), ((), -1)):
        out = Outputs(n, wanted)
        rc, run = sh.emu_sizes_host(make_batch(buf, off=off, lens=lens, n=n), out, pool_floor=pool_floor)
        assert rc == 0, run.error
        out.check(want)
        if n:
            assert run.intact == 1 and run.reserves == 1 and run.uploads == 3 and run.syncs == 1
            assert run.downloads == len(wanted)                        # results, offsets, sizes, info: no block payload comes back
            assert run.image_bytes < buf.size + 40 * n + 8192
        else:
            assert (run.reserves, run.uploads, run.downloads, run.syncs) == (0, 0, 0, 0)


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_stride_and_one_length_for_all(pool, n):
    good, g, bad, b = pool
    length = len(good[5])
    broken = good[5].copy()
    for at in range(length):                                           # the same length, and a walk that fails
        broken = good[5].copy()
        broken[at] ^= 0xFF
        if sh.reference_sizes([broken])[0] < 0:
            break
    r_bad = sh.reference_sizes([broken])[0]
    assert r_bad < 0
    stride = length + 3                                                # odd row starts from the second row on
    rows = np.full((n, stride), 0xEE, np.uint8)
    want = np.full(n, g[5], np.int32)
    for i in range(n):
        fails = i in (n // 2, n - 1) and n > 1
        rows[i, :length] = broken if fails else good[5]
        want[i] = r_bad if fails else g[5]
    flat = np.concatenate([np.full(1, 0xEE, np.uint8), rows.reshape(-1)])[1:]
    for run in ("device", "host"):
        out = Outputs(n)
        batch = make_batch(flat, stride=stride, len_all=length, n=n)
        if run == "device":
            rc, text = sh.emu_sizes(batch, out)
        else:
            rc, text = sh.emu_sizes_host(batch, out)
        assert rc == 0
        out.check(want)


def test_argument_checks_under_the_emulator(pool):
    blocks, want = layout(pool, 5, "none")
    buf, off, lens = sh.pack_offsets(blocks)
    lib = sh.emu()
    text = C.create_string_buffer(200)
    assert lib.emu_decoded_sizes(None, None, None, None, 0, None, 0, text, 200) == sh.E_ARGUMENT and b"NULL" in text.value
    out = Outputs(5)
    assert sh.emu_sizes(make_batch(buf, off=off, lens=lens, n=-1), Outputs(0))[0] == sh.E_ARGUMENT
    need = lib.emu_sizes_scratch_bytes(5)
    rc, msg = sh.emu_sizes(make_batch(buf, off=off, lens=lens, n=5), out, scratch_bytes=need - 1)
    assert rc == sh.E_ARGUMENT and "scratch" in msg
    assert out.result[1] == -77 and out.info.blocks == -7              # nothing was written
    assert sh.emu_sizes(make_batch(None, off=off, lens=lens, n=5), out)[0] == sh.E_ARGUMENT
    assert sh.emu_sizes(make_batch(buf, stride=8, len_all=-1, n=5), out)[0] == sh.E_ARGUMENT
    # an empty batch: 0, a zeroed info (no error: first_error = -1) and dst_off[0] = 0, without any scratch
    out = Outputs(0)
    assert sh.emu_sizes(make_batch(None, n=0), out)[0] == 0
    out.check(np.zeros(0, np.int32))
    assert (out.info.blocks, out.info.decoded_bytes, out.info.first_error, out.info.error) == (0, 0, -1, 0)
    # a negative length among the rows: that block's result on the device, the whole call on the host (which can see it)
    lens2 = lens.copy()
    lens2[2] = -5
    out = Outputs(5)
    assert sh.emu_sizes(make_batch(buf, off=off, lens=lens2, n=5), out)[0] == 0
    want2 = want.copy()
    want2[2] = sh.E_ARGUMENT
    out.check(want2)
    rc, run = sh.emu_sizes_host(make_batch(buf, off=off, lens=lens2, n=5), Outputs(5))
    assert rc == sh.E_ARGUMENT and b"negative" in run.error
    assert sh.emu_sizes_host(make_batch(None, off=off, lens=lens, n=5), Outputs(5))[0] == sh.E_ARGUMENT
    assert lib.emu_decoded_sizes_host(None, None, None, None, 0, -1, C.byref(sh.EmuHostRun())) == sh.E_ARGUMENT


def test_scratch_bytes():
    from lz4net_amd import _lib
    L = _lib.lib()
    assert L.lz4hip_decoded_sizes_scratch_bytes(0) == 0 and L.lz4hip_decoded_sizes_scratch_bytes(-3) == 0
    sizes = [L.lz4hip_decoded_sizes_scratch_bytes(n) for n in (1, 2, 63, 64, 65, 4096, 4097, 1 << 20, (1 << 31) - 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    assert [sh.emu().emu_sizes_scratch_bytes(n) for n in (1, 65, 4097)] == [sizes[0], sizes[4], sizes[6]]


def test_library_argument_checks_need_no_device():
    from lz4net_amd import _lib
    L = _lib.lib()
    src = np.zeros(64, np.uint8)
    lens = np.full(4, 16, np.int32)
    res = np.zeros(4, np.int32)
    b = _lib.Batch(src=src.ctypes.data, src_stride=16, src_len=lens.ctypes.data, result=res.ctypes.data, n_blocks=4)
    need = L.lz4hip_decoded_sizes_scratch_bytes(4)
    assert L.lz4hip_decoded_sizes_device(None, None, None, None, 0, None, None) == _lib.E_ARGUMENT
    assert b"NULL" in L.lz4hip_last_error()
    assert L.lz4hip_decoded_sizes_device(C.byref(b), None, None, src.ctypes.data, need - 1, None, None) == _lib.E_ARGUMENT
    assert b"scratch" in L.lz4hip_last_error()
    b.n_blocks = -1
    assert L.lz4hip_decoded_sizes_device(C.byref(b), None, None, None, 0, None, None) == _lib.E_ARGUMENT
    assert b"n_blocks" in L.lz4hip_last_error()
    b.n_blocks = 0
    assert L.lz4hip_decoded_sizes_device(C.byref(b), None, None, None, 0, None, None) == 0     # nothing to write, nothing to launch
    if L.lz4hip_device_count() == 0:
        b.n_blocks = 4
        info = _lib.SizesInfo()
        assert L.lz4hip_decoded_sizes_host(C.byref(b), None, None, C.byref(info)) == _lib.E_DEVICE
        assert len(L.lz4hip_last_error()) > 0
        assert L.lz4hip_decoded_sizes_device(C.byref(b), None, None, src.ctypes.data, need, None, None) == _lib.E_DEVICE
