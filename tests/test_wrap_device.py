"""Batches of wrapped messages on the device (lz4hip_wrap_* / lz4hip_unwrap_* of include/lz4hip.h, lz4net_amd/wrap.py).  CPU: the bound,
the scratch sizes and the argument checks.  GPU: byte parity with messages wrapped HERE from the oracle's blocks, both mappings of
each codec, round trips on a non-default torch stream, foreign messages, every failure kind in one batch, guard bytes, the host pair
and a batch large enough for the lane decoder.  The CPU twin of the GPU part -- the framing kernels themselves under the SIMT
emulator, without the block codec -- lives in test_simt_framing.py."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from lz4net_amd import LZ4Codec, _lib
from lz4net_amd import wrap as wr
from lz4net_amd.codec import ArgumentException

from conftest import ForcedMapping

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_wrap_bound_formula():
    L = _lib.lib()
    for n in (0, 1, 7, 1 << 20, 1 << 31, 1 << 40):
        for src_len in (0, 1, 65536, (1 << 31) - 1, 1 << 33, 1 << 50):
            assert L.lz4hip_wrap_bound(n, src_len) == src_len + 8 * n, (n, src_len)


def test_wrap_scratch_sizes_are_monotonic():
    L = _lib.lib()
    ns = (0, 1, 2, 255, 256, 4095, 4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 26)
    lens = (0, 1, 4096, 65536, 1 << 30, 1 << 34)
    for src_len in lens:
        prev = 0
        for n in ns:
            s = L.lz4hip_wrap_scratch_bytes(n, src_len)
            assert s >= prev and s >= 0, (n, src_len)
            assert n == 0 or s >= src_len + 16 * n, (n, src_len)      # the encoder's output, its offsets, lengths and results
            prev = s
    for n in ns:
        prev = 0
        for src_len in lens:
            s = L.lz4hip_wrap_scratch_bytes(n, src_len)
            assert s >= prev, (n, src_len)
            prev = s
    prev = 0
    for n in ns:
        s = L.lz4hip_unwrap_scratch_bytes(n)
        assert s >= prev and s >= 40 * n, n
        prev = s


def test_device_functions_reject_bad_arguments():
    import torch
    off = np.array([0, 3], np.int64)
    for bad in (b"abc", np.zeros(3, np.uint8)):
        with pytest.raises(ArgumentException):
            wr.wrap_device(bad, off)
        with pytest.raises(ArgumentException):
            wr.unwrap_device(bad, off)
    with pytest.raises(ArgumentException):                           # offsets on the host
        wr.wrap_device(torch.zeros(3, dtype=torch.uint8), off)
    if torch.cuda.is_available():
        x = torch.zeros(3, dtype=torch.uint8, device="cuda")
        for o in (torch.tensor([0, 3], dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"),
                  torch.zeros((2, 2), dtype=torch.int64, device="cuda")):
            with pytest.raises(ArgumentException):
                wr.wrap_device(x, o)
            with pytest.raises(ArgumentException):
                wr.unwrap_device(x, o)
        with pytest.raises(ArgumentException):                       # wrong dtype of the buffer
            wr.wrap_device(x.to(torch.int32), torch.tensor([0, 3], dtype=torch.int64, device="cuda"))
    for o in (np.array([0, 3], np.int32), np.zeros(0, np.int64), np.zeros((2, 2), np.int64)):
        with pytest.raises(ArgumentException):
            wr.wrap_host(np.zeros(3, np.uint8), o)
        with pytest.raises(ArgumentException):
            wr.unwrap_host(np.zeros(3, np.uint8), o)


def test_unwrap_error_texts():
    assert str(wr.unwrap_error(_lib.WRAP_SIZE_INVALID, 3)) == "inputBuffer size is invalid"
    assert str(wr.unwrap_error(_lib.WRAP_CORRUPT_HEADER, 3)) == "inputBuffer size is invalid or has been corrupted"
    e = wr.unwrap_error(_lib.WRAP_CORRUPT_BLOCK, 7)
    assert str(e) == "LZ4 block is corrupted, or invalid length has been given." and e.message_index == 7


# ---- GPU: the expected bytes come from the oracle and the test's own framing -------------------------------------------------

def header(original, payload):
    return int(original).to_bytes(4, "little", signed=True) + int(payload).to_bytes(4, "little", signed=True)


def expected_wrap(oracle, msg, hc):
    """LZ4Codec.Wrap / WrapHC (src/LZ4/LZ4Codec.cs:510-549) from the oracle's block encoder."""
    msg = np.ascontiguousarray(msg, np.uint8)
    n = msg.size
    if n == 0:
        return bytes(8)
    r, buf = oracle.compress_raw(msg, n, hc=hc)
    if 0 < r < n:
        return header(n, r) + buf[:r].tobytes()
    return header(n, n) + msg.tobytes()


_REAL = None


def real_bytes():
    global _REAL
    if _REAL is None:
        files = sorted(glob.glob(os.path.join(ROOT, "*.md")) + glob.glob(os.path.join(ROOT, "lz4net_amd", "**", "*.hip"), recursive=True) +
                       glob.glob(os.path.join(ROOT, "lz4net_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py")))
        _REAL = np.frombuffer(b"".join(open(f, "rb").read() for f in files), dtype=np.uint8)
    return _REAL


def data_of(oracle, kind, size, seed=0):
    if kind in (0, 1, 2, 3):
        rows = max(-(-size // 65536), 1)
        return oracle.gen(kind, 21 + kind + seed, 3, rows).reshape(-1)[:size].copy()
    if kind == "random":
        return np.random.default_rng(size + 7919 * seed).integers(0, 256, size, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(size, np.uint8)
    r = real_bytes()
    start = (seed * 7777) % max(r.size, 1)
    return np.resize(np.roll(r, -start), size) if size else np.zeros(0, np.uint8)


KINDS = [0, 1, 2, 3, "random", "zeros", "real"]
FIXED = [0, 1, 12, 13, 65536, 65547, 200000]


def message_mix(oracle, budget, seed):
    """Fixed edge lengths for every kind, then log-uniform random lengths up to 1 MiB until about `budget` bytes."""
    rng = np.random.default_rng(seed)
    msgs = [data_of(oracle, k, s, seed) for s in FIXED for k in KINDS]
    total = sum(m.size for m in msgs)
    i = 0
    while total < budget:
        size = int(np.exp(rng.uniform(0, np.log(1 << 20))))
        msgs.append(data_of(oracle, KINDS[i % len(KINDS)], size, seed + i))
        total += size
        i += 1
    rng.shuffle(msgs)
    return msgs


def small_mix(oracle, seed, count=64, top=5000):
    rng = np.random.default_rng(seed)
    return [data_of(oracle, KINDS[i % len(KINDS)], int(rng.integers(0, top)), seed + i) for i in range(count)]


def concat(msgs):
    msgs = [np.frombuffer(bytes(m), np.uint8) if not isinstance(m, np.ndarray) else m for m in msgs]
    offs = np.zeros(len(msgs) + 1, np.int64)
    offs[1:] = np.cumsum([m.size for m in msgs])
    data = np.concatenate(msgs) if msgs else np.zeros(0, np.uint8)
    return data.astype(np.uint8), offs


def split(data, offs):
    data = np.asarray(data)
    offs = np.asarray(offs)
    return [data[offs[i]:offs[i + 1]].tobytes() for i in range(offs.size - 1)]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def wrap_on_device(torch, msgs, hc=False):
    data, offs = concat(msgs)
    packed, poff = wr.wrap_device(_dev(torch, data), _dev(torch, offs), high_compression=hc)
    return packed.cpu().numpy(), poff.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("hc", [False, True])
def test_wrap_parity(oracle, hc):
    torch = _torch()
    msgs = message_mix(oracle, (3 << 20) if hc else (24 << 20), 101 + hc)
    packed, poff = wrap_on_device(torch, msgs, hc)
    assert poff[0] == 0 and poff[-1] == packed.size
    got = split(packed, poff)
    for i, m in enumerate(msgs):
        assert got[i] == expected_wrap(oracle, m, hc), (i, m.size, hc)
    # a subset against the host API itself
    sub = msgs[:12]
    w = LZ4Codec.WrapHC if hc else LZ4Codec.Wrap
    assert got[:12] == [w(m.tobytes()) for m in sub]
    assert got[:12] == LZ4Codec.WrapMany([m.tobytes() for m in sub], high_compression=hc)


@pytest.mark.gpu
@pytest.mark.parametrize("mapping", ["wave", "lane"])
def test_both_encoder_mappings(oracle, mapping):
    torch = _torch()
    msgs = small_mix(oracle, 7, count=300, top=20000)
    with ForcedMapping("LZ4HIP_ENCODER", mapping):
        packed, poff = wrap_on_device(torch, msgs, False)
        torch.cuda.synchronize()
    got = split(packed, poff)
    for i, m in enumerate(msgs):
        assert got[i] == expected_wrap(oracle, m, False), (mapping, i, m.size)


@pytest.mark.gpu
@pytest.mark.parametrize("mapping", ["wave", "lane"])
def test_both_decoder_mappings(oracle, mapping):
    torch = _torch()
    msgs = small_mix(oracle, 8, count=300, top=20000)
    packed, poff = wrap_on_device(torch, msgs, False)
    with ForcedMapping("LZ4HIP_DECODER", mapping):
        data, doff = wr.unwrap_device(_dev(torch, packed), _dev(torch, poff))
        torch.cuda.synchronize()
    assert split(data.cpu().numpy(), doff.cpu().numpy()) == [m.tobytes() for m in msgs]


@pytest.mark.gpu
def test_round_trips_on_a_side_stream(oracle):
    torch = _torch()
    side = torch.cuda.Stream()
    for hc, msgs in ((False, message_mix(oracle, 8 << 20, 5)), (True, small_mix(oracle, 6, count=200, top=30000)), (False, []),
                     (False, [np.zeros(0, np.uint8)] * 5)):
        data, offs = concat(msgs)
        x, o = _dev(torch, data), _dev(torch, offs)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            back, boff = wr.unwrap_device(*wr.wrap_device(x, o, high_compression=hc))
            ok = bool(torch.equal(back, x)) and bool(torch.equal(boff, o))
        assert ok, (hc, len(msgs))
    # the output of the host WrapMany
    msgs = small_mix(oracle, 9, count=100, top=70000)
    wrapped = LZ4Codec.WrapMany([m.tobytes() for m in msgs])
    packed, poff = concat(wrapped)
    data, doff = wr.unwrap_device(_dev(torch, packed), _dev(torch, poff))
    assert split(data.cpu().numpy(), doff.cpu().numpy()) == [m.tobytes() for m in msgs]


@pytest.mark.gpu
def test_foreign_messages(oracle):
    torch = _torch()
    a = data_of(oracle, 2, 5000)
    r, buf = oracle.compress_raw(a, 5000)
    assert 0 < r < 5000
    comp = buf[:r].tobytes()
    msgs = [
        header(5000, r) + comp + b"trailing bytes",                  # trailing bytes after a compressed payload
        header(5, 5) + b"hello" + b"\x00" * 9,                       # ... and after a raw one
        header(11, 11) + b"hello world",                             # payloadLength == originalLength
        header(-3, 4) + b"abcd",                                     # negative originalLength, valid raw payload
        header(-3, 0),                                               # ... and an empty payload
        header(0, 0),                                                # a wrapped empty message
        header(0, 0) + b"xyz",
        header(2, 6) + b"abcdef",                                    # payloadLength > originalLength: the payload as it is
        bytes(8),
    ]
    packed, poff = concat(msgs)
    data, doff = wr.unwrap_device(_dev(torch, packed), _dev(torch, poff))
    assert split(data.cpu().numpy(), doff.cpu().numpy()) == [LZ4Codec.Unwrap(m) for m in msgs]
    # empty batch
    data, doff = wr.unwrap_device(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert data.numel() == 0 and doff.tolist() == [0]


def _bad_block(original=100):
    """A payload the decoder must reject: one literal, then a match 65 535 bytes back."""
    return header(original, 10) + bytes([0x1F, 0x41, 0xFF, 0xFF]) + bytes(6)


def error_batch(oracle):
    """(messages, expected status per message): good messages mixed with every failure kind."""
    a = data_of(oracle, 2, 3000)
    r, buf = oracle.compress_raw(a, 3000)
    comp = buf[:r].tobytes()
    good = [header(3000, r) + comp, header(5, 5) + b"hello", bytes(8)]
    cases = [
        (good[0], 0), (b"1234567", _lib.WRAP_SIZE_INVALID), (good[1], 0), (b"", _lib.WRAP_SIZE_INVALID),
        (header(10, 11) + bytes(10), _lib.WRAP_CORRUPT_HEADER),      # payloadLength past the end
        (good[2], 0), (header(10, -1) + bytes(10), _lib.WRAP_CORRUPT_HEADER),   # negative payloadLength
        (good[0], 0), (_bad_block(), _lib.WRAP_CORRUPT_BLOCK),
        (header(3001, r) + comp, _lib.WRAP_CORRUPT_BLOCK),            # originalLength + 1 on a compressed message
        (header(2999, r) + comp, _lib.WRAP_CORRUPT_BLOCK),            # originalLength - 1
        (good[1], 0), (good[0], 0),
    ]
    return [c[0] for c in cases], [c[1] for c in cases], a.tobytes()


def _host_unwrap_exc(w):
    try:
        LZ4Codec.Unwrap(w)
    except ArgumentException as e:
        return str(e)
    return None


@pytest.mark.gpu
def test_errors(oracle):
    torch = _torch()
    msgs, want_status, a = error_batch(oracle)
    packed, poff = concat(msgs)
    data, doff, status = wr.unwrap_device(_dev(torch, packed), _dev(torch, poff), check=False)
    assert status.cpu().tolist() == want_status
    data, doff = data.cpu().numpy(), doff.cpu().numpy()
    got = split(data, doff)
    for i, (m, s) in enumerate(zip(msgs, want_status)):
        if s == 0:
            assert got[i] == LZ4Codec.Unwrap(m), i
        elif s != _lib.WRAP_CORRUPT_BLOCK:
            assert got[i] == b"", i                                  # header failures take no output
    # every suffix of the batch: the first failure is the lowest failing index, and raises what Unwrap raises for it
    for start in range(len(msgs)):
        sub = msgs[start:]
        fails = [i for i, s in enumerate(want_status[start:]) if s]
        p, o = concat(sub)
        if not fails:
            wr.unwrap_device(_dev(torch, p), _dev(torch, o))
            continue
        with pytest.raises(ArgumentException) as ei:
            wr.unwrap_device(_dev(torch, p), _dev(torch, o))
        first = fails[0]
        assert ei.value.message_index == first, start
        host_text = _host_unwrap_exc(sub[first])
        if int.from_bytes(sub[first][4:8], "little", signed=True) < 0 and len(sub[first]) >= 8:
            # negative payloadLength: the reference throws no ArgumentException of its own there (see include/lz4hip.h)
            assert str(ei.value) == "inputBuffer size is invalid or has been corrupted"
        else:
            assert str(ei.value) == host_text, (start, first)
    # the C entry points: info from the index, then after the decode
    L = _lib.lib()
    n = len(msgs)
    pd, od = _dev(torch, packed), _dev(torch, poff)
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    scratch = torch.empty(L.lz4hip_unwrap_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_unwrap_index_device(pd.data_ptr(), pd.numel(), od.data_ptr(), n, out_off.data_ptr(), st.data_ptr(), scratch.data_ptr(),
                                        scratch.numel(), info_dev.data_ptr(), None) == 0
    info = _lib.UnwrapInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    assert (info.messages, info.first_error, info.error) == (n, 1, _lib.WRAP_SIZE_INVALID)
    assert info.compressed == 6 and info.decoded_bytes == int(out_off[n])
    out = torch.empty(int(info.decoded_bytes), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_unwrap_decode_device(pd.data_ptr(), pd.numel(), od.data_ptr(), n, C.byref(info), scratch.data_ptr(), scratch.numel(),
                                         out.data_ptr(), out.numel() - 1, out_off.data_ptr(), st.data_ptr(), info_dev.data_ptr(),
                                         None) == _lib.E_ARGUMENT            # decoded_bytes > dst_cap is refused


@pytest.mark.gpu
def test_guard_bytes(oracle):
    torch = _torch()
    L = _lib.lib()
    msgs, want_status, _ = error_batch(oracle)
    msgs = msgs + LZ4Codec.WrapMany([m.tobytes() for m in small_mix(oracle, 13, count=40, top=9000)])
    want_status = want_status + [0] * 40
    packed, poff = concat(msgs)
    n = len(msgs)
    pd, od = _dev(torch, packed), _dev(torch, poff)
    out_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    scratch = torch.empty(L.lz4hip_unwrap_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    info_dev = torch.zeros(C.sizeof(_lib.UnwrapInfo), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_unwrap_index_device(pd.data_ptr(), pd.numel(), od.data_ptr(), n, out_off.data_ptr(), st.data_ptr(), scratch.data_ptr(),
                                        scratch.numel(), info_dev.data_ptr(), None) == 0
    info = _lib.UnwrapInfo.from_buffer_copy(info_dev.cpu().numpy().tobytes())
    total = int(info.decoded_bytes)
    dst = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    assert L.lz4hip_unwrap_decode_device(pd.data_ptr(), pd.numel(), od.data_ptr(), n, C.byref(info), scratch.data_ptr(), scratch.numel(),
                                         dst.data_ptr(), total, out_off.data_ptr(), st.data_ptr(), info_dev.data_ptr(), None) == 0
    torch.cuda.synchronize()
    host, offs = dst.cpu().numpy(), out_off.cpu().numpy()
    assert st.cpu().tolist() == want_status
    assert (host[total:] == 0xA5).all()
    # the good messages on either side of every failed one are intact; header failures take no bytes at all
    for i, m in enumerate(msgs):
        if want_status[i] == 0:
            assert host[offs[i]:offs[i + 1]].tobytes() == LZ4Codec.Unwrap(m), i
        elif want_status[i] != _lib.WRAP_CORRUPT_BLOCK:
            assert offs[i + 1] == offs[i], i
    # the wrap side: canaries past dst_off[n]
    data, woffs = concat(small_mix(oracle, 14, count=50, top=30000))
    m = woffs.size - 1
    bound = L.lz4hip_wrap_bound(m, data.size)
    wdst = torch.full((bound + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    woff = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    res = torch.empty(m, dtype=torch.int32, device="cuda")
    wscratch = torch.empty(L.lz4hip_wrap_scratch_bytes(m, data.size), dtype=torch.uint8, device="cuda")
    src, so = _dev(torch, data), _dev(torch, woffs)
    assert L.lz4hip_wrap_device(src.data_ptr(), data.size, so.data_ptr(), m, 0, wdst.data_ptr(), bound, woff.data_ptr(), res.data_ptr(),
                                wscratch.data_ptr(), wscratch.numel(), None) == 0
    torch.cuda.synchronize()
    w = int(woff[m])
    assert (wdst.cpu().numpy()[w:] == 0xA5).all()
    assert L.lz4hip_wrap_device(src.data_ptr(), data.size, so.data_ptr(), m, 0, wdst.data_ptr(), bound - 1, woff.data_ptr(), res.data_ptr(),
                                wscratch.data_ptr(), wscratch.numel(), None) == _lib.E_ARGUMENT
    assert L.lz4hip_wrap_device(src.data_ptr(), data.size, so.data_ptr(), m, 0, wdst.data_ptr(), bound, woff.data_ptr(), res.data_ptr(),
                                wscratch.data_ptr(), wscratch.numel() - 1, None) == _lib.E_ARGUMENT


@pytest.mark.gpu
def test_wrap_bad_offsets(oracle):
    torch = _torch()
    data = data_of(oracle, 2, 4000)
    offs = np.array([0, 1000, 500, 2000, 2000, 5000, 3000, 4000], np.int64)   # decreasing at 1, past the end at 4, decreasing at 5
    L = _lib.lib()
    n = offs.size - 1
    src, so = _dev(torch, data), _dev(torch, offs)
    bound = L.lz4hip_wrap_bound(n, data.size)
    dst = torch.full((bound + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    doff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    res = torch.empty(n, dtype=torch.int32, device="cuda")
    scratch = torch.empty(L.lz4hip_wrap_scratch_bytes(n, data.size), dtype=torch.uint8, device="cuda")
    assert L.lz4hip_wrap_device(src.data_ptr(), data.size, so.data_ptr(), n, 0, dst.data_ptr(), bound, doff.data_ptr(), res.data_ptr(),
                                scratch.data_ptr(), scratch.numel(), None) == 0
    torch.cuda.synchronize()
    r, d = res.cpu().numpy(), doff.cpu().numpy()
    assert [i for i in range(n) if r[i] == _lib.E_ARGUMENT] == [1, 4, 5]
    for i in (1, 4, 5):
        assert d[i + 1] == d[i]                                      # no bytes
    assert (dst.cpu().numpy()[bound:] == 0xA5).all()
    with pytest.raises(ArgumentException):
        wr.wrap_device(src, so)


@pytest.mark.gpu
def test_host_pair(oracle):
    torch = _torch()
    for hc in (False, True):
        msgs = small_mix(oracle, 20 + hc, count=80, top=40000)
        data, offs = concat(msgs)
        packed_d, poff_d = wr.wrap_device(_dev(torch, data), _dev(torch, offs), high_compression=hc)
        packed_h, poff_h = wr.wrap_host(data, offs, high_compression=hc)
        assert packed_h.tobytes() == packed_d.cpu().numpy().tobytes() and np.array_equal(poff_h, poff_d.cpu().numpy())
        back, boff = wr.unwrap_host(packed_h, poff_h)
        assert back.tobytes() == data.tobytes() and np.array_equal(boff, offs)
    msgs, want_status, _ = error_batch(oracle)
    packed, poff = concat(msgs)
    dd, dof, dst = wr.unwrap_device(_dev(torch, packed), _dev(torch, poff), check=False)
    hd, hof, hst = wr.unwrap_host(packed, poff, check=False)
    assert hst.tolist() == dst.cpu().tolist() == want_status and np.array_equal(hof, dof.cpu().numpy())
    good = [i for i, s in enumerate(want_status) if s == 0]
    assert [split(hd, hof)[i] for i in good] == [split(dd.cpu().numpy(), hof)[i] for i in good]
    with pytest.raises(ArgumentException) as ei:
        wr.unwrap_host(packed, poff)
    assert ei.value.message_index == 1 and str(ei.value) == "inputBuffer size is invalid"
    # the C call's return value is the first failure's status
    L = _lib.lib()
    n = len(msgs)
    out = np.zeros(int(hof[n]) + 16, np.uint8)
    o, s, info = np.zeros(n + 1, np.int64), np.zeros(n, np.int32), _lib.UnwrapInfo()
    assert L.lz4hip_unwrap_host(packed.ctypes.data, packed.size, poff.ctypes.data, n, out.ctypes.data, out.size, o.ctypes.data, s.ctypes.data,
                                C.byref(info)) == _lib.WRAP_SIZE_INVALID
    assert info.first_error == 1 and np.array_equal(o, hof)


@pytest.mark.gpu
def test_scale_d2_round_trip():
    """16 384 x 64 KiB of D2: enough compressed messages for the lane decoder's batch size."""
    torch = _torch()
    from lz4net_amd import batch
    n, B = 16384, 65536
    x = batch.synth(2, 77, 0, n).reshape(-1)
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * B
    before = _lib.dispatch_counts()
    packed, poff = wr.wrap_device(x, offs)
    back, boff = wr.unwrap_device(packed, poff)
    after = _lib.dispatch_counts()
    assert torch.equal(back, x) and torch.equal(boff, offs)
    assert after[_lib.K_DECODE_LANE] > before[_lib.K_DECODE_LANE]
    assert int(poff[n]) < x.numel()
