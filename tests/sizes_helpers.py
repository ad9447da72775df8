"""TEST INFRASTRUCTURE for the size query of a block batch (lz4hip_decoded_sizes_*): the corpora of tests/test_decoded_sizes.py (CPU,
under the SIMT emulator) and tests/test_gpu_decoded_sizes.py (the device), what the reference returns for every block of them, and
the ctypes front of the size query's entry points in tests/simt/libsimt_framing.so."""
import ctypes as C
import functools

import numpy as np

import emu_lib
from emu_lib import E_ARGUMENT, GUARD, EmuHostRun  # noqa: F401  (E_ARGUMENT: the tests take it from here)
from lz4net_amd._lib import Batch, SizesInfo

FUZZ_SEED, FUZZ_BLOCKS = 20261017, 20480


# ---- the reference ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def codec():
    """The reference's own C where it could be built (oracle/_ref), else the port that tests/test_oracle_vs_ref.py holds against it."""
    from oracle.oracle import Oracle, Reference
    return Reference() if Reference.available() else Oracle()


def compress(raw, hc=False):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    cap = raw.size + raw.size // 255 + 16
    ret, out = codec().compress_raw(raw, cap, hc)
    assert 0 < ret <= cap, ret
    return out[:ret].copy()


def reference_sizes(blocks):
    """LZ4_uncompress_unknownOutputSize(src, dest, len, 255 * len + 64) for every block, into a real buffer of that size."""
    decu = codec()._decu
    longest = max([len(b) for b in blocks] + [0])
    out = np.empty(255 * longest + 64 + 64, np.uint8)
    res = np.empty(len(blocks), np.int32)
    for i, b in enumerate(blocks):
        src = np.zeros(len(b) + 64, np.uint8)
        src[:len(b)] = b
        res[i] = decu(src.ctypes.data, out.ctypes.data, len(b), 255 * len(b) + 64)
    return res


# ---- corpora ----------------------------------------------------------------------------------------------------------------
def data(oracle, dist, length, seed=7):
    return oracle.gen(dist, seed, 3, 1, length=max(length, 1))[0, :length]


def encoder_corpus(oracle):
    """fast and HC output for sources of every length the end rules turn on, of the four distributions"""
    blocks = []
    for length in (0, 1, 12, 13, 64, 65535, 65536, 65547, 200000):
        for dist in (0, 1, 2, 3):
            for hc in (False, True):
                blocks.append(compress(data(oracle, dist, length), hc))
    return blocks


def hand_blocks():
    b = lambda *x: np.array(x, np.uint8)                                      # noqa: E731
    out = [b(0x00),                                                            # the one-byte block
           b(0xF0, 255, 255, 255),                                             # a literal-length run of 255s that ends exactly at iend
           b(0xF0, 255, 255, 255, 255, 255, 255, 255, 255),                    # ... the same through the dword step
           b(0xF0), b(0xF0, 3), b(0x0F), b(0xFF)]
    for extra in (4, 5, 6):                                                    # a last literal run ending at iend - 1, iend, iend + 1
        out.append(b(0x50, *range(extra)))
    tail = (0x50, 1, 2, 3, 4, 5)
    out.append(b(0x10, 0x30, 1, 0, *tail))                                     # ip + ll == iend - 8: a match follows
    out.append(b(0x10, 0x30, 1, 0, *tail[:-1]))                                # ip + ll == iend - 7: the last sequence, and not at iend
    out.append(b(0x10, 0x30, 2, 0, *tail))                                     # offset == produced + 1
    out.append(b(0x10, 0x30, 0, 0, *tail))                                     # offset 0
    out.append(b(0x20, 0x30, 0x31, 2, 0, *tail))                               # offset == produced (two literals)
    out.append(b(0x20, 0x30, 0x31, 3, 0, *tail))
    out.append(b(0x00, 0, 0, *tail))                                           # no literal at all: offset 0 == produced, offset 1 > produced
    out.append(b(0x00, 1, 0, *tail))
    for k in (1, 2, 3, 4, 5, 7, 8, 9, 13, 300):                                # a match-length run of 255s that meets iend - 6 ...
        out.append(b(0x1F, 0x41, 1, 0, *([255] * k), *tail))
        out.append(b(0x1F, 0x41, 1, 0, *([255] * k), 9, *tail))                # ... ends one byte before it ...
        out.append(b(0x1F, 0x41, 1, 0, *([255] * k), *tail[:-1]))              # ... and leaves a last sequence that is not at iend
    out.append(compress(np.zeros(1 << 20, np.uint8)))                          # 1 MiB out of a few KiB of length bytes
    out.append(compress(np.zeros(1 << 20, np.uint8), hc=True))
    return out


def prefixes(oracle):
    """every prefix of two small encoder outputs: a truncation at every byte of every element"""
    out = []
    for dist, n in ((2, 700), (3, 500)):
        comp = compress(data(oracle, dist, n, seed=11))
        out += [comp[:k].copy() for k in range(len(comp) + 1)]
    return out


def window_blocks(window):
    """Blocks that walk up to a window edge in short sequences of 3 and 4 bytes -- every phase from 10 to 3 * window + 8 bytes -- and then
    put a token, literal-length bytes (also through the dword step), an offset, match-length bytes and literal runs on it: whatever the
    window's base was when it was filled, some block has each element straddling its last byte, at the first window and the second."""
    seq3, seq4 = [0x00, 1, 0], [0x10, 0x61, 1, 0]
    tails = [[0x0F, 1, 0, 255, 255, 7],
             [0xF0, 255, 2] + [0x62] * 272 + [1, 0],
             [0xF0, 255, 255, 255, 255, 255, 0] + [0x63] * (15 + 5 * 255) + [1, 0],
             [0xE0] + [0x64] * 14 + [1, 0],
             [0x0F, 1, 0] + [255] * 9 + [3],
             [0x7F] + [0x65] * 7 + [1, 0, 255, 0],
             [0xFF, 0] + [0x66] * 15 + [1, 0, 4]]
    end = [0x00, 1, 0, 0x50, 1, 2, 3, 4, 5]                                      # (a match, then the last literals: keeps the tail's sequence valid)
    out = []
    for j in range(10, 3 * window + 9):
        fours = next(f for f in range(1, j // 4 + 1) if (j - 4 * f) % 3 == 0)  # the first sequence has a literal: offset 1 <= produced
        head = seq4 * fours + seq3 * ((j - 4 * fours) // 3)
        assert len(head) == j
        for t in tails:
            out.append(np.array(head + t + end, np.uint8))
    return out


def fuzz_blocks(oracle, count=FUZZ_BLOCKS, seed=FUZZ_SEED):
    """`count` blocks of 16 to 600 bytes: valid encoder output, and mutations of it by byte flips, truncation and extension"""
    rng = np.random.default_rng(seed)
    raw = np.concatenate([oracle.gen(d, 99, 0, 4)[:, :65536].reshape(-1) for d in (2, 3)])
    pool = []
    while len(pool) < 1024:
        n = int(rng.integers(20, 1600))
        at = int(rng.integers(0, raw.size - n))
        piece = raw[at:at + n].copy()
        if rng.integers(0, 4) == 0:
            piece[n // 3:] = piece[n // 3 - 1]                                # a long run: length bytes
        comp = compress(piece, hc=bool(rng.integers(0, 2)))
        if 16 <= len(comp) <= 600:
            pool.append(comp)
    out = []
    while len(out) < count:
        v = pool[int(rng.integers(0, len(pool)))].copy()
        kind = int(rng.integers(0, 4))
        if kind == 1:
            for _ in range(int(rng.integers(1, 4))):
                v[int(rng.integers(0, len(v)))] = int(rng.integers(0, 256))
        elif kind == 2:
            v = v[:int(rng.integers(16, len(v) + 1))]
        elif kind == 3:
            v = np.concatenate([v, rng.integers(0, 256, int(rng.integers(1, 601 - len(v) if len(v) < 600 else 2)), dtype=np.uint8)])[:600]
        out.append(np.ascontiguousarray(v))
    return out


# ---- layouts ----------------------------------------------------------------------------------------------------------------
def pack_offsets(blocks, odd=True, rng=None):
    """The blocks in one buffer at offsets of their own; odd=True: every block starts at an odd byte offset, gaps of garbage between them."""
    rng = rng or np.random.default_rng(5)
    off = np.zeros(len(blocks), np.int64)
    at = 1 if odd else 0
    for i, b in enumerate(blocks):
        off[i] = at
        at += len(b) + (int(rng.integers(0, 3)) * 2 if odd else 0)
        if odd and at % 2 == 0:
            at += 1
    buf = rng.integers(0, 256, at + 1, dtype=np.uint8)
    for i, b in enumerate(blocks):
        buf[off[i]:off[i] + len(b)] = b
    return buf, off, np.array([len(b) for b in blocks], np.int32)


def expected(results):
    """(dst_cap, dst_off, decoded_bytes, first_error, error) that go with per-block results"""
    results = np.asarray(results, np.int32)
    cap = np.maximum(results, 0).astype(np.int32)
    off = np.zeros(len(results) + 1, np.int64)
    np.cumsum(cap, dtype=np.int64, out=off[1:])
    bad = np.flatnonzero(results < 0)
    first = int(bad[0]) if len(bad) else -1
    return cap, off, int(off[-1]), first, int(results[first]) if len(bad) else 0


# ---- the emulator ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emu():
    lib = emu_lib.framing()
    lib.emu_sizes_window.restype = C.c_int64
    lib.emu_sizes_scratch_bytes.restype = C.c_int64
    lib.emu_sizes_scratch_bytes.argtypes = [C.c_int64]
    lib.emu_decoded_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    lib.emu_decoded_sizes_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.POINTER(EmuHostRun)]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data


class Outputs:
    """result, dst_off, dst_cap and info of one call, each between guard values and each optional"""

    def __init__(self, n, want=("result", "dst_off", "dst_cap", "info")):
        self.n = n
        self.result = np.full(n + 2, -77, np.int32) if "result" in want else None
        self.dst_off = np.full(n + 3, -77, np.int64) if "dst_off" in want else None
        self.dst_cap = np.full(n + 2, -77, np.int32) if "dst_cap" in want else None
        self.info = SizesInfo(-7, -7, -7, -7, -7) if "info" in want else None

    def ptr(self, name):
        a = getattr(self, name)
        return None if a is None else a.ctypes.data + a.itemsize

    def info_ptr(self):
        return None if self.info is None else C.addressof(self.info)

    def check(self, results):
        cap, off, total, first, error = expected(results)
        n = self.n
        if self.result is not None:
            assert np.array_equal(self.result[1:n + 1], results) and self.result[0] == -77 and self.result[n + 1] == -77
        if self.dst_cap is not None:
            assert np.array_equal(self.dst_cap[1:n + 1], cap) and self.dst_cap[0] == -77 and self.dst_cap[n + 1] == -77
        if self.dst_off is not None:
            assert np.array_equal(self.dst_off[1:n + 2], off) and self.dst_off[0] == -77 and self.dst_off[n + 2] == -77
        if self.info is not None:
            got = (self.info.blocks, self.info.decoded_bytes, self.info.first_error, self.info.error, self.info.reserved)
            assert got == (n, total, first, error, 0), (got, (n, total, first, error, 0))


def make_batch(buf, off=None, stride=0, lens=None, len_all=0, n=0, result=None):
    return Batch(src=_p(buf), src_off=_p(off), src_stride=stride, src_len=_p(lens), dst=None, dst_off=None, dst_stride=0, dst_cap=None,
                 dst_cap_all=0, src_len_all=len_all, result=result, n_blocks=n)


def emu_sizes(batch, out, groups=0, scratch_bytes=None):
    """framing::decoded_sizes under the emulator; returns (rc, error text); the scratch is checked for writes outside it"""
    n = batch.n_blocks
    need = emu().emu_sizes_scratch_bytes(n)
    nbytes = need if scratch_bytes is None else scratch_bytes
    scratch = np.full(max(nbytes, 0) + 512, GUARD, np.uint8)
    base = (scratch.ctypes.data + 255) // 256 * 256
    lead = base - scratch.ctypes.data
    text = C.create_string_buffer(200)
    batch.result = out.ptr("result")
    rc = emu().emu_decoded_sizes(C.addressof(batch), out.ptr("dst_off"), out.ptr("dst_cap"), base if nbytes > 0 else None, nbytes,
                                 out.info_ptr(), groups, text, 200)
    assert (scratch[:lead] == GUARD).all() and (scratch[lead + max(nbytes, 0):] == GUARD).all(), "wrote outside the scratch"
    return rc, text.value.decode()


def emu_sizes_host(batch, out, groups=0, pool_floor=-1):
    run = EmuHostRun()
    batch.result = out.ptr("result")
    rc = emu().emu_decoded_sizes_host(C.addressof(batch), out.ptr("dst_off"), out.ptr("dst_cap"), out.info_ptr(), groups, pool_floor, C.byref(run))
    return rc, run
