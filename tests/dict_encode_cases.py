"""TEST INFRASTRUCTURE shared by tests/test_dict_encode_ref.py, tests/test_simt_dict_encode.py and tests/test_gpu_dict_encode.py: blocks BUILT
for the edges of the dictionary encode (lz4hip_encode_batch_dict_*, encode_fast_block's DICT mode in lz4hip_encode.hpp over the view of
lz4hip_encode_dict.hpp), each with its dictionary, what the twin's parse (tests/dict_encode_ref.py) must look like for it -- asserted
when the case is built, so a case that misses its edge never reaches a test -- and which of the emulator's DICT counters
(LZ4HIP_STAT_ENCDICT, lz4hip::EncDictStat) it must move.  Also the emulator library of tests/simt/emu_dict_encode.cpp, built here with
build_emu's functions.

Block bytes are >= 0xA6 and the dictionaries of dict_cases.dictionary() are < 0xA5, so nothing matches by accident; a candidate only
survives in the primed table if no later position of the tail shares its bucket, so the builders LOOK for positions that do."""
import ctypes as C
import functools
import os
import sys

import numpy as np

import dict_cases
import dict_encode_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
REACH = ref.REACH
MAX_BLOCK = 12 * 1024
HOLE = 0x5C                   # what every output buffer is filled with
DICT_LENS = dict_cases.DICT_LENS + (3,)
DICT_ALIGN = dict_cases.DICT_ALIGN

# lz4hip::EncDictStat
(WORD_IN_DICT, WORD_STRADDLES, BYTE_IN_DICT, CANDIDATE, CANDIDATE_ZERO, REPROBE, CATCH_UP_INTO, CATCH_UP_AT_ZERO, CROSS_FIRST, CROSS_LATER,
 BLOCKS, N_STATS) = range(12)


@functools.lru_cache(maxsize=None)
def emu():
    """libsimt_dict_encode.so (tests/simt/emu_dict_encode.cpp)"""
    sys.path.insert(0, os.path.join(HERE, "simt"))
    import build_emu
    L = C.CDLL(build_emu._build_kernels("libsimt_dict_encode.so", "emu_dict_encode.cpp", ["-pthread"]))
    L.emu_encdict_sizeof.restype = C.c_int64
    assert L.emu_encdict_stats((C.c_ulonglong * 16)(), 0) == N_STATS
    return L


class Case:
    def __init__(self, note, dic, block, cap=None, moves=()):
        self.note, self.dic, self.block, self.moves = note, dic, bytes(block), tuple(moves)
        assert len(self.block) <= MAX_BLOCK, note
        self.cap = ref.bound(len(self.block)) if cap is None else cap
        self.dict_len = int(dic.size)
        self.T = min(self.dict_len, REACH)


def _hi(rng, n, lo=0xA6, hi=0x100):
    return bytes(rng.integers(lo, hi, n, dtype=np.uint8))


def _trace(dic, block):
    t = []
    r, b = ref.encode(block, dic.tobytes(), trace=t)
    assert r == len(b) > 0
    return t


def _survivors(dic, need):
    """positions s of the tail, highest first, that the primed table holds and that have `need` bytes behind them inside the tail"""
    tail = ref.tail_of(dic.tobytes())
    table = ref.primed_table(dic.tobytes())
    s = np.unique(table[table > 0].astype(np.int64))[::-1]
    return [int(p) for p in s if p + need <= len(tail)]


def generic(dict_len):
    """the cases of the seeded dictionary of that length"""
    rng = np.random.default_rng(7000 + dict_len)
    dic = dict_cases.dictionary(dict_len)
    tail = ref.tail_of(dic.tobytes())
    T = len(tail)
    out = []
    for n in (0, 1, 12, 13, 14, 100):
        out.append(Case("n = %d, nothing to find" % n, dic, _hi(rng, n), moves=(BLOCKS,) if n >= 13 and T else ()))
    if T == 0:
        out.append(Case("no dictionary: text", dic, (b"the quick brown fox " * 40)[:777]))
        out.append(Case("no dictionary: a block that does not fit", dic, _hi(rng, 300), cap=200))
        return out
    surv = _survivors(dic, 12)
    if surv:                                                          # a candidate inside the dictionary
        s = surv[0]
        blk = _hi(rng, 20) + tail[s:s + 12] + _hi(rng, 20)
        t = _trace(dic, blk)
        assert t and t[0][:3] == (T, T + 20, s) and t[0][3] >= 12 and t[0][4] == 0, (dict_len, t)
        out.append(Case("a candidate inside the dictionary", dic, blk, moves=(CANDIDATE, WORD_IN_DICT)))
        r, _ = ref.encode(blk, dic.tobytes())
        out.append(Case("dst_cap at exactly the result", dic, blk, cap=r, moves=(CANDIDATE,)))
        out.append(Case("dst_cap one below the result", dic, blk, cap=r - 1))
        assert ref.encode(blk, dic.tobytes(), cap=r)[0] == r and ref.encode(blk, dic.tobytes(), cap=r - 1)[0] == 0
    # a forward count that starts in the dictionary and crosses T: in round `rnd` of the count, the straddling dword in lane `lane`
    for rnd in (0, 1):
        for lane in (0, 31, 63):
            for k in [4 + 256 * r + 4 * lane + sub for r in ((0,) if rnd == 0 else (1, 2, 3)) for sub in (2, 1, 3)]:
                if k > T or ref.primed_table(dic.tobytes())[ref._hash(ref._r32(tail, T - k))] != T - k:
                    continue
                a = _hi(rng, 24, 0xA6, 0xD0)
                blk = a + tail[T - k:] + a + _hi(rng, 20, 0xD0)
                t = _trace(dic, blk)
                assert t[0] == (T, T + 24, T - k, k + 24, 0), (dict_len, k, t)
                out.append(Case("the count crosses T in round %d, lane %d straddles (k = %d)" % (rnd, lane, k), dic, blk,
                                moves=(CANDIDATE, WORD_STRADDLES, CROSS_LATER if rnd else CROSS_FIRST)))
                break
    # the block is the dictionary's last m bytes repeated: zero literals, one match from T across the boundary
    for m in (5, 8, 300):
        if m <= T and ref.primed_table(dic.tobytes())[ref._hash(ref._r32(tail, T + 1 - m))] == T + 1 - m:
            blk = (tail[T - m:] * (2000 // m + 1))[:2000]
            t = _trace(dic, blk)
            assert t == [(T, T, T - m, 2000 - 5, 1)], (dict_len, m, t)
            out.append(Case("the last %d bytes repeated" % m, dic, blk, moves=(CANDIDATE, BYTE_IN_DICT) + (() if m == 5 else (CROSS_LATER if m - 5 >= 256 else CROSS_FIRST,))))   # (the count starts m - 5 bytes before T)
    # the catch-up steps the ref side from the block back into the dictionary
    j = min(3, T)
    c = _hi(rng, 12, 0xA6, 0xD0)
    blk = c + _hi(rng, 10, 0xD0, 0xE8) + tail[T - j:] + c + _hi(rng, 20, 0xE8)
    t = _trace(dic, blk)
    if T >= 4:
        assert t[0] == (T, T + 22, T - j, 12 + j, j), (dict_len, t)
        out.append(Case("the catch-up goes back into the dictionary", dic, blk, moves=(CATCH_UP_INTO, BYTE_IN_DICT)))
    else:                                                             # (the whole tail is in front: V[0 .. 4) is found through its empty bucket first)
        assert t[0] == (T, T + 22, 0, 12 + T, 0), (dict_len, t)
        out.append(Case("T = %d: the tail and the block's start again" % T, dic, blk, moves=(CANDIDATE_ZERO, WORD_STRADDLES)))
    if T < 4:                                                         # the candidate word straddles T, out of an empty bucket
        r = _hi(rng, 10, 0xA6, 0xD0)
        blk = r + tail + r[:8 - T] + _hi(rng, 20, 0xD0)
        t = _trace(dic, blk)
        assert t[0] == (T, T + 10, 0, 8, 0), (dict_len, t)
        out.append(Case("T = %d: the candidate at position 0 straddles T" % T, dic, blk, moves=(CANDIDATE_ZERO, CANDIDATE, WORD_STRADDLES)))
    if 16 <= T <= 60000 and ref.primed_table(dic.tobytes())[ref._hash(ref._r32(tail, 0))] == 0:
        blk = _hi(rng, 10) + tail[:12] + _hi(rng, 20)
        t = _trace(dic, blk)
        assert t[0] == (T, T + 10, 0, 12, 0), (dict_len, t)
        out.append(Case("the position-0 candidate of a bucket that holds 0 matches", dic, blk, moves=(CANDIDATE_ZERO,)))
    if 16 <= T <= 60000 and ref.primed_table(dic.tobytes())[ref._hash(ref._r32(tail, 1))] == 1:
        for lead in range(62, 72):                                    # a probe that lands ONE byte behind the copy of the tail's start
            blk = _hi(rng, lead) + tail[:12] + _hi(rng, 20)
            t = _trace(dic, blk)
            if t and t[0] == (T, T + lead, 0, 12, 1):
                out.append(Case("the catch-up is stopped by ref > 0 at V[0]", dic, blk, moves=(CATCH_UP_AT_ZERO, BYTE_IN_DICT)))
                break
    surv = _survivors(dic, 17)
    if len(surv) >= 2:                                                # the zero-literal re-probe hits a candidate inside the dictionary
        for s2 in surv[1:]:
            s1 = surv[0]
            blk = _hi(rng, 20) + tail[s1:s1 + 16] + tail[s2:s2 + 16] + _hi(rng, 20)
            t = _trace(dic, blk)
            if len(t) >= 2 and t[0][:4] == (T, T + 20, s1, 16) and t[1][:4] == (T + 36, T + 36, s2, 16):
                out.append(Case("the re-probe hits a candidate inside the dictionary", dic, blk, moves=(REPROBE, CANDIDATE)))
                break
    # records made of the dictionary's phrases, as the populations of DESIGN.md 7 are
    parts = []
    while sum(map(len, parts)) < 3000 and T >= 64:
        at = int(rng.integers(0, T - 40))
        parts += [tail[at:at + int(rng.integers(6, 40))], _hi(rng, int(rng.integers(0, 9)))]
    if parts:
        out.append(Case("phrases of the dictionary", dic, b"".join(parts), moves=(CANDIDATE,)))
        blk = out[-1].block
        out.append(Case("phrases of the dictionary, dst_cap at the bound", dic, blk, cap=ref.bound(len(blk))))
    return out


def far_dictionary(dict_len):
    """a dictionary whose FIRST reachable bytes stay in the primed table: 64 distinct bytes, then one byte repeated (one bucket)"""
    assert dict_len >= REACH
    front = bytes(range(0x30, 0x70))
    return np.frombuffer(bytes([0xEE]) * (dict_len - REACH) + front + b"\x01" * (REACH - 64), np.uint8).copy()


def far(dict_len):
    """the furthest offset: 65 535 taken, the same data at 65 536 refused"""
    rng = np.random.default_rng(8000 + dict_len)
    dic = far_dictionary(dict_len)
    tail = ref.tail_of(dic.tobytes())
    T = REACH
    assert all(int(ref.primed_table(dic.tobytes())[ref._hash(ref._r32(tail, p))]) == p for p in range(20, 30))
    taken = _hi(rng, 20) + tail[20:32] + _hi(rng, 20)
    t = _trace(dic, taken)
    assert t == [(T, T + 20, 20, 12, 0)] and T + 20 - 20 == REACH, t
    refused = _hi(rng, 21) + tail[20:32] + _hi(rng, 20)
    assert _trace(dic, refused) == []
    return [Case("a match at distance 65 535 is taken", dic, taken, moves=(CANDIDATE, WORD_IN_DICT)),
            Case("the same data at distance 65 536 is refused", dic, refused, moves=(WORD_IN_DICT,))]


@functools.lru_cache(maxsize=None)
def cases(group):
    """group: ("generic", dict_len) or ("far", dict_len)"""
    return tuple(generic(group[1]) if group[0] == "generic" else far(group[1]))


GROUPS = tuple(("generic", n) for n in DICT_LENS) + tuple(("far", n) for n in (65535, 65536, 70000))
IDS = ["%s-%d" % g for g in GROUPS]


@functools.lru_cache(maxsize=None)
def expected(oracle_compress, group):
    """[(result, bytes)] per case: the twin's, or with no dictionary the plain call's (the reference's, 64k variant for these lengths)"""
    out = []
    for c in cases(group):
        if c.dict_len == 0:
            r, buf = oracle_compress(np.frombuffer(c.block, np.uint8), c.cap)
            out.append((r, bytes(buf[:r])))
        else:
            out.append(ref.encode(c.block, c.dic.tobytes(), cap=c.cap))
    return out


def check(oracle, group, encode, only=None, align=0, one_by_one=False):
    """encode(blocks, caps, dic, align) -> (results, [cap + 64 output bytes per block]) over the group's cases (or those of `only`):
    results and bytes equal the expected ones, nothing is written at or past dst_cap, and what fits decodes back by the twin decoder"""
    import lz4f_ref
    cs = cases(group)
    want = expected(oracle.compress_raw, group)
    idx = list(range(len(cs))) if only is None else list(only)
    runs = [[i] for i in idx] if one_by_one else [idx]
    for run in runs:
        res, outs = encode([cs[i].block for i in run], [cs[i].cap for i in run], cs[run[0]].dic, align)
        for i, r, o in zip(run, res, outs):
            c, (wr, wb) = cs[i], want[i]
            assert int(r) == wr, (group, c.note, int(r), wr)
            assert bytes(o[:wr]) == wb, (group, c.note, "bytes")
            assert (np.asarray(o[max(c.cap, 0):]) == HOLE).all(), (group, c.note, "wrote at or past dst_cap")
            if wr > 0:
                assert lz4f_ref.decode_block(wb, len(c.block), history=ref.tail_of(c.dic.tobytes())) == (len(c.block), c.block), (group, c.note)
