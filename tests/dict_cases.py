"""TEST INFRASTRUCTURE for tests/test_simt_dict_decode.py and tests/test_gpu_dict_decode.py, which are one design: LZ4 blocks decoded against
a SHARED DICTIONARY (lz4hip_decode_batch_dict_*, decode_block's DICT mode in lz4hip_decode.hpp), BUILT sequence by sequence
(lz4f_built.sequence, lane_flush_cases.emit) so that every path of the wavefront decoder meets a source before the block on both
sides of its edges: how far a match may reach, matches that begin in the dictionary and end in the block, the LDS mirror's preload and
what each path takes from it, and what must come from memory after a long copy.  Every block decodes to at most 12 KiB.

TRUTH.  The CPU oracle has no dictionary form, so truth comes from SPLICING: for a block B and the prefix P -- the dictionary's reachable
tail, its last 65 535 bytes -- the plain block B' is B with P in front of its first sequence's literals.  The oracle's two decoders on B'
give P + (what B decodes to against the dictionary), and their return values are B's shifted by len(B') - len(B) (a count of output
bytes: by len(P)).  The twin decoder lz4f_ref.decode_block(B, cap, history=P) is asserted against that on every case, and where
liblz4 is installed LZ4_decompress_safe_usingDict on the valid ones: all on the CPU, before a kernel sees a case.  Damaged blocks (two
per family: cut inside the last literals, the last token changed) expect what the oracle says of their spliced form.

A family is a list of cases plus what the emulator's DICT counters (LZ4HIP_STAT_DICT, lz4hip::DictStat) must show for it: the counters
that must move, and pairs (a, b, counter) of cases on the two sides of one edge, for which the counter of case a decoded alone must be
BELOW that of case b decoded alone."""
import ctypes as C
import ctypes.util
import os

import numpy as np

import emu_lib
import lz4f_ref
from lane_flush_cases import TAIL, emit, far_block, length_block
from lz4f_built import sequence
from wave_decode_cases import short_run

RING = 4096                  # kWaveRingBytes
SHORT_SERVED = RING - 20     # kWaveRingShortServed
REACH = 65535
EXTRA = 5                    # spare capacity of the unknown-size decodes
MAX_OUT = 12 * 1024
HOLE = 0xA5                  # what every output buffer is filled with; no built byte has this value
DICT_LENS = (0, 1, 17, 4095, 4096, 4097, 65535, 65536, 70000)
DICT_ALIGN = (0, 1, 3)       # the dictionary's first byte, from a 16-byte boundary

# lz4hip::DictStat
PRELOAD, BURST_MIRROR, SHORT_MIRROR, GEN_MEMORY, GEN_MIRROR, LONG_BYTES, LONG_COPIES, REFUSED, N_STATS = range(9)

_MASTER = np.random.default_rng(20240229).integers(1, HOLE, DICT_LENS[-1], dtype=np.uint8)


def dictionary(dict_len):
    """the dictionary of that length: made from a seed, and every length's ends with the same bytes"""
    return _MASTER[_MASTER.size - dict_len:].copy()


def prefix_of(dict_len):
    """P: the bytes of that dictionary a match can reach"""
    return bytes(dictionary(dict_len)[-REACH:]) if dict_len else b""


def _rb(rng, n):
    return bytes(rng.integers(1, HOLE, n, dtype=np.uint8))


class Case:
    """seqs = [(literals, offset, match length)], the last literals, the dictionary's length.  block: B.  spliced: B'.  raw: what B decodes
    to (None: the case is refused, or damaged).  first: the bytes of B's first sequence up to and including its literals."""

    def __init__(self, seqs, tail, dict_len, valid=True, note=""):
        self.seqs, self.tail, self.dict_len, self.note = seqs, tail, dict_len, note
        self.block = b"".join(sequence(*s) for s in seqs) + sequence(tail)
        self.cap = sum(len(lit) + ml for lit, _, ml in seqs) + len(tail)
        self.raw = None
        if valid:
            lit0, off0, ml0 = seqs[0]
            built, out = emit([(prefix_of(dict_len) + lit0, off0, ml0)] + list(seqs[1:]), tail)
            assert bytes(built) == self.spliced(self.block)
            self.raw = out[len(prefix_of(dict_len)):]
            assert self.raw.size == self.cap

    def _head(self):
        """(bytes of the first token and its length bytes, the first literals)"""
        lit0 = self.seqs[0][0]
        n = 1 + (0 if len(lit0) < 15 else 1 + (len(lit0) - 15) // 255)
        return n, lit0

    def spliced(self, block):
        """B' of `block` (B, or a damaged copy that keeps B's first token and literals): P in front of the first literals"""
        n, lit0 = self._head()
        p = prefix_of(self.dict_len)
        assert bytes(block[:n + len(lit0)]) == self.block[:n + len(lit0)]
        head = sequence(p + lit0, 1, 4)[:-2]                 # token, length bytes, literals; the match nibble is the block's own
        head = bytes([head[0] & 0xF0 | block[0] & 0x0F]) + head[1:]
        return head + bytes(block[n + len(lit0):])

    def damaged(self, k):
        """a damaged copy: cut inside the last literals (k = 0), the last token changed (k = 1)"""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        b = bytearray(self.block)
        if k == 0:
            b = b[:len(b) - 7]
        else:
            b[len(b) - len(sequence(self.tail))] ^= 0x5F
        assert len(b) >= sum(self._head()[:1]) + len(self._head()[1]) + 3
        c.block, c.raw, c.note = bytes(b), None, self.note + " damaged %d" % k
        return c


class Family:
    def __init__(self):
        self.cases, self.moves, self.pairs = [], [], []

    def add(self, seqs, tail, dict_len, valid=True, note=""):
        self.cases.append(Case(seqs, tail, dict_len, valid, note))
        return len(self.cases) - 1

    def pair(self, a, b, counter):
        self.pairs.append((a, b, counter))

    def damage(self):
        """two damaged blocks: of the first and of the last valid case"""
        good = [c for c in self.cases if c.raw is not None]
        self.cases += [good[0].damaged(0), good[-1].damaged(1)]
        return self


def _tail(rng, n=TAIL):
    return _rb(rng, n)


# ---- reach -------------------------------------------------------------------------------------------------------------------------------
def reach():
    """the first sequence without literals at offset min(dict_len, 65 535) -- accepted -- and one byte further -- refused with a plain
    block's code; offset 65 535 at op = 0 is the format's furthest"""
    f, rng = Family(), np.random.default_rng(1)
    for L in DICT_LENS[1:]:
        r = min(L, REACH)
        a = f.add([(b"", r, 8)], _tail(rng), L, note="reach %d" % L)
        if r < REACH:
            b = f.add([(b"", r + 1, 8)], _tail(rng), L, valid=False, note="reach %d + 1" % L)
            f.pair(a, b, REFUSED)
        # the same behind literals and a sequence of the block's own: op > 0
        if r + 17 <= REACH:
            f.add([(_rb(rng, 9), 4, 6), (b"ab", 15 + 2 + r, 5)], _tail(rng), L, note="reach %d from op 15" % L)
        if r + 17 < REACH:
            f.add([(_rb(rng, 9), 4, 6), (b"ab", 15 + 2 + r + 1, 5)], _tail(rng), L, valid=False, note="reach %d + 1 from op 15" % L)
    f.moves = [PRELOAD, REFUSED]
    return f.damage()


# ---- straddle ----------------------------------------------------------------------------------------------------------------------------
def straddle():
    """matches that begin in the dictionary and end in the block: ll + ml on both sides of the general path's 64, the long path's
    lengths, and overlapping offsets whose period runs through the dictionary, this sequence's literals and the match itself"""
    f, rng = Family(), np.random.default_rng(2)
    at = {}
    for total in (63, 64, 65):
        at[total] = f.add([(_rb(rng, 10), 30, total - 10)], _tail(rng), 4097, note="ll + ml = %d" % total)
    f.pair(at[64], at[65], LONG_COPIES)
    f.pair(at[65], at[64], GEN_MIRROR)
    for ml in (300, 1024, 3000):
        f.add([(_rb(rng, 5), 105, ml)], _tail(rng), 4097, note="long, overlapping, %d" % ml)
        f.add([(_rb(rng, 5), 2005, ml)], _tail(rng), 4097, note="long, 2 000 in the dictionary, %d" % ml)
        f.add([(_rb(rng, 5), 4005, ml)], _tail(rng), 65535, note="long, all in the dictionary, %d" % ml)
    for off in range(1, 18):
        for ml in (40, 300):
            f.add([(b"", off, ml)], _tail(rng), 17, note="overlap %d x %d at op 0" % (off, ml))
            if off > 3:
                f.add([(b"xyz", off, ml)], _tail(rng), 4096, note="overlap %d x %d, lit_end 3" % (off, ml))
    f.moves = [GEN_MIRROR, LONG_BYTES, LONG_COPIES]
    return f.damage()


# ---- mirror ------------------------------------------------------------------------------------------------------------------------------
def mirror():
    """sources at op - 4 095, op - 4 096 and op - 4 097 with op at 0, 1, 20, 63 and 64 (blocks too small for a burst: the short and the
    general path; and with room for one), both sides of the short path's op - 4 096 + 20 and of the general path's match_end - 4 096"""
    f, rng = Family(), np.random.default_rng(3)
    for L in (4097, 65535):
        for op in (0, 1, 20, 63, 64):
            for d in (4095, 4096, 4097):
                f.add([(_rb(rng, op), op + d, 8)], _tail(rng), L, note="source op - %d, op = %d literals" % (d, op))
                f.add([(_rb(rng, op), op + d, 8)] + short_run(rng, 96, op + 8), _tail(rng, 120), L, note="source op - %d, op = %d, a burst" % (d, op))
                if op >= 20:                                       # op bytes of the block's own in front: a sequence of its own
                    f.add([(_rb(rng, op - 4), 3, 4), (b"", op + d, 8)], _tail(rng), L, note="source op - %d behind %d bytes" % (d, op))
    # the short path: a source at op - 4 076 is the mirror's, one byte further back the general path's (which the mirror still serves)
    a = f.add([(b"", SHORT_SERVED, 8)], _tail(rng, 40), 4097, note="short path, op - 4 096 + 20")
    b = f.add([(b"", SHORT_SERVED + 1, 8)], _tail(rng, 40), 4097, note="short path, one further")
    f.pair(b, a, SHORT_MIRROR)
    f.pair(a, b, GEN_MIRROR)
    a = f.add([(b"ab", 2 + SHORT_SERVED, 8)], _tail(rng, 40), 65535, note="short path behind 2 literals")
    b = f.add([(b"ab", 2 + SHORT_SERVED + 1, 8)], _tail(rng, 40), 65535, note="short path behind 2 literals, one further")
    f.pair(b, a, SHORT_MIRROR)
    # the general path (15 literals: a length byte): match_end = 23, the mirror serves from 23 - 4 096 on
    lit = _rb(rng, 15)
    a = f.add([(lit, 15 + RING - 23, 8)], _tail(rng), 65535, note="general path, match_end - 4 096")
    b = f.add([(lit, 15 + RING - 23 + 1, 8)], _tail(rng), 65535, note="general path, one further")
    f.pair(a, b, GEN_MEMORY)
    f.moves = [SHORT_MIRROR, GEN_MIRROR, GEN_MEMORY, BURST_MIRROR]
    return f.damage()


# ---- paths -------------------------------------------------------------------------------------------------------------------------------
def _dict_run(rng, n, back):
    """n short sequences (2 literals, a match of 6) whose sources all lie `back` + 7 j bytes before the block"""
    seqs, pos = [], 0
    for j in range(n):
        seqs.append((_rb(rng, 2), pos + 2 + back + 7 * j, 6))
        pos += 8
    return seqs


def paths():
    """a run of short sequences that all copy from the dictionary (bursts), the short path alone, the general path, the long path: out of
    the mirror where it holds the source, out of memory where it does not"""
    f, rng = Family(), np.random.default_rng(4)
    near = f.add(_dict_run(rng, 24, 100), _tail(rng, 120), 4097, note="burst, sources in the mirror")
    far = f.add(_dict_run(rng, 24, 5000), _tail(rng, 120), 65535, note="burst, sources behind the mirror")
    f.pair(far, near, BURST_MIRROR)
    f.pair(near, far, GEN_MEMORY)
    f.add(_dict_run(rng, 3, 50), _tail(rng), 4096, note="short path alone")
    f.add(_dict_run(rng, 3, 50), _tail(rng), 17, valid=False, note="short path alone, before a dictionary of 17")
    a = f.add([(_rb(rng, 15), 15 + 300, 20)], _tail(rng), 65535, note="general path, mirror")
    b = f.add([(_rb(rng, 15), 15 + 30000, 20)], _tail(rng), 65535, note="general path, memory")
    f.pair(a, b, GEN_MEMORY)
    f.add([(_rb(rng, 5), 5 + 700, 500)], _tail(rng), 4095, note="long path")
    f.add([(_rb(rng, 70), 70 + 60000, 70)], _tail(rng), 70000, note="long literals, long path, far")
    f.moves = [BURST_MIRROR, SHORT_MIRROR, GEN_MIRROR, GEN_MEMORY, LONG_BYTES]
    return f.damage()


# ---- after a long copy ---------------------------------------------------------------------------------------------------------------------
def after_long_copy():
    """a dictionary source after ring_from has moved, and one after the block's own output has passed 4 096 bytes: the mirror no longer
    holds the bytes before the block, both must come from memory"""
    f, rng = Family(), np.random.default_rng(5)
    lit = _rb(rng, 4)
    a = f.add([(lit, 4, 8), (b"", 12 + 200, 8)], _tail(rng, 40), 4097, note="short first, then the dictionary")
    b = f.add([(lit, 4, 200), (b"", 204 + 200, 8)], _tail(rng, 40), 4097, note="a long copy first, then the dictionary")
    f.pair(a, b, GEN_MEMORY)
    f.pair(b, a, SHORT_MIRROR)
    b2 = f.add([(lit, 4, 200)] + _shift(_dict_run(rng, 12, 100), 204), _tail(rng, 120), 4097, note="a long copy, then a run out of the dictionary")
    f.pair(a, b2, GEN_MEMORY)
    fill = short_run(rng, 4200, 0)
    c = f.add(fill + [(b"", 4200 + 50, 8)], _tail(rng, 40), 4097, note="the dictionary behind 4 200 bytes of output")
    d = f.add(fill[:8] + [(b"", 64 + 50, 8)], _tail(rng, 40), 4097, note="the dictionary behind 64 bytes of output")
    f.pair(d, c, GEN_MEMORY)
    f.moves = [GEN_MEMORY]
    return f.damage()


def _shift(seqs, by):
    return [(lit, off + by, ml) for lit, off, ml in seqs]


# ---- identity --------------------------------------------------------------------------------------------------------------------------------
def identity():
    """dict_len = 0: the plain call, result for result and byte for byte"""
    f, rng = Family(), np.random.default_rng(6)
    f.add([(_rb(rng, 20), 7, 30), (b"", 1, 100), (b"q", 40, 5)], _tail(rng), 0, note="plain")
    f.add([(b"", 1, 8)], _tail(rng), 0, valid=False, note="a source before the block")
    f.add([(_rb(rng, 9), 10, 8)], _tail(rng), 0, valid=False, note="a source one byte before the block")
    f.add(short_run(rng, 400, 0) + [(_rb(rng, 3), 300, 700)], _tail(rng, 100), 0, note="bursts and a long copy")
    return f.damage()


BUILDERS = {"reach": reach, "straddle": straddle, "mirror": mirror, "paths": paths, "after_long_copy": after_long_copy, "identity": identity}
NAMES = tuple(BUILDERS)
_families, _expected = {}, {}


def family(name):
    if name not in _families:
        f = BUILDERS[name]()
        assert all(c.cap <= MAX_OUT for c in f.cases), name
        assert sum(c.raw is None and "damaged" in c.note for c in f.cases) == 2, name
        _families[name] = f
    return _families[name]


# ---- a live liblz4, where there is one ----------------------------------------------------------------------------------------------------
def liblz4():
    path = ctypes.util.find_library("lz4")
    if not path:
        return None
    try:
        L = C.CDLL(path)
        L.LZ4_decompress_safe_usingDict.restype = C.c_int
        L.LZ4_decompress_safe_usingDict.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        return L
    except (OSError, AttributeError):
        return None


def using_dict(L, block, cap, dic):
    """LZ4_decompress_safe_usingDict -> (result, bytes)"""
    out = C.create_string_buffer(max(cap, 1))
    dic = bytes(dic)
    r = L.LZ4_decompress_safe_usingDict(bytes(block), out, len(block), cap, dic, len(dic))
    return r, out.raw[:max(r, 0)]


# ---- truth ---------------------------------------------------------------------------------------------------------------------------------
def expected(oracle, name, known):
    """(family, expected result per case, expected bytes per case or None): the oracle on the spliced blocks, shifted back; computed
    once per family and decoder kind, the twin and liblz4 asserted on the way"""
    key = (name, known)
    if key not in _expected:
        f = family(name)
        lz4 = liblz4()
        res, outs = [], []
        for i, c in enumerate(f.cases):
            p = prefix_of(c.dict_len)
            sp = np.frombuffer(c.spliced(c.block), np.uint8)
            shift = sp.size - len(c.block)
            if known:
                r, o = oracle.uncompress_raw(sp, c.cap + len(p))
                want = r - shift if r >= 0 else r + shift
            else:
                r, o = oracle.uncompress_unknown_raw(sp, sp.size, c.cap + EXTRA + len(p))
                want = r - len(p) if r >= 0 else r + shift
                # the twin with a history, on every case
                tr, tb = lz4f_ref.decode_block(c.block, c.cap + EXTRA, history=p)
                assert tr == want, (name, i, c.note, "twin", tr, want)
                if want >= 0:
                    assert tb == bytes(o[len(p):len(p) + want]), (name, i, c.note, "twin's bytes")
            if r >= 0:
                assert bytes(o[:len(p)]) == p, (name, i, c.note)
            if c.raw is not None:                                     # a valid case decodes to what emit() said
                assert want == (len(c.block) if known else c.cap) and np.array_equal(o[len(p):len(p) + c.cap], c.raw), (name, known, i, c.note, want)
                if lz4 is not None and not known:
                    lr, lb = using_dict(lz4, c.block, c.cap + EXTRA, dictionary(c.dict_len))
                    assert lr == c.cap and lb == bytes(c.raw), (name, i, c.note, "liblz4", lr)
            elif "damaged" not in c.note:
                assert want < 0, (name, known, i, c.note, "a case built to be refused is refused")
            res.append(want)
            outs.append(o[len(p):] if want >= 0 else None)
        _expected[key] = (f, res, outs)
    return _expected[key]


def groups(f, only=None):
    """dict_len -> the indices of the cases that share that dictionary (one batch has one dictionary)"""
    g = {}
    for i, c in enumerate(f.cases):
        if only is None or i in only:
            g.setdefault(c.dict_len, []).append(i)
    return g


def check(oracle, name, known, decode, only=None, align=0, one_by_one=False):
    """decode(streams, capacities, known, stream lengths, dictionary bytes, align) -> (results, rows with 64 guard bytes of HOLE behind the
    capacity), one call per dictionary (one_by_one: per case)"""
    f, want, outs = expected(oracle, name, known)
    for dict_len, idx in sorted(groups(f, only).items()):
        batches = [[j] for j in idx] if one_by_one else [idx]
        for js in batches:
            # (the known-size codec takes no input length: a damaged stream runs on into the zeros the oracle's wrapper puts behind it, so here too)
            comps = [np.frombuffer(f.cases[j].block + (bytes(f.cases[j].cap + 1024) if known and f.cases[j].raw is None else b""), np.uint8) for j in js]
            caps = [f.cases[j].cap + (0 if known else EXTRA) for j in js]
            res, dst = decode(comps, caps, known, [len(c) for c in comps], dictionary(dict_len), align)
            for i, j in enumerate(js):
                c = f.cases[j]
                assert res[i] == want[j], (name, known, j, c.note, int(res[i]), want[j])
                if want[j] >= 0:
                    n = c.cap if known else want[j]
                    bad = np.flatnonzero(dst[i][:n] != outs[j][:n])
                    assert bad.size == 0, (name, known, j, c.note, "first wrong byte", int(bad[0]), "of", n)
                assert (dst[i][caps[i]:caps[i] + 64] == HOLE).all(), (name, known, j, c.note, "wrote past the block")


def plain_blocks():
    """(stream, bytes, capacity) of ordinary blocks, for the identity of dict_len = 0 with the plain call"""
    return [length_block(L, L) for L in (127, 256, 385)] + [far_block(o, 0, 2, 900 + o) for o in (173, 300)]


# ---- the emulator library -------------------------------------------------------------------------------------------------------------------
emu = emu_lib.dict_kernels    # libsimt_dict.so (tests/simt/emu_dict.cpp), built once


# ---- the fixture: records compressed by liblz4 against a dictionary ---------------------------------------------------------------------------
# tests/golden/dict_blocks.json (written by tests/golden/make_dict_golden.py with liblz4's LZ4_loadDict + LZ4_compress_fast_continue) holds the
# records' plain text and their blocks; the dictionary is made here from a seed, not stored.
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dict_blocks.json")
FIXTURE_SEED, FIXTURE_DICT_LEN = 20240301, 65536


def _vocabulary(rng, n=700):
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz_", np.uint8)
    return [bytes(rng.choice(letters, int(rng.integers(3, 12)))) for _ in range(n)]


def _field(rng, words):
    kind = int(rng.integers(0, 4))
    key = words[int(rng.integers(0, len(words)))]
    if kind == 0:
        return b'"%s": %d' % (key, int(rng.integers(0, 100000)))
    if kind == 1:
        return b'"%s": "%s %s"' % (key, words[int(rng.integers(0, len(words)))], words[int(rng.integers(0, len(words)))])
    if kind == 2:
        return b'"%s": {"id": %d, "%s": true}' % (key, int(rng.integers(0, 1000)), words[int(rng.integers(0, 64))])
    return b'"%s": [%d, %d, %d]' % (key, int(rng.integers(0, 99)), int(rng.integers(0, 99)), int(rng.integers(0, 99)))


def fixture_dictionary(seed=FIXTURE_SEED, length=FIXTURE_DICT_LEN):
    """the fixture's dictionary: JSON-like fields over a vocabulary, both from the seed"""
    rng = np.random.default_rng(seed)
    words = _vocabulary(rng)
    out = bytearray()
    while len(out) < length:
        out += b"{" + b", ".join(_field(rng, words) for _ in range(int(rng.integers(2, 9)))) + b"}\n"
    return np.frombuffer(bytes(out[:length]), np.uint8).copy()


def fixture_record(seed, k, size):
    """record k: `size` bytes of the same kind of text over the same vocabulary, with fields of its own"""
    words = _vocabulary(np.random.default_rng(seed))
    rng = np.random.default_rng(seed + 1 + k)
    out = bytearray()
    while len(out) < size:
        out += b"{" + b", ".join(_field(rng, words) for _ in range(int(rng.integers(2, 9)))) + b"}\n"
    return bytes(out[:size])


def load_fixture():
    """(dictionary, [(plain bytes, block bytes)], the json's header)"""
    import base64
    import json
    with open(FIXTURE) as fh:
        j = json.load(fh)
    dic = fixture_dictionary(j["dictionary"]["seed"], j["dictionary"]["length"])
    import hashlib
    assert hashlib.sha256(dic.tobytes()).hexdigest() == j["dictionary"]["sha256"], "the dictionary made from the seed is not the one the fixture was written with"
    return dic, [(base64.b64decode(r["plain"]), base64.b64decode(r["block"])) for r in j["records"]], j
