"""TEST INFRASTRUCTURE for tests/test_simt_lane_decode_cases.py and tests/test_gpu_lane_decode_cases.py, which are one design: small LZ4
blocks BUILT sequence by sequence (lane_flush_cases.emit) so that the lane decoder (lz4hip_decode_lane4.hpp, one lane per block) meets both
sides of every threshold of its parser (T4 and the byte-wise trap T4x) and of its ring logic (T1c, T3, T5, B3 .. B5), and the comparison
with the CPU codec.  The cooperative flush and the input window have their own libraries (lane_flush_cases.py, lane_window_cases.py).

A family is a list of items (stream, expected bytes or None, output size), each with a name, plus what the emulator's counters must show
for it: `moves`, the slots that must be non-zero after the family, and `pairs` (a, b, slot, known), two items on the two sides of one
threshold: decoded alone, the slot's count of item a must be BELOW that of item b.  Slots 0 .. 39 are LZ4HIP_STAT's, slot L4 + k is slot k
of LZ4HIP_STAT_L4 (lz4hip::L4Stat).  Every item's result and bytes are asserted against both CPU decoders before a kernel sees it; a
damaged known-size stream is followed by zeros, as the oracle's wrapper does it.  Bytes "copied" by an offset-0 match are compared by
result only.  Every block produces at most 2 KiB, every batch has 64 .. 130 blocks (a short family is repeated up to 64)."""
import numpy as np

import lane_flush_cases as flush
from lane_flush_cases import TAIL, emit
from wave_decode_cases import _nlen, _out, _pos

EXTRA = flush.EXTRA
MAX_OUT = 2048
RING = 192                   # bytes of output ring per lane
NEAR_MAX = RING - 20         # the greatest offset served from the ring
UNIT = 128                   # flush unit
HOLE = 0xA5                  # what every output buffer is filled with; no built byte has this value

# LZ4HIP_STAT slots of the lane decoder that the families name
NO_ROOM_COPY, FAR_WAITS, NO_ROOM_PROMOTE, FAR_NOT_FLUSHED = 7, 8, 13, 16
# LZ4HIP_STAT_L4: lz4hip::L4Stat, in its order
L4 = 40
(FAST, TRAP_TOKEN, TRAP_HEADER, WHY_INPUT_END, WHY_LIT_255, WHY_LIT_PAST_INPUT, WHY_MATCH_255, WHY_OFFSET, WHY_MATCH_END, WHY_LAST_KNOWN,
 WHY_LAST_OUTPUT, WHY_LAST_INPUT, WHY_MATCH_BYTE_INPUT, TO_NEAR, TO_FAR, TO_ZERO, TO_LIT, DOUBLING, NEAR_WRAP, TAIL0, TAIL1, TAIL2, TAIL3,
 ROOM_BELOW, ROOM_LAST, ROOM_NONE) = range(L4, L4 + 26)
N_L4 = 26
N_SLOTS = L4 + 32


class Family:
    def __init__(self, extra=EXTRA):
        self.items, self.names, self.moves, self.pairs, self.extra = [], [], [], [], extra
        self.moves_known, self.moves_unknown = [], []   # slots that only the decodes of one kind move
        self.valid = {}              # item -> None: both decoders must accept it; True / False: the known- / unknown-size one; absent: the CPU codec says
        self.used = {}               # item -> what the known-size decoder returns for it, if not the stream's length (bytes behind the block)
        self.ucap = {}               # item -> capacity of its unknown-size decode, if not output size + extra
        self.holes = set()           # items with an offset-0 match: compared by result
        self.batches = None          # lists of item indices, if not the items in order

    def add(self, name, seqs, tail, min_tail=TAIL, valid=None, garbage=0, ucap=None):
        """a block that (at least) the decoders named by `valid` must accept ("cpu": whatever the CPU codec says); returns its index"""
        c, raw = emit(seqs, tail, min_tail)
        if garbage:
            c = np.concatenate([c, np.full(garbage, 0x11, np.uint8)])
            self.used[len(self.items)] = c.size - garbage
        return self.add_stream(name, c, raw.size, ucap, raw, valid)

    def add_stream(self, name, c, cap, ucap=None, raw=None, valid="cpu", hole=False):
        """a stream as it stands; raw: what it decodes to where it is accepted"""
        i = len(self.items)
        self.items.append((np.asarray(c, np.uint8).copy(), raw, cap))
        self.names.append(name)
        if valid != "cpu":
            self.valid[i] = valid
        if ucap is not None:
            self.ucap[i] = ucap
        if hole:
            self.holes.add(i)
        return i

    def pair(self, a, b, slot, known=None):
        for k in (True, False) if known is None else (known,):
            self.pairs.append((a, b, slot, k))

    def batch_lists(self):
        """the family as batches of 64 .. 130 blocks"""
        lists = self.batches
        if lists is None:
            n = len(self.items)
            parts = -(-n // 130)
            lists = [list(range(n * p // parts, n * (p + 1) // parts)) for p in range(parts)]
        out = []
        for idx in lists:
            while len(idx) < 64:
                idx = idx + idx[:64 - len(idx)]
            assert 64 <= len(idx) <= 130
            out.append(idx)
        return out


def _rb(rng, n):
    return bytes(rng.integers(1, HOLE, n, dtype=np.uint8))


def _offset_at(seqs, k):
    """where sequence k's offset field is in the stream"""
    ll = len(seqs[k][0])
    return _pos(seqs, k) + 1 + _nlen(ll) + ll


def _with_offset(c, seqs, k, value):
    d = c.copy()
    at = _offset_at(seqs, k)
    d[at], d[at + 1] = value & 255, value >> 8
    return d


def _lead(rng):
    """a first sequence, so that the one a case is about is a later one: 12 bytes"""
    return [(_rb(rng, 8), 3, 4)]


def _closing(rng):
    """a sequence behind the one a case is about: with the last literals, 21 bytes of stream, so that the cursor's 16-byte view ends inside
    the source"""
    return [(_rb(rng, 5), 7, 4)]


# ---- H: the header within the 16-byte view ---------------------------------------------------------------------------------------------
def header():
    f = Family()
    f.moves = [FAST, TRAP_TOKEN, TRAP_HEADER, WHY_LIT_255, WHY_MATCH_255, TO_LIT, TO_NEAR]
    rng = np.random.default_rng(4100)
    at = {}
    for t4 in range(12):                                      # the offset field at byte o = 1 + t4 of the view: every q and byte phase of the `ot` pick
        at["o", t4] = f.add("H offset field at byte %d of the view" % (1 + t4), _lead(rng) + [(_rb(rng, t4), 5 + t4, 6)] + _closing(rng), _rb(rng, TAIL))
    for ll in (11, 12, 14, 15, 16, 15 + 254, 15 + 255, 15 + 255 + 7):     # the edge of in_win; a length byte of 0, 1, 254, 255 + 0, 255 + 7
        at["ll", ll] = f.add("H literal run of %d" % ll, _lead(rng) + [(_rb(rng, ll), 9, 5)] + _closing(rng), _rb(rng, TAIL))
    f.pair(at["ll", 11], at["ll", 12], TO_LIT)
    f.pair(at["ll", 15 + 254], at["ll", 15 + 255], WHY_LIT_255)
    # match nibble 14; 15 with an extension byte of 0, 254, 255 + 0, 255 + 3, 255 + 255 + 0: on the fast path and in header position
    for where, ll in (("fast path", 3), ("fast path, offset at byte 12", 11), ("header position", 13), ("header position behind 270", 270)):
        for ml in (18, 19, 19 + 254, 19 + 255, 19 + 255 + 3, 19 + 510):
            at[where, ml] = f.add("H match of %d, %s" % (ml, where), _lead(rng) + [(_rb(rng, ll), 10, ml)] + _closing(rng), _rb(rng, TAIL))
    f.pair(at["fast path", 19 + 254], at["fast path", 19 + 255], WHY_MATCH_255)
    f.pair(at["fast path", 19 + 254], at["fast path", 19 + 255], TRAP_TOKEN)
    f.pair(at["header position", 19 + 254], at["header position", 19 + 255], WHY_MATCH_255)
    f.pair(at["header position", 19 + 254], at["header position", 19 + 255], TRAP_HEADER)
    return f


# ---- O: offsets against the start of the block ------------------------------------------------------------------------------------------
O_RUNS = tuple(range(12)) + (12, 15, 16, 270)


def offsets():
    """offset == lit_end reaches byte 0 of the block, lit_end + 1 and lit_end + 2 reach in front of it: for the first and for a later sequence,
    with 0 .. 11 inline literals (the fast path's test) and behind streamed runs (the byte-wise header parse's)"""
    f = Family()
    f.moves = [WHY_OFFSET, TRAP_HEADER, TO_NEAR, TO_ZERO]
    rng = np.random.default_rng(4200)
    for later in (False, True):
        for ll in O_RUNS:
            lead = [(_rb(rng, 9), 4, 5)] if later else []
            lit_end = _out(lead) + ll
            where = "%s sequence, %d literals" % ("a later" if later else "the first", ll)
            if lit_end == 0:
                # a block that begins with a match: offset 0 "copies" what the output held (by result only), 1 and 2 are refused
                for off in (0, 1, 2):
                    c = bytes([0x02, off, 0, 0xC0]) + _rb(rng, 12)
                    i = f.add_stream("O offset %d, %s" % (off, where), np.frombuffer(c, np.uint8), 18, hole=off == 0)
                    if off == 0:
                        ok = i
                    elif off == 1:
                        f.pair(ok, i, WHY_OFFSET)
                continue
            seqs = lead + [(_rb(rng, ll), lit_end, 6)] + _closing(rng)
            k = len(lead)
            ok = f.add("O offset == lit_end, " + where, seqs, _rb(rng, TAIL))
            c, raw, cap = f.items[ok]
            for d in (1, 2):
                i = f.add_stream("O offset == lit_end + %d, %s" % (d, where), _with_offset(c, seqs, k, lit_end + d), cap)
                if d == 1:
                    f.pair(ok, i, WHY_OFFSET)
                    if ll >= 12:
                        f.pair(ok, i, TRAP_HEADER)
    return f


# ---- E: the end of the output and of the input ------------------------------------------------------------------------------------------
def ends():
    f = Family()
    f.moves = [WHY_INPUT_END, WHY_MATCH_END, TRAP_TOKEN, TRAP_HEADER, TAIL0, TAIL1, TAIL2, TAIL3]
    f.moves_known, f.moves_unknown = [WHY_LAST_KNOWN], [WHY_LAST_OUTPUT, WHY_LAST_INPUT, WHY_MATCH_BYTE_INPUT]
    rng = np.random.default_rng(4300)
    at = {}
    for t in range(5, 13):                                    # last literals of 5 .. 12 bytes
        at["tail", t] = f.add("E last literals of %d" % t, _lead(rng) + [(_rb(rng, 4), 6, 8)], _rb(rng, t), min_tail=5)
    # the last match ends at oend - 5 and at oend - 4: parsed with the end of the source in the view (the byte-wise parser) and, for the
    # known-size decoder, with bytes behind the block (the 16-byte view's own test)
    for where, ll in (("fast path", 3), ("header position", 13)):
        for garbage in (0, 24):
            for t in (5, 4):
                seqs = _lead(rng) + [(_rb(rng, ll), 5, 8)]         # (a match of 8: the literals in front end at oend - 13 / - 12, no last run for either decoder)
                name = "E last match ends at oend - %d, %s%s" % (t, where, ", bytes behind the block" if garbage else "")
                if t == 5:
                    at["mend", where, garbage, t] = f.add(name, seqs, _rb(rng, t), min_tail=5, valid=True if garbage else None, garbage=garbage, ucap=_out(seqs) + t)
                else:                                         # (five last literals again and one byte less of output: four would be the unknown-size decoder's last run)
                    c, raw = emit(seqs, _rb(rng, 5), min_tail=5)
                    at["mend", where, garbage, t] = f.add_stream(name, np.concatenate([c, np.full(garbage, 0x11, np.uint8)]), raw.size - 1, ucap=raw.size - 1)
            f.pair(at["mend", where, garbage, 5], at["mend", where, garbage, 4], WHY_MATCH_END, None if not garbage else True)
    # known size: a literal run in front of a match that ends at oend - 9 (the match fits), oend - 8 (no match fits behind it), oend - 7 (taken
    # for the last run, which it is not): one stream, three output sizes
    seqs = _lead(rng) + [(_rb(rng, 6), 4, 4)]
    at["krun", 9] = f.add("E known size: literal run ends at oend - 9", seqs, _rb(rng, 5), min_tail=5)
    c, raw, cap = f.items[at["krun", 9]]
    for d in (8, 7):
        at["krun", d] = f.add_stream("E known size: literal run ends at oend - %d" % d, c, cap - (9 - d))
    f.pair(at["krun", 8], at["krun", 7], WHY_LAST_KNOWN, True)
    # unknown size: a literal run that ends at oend - 13, - 12 (a sequence like any other), - 11 (the last run, which it is not), for last
    # literals of 7 (at - 11 the capacity is exact) and of 8 (at - 12 it is, at - 11 it is one less)
    for t in (7, 8):
        seqs = _lead(rng) + [(_rb(rng, 11), 9, 4)]
        E = _out(seqs) - 4
        c, raw = emit(seqs, _rb(rng, t), min_tail=5)
        for d in (13, 12, 11):
            at["urun", t, d] = f.add_stream("E unknown size: literal run ends at oend - %d, last literals of %d" % (d, t), c, raw.size, ucap=E + d, raw=raw)
        # (a block's last token meets the rule too, so the slot counts 1 on both sides: what differs is whether a match was promoted behind the run)
        f.pair(at["urun", t, 11], at["urun", t, 12], TO_NEAR, False)
    # unknown size: the literals end at iend - 9, - 8 (a sequence like any other), - 7 (the last run, which it is not)
    for t in (6, 5, 4):
        seqs = _lead(rng) + [(_rb(rng, 9), 4, 4)]
        c, raw = emit(seqs, _rb(rng, t), min_tail=4)
        at["uin", t] = f.add_stream("E unknown size: literals end at iend - %d" % (3 + t), c, raw.size, raw=raw)
    f.pair(at["uin", 4], at["uin", 5], TO_NEAR, False)
    # unknown size: a match nibble of 15 whose extension byte would lie at iend - 7 (read), iend - 6 and iend - 5 (not read: the byte is the
    # next token); enough capacity that the output side never decides
    seqs = _lead(rng) + [(_rb(rng, 8), 6, 19)]
    c, raw = emit(seqs, _rb(rng, 5), min_tail=5)
    ext = _offset_at(seqs, 1) + 2
    assert c[ext] == 0 and ext == c.size - 7
    at["uext", 7] = f.add_stream("E unknown size: extension byte at iend - 7", c, raw.size, ucap=raw.size + 128, raw=raw, valid=None)
    at["uext", 6] = f.add_stream("E unknown size: no extension byte at iend - 6", np.delete(c, ext), raw.size, ucap=raw.size + 128, raw=raw, valid=False)
    c4, raw4 = emit(seqs, _rb(rng, 4), min_tail=4)
    # (at iend - 5 the literals in front end at iend - 7: the CPU codec takes them for the last run and refuses)
    at["uext", 5] = f.add_stream("E unknown size: no extension byte at iend - 5", np.delete(c4, ext), raw4.size, ucap=raw4.size + 128)
    f.pair(at["uext", 7], at["uext", 6], WHY_MATCH_BYTE_INPUT, False)
    # a token 17, 16 and 15 bytes before the end of the source: the last view that lies inside it, and the first that does not
    for t in (10, 9, 8):
        at["view", t] = f.add("E token %d bytes before the end of the source" % (7 + t), _lead(rng) + [(_rb(rng, 3), 2, 4)], _rb(rng, t), min_tail=5)
    f.pair(at["view", 9], at["view", 8], WHY_INPUT_END)
    # unknown size: the last literals end at oend (accepted) and at oend + 1 (refused, and the byte behind the capacity stays), behind a
    # match and as the block's only run
    seqs = _lead(rng) + [(_rb(rng, 2), 6, 8)]
    c, raw = emit(seqs, _rb(rng, 20))
    at["ulast", 0] = f.add_stream("E unknown size: last literals end at oend", c, raw.size, ucap=raw.size, raw=raw, valid=None)
    at["ulast", 1] = f.add_stream("E unknown size: last literals end at oend + 1", c, raw.size, ucap=raw.size - 1)
    c, raw = emit([], _rb(rng, 30))
    f.add_stream("E unknown size: a block of 30 literals ends at oend + 1", c, raw.size, ucap=raw.size - 1)
    f.add_stream("E unknown size: a block of 30 literals ends at oend + 2", c, raw.size, ucap=raw.size - 2)
    f.pair(at["ulast", 1], at["ulast", 0], TO_LIT, False)
    # no input at all, and blocks of 0 .. 5 literals: into their exact capacity and into a larger one
    f.add_stream("E empty input", np.zeros(0, np.uint8), 0, ucap=0)
    f.add_stream("E empty input, capacity 7", np.zeros(0, np.uint8), 7, ucap=7)
    for n in range(6):
        lit = _rb(rng, n)
        c = np.frombuffer(bytes([n << 4]) + lit, np.uint8)
        f.add_stream("E block of %d literals, exact capacity" % n, c, n, ucap=n, raw=np.frombuffer(lit, np.uint8))
        f.add_stream("E block of %d literals" % n, c, n, raw=np.frombuffer(lit, np.uint8))
    return f


# ---- C: every prefix ----------------------------------------------------------------------------------------------------------------------
def prefixes():
    """two blocks of at most 64 bytes of stream -- a streamed run, an extension byte and a near match between them -- cut at every length"""
    f = Family()
    f.moves, f.moves_unknown = [TRAP_TOKEN, TRAP_HEADER, WHY_INPUT_END], [WHY_LIT_PAST_INPUT]
    rng = np.random.default_rng(4400)
    for which, seqs in (("a", [(_rb(rng, 14), 6, 25)]), ("b", [(_rb(rng, 3), 2, 5), (_rb(rng, 16), 9, 4)])):
        c, raw = emit(seqs, _rb(rng, TAIL))
        assert c.size <= 64
        for n in range(c.size):
            f.add_stream("C block %s cut at %d of %d" % (which, n, c.size), c[:n], raw.size)
        f.add_stream("C block %s whole" % which, c, raw.size, raw=raw, valid=None)
    return f


# ---- N: near matches over the ring ------------------------------------------------------------------------------------------------------
N_OFFSETS = (17, 31, 32, 33, 61, 64, 100, 128, 160, 170, 171, 172, 173, 174)
N_LENGTHS = (4, 16, 17, 48)
N_PLACES = (("before the wrap", 96), ("across the wrap", 180), ("behind the wrap", 4))


def near():
    """a match of offset `off` that starts at output byte op, (op - off) % 192 chosen: its five source rows lie before, across and behind the
    ring's wrap (48 rows); `a` moves it through the byte phases of op - off, and with them (off % 4 is given) of op"""
    f = Family()
    f.moves = [TO_NEAR, TO_FAR, NEAR_WRAP]
    rng = np.random.default_rng(4500)
    at = {}
    for oi, off in enumerate(N_OFFSETS):
        for pi, (place, base) in enumerate(N_PLACES):
            for a in range(4):
                t = base + a
                op = off + t + (RING if t < 8 else 0)
                ml = N_LENGTHS[(a + pi) % 4]
                seqs = [(_rb(rng, op - 8), 3, 6), (_rb(rng, 2), off, ml)] + _closing(rng)
                assert _out(seqs[:1]) + 2 == op
                at[off, place, a] = f.add("N offset %d, source %s, op %% 4 = %d, length %d" % (off, place, op % 4, ml), seqs, _rb(rng, TAIL))
    # the append that reaches farthest in front of a near match: a whole 16-byte chunk and 11 inline literals, then the greatest near
    # offset (and the offsets on both sides of it) at every byte phase
    for off in (171, 172, 173):
        for ph in range(4):
            seqs = [(_rb(rng, 160 + ph), 3, 16), (_rb(rng, 11), off, 20)] + _closing(rng)
            at["far append", off, ph] = f.add("N offset %d behind a chunk of 16 and 11 literals, op %% 4 = %d" % (off, (160 + ph + 27) % 4), seqs, _rb(rng, TAIL))
    f.pair(at[173, "before the wrap", 0], at[172, "before the wrap", 0], TO_NEAR)
    f.pair(at[172, "before the wrap", 0], at[173, "before the wrap", 0], TO_FAR)
    f.pair(at[64, "before the wrap", 1], at[64, "across the wrap", 1], NEAR_WRAP)
    f.pair(at[172, "before the wrap", 2], at[172, "across the wrap", 2], NEAR_WRAP)
    return f


# ---- D: doubling --------------------------------------------------------------------------------------------------------------------------
def doubling():
    """a match of offset 1 .. 16 copies `off` bytes and doubles off until it is 16 or more: lengths at which that happens once, twice, ...,
    and one more byte; every byte phase of op; offset 16 and 17, which never double, beside them"""
    f = Family()
    f.moves = [DOUBLING, TO_NEAR]
    rng = np.random.default_rng(4600)
    at = {}
    for off in range(1, 18):
        lens, o = {4, 70}, off
        while o < 16:                                         # a step copies `o` bytes and doubles o: the lengths that end with a step, and one more byte
            lens |= {x for x in (2 * o - off, 2 * o - off + 1) if 4 <= x <= 70}
            o *= 2
        for j, ml in enumerate(sorted(lens)):
            ph = (j + off) % 4
            at[off, ml] = f.add("D offset %d, length %d, op %% 4 = %d" % (off, ml, ph), [(_rb(rng, 20 + ph), off, ml)] + _closing(rng), _rb(rng, TAIL))
        for ph in range(4):
            f.add("D offset %d, length 37, op %% 4 = %d" % (off, ph), [(_rb(rng, 32 + ph), off, 37)] + _closing(rng), _rb(rng, TAIL))
    f.pair(at[16, 70], at[15, 70], DOUBLING)
    f.pair(at[17, 70], at[15, 70], DOUBLING)
    f.pair(at[3, 9], at[3, 10], DOUBLING)                    # steps of 3 and 6 bytes; a third one
    f.pair(at[1, 7], at[1, 8], DOUBLING)                     # steps of 1, 2 and 4 bytes; a fourth one
    f.pair(at[5, 5], at[5, 6], DOUBLING)
    return f


# ---- F: far matches by how they begin ---------------------------------------------------------------------------------------------------
F_LENGTHS = (4, 15, 16, 17, 32, 33, 274)


def far():
    f = Family()
    f.moves = [TO_FAR, FAR_WAITS, FAR_NOT_FLUSHED]
    rng = np.random.default_rng(4700)
    at = {}
    n = 0
    for begin in ("0 literals", "1 literal", "11 literals", "a streamed run", "another far match"):
        for ml in F_LENGTHS:
            for off in (173, 200 + n % 7):
                # the match starts at op: its first 16 source bytes end one byte before, at and one byte behind a multiple of 128 in turn (the
                # unit that holds them is flushed late, or not yet), or far below (flushed long ago)
                op = UNIT * 2 + (n % 3 - 1) - 16 + off if n % 4 else off + 40
                ll = {"0 literals": 0, "1 literal": 1, "11 literals": 11, "a streamed run": 14, "another far match": 0}[begin]
                if begin == "another far match":
                    seqs = [(_rb(rng, op - 20), 3, 4), (b"", 180, 16)]
                else:
                    seqs = [(_rb(rng, op - ll - 6), 3, 6)]
                assert _out(seqs) + ll == op
                seqs += [(_rb(rng, ll), off, ml)] + _closing(rng)
                at[begin, ml, off == 173] = f.add("F offset %d, length %d, behind %s, at %d" % (off, ml, begin, op), seqs, _rb(rng, TAIL))
                n += 1
    # twelve far matches of 16 bytes with 11 literals each (27 bytes per sequence), at the smallest far offsets, behind 184 .. 247 leading bytes:
    # between them the lanes parse a far match with its source flushed, and with the flush still to come (the lane asks again, and waits)
    for lead in range(64):
        seqs = [(_rb(rng, lead + 180), 1, 4)] + [(_rb(rng, 11), 173 + i % 3, 16) for i in range(12)] + _closing(rng)
        at["late", lead] = f.add("F twelve far matches of 16 with 11 literals each behind %d leading bytes" % (lead + 184), seqs, _rb(rng, TAIL))
    for off in (172, 173):                                    # the greatest near offset and the smallest far one, in one place
        at["edge", off] = f.add("F offset %d, length 16, behind 1 literal, at 257" % off, [(_rb(rng, 250), 3, 6), (_rb(rng, 1), off, 16)] + _closing(rng), _rb(rng, TAIL))
    f.pair(at["edge", 172], at["edge", 173], TO_FAR)
    return f


# ---- M: ring room -------------------------------------------------------------------------------------------------------------------------
def room():
    """sequences of 11 inline literals and a match of 16 (27 bytes per iteration: a whole chunk, then the literals of the next sequence), and of
    16 streamed literals and a match of 11, behind 0 .. 63 leading bytes: between them the lanes meet every op - fl up to the ring's size at the
    top of an iteration that does not flush, the values around the last one with room (ROOM_BELOW, ROOM_LAST, ROOM_NONE) among them"""
    f = Family()
    f.moves = [NO_ROOM_COPY, NO_ROOM_PROMOTE, ROOM_BELOW, ROOM_LAST, ROOM_NONE]
    rng = np.random.default_rng(4800)
    for shape, (ll, ml) in (("11 literals + 16", (11, 16)), ("16 literals + 11", (16, 11))):
        for lead in range(64):
            seqs = [(_rb(rng, lead + 1), 1, 4)] + [(_rb(rng, ll), 7, ml) for _ in range(14)]
            f.add("M %s, %d leading bytes" % (shape, lead + 5), seqs, _rb(rng, TAIL))
    return f


# ---- S: restart in the persistent kernel ------------------------------------------------------------------------------------------------
def restart():
    """130 blocks for ONE wavefront of the persistent kernel, in this order: the first 64, one per lane, end in a refused header behind a streamed
    run, in a refusal directly behind a far match, at a first token, or in a final run -- a block of no bytes and of one byte among them; the lanes
    then take the other 66, valid blocks that begin with a short sequence near the block's start"""
    f = Family()
    f.moves = [TO_FAR, TRAP_HEADER, WHY_OFFSET, TO_LIT]
    rng = np.random.default_rng(4900)
    for i in range(64):
        kind = i % 6
        if kind == 0:                                         # refused in header position: the offset behind a streamed run reaches before the block
            seqs = [(_rb(rng, 40 + i), 3, 4), (_rb(rng, 16 + i % 5), 7, 9)] + _closing(rng)
            c, raw = emit(seqs, _rb(rng, TAIL))
            f.add_stream("S ends refused in header position (%d)" % i, _with_offset(c, seqs, 1, 60000), raw.size)
        elif kind == 1:                                       # refused directly behind a far match
            seqs = [(_rb(rng, 300 + i), 3, 4), (_rb(rng, 2), 200, 40), (_rb(rng, 3), 9, 9)] + _closing(rng)
            c, raw = emit(seqs, _rb(rng, TAIL))
            f.add_stream("S ends refused behind a far match (%d)" % i, _with_offset(c, seqs, 2, 60000), raw.size)
        elif kind == 2:                                       # refused inside a far match's wait: the stream ends in the middle of the next sequence
            seqs = [(_rb(rng, 260 + i), 3, 4), (_rb(rng, 1), 190, 300)]
            c, raw = emit(seqs, _rb(rng, TAIL))
            f.add_stream("S ends cut behind a far match's header (%d)" % i, c[:_offset_at(seqs, 1) + 2], raw.size)
        elif kind == 3:
            f.add_stream("S no bytes (%d)" % i, np.zeros(0, np.uint8), 0, ucap=0)
        elif kind == 4:
            lit = _rb(rng, 1)
            f.add_stream("S one byte (%d)" % i, np.frombuffer(b"\x10" + lit, np.uint8), 1, ucap=1, raw=np.frombuffer(lit, np.uint8))
        else:                                                 # a final run, its length and alignment the lane's own
            f.add("S ends in a final run (%d)" % i, [(_rb(rng, 50 + 3 * i), 5, 30)], _rb(rng, TAIL + i % 7))
    for i in range(66):
        if i % 11 == 5:                                       # (no bytes: the unknown-size decoder's result is 0 whatever the lane's last block returned)
            f.add_stream("S next block %d: no bytes" % i, np.zeros(0, np.uint8), 0, ucap=0)
            continue
        if i % 11 == 8:
            lit = _rb(rng, 1)
            f.add_stream("S next block %d: one byte" % i, np.frombuffer(b"\x10" + lit, np.uint8), 1, ucap=1, raw=np.frombuffer(lit, np.uint8))
            continue
        if i % 11 == 2:                                       # (one byte of output short: the last match ends at oend - 4, by THIS block's oend)
            c, raw = emit([(_rb(rng, 3), 2, 5), (_rb(rng, 3), 5, 8)], _rb(rng, 5), min_tail=5)
            f.add_stream("S next block %d: its last match ends at oend - 4" % i, c, raw.size - 1, ucap=raw.size - 1)
            continue
        seqs = [(_rb(rng, 3), 2, 5)]
        if i % 3 == 0:
            seqs += [(_rb(rng, 7), 4, 21), (_rb(rng, 230 + i), 11, 8), (b"", 181 + i, 33)]
        elif i % 3 == 1:
            seqs += [(_rb(rng, 13 + i % 4), 1, 40), (_rb(rng, 100), 50, 6)]
        else:
            seqs += [(b"", 8, 4), (_rb(rng, 1), 13, 18)] * 6
        f.add("S next block %d" % i, seqs + _closing(rng), _rb(rng, TAIL))
    f.batches = [list(range(130))]
    return f


BUILDERS = {"H": header, "O": offsets, "E": ends, "C": prefixes, "N": near, "D": doubling, "F": far, "M": room, "S": restart}
NAMES = tuple(BUILDERS)
_families, _expected = {}, {}


def family(name):
    if name not in _families:
        f = BUILDERS[name]()
        assert all(cap <= MAX_OUT for _, _, cap in f.items), name
        assert all(64 <= len(b) <= 130 for b in f.batch_lists()), name
        _families[name] = f
    return _families[name]


def plain(oracle, name):
    """the family's shape with plain encoder output in place of its inputs (what the reach assertions must NOT accept)"""
    f = family(name)
    g = Family(f.extra)
    g.moves, g.moves_known, g.moves_unknown, g.pairs, g.batches = f.moves, f.moves_known, f.moves_unknown, f.pairs, f.batches
    rng = np.random.default_rng(1)
    for (c, raw, cap), nm in zip(f.items, f.names):
        data = np.repeat(rng.integers(1, HOLE, cap // 8 + 1, dtype=np.uint8), 8)[:cap] if cap >= 64 else rng.integers(1, HOLE, cap, dtype=np.uint8)
        g.add_stream("plain " + nm, oracle.compress(data), cap, raw=data, valid=None)
    return g


def expected(oracle, name, known, fam=None):
    """(family, CPU codec's result per block, its bytes per block): computed once per family and decoder kind"""
    key = (name, known)
    if fam is not None or key not in _expected:
        f = family(name) if fam is None else fam
        res, outs = [], []
        for i, (c, raw, cap) in enumerate(f.items):
            if known:
                r, o = oracle.uncompress_raw(c, cap)
            else:
                r, o = oracle.uncompress_unknown_raw(c, len(c), f.ucap.get(i, cap + f.extra))
            if raw is not None and i in f.valid and f.valid[i] in (None, known):     # a block built here is a valid one, and decodes to what emit() said
                assert r == (f.used.get(i, len(c)) if known else raw.size) and np.array_equal(o[:raw.size], raw), (name, known, f.names[i], r)
            res.append(r)
            outs.append(o)
        if fam is not None:
            return f, res, outs
        _expected[key] = (f, res, outs)
    return _expected[key]


def check(oracle, name, known, decode, only=None, fam=None, repeat=1):
    """decode(streams, capacities, known) -> (results, rows with 64 guard bytes of 0xA5 behind the capacity), once per batch of the family;
    only: indices to decode as one batch of their own; repeat: each batch is decoded `repeat` times over in one call"""
    f, want, outs = expected(oracle, name, known, fam)
    for idx in (f.batch_lists() if only is None else [list(only)]):
        idx = idx * repeat
        # (the known-size codec takes no input length: a stream it does not accept runs on into the zeros the oracle's wrapper puts behind it, so here too)
        comps = [np.concatenate([f.items[j][0], np.zeros(f.items[j][2] + 1024, np.uint8)]) if known and f.valid.get(j, "cpu") in ("cpu", False) and j not in f.used
                 else f.items[j][0] for j in idx]
        caps = [f.items[j][2] if known else f.ucap.get(j, f.items[j][2] + f.extra) for j in idx]
        res, dst = decode(comps, caps, known)
        for i, j in enumerate(idx):
            assert res[i] == want[j], (name, known, f.names[j], int(res[i]), want[j])
            if want[j] >= 0 and j not in f.holes:
                n = f.items[j][2] if known else want[j]
                bad = np.flatnonzero(dst[i, :n] != outs[j][:n])
                assert bad.size == 0, (name, known, f.names[j], "first wrong byte", int(bad[0]), "of", n)
            assert (dst[i, caps[i]:caps[i] + 64] == 0xA5).all(), (name, known, f.names[j], "wrote past the block")
