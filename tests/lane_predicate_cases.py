"""TEST INFRASTRUCTURE for tests/test_simt_lane_predicates.py and tests/test_gpu_lane_predicates.py, which are one design: blocks BUILT so that
each predicate the lane decoder makes ONCE per iteration and then combines as lane masks (lz4hip_decode_lane4.hpp: the kinds, `rem > 0`,
`rem_after == 0`, room, `hdr == 0`, the class word of the parsed-ahead sequence, the merged test against the end of the source, the half of
the sector in a refill) is met on both sides of its edge.  The families are lane_decode_cases.Family objects -- items, the counters that must
move, pairs of items on the two sides of one threshold -- of at most 64 blocks of at most 1 KiB: one wavefront each.  The truth is the CPU
codec's, through lane_decode_cases.check."""
import numpy as np

import lane_decode_cases as base
import lane_window_cases as window
from lane_decode_cases import (DOUBLING, FAR_NOT_FLUSHED, FAR_WAITS, FAST, NEAR_MAX, NO_ROOM_COPY, NO_ROOM_PROMOTE, RING, ROOM_BELOW, ROOM_LAST, ROOM_NONE, TAIL,
                               TO_FAR, TO_LIT, TO_NEAR, TO_ZERO, TRAP_HEADER, TRAP_TOKEN, WHY_INPUT_END, WHY_LAST_KNOWN, WHY_LIT_255, WHY_LIT_PAST_INPUT,
                               WHY_MATCH_255, WHY_MATCH_END, WHY_OFFSET, Family, _closing, _lead, _rb, _with_offset, emit)
from wave_decode_cases import _out

MAX_OUT = 1024
OFFSETS = (0, 1, 2, 3, 15, 16, 172, 173)


def kinds():
    """the class word's kind: a match of offset 0 (by result only), 1, 2, 3, 15 (all doubling), 16, 172 (the greatest near offset), 173 (far),
    on the fast path behind 2 inline literals and in header position behind a streamed run of 13; match lengths 6 and 40"""
    f = Family()
    f.moves = [TO_ZERO, TO_NEAR, TO_FAR, TO_LIT, DOUBLING, FAST]
    rng = np.random.default_rng(5100)
    at = {}
    for where, ll in (("fast path", 2), ("header position", 13)):
        for ml in (6, 40):
            for off in OFFSETS:
                seqs = [(_rb(rng, 190), 5, 4), (_rb(rng, ll), max(off, 1), ml)] + _closing(rng)
                name = "K offset %d, length %d, %s" % (off, ml, where)
                if off:
                    at[where, ml, off] = f.add(name, seqs, _rb(rng, TAIL))
                else:
                    c, raw = emit(seqs, _rb(rng, TAIL))
                    at[where, ml, off] = f.add_stream(name, _with_offset(c, seqs, 1, 0), raw.size, hole=True)
    for where in ("fast path", "header position"):
        f.pair(at[where, 40, 1], at[where, 40, 0], TO_ZERO)
        f.pair(at[where, 40, 0], at[where, 40, 1], TO_NEAR)
        f.pair(at[where, 40, 16], at[where, 40, 15], DOUBLING)
        f.pair(at[where, 40, 172], at[where, 40, 173], TO_FAR)
        f.pair(at[where, 40, 173], at[where, 40, 172], TO_NEAR)
    f.pair(at["fast path", 6, 3], at["header position", 6, 3], TO_LIT)
    return f


def tokens():
    """the token's high nibble 0 .. 10 (where the offset field lies in the view), 11 (the last inline run), 12 (the first streamed one), 15 with a length byte of 0, 254, 255 + 0; the match
    nibble 15 with a length byte of 254 and 255 + 0, on the fast path and in header position; a header behind streamed literals of 12 .. 33
    bytes (the cursor view of the header at every byte phase); blocks whose last sequence has no match, with 0 .. 20 last literals"""
    f = Family()
    f.moves = [FAST, TRAP_TOKEN, TRAP_HEADER, WHY_LIT_255, WHY_MATCH_255, TO_LIT, TO_NEAR]
    rng = np.random.default_rng(5200)
    at = {}
    for t4 in range(11):                                      # the offset field at byte 1 + t4 of the view: bit 1 of its dword index is a range test on the token
        f.add("T offset field at byte %d of the view" % (1 + t4), _lead(rng) + [(_rb(rng, t4), 5 + t4, 6)] + _closing(rng), _rb(rng, TAIL))
    for ll in (11, 12, 15, 15 + 254, 15 + 255):
        at["ll", ll] = f.add("T literal run of %d" % ll, _lead(rng) + [(_rb(rng, ll), 9, 5)] + _closing(rng), _rb(rng, TAIL))
    f.pair(at["ll", 11], at["ll", 12], TO_LIT)
    f.pair(at["ll", 15 + 254], at["ll", 15 + 255], WHY_LIT_255)
    for where, ll in (("fast path", 3), ("header position", 13)):
        for ml in (18, 19, 19 + 254, 19 + 255):
            at[where, ml] = f.add("T match of %d, %s" % (ml, where), _lead(rng) + [(_rb(rng, ll), 10, ml)] + _closing(rng), _rb(rng, TAIL))
        f.pair(at[where, 19 + 254], at[where, 19 + 255], WHY_MATCH_255)
    f.pair(at["fast path", 19 + 254], at["fast path", 19 + 255], TRAP_TOKEN)
    f.pair(at["header position", 19 + 254], at["header position", 19 + 255], TRAP_HEADER)
    for ll in range(12, 34):
        f.add("T header behind %d streamed literals" % ll, _lead(rng) + [(_rb(rng, ll), 7 + ll % 5, 4 + ll % 3)] + _closing(rng), _rb(rng, TAIL))
    for t in (0, 1, 4, 5, 11, 12, 14, 15, 16, 20):            # the final run: no match behind it (what the CPU codec makes of the short ones decides)
        c, raw = emit(_lead(rng) + [(_rb(rng, 3), 6, 9)], _rb(rng, t), min_tail=0)
        f.add_stream("T last sequence without a match, %d last literals" % t, c, raw.size)
    return f


def ends():
    """offset == lit_end and lit_end + 1; the match's end at oend - 5 (= out_limit) and oend - 4; a literal run's end at oend - 8 and oend - 7
    (known size: one stream, two output sizes); a token 16 and 15 bytes before the end of the source; a literal run with a length byte that
    ends at the end of the source, and one byte past it (the test merged with the view's)"""
    f = Family()
    f.moves = [WHY_OFFSET, WHY_MATCH_END, WHY_INPUT_END, TRAP_TOKEN, TRAP_HEADER]
    f.moves_known, f.moves_unknown = [WHY_LAST_KNOWN], [WHY_LIT_PAST_INPUT]
    rng = np.random.default_rng(5300)
    at = {}
    for ll in (0, 3, 11, 13):                                 # offset against the start of the block: on the fast path and in header position
        lead = [(_rb(rng, 9), 4, 5)]
        lit_end = _out(lead) + ll
        seqs = lead + [(_rb(rng, ll), lit_end, 6)] + _closing(rng)
        ok = f.add("E offset == lit_end, %d literals" % ll, seqs, _rb(rng, TAIL))
        c, raw, cap = f.items[ok]
        bad = f.add_stream("E offset == lit_end + 1, %d literals" % ll, _with_offset(c, seqs, 1, lit_end + 1), cap)
        f.pair(ok, bad, WHY_OFFSET)
    for where, ll in (("fast path", 3), ("header position", 13)):
        for garbage in (0, 24):                               # (bytes behind the block: the 16-byte view's own test, not the byte-wise parser's)
            seqs = _lead(rng) + [(_rb(rng, ll), 5, 8)]
            a = f.add("E match ends at oend - 5, %s%s" % (where, ", bytes behind" if garbage else ""), seqs, _rb(rng, 5), min_tail=5,
                      valid=True if garbage else None, garbage=garbage, ucap=_out(seqs) + 5)
            c, raw = emit(seqs, _rb(rng, 5), min_tail=5)
            b = f.add_stream("E match ends at oend - 4, %s%s" % (where, ", bytes behind" if garbage else ""),
                             np.concatenate([c, np.full(garbage, 0x11, np.uint8)]), raw.size - 1, ucap=raw.size - 1)
            f.pair(a, b, WHY_MATCH_END, None if not garbage else True)
    seqs = _lead(rng) + [(_rb(rng, 6), 4, 4)]
    k9 = f.add("E known size: literal run ends at oend - 9", seqs, _rb(rng, 5), min_tail=5)
    c, raw, cap = f.items[k9]
    k8 = f.add_stream("E known size: literal run ends at oend - 8", c, cap - 1)
    k7 = f.add_stream("E known size: literal run ends at oend - 7", c, cap - 2)
    f.pair(k8, k7, WHY_LAST_KNOWN, True)
    for t in (10, 9, 8):                                      # ip + 16 one below, at and one past iend
        at["view", t] = f.add("E token %d bytes before the end of the source" % (7 + t), _lead(rng) + [(_rb(rng, 3), 2, 4)], _rb(rng, t), min_tail=5)
    f.pair(at["view", 9], at["view", 8], WHY_INPUT_END)
    for b1 in (0, 1, 40):                                     # a run of 15 + b1 literals in front of a match: the source ends behind them, and one byte earlier
        seqs = _lead(rng) + [(_rb(rng, 15 + b1), 6, 5)]
        c, raw = emit(seqs, _rb(rng, TAIL))
        cut = base._offset_at(seqs, 1)                        # (where the offset field would begin)
        a = f.add_stream("E run of %d literals ends at the end of the source" % (15 + b1), c[:cut], raw.size)
        b = f.add_stream("E run of %d literals ends one byte past the source" % (15 + b1), c[:cut - 1], raw.size)
        f.pair(a, b, WHY_LIT_PAST_INPUT, False)
    return f


def far_sources():
    """six far matches of 16 bytes with 11 literals each at offsets 173 and 237, behind 184 .. 215 leading bytes: the end of a match's first 16
    source bytes takes every residue of the 128-byte flush unit, exactly at fl and one byte past it among them -- a lane whose source is not
    flushed asks again and waits"""
    f = Family()
    f.moves = [TO_FAR, FAR_WAITS, FAR_NOT_FLUSHED]
    rng = np.random.default_rng(5400)
    for off in (NEAR_MAX + 1, NEAR_MAX + 65):
        for lead in range(32):
            seqs = [(_rb(rng, lead * 2 + 180 + (off - NEAR_MAX - 1)), 1, 4)] + [(_rb(rng, 11), off + i % 2, 16) for i in range(6)] + _closing(rng)
            f.add("F six far matches at offset %d behind %d leading bytes" % (off, _out(seqs[:1])), seqs, _rb(rng, TAIL))
    return f


def promotion_room():
    """sequences of 11 inline literals and a match of 16, and of 16 streamed literals and a match of 11, behind 1 .. 32 leading bytes: a sequence is
    promoted with op - fl at every value around the last one with room (R - 46), and waits one byte above it"""
    f = Family()
    f.moves = [NO_ROOM_COPY, NO_ROOM_PROMOTE, ROOM_BELOW, ROOM_LAST, ROOM_NONE]
    rng = np.random.default_rng(5500)
    for shape, (ll, ml) in (("11 literals + 16", (11, 16)), ("16 literals + 11", (16, 11))):
        for lead in range(32):
            seqs = [(_rb(rng, lead * 2 + 1), 1, 4)] + [(_rb(rng, ll), 7, ml) for _ in range(14)]
            f.add("R %s, %d leading bytes" % (shape, lead * 2 + 5), seqs, _rb(rng, TAIL))
    return f


def refills():
    """sequences of 4 literals and a near match (7 bytes of stream each), 5 .. 12 of them: with row i of the batch at alignment i of its sector
    the cursor rests at every window offset, 31 (no refill) and 32 (a refill) among them, for either half of the sector and for a block's last piece"""
    f = Family()
    f.moves = [FAST, TO_NEAR]
    rng = np.random.default_rng(5600)
    for i in range(64):
        seqs = [(_rb(rng, 4), 3, 4 + i % 3) for _ in range(5 + (i // 8) % 8)]   # (the length moves slower than the alignment: every piece of a block meets both edges)
        f.add("W %d sequences of 7 bytes at alignment %d" % (len(seqs), i), seqs, _rb(rng, TAIL))
    return f


def refill_reach(f):
    """by the cursor model of lane_window_cases: the window offsets at which the cursor rests without a refill, and (d, high half, last piece)
    of every refill, for row i at alignment i"""
    views, crossings = set(), set()
    for i, (c, raw, _) in enumerate(f.items):
        skew = i % 64
        v, x = window.cursor_trace(c, skew)
        views.update(v)
        in_total = (skew + c.size + 31) & ~31
        for j, (d, half) in enumerate(x):
            wb = -48 + 32 * j                                 # the window's base before refill j; the piece that comes in lies at wb + 48
            crossings.add((d, half, wb + 48 + 32 >= in_total))
    return views, crossings


BUILDERS = {"kinds": kinds, "tokens": tokens, "ends": ends, "far_sources": far_sources, "promotion_room": promotion_room, "refills": refills}
NAMES = tuple(BUILDERS)
_families = {}


def family(name):
    if name not in _families:
        f = BUILDERS[name]()
        assert len(f.items) <= 64 and all(cap <= MAX_OUT for _, _, cap in f.items), name
        _families[name] = f
    return _families[name]


def check(oracle, name, known, decode, only=None, repeat=1):
    """lane_decode_cases.check over one of these families; the CPU codec's results are computed once per family and decoder kind (the names
    differ from that library's, so they share its cache)"""
    if (name, known) not in base._expected:
        base._expected[name, known] = base.expected(oracle, name, known, family(name))
    base.check(oracle, name, known, decode, only=only, repeat=repeat)
