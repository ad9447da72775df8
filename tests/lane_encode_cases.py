"""Blocks BUILT for single branches of the fast lane encoder (lz4hip_encode_lane.hpp: LaneTable's epoch, tag and empty-bucket rules, the
forward window, the one-store emit and its three conditions, lane_count_equal and lane_copy), shared by
tests/test_simt_lane_encode_cases.py and tests/test_gpu_lane_encode_cases.py, in the manner of tests/wave_encode_cases.py, whose Build,
probe, Family and expectations they use.  Every builder returns (name, block, expectation); the expectation is about the ORACLE's own
parse and is asserted against oracle.compress before any kernel is asked (checked()).  A family names the LaneEncStat slots
(LZ4HIP_STAT_LANE, emu_lane_enc_stats) that must move for it, and pairs of blocks on the two sides of a threshold.  All randomness comes
from np.random.default_rng(fixed seed).

The lane kernel is the serial search: every probe inserts its position, so a word stands "under a probe" when it stands at probe(s, i)
of the search that starts at s.  The common frame (k_case): a source F of distinct bytes and a word Y inside the first search's first
61 positions (stride 1: every one of them is inserted), Y again at a later probe -- the first match, which sets the anchor --, then ll
literals and F's first 4 + extra bytes: the sequence under test, at a chosen offset.

Family T  tag and bucket          a word A, then B in A's bucket (equal, A's tag, another tag, products one bit apart), then A again; at both sites
Family P  put                     the word two bytes in front of a match's end stands again under a probe
Family K  one-store emit (G)      ll = 0 .. 16 x extra (0, 14, 15) x three offsets, followed by literals, a zero-literal sequence, the end
Family KS capacity sweep          ll = 0 .. 13 and both ll = 0 sites as the last sequence before five last literals
Family N  count tiers (G)         matches of 4 .. 44 ended by a mismatch, by matchlimit, by one differing byte
Family L  copy tiers (G)          literal runs of 14 .. 40, last literals of 5 .. 40
Family V  window, catch-up        searches won in step 1, 2, 3; position 0; a hit directly behind a catch-up
Family R  refusals (G only)       the three tests that keep the length bytes of runs beyond 195 840 bytes inside the capacity
Family Q  one lane, many blocks   eight kinds that fill each other's buckets, and a pair of which the second holds the first's word where it was"""
import numpy as np

from encoder_cases import compress_bound, parse_sequences
from wave_encode_cases import (Build, Family, Retry, Y_LEN, Y_OFF, _b, _exactly, _has, _none, _put_word, _source, _tail, build,
                               c_back, c_back_to_start, le, opener, probe, product, s_winner_at, word_of, z_search, z_test)

# lz4hip::LaneEncStat, in the kernel's order
SLOTS = ["TableZeroed", "TableKept", "Stamp63", "GenericClear", "ZeroHitS", "ZeroHitT", "ZeroMissS", "ZeroMissT", "OldHitS", "OldHitT", "OldMissS",
         "OldMissT", "OldTagEqualS", "OldTagEqualT", "TagRejectS", "TagRejectT", "WordDiffersS", "WordDiffersT", "HitS", "HitT", "GenericRefusedS",
         "GenericRefusedT", "FwdRefill", "FwdServed0", "FwdServed1", "FwdServed2", "FwdServed3", "FwdServed4", "FwdClamped", "FwdBehind",
         "CatchStopAnchor", "CatchStopRef0", "CatchStopMismatch", "PackSh8To40", "PackSh48", "PackSh56", "PackSh64Up", "PlainLong", "PlainCap",
         "PlainTail", "ZeroPacked", "ZeroPlainCap", "RefuseLiterals", "RefuseLiteralLength", "RefuseOffset", "RefuseMatch", "RefuseMatchLength",
         "RefuseLastLiterals", "Count16Low", "Count16High", "Count16Equal", "Count16Limit", "Count8Diff", "Count8Equal", "Count8Limit",
         "Count1Equal", "Count1Diff", "Count1Limit", "Copy16", "Copy8", "Copy1"]
S = {name: i for i, name in enumerate(SLOTS)}
# Slots no block moves, asserted to stay at 0 over every block (profiles/lane_encode_cases/README.md).
#   FwdClamped            every refill position is a probe or a search's start, at most mflimit + 1 = n - 11: pos + 8 <= n always
#   FwdBehind             a search only moves forward, and the test of the next position sets the window itself
UNREACHED = ("FwdClamped", "FwdBehind")
TABLE_BLOCKS = 63                      # the kernel's: blocks of one lane per zeroing of its table (LaneTable<false>::clear)


# ---- the common frame ------------------------------------------------------------------------------------------------------------------
OFFSET_KINDS = ("high byte 0", "both bytes", "low byte 0")


def _offset_is(kind, off):
    lo, hi = off & 255, off >> 8
    return {"high byte 0": hi == 0 and lo != 0, "both bytes": lo != 0 and hi != 0 and lo != hi, "low byte 0": lo == 0 and hi != 0}[kind]


def _distinct(b, n, avoid=(), last_avoid=()):
    """n fresh bytes, all different and none of `avoid`; the last not in last_avoid"""
    seen = set(avoid)
    for k in range(n):
        b.fresh(1, avoid=tuple(seen | (set(last_avoid) if k == n - 1 else set())))
        seen.add(b.b[-1])


def k_case(ll, extra, kind="high byte 0", follow="literals", tail=20, n_f=30, differ=False):
    """F (n_f distinct bytes) at src_at, Y behind it, both inside the first search's stride-1 probes; Y again at a later probe `at` (the
    first match); ll distinct literals; F[:4 + extra] at t = at + 6 + ll, t - src_at an offset of the kind asked for.  ll = 0: the hit of
    the test of the next position; otherwise the search behind it, won at its probe ll - 1.  follow: "literals" (`tail` fresh bytes, the
    first not F's next), "zero" (F[20:26] directly behind: a zero-literal sequence), "end" (the shortest tail the format allows), "limit"
    (five more bytes of F and the end: the count runs into matchlimit).  differ: the byte behind the copy differs from F's, and F goes on
    behind it -- the candidate differs from the position in exactly that byte."""
    def body(b, s):
        for i in range(62, 3000):
            at = probe(s, i)
            t = at + Y_LEN + ll
            src = [x for x in range(s, s + 60 - n_f - 2) if _offset_is(kind, t - x) and at >= x + n_f + 2 + Y_LEN + 3]
            if src:
                src_at = src[int(b.rng.integers(0, len(src)))]
                break
        else:
            raise AssertionError("no probe gives this offset")
        _, F = _source(b, src_at, n_f)
        b.fresh(1)
        Y = b.word() + _b(b.rng.permutation(200)[:2] + 1)
        y_at = b.put(Y)
        assert y_at <= s + 61
        b.fresh(1)
        b.goto(at, avoid_last=(b.b[y_at - 1],))
        b.put(Y)
        if ll:
            _distinct(b, ll, avoid=(b.b[y_at + Y_LEN],), last_avoid=(b.b[src_at - 1],))
        elif F[0] == b.b[y_at + Y_LEN]:
            raise Retry("the source would extend the first match")
        assert b.pos == t
        b.put(F[:4 + extra])
        ms = [(at, at - y_at, Y_LEN), (t, t - src_at, 4 + extra)]
        if differ:
            b.fresh(1, avoid=(F[4 + extra],))
            b.put(F[4 + extra + 1:4 + extra + 9])
            b.fresh(20)
            return _has(*ms)
        if follow == "zero":
            assert 4 + extra < 20 and n_f >= 27
            z = b.put(F[20:26])
            ms.append((z, z - (src_at + 20), 6))
            b.fresh(1, avoid=(F[26],))
            b.fresh(19)
        elif follow == "limit":
            assert extra >= (4 if ll else 3)                               # (a search's match starts at n - 13 at the latest and ends at n - 5)
            b.put(F[4 + extra:4 + extra + 5])
        else:
            # the shortest tail: a search looks at ip only if ip + step <= mflimit (lz4.c:645), the test of the next position if ip <= mflimit
            n = max(5, (9 if ll else 8) - extra) if follow == "end" else tail
            b.fresh(1, avoid=(F[4 + extra],))
            b.fresh(n - 1)
        return _exactly(at, ms)
    return body


def k_ll0_search(extra, follow="literals"):
    """ll = 0 at the SEARCH site.  G stands where the first search's stride is 2, its first byte on a position the search skips: G[1:5] is
    in the table, G[0:4] is not.  Behind the first match, G[:4 + extra]: the test of the next position meets a bucket that reads zero,
    the search wins one byte on, and the catch-up takes that byte back -- it stops at the anchor."""
    def body(b, s):
        assert extra >= 1
        b.goto(s + 1)
        Y = b.word() + _b(b.rng.permutation(200)[:2] + 1)
        y_at = b.put(Y)
        g_at = s + 62
        assert probe(s, 61) == g_at - 1 and probe(s, 62) == g_at + 1
        _, G = _source(b, g_at, 24)
        at = probe(s, 80)
        b.goto(at, avoid_last=(b.b[y_at - 1],))
        b.put(Y)
        if G[0] == b.b[y_at + Y_LEN]:
            raise Retry("G would extend the first match")
        t = b.put(G[:4 + extra])
        ms = [(at, at - y_at, Y_LEN), (t, t - g_at, 4 + extra)]
        if follow == "zero":
            z = b.put(Y)
            ms.append((z, z - at, Y_LEN))
            b.fresh(1, avoid=(b.b[at + Y_LEN],))
            b.fresh(19)
        else:
            b.fresh(1, avoid=(G[4 + extra],))
            b.fresh((max(5, 10 - extra) if follow == "end" else 20) - 1)     # (the hit is one byte on, and its successor must be inside mflimit)
        return _exactly(at, ms)
    return body


# ---- T: tag and bucket -------------------------------------------------------------------------------------------------------------------
T_FORMS = ("equal", "tag-equal", "tag-other", "bit 3", "bit 4", "bit 13", "bit 14")


def _second_word(b, A, form):
    if form == "equal":
        return A
    if form.startswith("bit"):
        w = word_of(product(le(A)) ^ 1 << int(form[4:]))
        if 0 in w:
            raise Retry("a zero byte")
        return w
    return b.tagged(A, form == "tag-equal")[0]


def t_search(form):
    """A under probe 5 of the first search, B under probe 20, A once more behind them"""
    def body(b, s):
        A = b.word()
        B = _second_word(b, A, form)
        pa, pb = probe(s, 5), probe(s, 20)
        _put_word(b, pa, A)
        if form == "equal":
            b.goto(pb, avoid_last=(b.b[pa - 1],))
            _put_word(b, pb, A, not_like=pa)
            pc = pb + 4 + 1 + 15                                           # probe 15 of the search behind the match
            b.goto(pc, avoid_last=(b.b[pb - 1],))
            _put_word(b, pc, A, not_like=pb)
            _tail(b, 30)
            return _exactly(0, [(pb, pb - pa, 4), (pc, pc - pb, 4)])
        _put_word(b, pb, B)
        _put_word(b, probe(s, 40), A)
        _tail(b, 30)
        return _none(0, b.pos)
    return body


def t_test(form):
    """A under probe 8 of the first search; B directly behind the first match, where the test of the next position probes; A once more"""
    def body(b, s):
        s2, y_at, Y, a_at, A = opener(b, s, old=True)
        B = _second_word(b, A, form)
        b.b.pop()
        if B[0] == b.b[y_at - Y_OFF + Y_LEN]:
            raise Retry("B would extend the first match")
        e = b.put(B)
        assert e == s2 - 1
        if form == "equal":
            b.fresh(1, avoid=(b.b[a_at + 4],))
            _tail(b, 30)
            return _exactly(s, [(y_at, Y_OFF, Y_LEN), (e, e - a_at, 4)])
        _put_word(b, probe(s2, 10), A)
        _tail(b, 30)
        return _exactly(s, [(y_at, Y_OFF, Y_LEN)])
    return body


def family_T():
    f = Family("T")
    for k, form in enumerate(T_FORMS):
        f.add(f"search {form}", *build(t_search(form), 11000 + k))
        f.add(f"test {form}", *build(t_test(form), 11100 + k))
    f.moves = ["TagRejectS", "TagRejectT", "WordDiffersS", "WordDiffersT", "HitS", "HitT"]
    for site, slot in (("search", "S"), ("test", "T")):
        f.pair(f"{site} tag-equal", f"{site} tag-other", "TagReject" + slot)
        f.pair(f"{site} tag-other", f"{site} tag-equal", "WordDiffers" + slot)
        f.pair(f"{site} bit 3", f"{site} bit 4", "TagReject" + slot)       # the two ends of the tag field, and the bits just outside
        f.pair(f"{site} bit 14", f"{site} bit 13", "TagReject" + slot)
        f.pair(f"{site} bit 4", f"{site} bit 3", "WordDiffers" + slot)
        f.pair(f"{site} bit 13", f"{site} bit 14", "WordDiffers" + slot)
        f.pair(f"{site} tag-equal", f"{site} equal", "Hit" + slot)
    return f


# ---- P: the candidate that put() inserts -----------------------------------------------------------------------------------------------------
def p_case(b, s):
    """the first match ends at e; the word at e - 2, which only put() inserts, stands again under probe 15 of the search behind it"""
    s2, y_at, Y, _, _ = opener(b, s)
    e = s2 - 1
    b.fresh(1)
    W = bytes(b.b[e - 2:e + 2])
    q = probe(s2, 15)
    b.goto(q, avoid_last=(b.b[e - 3],))
    b.put(W)
    b.fresh(1, avoid=(b.b[e + 2],))
    _tail(b, 30)
    return _exactly(s2, [(q, q - (e - 2), 4)])


def family_P():
    f = Family("P")
    f.add("the word at e - 2 again", *build(p_case, 12000))
    f.add("the word at e - 2 again, another seed", *build(p_case, 12001))
    f.moves = ["HitS"]
    return f


# ---- K: the one-store emit ---------------------------------------------------------------------------------------------------------------------
K_LL, K_EXTRA = tuple(range(17)), (0, 14, 15)


def family_K():
    f = Family("K")
    for ll in K_LL:
        for x, extra in enumerate(K_EXTRA):
            for o, kind in enumerate(OFFSET_KINDS):
                f.add(f"ll={ll} extra={extra} offset {kind}", *build(k_case(ll, extra, kind), 13000 + 64 * ll + 4 * x + o))
            f.add(f"ll={ll} extra={extra} then zero-literal", *build(k_case(ll, extra, OFFSET_KINDS[(ll + x) % 3], "zero"), 14000 + 4 * ll + x))
            f.add(f"ll={ll} extra={extra} then the end", *build(k_case(ll, extra, OFFSET_KINDS[(ll + x + 1) % 3], "end"), 14100 + 4 * ll + x))
    # the last sequence's literals begin at n - 16 and at n - 15, the match at n - 13, the last position a search looks at (eight bytes,
    # five last literals)
    f.add("anchor at n - 16", *build(k_case(3, 4, follow="end"), 14200))
    f.add("anchor at n - 15", *build(k_case(2, 4, follow="end"), 14201))
    for x, extra in enumerate((1, 14, 15)):
        f.add(f"ll=0 by catch-up extra={extra}", *build(k_ll0_search(extra), 14210 + x))
    f.add("ll=0 by catch-up then zero-literal", *build(k_ll0_search(3, "zero"), 14220))
    for ll in (5, 6, 7, 14):
        f.add(f"ll={ll} extra=15 generic", *build(k_case(ll, 15, "both bytes", "zero"), 14300 + ll, generic=True))
    f.moves = ["PackSh8To40", "PackSh48", "PackSh56", "PackSh64Up", "PlainLong", "PlainTail", "ZeroPacked", "CatchStopAnchor", "ZeroMissT", "HitS", "HitT",
               "GenericClear"]
    f.pair("anchor at n - 16", "anchor at n - 15", "PlainTail")
    f.pair("ll=14 extra=0 offset both bytes", "ll=13 extra=0 offset both bytes", "PackSh64Up")
    f.pair("ll=13 extra=0 offset both bytes", "ll=14 extra=0 offset both bytes", "PlainLong")
    f.pair("ll=4 extra=0 offset both bytes", "ll=5 extra=0 offset both bytes", "PackSh48")
    f.pair("ll=5 extra=0 offset both bytes", "ll=6 extra=0 offset both bytes", "PackSh56")
    f.pair("ll=6 extra=0 offset both bytes", "ll=7 extra=0 offset both bytes", "PackSh64Up")
    f.pair("ll=5 extra=0 offset both bytes", "ll=4 extra=0 offset both bytes", "PackSh8To40")
    return f


SWEEP_LL = tuple(range(14))
SWEEP_DELTAS = tuple(range(-12, 17))


def family_KS():
    """Each ll = 0 .. 13 as the LAST sequence before the shortest tail the format allows: a match of 11 bytes (extra = 7) and five last
    literals, so that anchor + 16 <= n holds for every ll and the capacity alone decides between the one store and the plain emit."""
    f = Family("KS")
    for ll in SWEEP_LL:
        f.add(f"last ll={ll}", *build(k_case(ll, 7, follow="end"), 15000 + ll))
    f.add("last ll=0 by catch-up", *build(k_ll0_search(7, "end"), 15100))
    # five last literals always fit behind a match that passed its own limit test (lz4.c:728 asks for six bytes): the last refusal needs more
    f.add("twelve last literals", *build(k_case(2, 7, tail=12), 15101))
    f.moves = ["PackSh8To40", "PackSh64Up", "ZeroPacked"]
    return f


def sweep_ll(name):
    """(ll, zero-literal site) of a block of family KS whose last sequence stands before the shortest tail"""
    if "twelve" in name:
        return None
    return (0, False) if "catch-up" in name else (int(name.split("=")[1]), name.endswith("ll=0"))


def limited_cases(oracle, cases):
    """[(name, block, cap, oracle's return value, oracle's bytes)] at every capacity from 12 below to 16 above the compressed size, and the full bound"""
    out = []
    for name, block, want, _ in cases:
        for cap, tag in [(len(want) + d, f"{d:+d}") for d in SWEEP_DELTAS] + [(compress_bound(len(block)), "bound")]:
            out.append((f"{name} cap={tag}", block, cap, oracle.compress_raw(block, cap)[0], want))
    assert {r > 0 for _, _, _, r, _ in out} == {False, True}
    return out


# what the capacity sweep must reach
LIMITED_MOVES = ("PlainCap", "ZeroPlainCap", "ZeroPacked", "PackSh8To40", "PackSh64Up", "RefuseLiterals", "RefuseMatch", "RefuseLastLiterals", "Copy8", "Copy1")


# ---- N: the count's tiers ----------------------------------------------------------------------------------------------------------------------
N_EXTRA = tuple(range(41))
N_DIFFER = tuple(range(24))


def family_N():
    f = Family("N")
    for e in N_EXTRA:
        f.add(f"match of 4+{e}, mismatch", *build(k_case(2, e, n_f=50), 16000 + e))
        if e >= 4:
            f.add(f"match of 4+{e}, matchlimit", *build(k_case(2, e, n_f=50, follow="limit"), 16100 + e))
    for k in N_DIFFER:
        f.add(f"candidate differs in byte {k} alone", *build(k_case(2, k, n_f=50, differ=True), 16200 + k))
    # a mismatch with fewer than 8, and fewer than 16, bytes left in front of matchlimit: the byte steps and the 8-byte step see it
    f.add("match of 4+2, mismatch 6 in front of matchlimit", *build(k_case(2, 2, n_f=50, tail=9), 16250))
    f.add("match of 4+10, mismatch 14 in front of matchlimit", *build(k_case(2, 10, n_f=50, tail=9), 16251))
    f.add("match of 4+3, mismatch 10 in front of matchlimit", *build(k_case(2, 3, n_f=50, tail=12), 16252))
    f.add("match of 4+16, mismatch generic", *build(k_case(2, 16, n_f=50), 16300, generic=True))
    f.add("match of 4+24, mismatch generic", *build(k_case(2, 24, n_f=50), 16301, generic=True))
    f.add("match of 4+29, matchlimit generic", *build(k_case(2, 29, n_f=50, follow="limit"), 16302, generic=True))
    f.moves = ["Count16Low", "Count16High", "Count16Equal", "Count16Limit", "Count8Diff", "Count8Equal", "Count8Limit", "Count1Equal", "Count1Diff", "Count1Limit"]
    f.pair("match of 4+15, mismatch", "match of 4+16, mismatch", "Count16Equal")
    f.pair("match of 4+16, mismatch", "match of 4+15, mismatch", "Count16High")
    f.pair("match of 4+23, mismatch", "match of 4+24, mismatch", "Count16High")
    f.pair("match of 4+24, mismatch", "match of 4+23, mismatch", "Count16Low")
    f.pair("match of 4+7, mismatch", "match of 4+8, mismatch", "Count16High")
    f.pair("match of 4+15, matchlimit", "match of 4+16, matchlimit", "Count16Equal")
    f.pair("match of 4+23, matchlimit", "match of 4+24, matchlimit", "Count8Equal")
    f.pair("match of 4+24, matchlimit", "match of 4+23, matchlimit", "Count1Equal")
    f.pair("candidate differs in byte 15 alone", "candidate differs in byte 16 alone", "Count16Equal")
    f.pair("candidate differs in byte 7 alone", "candidate differs in byte 8 alone", "Count16High")
    f.pair("candidate differs in byte 16 alone", "candidate differs in byte 15 alone", "Count16High")
    return f


# ---- L: the copy's tiers -------------------------------------------------------------------------------------------------------------------------
L_RUNS, L_LAST = tuple(range(14, 41)), tuple(range(5, 41))


def family_L():
    f = Family("L")
    for ll in L_RUNS:
        f.add(f"literal run of {ll}", *build(k_case(ll, 2), 17000 + ll))
    for run in L_LAST:
        f.add(f"last literals of {run}", *build(k_case(1, 8, tail=run), 17100 + run))
    f.add("literal run of 27 generic", *build(k_case(27, 2), 17200, generic=True))
    f.add("last literals of 29 generic", *build(k_case(1, 8, tail=29), 17201, generic=True))
    f.moves = ["Copy16", "Copy8", "Copy1", "PlainLong"]
    f.pair("last literals of 7", "last literals of 8", "Copy8")
    f.pair("last literals of 15", "last literals of 16", "Copy16")
    f.pair("last literals of 16", "last literals of 15", "Copy8")
    f.pair("last literals of 31", "last literals of 32", "Copy16")
    f.pair("last literals of 8", "last literals of 7", "Copy1")
    return f


# ---- V: the window, the catch-up, position 0 ------------------------------------------------------------------------------------------------------
def family_V():
    f = Family("V")
    f.add("position 0 by a search", *build(z_search(9), 18230))            # (the first block of a launch: its table was zeroed for it)
    f.add("position 0 by a test of the next position", *build(z_test(9), 18231))
    for i in (0, 1, 2, 3, 4, 5, 6, 64 + 5, 64 + 6, 128 + 5, 128 + 6, 128 + 7):
        f.add(f"search won at probe {i}", *build(s_winner_at(i), 18000 + i))
    for back in (0, 1, 2):
        f.add(f"catch-up of {back}", *build(c_back(back), 18200 + back))
    f.add("catch-up to the block's first byte", *build(c_back_to_start, 18210))
    f.add("hit directly behind a catch-up", *build(k_ll0_search(3, "zero"), 18220))
    f.moves = ["FwdRefill", "FwdServed0", "FwdServed1", "FwdServed2", "FwdServed3", "FwdServed4", "CatchStopAnchor", "CatchStopRef0", "CatchStopMismatch",
               "ZeroHitS", "ZeroHitT", "ZeroMissS", "ZeroMissT", "ZeroPacked"]
    f.pair("catch-up of 2", "catch-up to the block's first byte", "CatchStopRef0")
    f.pair("catch-up of 2", "hit directly behind a catch-up", "CatchStopAnchor")
    return f


# ---- Q: one lane, many blocks ----------------------------------------------------------------------------------------------------------------------
Q_KINDS = 8
Q_P, Q_P2 = 136, 100                   # where block A inserts U and U2


def _q_base():
    base = Build(19000)
    W = [base.word() for _ in range(Q_KINDS)]
    C = [base.tagged(w, False)[0] for w in W]
    U, U2 = base.word(), base.word()
    return base, W, C, U, U2


def _q_kind(i, base, W, C):
    """W_i | the other kinds' words and a collider of each (same bucket, another tag), every one under a probe of the first search, in an
    order of the seed's | [odd i: Y, and Y again] | W_i [i >= 4: and the block's bytes 4 .. 6].  The one match the oracle has besides
    Y's is the repeat, at position 0: out of a bucket that reads zero in a fresh table, and out of whatever an earlier block of the lane
    left there otherwise.  Even i: the search meets the repeat; odd i: the test of the next position behind Y's match.  The kinds
    that repeat W_i ALONE are the ones an encoder that misses the empty bucket cannot mend: where bytes 4 .. 6 follow, the word one
    byte on is the word at position 1, which the first probe inserted, and the catch-up walks that match back to the same bytes."""
    for attempt in range(60):
        b = Build(19100 + i + 7919 * attempt, strict=False)
        b.used |= base.used
        try:
            b.put(W[i])
            plants = [w for j in range(Q_KINDS) if j != i for w in (W[j], C[j])]
            for k in b.rng.permutation(len(plants)):
                b.put(plants[int(k)])
            assert b.pos == 60
            ms = []
            if i % 2:
                y_at, at = probe(1, 62), probe(1, 70)
                b.goto(y_at)
                Y = b.word() + _b(b.rng.permutation(200)[:2] + 1)
                b.put(Y)
                b.fresh(1)
                b.goto(at, avoid_last=(b.b[y_at - 1],))
                b.put(Y)
                if W[i][0] == b.b[y_at + Y_LEN]:
                    raise Retry("W would extend Y's match")
                ms.append((at, at - y_at, Y_LEN))
            else:
                b.goto(probe(1, 63))
            again = W[i] + (bytes(b.b[4:7]) if i >= Q_KINDS // 2 else b"")
            q = b.put(again)
            ms.append((q, q, len(again)))
            b.fresh(1, avoid=(b.b[len(again)],))
            b.fresh(20)
            block = b.finish()
        except Retry:
            continue
        assert len(block) <= 200
        return f"kind {i}", block, _exactly(0, ms)
    raise AssertionError("no seed gives this block")


def _q_pair(base, U, U2):
    """A: fresh bytes with U at Q_P and U2 at Q_P2, both probes of its one search (stride 2 from position 62 on: the even positions).
    B: Y at 2 and again at 61, U2 directly behind that match (the test of the next position), U at Q_P, which B's search from 68 steps
    over (its stride is 2 from 129 on: the odd positions), and U again under probe 80 of that search.  The oracle finds nothing for U
    in B: the table's entry for it is A's."""
    for attempt in range(60):
        a = Build(19200 + 7919 * attempt)
        a.used |= base.used
        b = Build(19300 + 7919 * attempt)
        b.used |= base.used
        try:
            a.fresh(1)
            assert Q_P in [probe(1, k) for k in range(140)] and Q_P2 in [probe(1, k) for k in range(140)]
            _put_word(a, Q_P2, U2)
            _put_word(a, Q_P, U)
            a.fresh(30)
            b.fresh(2)
            Y = b.word() + _b(b.rng.permutation(200)[:2] + 1)
            y_at = b.put(Y)
            b.fresh(1)
            at = 61
            b.goto(at, avoid_last=(b.b[y_at - 1],))
            b.put(Y)
            if U2[0] == b.b[y_at + Y_LEN]:
                raise Retry("U2 would extend the first match")
            b.put(U2)
            s2 = at + Y_LEN + 1
            assert Q_P not in [probe(s2, k) for k in range(140)]
            _put_word(b, Q_P, U)
            _put_word(b, probe(s2, 80), U)
            b.fresh(20)
            A, B = a.finish(), b.finish()
        except Retry:
            continue
        assert len(A) <= 200 and len(B) <= 200 and bytes(B[Q_P:Q_P + 4]) == U == bytes(A[Q_P:Q_P + 4])
        return ("pair A", A, _none(0, len(A))), ("pair B", B, _exactly(0, [(at, at - y_at, Y_LEN)]))
    raise AssertionError("no seed gives this pair")


def family_Q():
    f = Family("Q")
    base, W, C, U, U2 = _q_base()
    for i in range(Q_KINDS):
        f.add(*_q_kind(i, base, W, C))
    for case in _q_pair(base, U, U2):
        f.add(*case)
    f.moves = ["TableZeroed", "TableKept", "ZeroHitS", "OldHitS", "OldHitT", "OldMissS", "OldMissT", "OldTagEqualS", "OldTagEqualT", "CatchStopRef0"]
    return f


Q_LENGTHS = (62, 63, 64, 65, 126, 127, 128)


def q_sequence(cases, n):
    """n blocks for one lane: Q's blocks cycled, B always behind A"""
    return [cases[k % len(cases)] for k in range(n)]


# ---- R: the three refusals the reference does not have ---------------------------------------------------------------------------------------------
# The reference's limit tests count ll >> 8 and extra >> 8 length bytes where (length - 15) / 255 + 1 are written; it then runs past the
# capacity by the difference and returns 0 from a later test.  The kernel returns that 0 without the write, from three tests of its own,
# which can only decide once the difference exceeds the slack of the reference's test: 8, 3 and 6 bytes, one byte per 65 280 of length.
R_LITERALS, R_OFFSET, R_MATCH = 8 * 65280 + 2000, 3 * 65280 + 2000, 6 * 65280 + 2000


def r_literal_length(seed):
    """R_LITERALS random bytes and more, then the bytes under the search's last two probes made equal up to the block's end: one sequence
    with all those literals, a match that runs into matchlimit, five last literals"""
    rng = np.random.default_rng(seed)
    i = next(i for i in range(20000) if probe(1, i) >= R_LITERALS)
    prev, p = probe(1, i - 1), probe(1, i)
    n = p + (p - prev) + 12                                                # p + step == mflimit: the last position a search looks at
    a = rng.integers(1, 256, n).astype(np.uint8)
    if a[p - 1] == a[prev - 1]:
        a[p - 1] = a[p - 1] % 255 + 1
    for k in range(p, n):
        a[k] = a[k - (p - prev)]
    return a, _exactly(0, [(p, p - prev, n - 5 - p)])


def r_offset(seed):
    """abc abc ... for R_OFFSET bytes, then bc bc ... to the end: the first match ends where b stands for a, put() inserts b c b c two
    bytes in front of that, and the test of the next position finds it -- a zero-literal sequence behind a match with 770 length bytes"""
    rng = np.random.default_rng(seed)
    head = rng.integers(1, 250, 24).astype(np.uint8)
    abc = np.array([251, 252, 253], np.uint8)
    a = np.concatenate([head, np.tile(abc, R_OFFSET // 3), np.tile(abc[1:], 10)])
    e = 24 + R_OFFSET // 3 * 3
    return a, _has((e, 2, len(a) - 5 - e))


def r_match_length(seed):
    """24 random bytes and R_MATCH zeros to the end: one match with more than 1 500 length bytes, five last literals"""
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.integers(1, 256, 24).astype(np.uint8), np.zeros(R_MATCH, np.uint8)])

    def expect(seqs):
        assert len(seqs) == 2 and seqs[0][1] == 1 and seqs[0][2] > R_MATCH - 8 and seqs[1][0] == 5, seqs
    return a, expect


def family_R():
    f = Family("R")
    f.add("literal length bytes", *r_literal_length(20000))
    f.add("offset behind match length bytes", *r_offset(20001))
    f.add("match length bytes", *r_match_length(20002))
    f.moves = ["GenericClear", "Count16Equal", "Copy16", "PlainLong", "ZeroPacked"]
    return f


R_MOVES = ("RefuseLiteralLength", "RefuseOffset", "RefuseMatchLength")


# ---- the sets ----------------------------------------------------------------------------------------------------------------------------------
BUILDERS = {"T": family_T, "P": family_P, "K": family_K, "KS": family_KS, "N": family_N, "L": family_L, "V": family_V, "Q": family_Q, "R": family_R}
NAMES = tuple(BUILDERS)
GENERIC = ("K", "N", "L")              # the families with a block of the generic variant next to the 64k variant's
LARGE = ("R",)                         # ... and the one of blocks of hundreds of KiB, in batches of its own
GENERIC_MOVES = ("GenericClear", "GenericRefusedS", "GenericRefusedT", "HitS", "HitT", "PackSh48", "PackSh56", "PackSh64Up", "PlainLong", "ZeroPacked", "Count16Equal", "Count16High", "Count16Low",
                 "Count16Limit", "Count8Limit", "Count1Limit", "Copy16", "Copy8", "Copy1")
_families, _checked = {}, {}


def family(name):
    if name not in _families:
        _families[name] = BUILDERS[name]()
    return _families[name]


def checked(oracle, name):
    """[(case name, block, oracle's bytes, oracle's parse)] of a family, every expectation asserted against the oracle: computed once"""
    if name not in _checked:
        out = []
        for cname, block, expect in family(name).cases:
            want = oracle.compress(block)
            seqs = parse_sequences(want)
            assert sum(lit + (ml or 0) for lit, _, ml in seqs) == len(block), cname
            try:
                expect(seqs)
            except AssertionError as e:
                raise AssertionError(f"{cname}: the oracle does not parse this block as it was built: {e}") from None
            out.append((cname, block, want, seqs))
        _checked[name] = out
    return _checked[name]


def everything(oracle):
    return [c for name in NAMES if name not in LARGE for c in checked(oracle, name)]
