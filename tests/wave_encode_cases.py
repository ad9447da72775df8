"""Blocks BUILT for single branches of the wavefront fast encoder (lz4hip_encode.hpp: wave_find_step, wave_find_match, encode_fast_block64k
and its one-store emit, the hand-over rule), shared by tests/test_simt_wave_encode_cases.py and tests/test_gpu_wave_encode_cases.py, in the
manner of tests/encoder_cases.py and tests/hc_lane_cases.py.  Every builder returns (name, block, expectation); the expectation is about
the ORACLE's own parse -- which match, at which position, with which offset and length -- and is asserted against oracle.compress before
any kernel is asked (checked()).  A family names the EncStat slots (LZ4HIP_STAT_ENC, emu_enc_stats) that must move for it, and pairs of
blocks on the two sides of a threshold: encoded alone, the slot is smaller for the first block than for the second.

How a block is built.  The probe positions of a search are a fixed function of where it starts (probe()), so a word can be put under a
chosen lane of a chosen step.  Everything that is not planted is FRESH: every byte is chosen so that the word ending at it falls into a
hash bucket no other word of the block has (the generic hash's, which the 64k variant's refines) -- fresh bytes share no bucket and
match nothing, so the only shared buckets and the only matches of a block are the planted ones.  Words that share a bucket are found by
search (Build.colliders).  The three words that run from fresh bytes INTO a planted piece cannot be steered; Build.finish() refuses a
block in which one of them shares a bucket, and build() then takes the next seed.  All randomness comes from
np.random.default_rng(fixed seed).

64k variant: the body starts at position 0 and the first search at 1.  Generic variant (families marked G): 24 fresh bytes, zeros, then
the same body at the END of a block of more than LIMIT_64K bytes: one match covers the zeros, the test of the next position misses at
the body's first byte, and the search that follows starts one byte on, as it does at the head of a block.

Family S  search step (G)         shared buckets of 2, 3, 4 lanes, 1..3 of them in a step, the winner below, inside, between and above
Family X  end of input (G)        a search that starts at mflimit (- 1), the winner's successor at mflimit (+ 1), out of input above a bucket
Family F  first-step words        a search fed from first_words that is decided by the last lane inside the input
Family W  window                  test-next-position hits that walk q - wbase to 244 and to 245, all four rel & 3
Family C  test and count          wide against byte-wise, candidates that differ in one byte, lengths around 256 and 512, catch-ups of 0 .. 94
Family Z  position 0 (64k only)   the block's first four bytes again, met by a search, by a test-next-position, in a shared bucket
Family E  one-store emit          (ll, extra) around 15, every capacity from 12 below to 4 above the compressed size
Family H  hand-over               the 16th (32nd) sequence at 1 023 and 1 024 bytes from the last check"""
import numpy as np

from encoder_cases import CAP_DELTAS, LIMIT_64K, parse_sequences, placed

GOLDEN = 2654435761
# lz4hip::EncStat, in the kernel's order
SLOTS = ["StepMatchAllv", "StepMissAllv", "StepMatchMasked", "StepMissMasked", "StepOutMasked", "Rounds0", "Rounds1", "Rounds2", "Bucket2", "Bucket3",
         "Bucket4", "CandLower", "CandGathered", "WinHasLower", "WinHasHigher", "WinHasBoth", "BucketAboveWinner",
         "BucketSplitByWinner", "BucketBelowWinner", "RestoreLive", "RestoreLiveKept", "RestoreIntoDict", "GenericRefusal", "WinStep1", "WinStep2", "WinStep3",
         "FirstWords", "WindowRebase", "WindowServed", "TestWide", "TestBytewise", "TestHit", "TestMiss", "TestHit256", "AfterCombined",
         "AfterGuarded", "Back0", "Back1To63", "Back64", "Back64Continued", "EmitOne", "EmitOneRefused", "EmitGeneral", "DeferPassed",
         "Deferred", "Pos0Search", "Pos0Test"]
S = {name: i for i, name in enumerate(SLOTS)}
# slots no block moves, asserted to stay at 0 over every block (profiles/wave_encode_cases/README.md):
#   StepMissMasked    a step runs under the lane mask because its LAST lane is outside the input, and that lane stops it
#   RestoreIntoDict   only the dictionary encoder has positions in front of input_start
UNREACHED = ("StepMissMasked", "RestoreIntoDict")


def bucket(word, generic=False):
    """the fast encoder's bucket of a little-endian 4-byte word: shift 19 (64k variant, 8192 buckets) or 20 (generic, 4096)"""
    return ((np.asarray(word, np.uint64) * np.uint64(GOLDEN)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20 if generic else 19)


GOLDEN_INVERSE = pow(GOLDEN, -1, 1 << 32)


def product(word):
    """the 32-bit hash product of a little-endian word: bucket = product >> 19 (64k variant), the lane encoder's tag = product >> 4 & 0x3FF"""
    return int(word) * GOLDEN & 0xFFFFFFFF


def word_of(prod):
    """the four bytes whose hash product is prod"""
    return int(int(prod) * GOLDEN_INVERSE & 0xFFFFFFFF).to_bytes(4, "little")


def _b(values):
    return bytes(bytearray(int(x) for x in values))


def le(b):
    return int(b[0]) | int(b[1]) << 8 | int(b[2]) << 16 | int(b[3]) << 24


def skip_sum(a):
    q, r = a >> 6, a & 63
    return 32 * q * (q - 1) + q * r


def probe(s, i):
    """position of the i-th probe (from 0) of a search that starts at s (lz4.c:636-647): step k (from 1), lane l is i = 64 (k - 1) + l"""
    return s + skip_sum(67 + i) - skip_sum(67)


class Retry(Exception):
    pass


class Build:
    """a block under construction, left to right"""

    def __init__(self, seed, wide=False, strict=True):
        self.rng = np.random.default_rng(seed)
        self.strict = strict                              # False: a word that runs into a planted piece may share a fresh word's bucket
        self.b = bytearray()
        self.wide = wide                                  # True: fresh by the 64k variant's buckets only (more than about 3 000 fresh bytes)
        self.used = {0}
        self.loose = []
        self.planted_to = -1

    @property
    def pos(self):
        return len(self.b)

    def _key(self, w):
        return int(bucket(w, generic=not self.wide))

    def fresh(self, n=1, avoid=()):
        """n fresh bytes (1..255), the first of them not in `avoid`"""
        for k in range(n):
            for _ in range(4000):
                c = int(self.rng.integers(1, 256))
                if k == 0 and c in avoid:
                    continue
                if len(self.b) < 3:
                    break
                key = self._key(le(bytes(self.b[-3:]) + bytes([c])))
                if key not in self.used:
                    self.used.add(key)
                    break
            else:
                raise Retry("no fresh byte left")
            self.b.append(c)
        return self

    def goto(self, pos, avoid_last=()):
        """fresh bytes up to position pos; the last of them not in avoid_last"""
        assert pos >= self.pos, (pos, self.pos)
        if pos > self.pos:
            self.fresh(pos - self.pos - 1)
            self.fresh(1, avoid=avoid_last)
        return self

    def put(self, data):
        """planted bytes; returns where they start"""
        at = self.pos
        joined = at == self.planted_to                    # directly behind another planted piece: the words across the joint are planted too
        if not joined:
            self.loose += [p for p in range(at - 3, at) if p >= 0]
        self.b += bytes(bytearray(data))
        for p in range(max(at - 3, 0), self.pos - 3):
            key = self._key(le(self.b[p:p + 4]))
            if p < at and key in self.used and self.strict and not joined:
                raise Retry("a word that runs into a planted piece shares a bucket")
            self.used.add(key)
        self.planted_to = self.pos
        return at

    def zeros(self, n):
        at = self.pos
        self.loose += [p for p in range(at - 3, at) if p >= 0] + list(range(at + n - 3, at + n))
        self.b += bytes(n)
        return at

    def word(self):
        """a 4-byte word (bytes 1..255, all different) in a bucket of its own"""
        while True:
            w = self.rng.permutation(255)[:4] + 1
            key = self._key(le(w))
            if key not in self.used:
                self.used.add(key)
                return bytes(bytearray(int(x) for x in w))

    def colliders(self, k, like=None):
        """k different words (bytes 1..255) in ONE bucket of the 64k variant's hash, so of the generic one too; like: in that word's bucket"""
        for _ in range(64):
            c = self.rng.integers(1, 256, (1 << 18, 4)).astype(np.uint64)
            w = c[:, 0] | c[:, 1] << np.uint64(8) | c[:, 2] << np.uint64(16) | c[:, 3] << np.uint64(24)
            h = bucket(w)
            target = int(bucket(le(like))) if like is not None else None
            if target is None:
                hs, counts = np.unique(h, return_counts=True)
                for cand in hs[counts >= k]:
                    if (int(cand) >> 1 if not self.wide else int(cand)) not in self.used:
                        target = int(cand)
                        break
                if target is None:
                    continue
            ws = [int(x) for x in np.unique(w[h == target])]
            if like is not None:
                ws = [x for x in ws if x != le(like)]
            if len(ws) >= k:
                self.used.add(target >> 1 if not self.wide else target)
                return [bytes([x & 255, x >> 8 & 255, x >> 16 & 255, x >> 24]) for x in ws[:k]]
        raise Retry("no colliding words")

    def tagged(self, like, same_tag, k=1):
        """k different words (bytes 1..255) in the bucket of the word `like` whose tag -- bits 4 .. 13 of the hash product, which the lane
        encoder keeps next to a position -- is `like`'s (same_tag) or another.  The multiplier is odd: the word of a chosen product is the
        product times the multiplier's inverse mod 2^32.  The bucket is bits 19 .. 31; bits 0 .. 3 and 14 .. 18 are free."""
        prod = product(le(like))
        out = []
        for _ in range(4000):
            free = int(self.rng.integers(0, 1 << 9))
            tag = prod >> 4 & 0x3FF if same_tag else int(self.rng.integers(0, 1 << 10))
            if not same_tag and tag == prod >> 4 & 0x3FF:
                continue
            w = word_of(prod & 0xFFF80000 | (free >> 4) << 14 | tag << 4 | free & 15)
            if 0 not in w and w != bytes(like) and w not in out:
                out.append(w)
                if len(out) == k:
                    return out
        raise Retry("no tagged words")

    def finish(self):
        a = np.frombuffer(bytes(self.b), np.uint8).astype(np.uint64)
        w = a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)
        h = bucket(w, generic=not self.wide)
        for p in self.loose if self.strict else ():
            if p < len(h) and int((h == h[p]).sum()) != 1 and not (w[h == h[p]] == w[p]).all():
                raise Retry("a word that runs into a planted piece shares a bucket")
        return np.frombuffer(bytes(self.b), np.uint8).copy()


ZEROS = LIMIT_64K + 40


def build(body, seed, generic=False, wide=False, strict=True):
    """body(b, s): plants the case into Build b, whose first search starts at s, and returns the expectation"""
    for attempt in range(40):
        b = Build(seed + 7919 * attempt, wide, strict and not wide)
        try:
            if generic:
                b.fresh(24)
                b.zeros(ZEROS)
            b.fresh(1)
            expect = body(b, b.pos)
            block = b.finish()
        except Retry:
            continue
        assert generic == (len(block) >= LIMIT_64K), len(block)
        return block, expect
    raise AssertionError("no seed gives this block")


# ---- expectations ----------------------------------------------------------------------------------------------------------------------
def _has(*matches):
    def expect(seqs):
        have = [(p, o, m) for p, _, o, m in placed(seqs)]
        for m in matches:
            assert m in have, ("expected match", m, "oracle's", have[-12:])
    return expect


def _none(lo, hi):
    def expect(seqs):
        inside = [(p, o, m) for p, _, o, m in placed(seqs) if lo <= p < hi]
        assert inside == [], ("expected no match in", (lo, hi), "oracle's", inside)
    return expect


def _all(*expects):
    def expect(seqs):
        for e in expects:
            e(seqs)
    return expect


def _exactly(base, matches):
    """the matches at and behind position base are exactly these"""
    def expect(seqs):
        have = [(p, o, m) for p, _, o, m in placed(seqs) if p >= base]
        assert have == list(matches), ("expected", list(matches), "oracle's", have)
    return expect


class Family:
    """cases: [(name, block, expectation)]; moves: slots that must move over the family in one launch; pairs: [(a, b, slot)], cases a and b
    each encoded alone, counter[a][slot] < counter[b][slot]; dict_pick: indices of the cases that also go through the dictionary encoder"""

    def __init__(self, name):
        self.name, self.cases, self.moves, self.pairs, self.index = name, [], [], [], {}

    def add(self, name, block, expect):
        self.cases.append((f"{self.name} {name}", np.asarray(block, np.uint8), expect))
        self.index[name] = len(self.cases) - 1
        return len(self.cases) - 1

    def both(self, name, body, seed, generic):
        """the 64k block, and the generic one where the family has one"""
        self.add(name, *build(body, seed))
        if generic:
            self.add(name + " generic", *build(body, seed, generic=True))

    def pair(self, a, b, slot, generic=False):
        self.pairs.append((self.index[a], self.index[b], slot))
        if generic:
            self.pairs.append((self.index[a + " generic"], self.index[b + " generic"], slot))


# ---- the opener ------------------------------------------------------------------------------------------------------------------------
Y_LEN, Y_OFF = 6, 64


def opener(b, s, old=False):
    """A first search (from s) that ends in a match, so that what follows meets a search that starts behind a test-next-position that
    missed -- in the 64k variant the one fed from first_words: Y (6 bytes) at s + 1, [old: a word O at s + 8, which the search inserts,]
    Y again at s + 65, the LAST lane of the first step: every lane of a step gathers and ballots, also those above the winner, and this
    way the first search sees nothing of what the second one is built for (its one shared bucket, lanes 1 and 63, is in every block).
    Returns (s2, y_at, Y, o_at, O): the second search starts at s2 = s + 72, and the table holds Y at y_at = s + 65."""
    b.goto(s + 1)
    Y = b.word() + _b(b.rng.permutation(200)[:2] + 1)
    b.put(Y)
    after_y = None
    O, o_at = None, None
    if old:
        b.goto(s + 8)
        O = b.word()
        o_at = b.put(O)
    b.goto(s + 1 + Y_OFF, avoid_last=(b.b[s],))
    after_y = b.b[s + 1 + Y_LEN]
    b.put(Y)
    b.fresh(1, avoid=(after_y,))
    return s + Y_OFF + 8, s + 1 + Y_OFF, Y, o_at, O


def _tail(b, n=100):
    b.fresh(n)


def _copy_y(b, at, Y, y_at):
    """Y again at `at`, a match of exactly 6 that nothing extends"""
    b.goto(at, avoid_last=(b.b[y_at - 1],))
    b.put(Y)
    b.fresh(1, avoid=(b.b[y_at + Y_LEN],))
    return (at, at - y_at, Y_LEN)


def _put_word(b, at, w, not_like=None):
    """the word w at `at`; not_like: a position whose following byte the byte behind w must differ from (a match of exactly 4)"""
    b.goto(at)
    b.put(w)
    if not_like is not None:
        b.fresh(1, avoid=(b.b[not_like + 4],))


# ---- S: the search step ------------------------------------------------------------------------------------------------------------------
def s_two_lanes(found):
    def body(b, s):
        s2, y_at, Y, _, _ = opener(b, s)
        A, B = b.colliders(2)
        _put_word(b, probe(s2, 10), A)
        _put_word(b, probe(s2, 20), B)
        at = probe(s2, 64 + 3)
        src = probe(s2, 20) if found else probe(s2, 10)
        b.goto(at, avoid_last=(b.b[src - 1],))
        _put_word(b, at, B if found else A, not_like=src)
        _tail(b)
        return _has((at, at - src, 4)) if found else _none(s2, b.pos)
    return body


def s_run(count):
    """one byte `count` times at lane 10: lanes 10 .. 10 + count - 4 hold the same word, the winner is lane 11, its candidate lane 10"""
    def body(b, s):
        s2, *_ = opener(b, s)
        b.goto(probe(s2, 10))
        w = b.word()
        b.put(bytes([w[0]]) * count)
        b.fresh(1, avoid=(w[0],))
        _tail(b)
        return _has((s2 + 11, 1, count - 1))
    return body


def s_same_word(i, j):
    """one word under probes i and j of the second search"""
    def body(b, s):
        s2, *_ = opener(b, s)
        X = b.word()
        a, c = probe(s2, i), probe(s2, j)
        _put_word(b, a, X)
        b.goto(c, avoid_last=(b.b[a - 1],))
        _put_word(b, c, X, not_like=a)
        _tail(b)
        return _has((c, c - a, 4))
    return body


def s_many_lanes(k):
    """k lanes in one bucket, the two highest with the same word: the winner's candidate is the NEXT lower lane"""
    def body(b, s):
        s2, *_ = opener(b, s)
        ws = b.colliders(k - 1)
        lanes = [10 * (i + 1) for i in range(k)]
        for lane, w in zip(lanes[:-1], ws):
            _put_word(b, probe(s2, lane), w)
        a, c = probe(s2, lanes[-2]), probe(s2, lanes[-1])
        b.goto(c, avoid_last=(b.b[a - 1],))
        _put_word(b, c, ws[-1], not_like=a)
        _tail(b)
        return _has((c, c - a, 4))
    return body


def s_buckets(k):
    """k shared buckets in one step: k - 1 of two different words each, and the one of the winning pair"""
    def body(b, s):
        s2, *_ = opener(b, s)
        plants = []
        for i in range(k - 1):
            A, B = b.colliders(2)
            plants += [(4 + 5 * i, A), (24 + 5 * i, B)]
        for lane, w in sorted(plants):
            _put_word(b, probe(s2, lane), w)
        X = b.word()
        a, c = probe(s2, 40), probe(s2, 45)
        _put_word(b, a, X)
        b.goto(c, avoid_last=(b.b[a - 1],))
        _put_word(b, c, X, not_like=a)
        _tail(b)
        return _has((c, 5, 4))
    return body


def s_winner_below(b, s):
    """the winner (lane 5) below every lane of a shared bucket whose old entry is O's position: the bucket comes back holding it -- the
    test of the next position behind the match probes O again and must find it there"""
    s2, y_at, Y, o_at, O = opener(b, s, old=True)
    m = _copy_y(b, s2 + 5, Y, y_at)
    assert b.pos == s2 + 12
    b.b.pop()                                                              # (the byte behind the copy is O's first: not Y's seventh, or build() retries)
    if O[0] == b.b[y_at + Y_LEN]:
        raise Retry("O would extend the match")
    b.put(O)
    b.fresh(1, avoid=(b.b[o_at + 4],))
    A, B = b.colliders(2, like=O)
    _put_word(b, s2 + 17, A)
    _put_word(b, s2 + 27, B)
    _tail(b)
    return _has(m, (s2 + 11, s2 + 11 - o_at, 4))


def s_winner_between(b, s):
    """a bucket's lanes 3 and 20 (and 14), the winner at lane 8: lane 3's position stays -- the test behind the match probes its word"""
    s2, y_at, Y, _, _ = opener(b, s)
    A, B = b.colliders(2)
    _put_word(b, s2 + 3, A)
    m = _copy_y(b, s2 + 8, Y, y_at)
    b.b.pop()
    if A[0] == b.b[y_at + Y_LEN]:
        raise Retry("A would extend the match")
    b.put(A)
    b.fresh(1, avoid=(b.b[s2 + 3 + 4],))
    _put_word(b, s2 + 22, B)
    _tail(b)
    return _has(m, (s2 + 14, 11, 4))


def s_winner_above(b, s):
    """a bucket's lanes 3 and 7 below the winner at lane 15: the higher one's position stays"""
    s2, y_at, Y, _, _ = opener(b, s)
    A, B = b.colliders(2)
    _put_word(b, s2 + 3, A)
    _put_word(b, s2 + 7, B)
    m = _copy_y(b, s2 + 15, Y, y_at)
    b.b.pop()
    if B[0] == b.b[y_at + Y_LEN]:
        raise Retry("B would extend the match")
    b.put(B)
    b.fresh(1, avoid=(b.b[s2 + 7 + 4],))
    _tail(b)
    return _has(m, (s2 + 21, 14, 4))


def s_winner_above_alone(b, s):
    """the same bucket below the winner, and nothing of it behind: no lane of it above the winner either"""
    s2, y_at, Y, _, _ = opener(b, s)
    A, B = b.colliders(2)
    _put_word(b, s2 + 3, A)
    _put_word(b, s2 + 7, B)
    m = _copy_y(b, s2 + 15, Y, y_at)
    _tail(b)
    return _exactly(s2, [m])


def s_lowest_matches_old(b, s):
    """a shared bucket whose lowest lane matches the gathered old entry"""
    s2, y_at, Y, o_at, O = opener(b, s, old=True)
    at = probe(s2, 10)
    b.goto(at, avoid_last=(b.b[o_at - 1],))
    _put_word(b, at, O, not_like=o_at)
    A, = b.colliders(1, like=O)
    _put_word(b, probe(s2, 20), A)
    _tail(b)
    return _has((at, at - o_at, 4))


def s_winner_at(i):
    """the second search won by probe i with the table's old entry"""
    def body(b, s):
        s2, y_at, Y, _, _ = opener(b, s)
        m = _copy_y(b, probe(s2, i), Y, y_at)
        _tail(b)
        return _has(m)
    return body


def s_far_entry(delta, seed):
    """generic variant only: O at position 5, zeros, and O twice in the second search's first step, at lanes 10 and 20, lane 10
    65 535 + delta bytes behind position 5.  delta = 0: lane 10 takes the old entry.  delta = 1: it is refused inside the shared bucket,
    and lane 20 takes lane 10's position."""
    for attempt in range(40):
        b = Build(seed + 7919 * attempt)
        try:
            b.fresh(5)
            O = b.word()
            q = b.put(O)
            b.goto(24)
            b.zeros(q + 65535 + delta - (24 + 1 + Y_OFF + 8 + 10))
            b.fresh(1)
            s2, *_ = opener(b, b.pos)
            p = s2 + 10
            assert p - q == 65535 + delta
            b.goto(p, avoid_last=(b.b[q - 1],))
            _put_word(b, p, O, not_like=q)
            _put_word(b, s2 + 20, O, not_like=p)
            _tail(b)
            return b.finish(), _has((p, 65535, 4)) if delta == 0 else _all(_has((s2 + 20, 10, 4)), _none(p, p + 1))
        except Retry:
            continue
    raise AssertionError("no seed gives this block")


WINNERS = (0, 60, 61, 62, 63, 64, 127)


def family_S():
    f = Family("S")
    G = True
    f.both("two lanes, the higher one's word again", s_two_lanes(True), 1000, G)
    f.both("two lanes, the lower one's word again", s_two_lanes(False), 1001, G)
    f.both("aaaaa", s_run(5), 1002, G)
    f.both("aaaaaa", s_run(6), 1003, G)
    f.both("one word at lanes 10 and 30", s_same_word(10, 30), 1004, G)
    f.both("one word at lanes 5 and 9 of step 2", s_same_word(64 + 5, 64 + 9), 1005, G)
    f.both("one word at lanes 5 and 9 of step 3", s_same_word(128 + 5, 128 + 9), 1006, G)
    f.both("three lanes in a bucket", s_many_lanes(3), 1007, G)
    f.both("four lanes in a bucket", s_many_lanes(4), 1008, G)
    f.both("two shared buckets", s_buckets(2), 1009, G)
    f.both("three shared buckets", s_buckets(3), 1010, G)
    f.both("winner below a bucket with a live entry", s_winner_below, 1011, G)
    f.both("winner between two lanes of a bucket", s_winner_between, 1012, G)
    f.both("winner above a bucket", s_winner_above, 1013, G)
    f.both("lowest lane matches the old entry", s_lowest_matches_old, 1014, G)
    f.both("winner above a bucket, nothing behind", s_winner_above_alone, 1015, G)
    for i in WINNERS:
        f.both(f"winner at probe {i}", s_winner_at(i), 1020 + i, G)
    f.add("old entry 65535 back generic", *s_far_entry(0, 1100))
    f.add("old entry 65536 back generic", *s_far_entry(1, 1101))
    f.pair("old entry 65535 back generic", "old entry 65536 back generic", "GenericRefusal")
    f.pair("old entry 65536 back generic", "old entry 65535 back generic", "WinHasHigher")
    f.moves = ["GenericRefusal", "StepMatchAllv", "StepMissAllv", "Rounds0", "Rounds1", "Rounds2", "Bucket2", "Bucket3", "Bucket4", "CandLower", "CandGathered",
               "WinHasLower", "WinHasHigher", "WinHasBoth", "BucketAboveWinner", "BucketSplitByWinner",
               "BucketBelowWinner", "RestoreLive", "RestoreLiveKept", "WinStep1", "WinStep2", "WinStep3", "FirstWords", "TestHit"]
    f.pair("aaaaa", "two shared buckets", "Rounds2", G)
    f.pair("winner at probe 0", "aaaaa", "Rounds1", G)
    f.pair("aaaaa", "aaaaaa", "Bucket3", G)
    f.pair("aaaaa", "aaaaaa", "WinHasBoth", G)
    f.pair("aaaaaa", "aaaaa", "WinHasLower", G)
    f.pair("three lanes in a bucket", "four lanes in a bucket", "Bucket4", G)
    f.pair("winner above a bucket", "winner below a bucket with a live entry", "RestoreLiveKept", G)
    f.pair("winner at probe 0", "winner between two lanes of a bucket", "BucketSplitByWinner", G)
    f.pair("winner between two lanes of a bucket", "winner above a bucket, nothing behind", "BucketBelowWinner", G)
    f.pair("winner at probe 63", "winner at probe 64", "WinStep2", G)
    f.pair("one word at lanes 5 and 9 of step 2", "one word at lanes 5 and 9 of step 3", "WinStep3", G)
    f.pair("aaaaa", "lowest lane matches the old entry", "WinHasHigher", G)
    return f


# ---- X: the end of the input inside a step -----------------------------------------------------------------------------------------------
def x_starts_at(delta):
    """the second search starts at mflimit - delta: lanes 0 .. delta - 1 probe, nothing is found"""
    def body(b, s):
        s2, y_at, Y, _, _ = opener(b, s)
        b.goto(s2 + delta + 12)                                            # n: mflimit = n - 12 = s2 + delta
        return _exactly(s, [(y_at, Y_OFF, Y_LEN)])
    return body


def x_successor(delta):
    """one word at lanes 5 and 10 of the second search; the block ends so that lane 10's successor is mflimit + delta"""
    def body(b, s):
        s2, y_at, Y, _, _ = opener(b, s)
        X = b.word()
        a, c = s2 + 5, s2 + 10
        _put_word(b, a, X)
        b.goto(c, avoid_last=(b.b[a - 1],))
        _put_word(b, c, X, not_like=a)
        b.goto(c + 1 - delta + 12)
        return _exactly(s2, [(c, 5, 4)] if delta <= 0 else [])
    return body


def x_out_above_bucket(b, s):
    """two lanes in one bucket, and the input ends at lane 12"""
    s2, *_ = opener(b, s)
    A, B = b.colliders(2)
    _put_word(b, s2 + 3, A)
    _put_word(b, s2 + 8, B)
    b.goto(s2 + 12 + 12)                                                   # lane 11's successor is mflimit, lane 12's is not
    return _none(s2, b.pos)


def family_X():
    f = Family("X")
    f.both("search starts at mflimit", x_starts_at(0), 2000, True)
    f.both("search starts at mflimit - 1", x_starts_at(1), 2001, True)
    f.both("winner's successor at mflimit", x_successor(0), 2002, True)
    f.both("winner's successor at mflimit + 1", x_successor(1), 2003, True)
    f.both("out of input above a shared bucket", x_out_above_bucket, 2004, True)
    f.moves = ["StepOutMasked", "StepMatchMasked", "Bucket2", "Rounds1", "BucketBelowWinner"]
    f.pair("winner's successor at mflimit + 1", "winner's successor at mflimit", "StepMatchMasked", True)
    f.pair("winner's successor at mflimit", "winner's successor at mflimit + 1", "StepOutMasked", True)
    return f


# ---- F: first-step words ------------------------------------------------------------------------------------------------------------------
def family_F():
    """The search behind a test-next-position that missed takes its first step's words from first_words, loaded by that test from
    addresses clamped to n - 4.  A lane is clamped from p = n - 4 on and probes up to p = n - 13 only, so a clamped lane never decides;
    the search is decided by the last lane inside the input (its successor at mflimit) or ends there (the pair).  Lanes 61 .. 63 are the
    ones first_probe_offset moves."""
    f = Family("F")
    f.add("near the end: the last lane inside the input wins", *build(x_successor(0), 3000))
    f.add("near the end: the first lane beyond", *build(x_successor(1), 3001))
    for i in (60, 61, 62, 63):
        f.add(f"far from the end: lane {i} wins", *build(s_winner_at(i), 3010 + i))
    f.moves = ["FirstWords", "StepMatchMasked", "StepOutMasked", "StepMatchAllv"]
    f.pair("near the end: the first lane beyond", "near the end: the last lane inside the input wins", "StepMatchMasked")
    return f


# ---- W and C: a source that the first search inserts, and copies of its pieces ----------------------------------------------------------
def _source(b, s, n):
    """n bytes, all different, at s .. s + n - 1 (n <= 60: every position is a probe of the first search's first step, and inserted)"""
    assert n <= 60
    b.goto(s)
    for _ in range(200):
        F = bytes(bytearray(int(x) for x in b.rng.permutation(254)[:n] + 1))
        keys = {b._key(le(F[i:i + 4])) for i in range(n - 3)}
        if len(keys) == n - 3 and not keys & b.used:
            at = b.put(F)
            b.fresh(1, avoid=tuple(F))                                     # (no piece of the source continues into this byte)
            return at, F
    raise Retry("no source")


def _chain(b, s, src_at, F, pieces, lead=8):
    """behind the source: `lead` bytes of it again, found by the first search, then the pieces [(start in F, length)], each the hit of a
    test-next-position.  Returns the matches."""
    b.fresh(4)
    b.fresh(1, avoid=(b.b[src_at - 1],))
    at = b.pos
    b.put(F[:lead])
    out = [(at, at - src_at, lead)]
    prev_end = lead
    for start, length in pieces:
        assert start + length <= len(F) and (prev_end == len(F) or F[start] != F[prev_end]), (start, length)
        at = b.pos
        b.put(F[start:start + length])
        out.append((at, at - (src_at + start), length))
        prev_end = start + length
    b.fresh(1, avoid=(b.b[src_at + prev_end],))
    return out


def w_walk(last, at_mflimit=False):
    """four hits of 55, 54, 53 and 52 bytes and one of `last`: the sixth test-next-position stands at q - wbase = 214 + last"""
    def body(b, s):
        src_at, F = _source(b, s, 56)
        b.fresh(3)
        ms = _chain(b, s, src_at, F, [(1, 55), (2, 54), (3, 53), (4, 52), (5, last), (7, 7)])
        if at_mflimit:
            # the sixth test at ip = mflimit: the block ends 12 bytes behind it, the hit runs into matchlimit
            b.goto(ms[-1][0] + 12)
            return _exactly(s, ms)
        b.fresh(8)                                                         # (no seventh test: it would re-base on either side)
        return _exactly(s, ms)
    return body


def w_rel(first):
    """hits of `first`, then 5, 5, 5, 5 bytes: rel & 3 takes all four values"""
    def body(b, s):
        src_at, F = _source(b, s, 56)
        b.fresh(3)
        ms = _chain(b, s, src_at, F, [(10, first), (30, 5), (20, 5), (40, 5), (12, 5), (45, 5)])
        b.fresh(300)
        return _exactly(s, ms)
    return body


def family_W():
    f = Family("W")
    f.add("walk to 244", *build(w_walk(30), 4000))
    f.add("walk to 245", *build(w_walk(31), 4001))
    f.add("re-base at 245, test at mflimit", *build(w_walk(31, at_mflimit=True), 4002))
    f.add("walk to 248", *build(w_walk(34), 4003))                         # (the first q - wbase whose third dword would be lane 64's)
    for first in (4, 5, 6, 7):
        f.add(f"rel & 3 from {first}", *build(w_rel(first), 4010 + first))
    f.moves = ["WindowRebase", "WindowServed", "TestHit", "TestWide", "TestBytewise", "TestMiss"]
    f.pair("walk to 244", "walk to 245", "WindowRebase")
    f.pair("walk to 245", "walk to 244", "WindowServed")
    return f


def _long_source(b, s, n):
    """n fresh bytes at s: the first search inserts the first of their words (lane 0)"""
    b.goto(s)
    at = b.pos
    b.fresh(n)
    return at, bytes(b.b[at:at + n])


def c_test_length(length, to_limit=False, tail=300):
    """Y | R (`length` + 8 fresh bytes, the first search inserts R's first word) | Y again (found by the search) | R[:length]: a
    test-next-position that hits for exactly `length` bytes; to_limit: the block ends five bytes behind them"""
    def body(b, s):
        b.goto(s)
        Y = bytes(bytearray(int(x) for x in b.rng.permutation(254)[:12] + 1))     # (twelve bytes: the search's stride is up to 4 where it meets them again)
        y_at = b.put(Y)
        b.fresh(1)
        r_at, R = _long_source(b, b.pos, length + 8)
        assert r_at - s <= 60
        b.fresh(39)
        b.fresh(1, avoid=(b.b[y_at - 1],))
        at = b.put(Y)
        if R[0] == b.b[y_at + 12]:
            raise Retry("R would extend the match")
        t = b.put(R[:length])
        if to_limit:
            b.put(R[length:length + 5])
            return _exactly(at, [(at, at - y_at, 12), (t, t - r_at, length)])
        b.fresh(1, avoid=(R[length],))
        b.fresh(tail)
        return _exactly(at, [(at, at - y_at, 12), (t, t - r_at, length)])
    return body


def c_wide_edge(delta):
    """the test-next-position at ip with ip + 256 = matchlimit + delta"""
    def body(b, s):
        e = c_test_length(9, tail=0)(b, s)
        ip = b.pos - 1 - 9
        b.goto(ip + 256 - delta + 5)
        return e
    return body


def c_differs_in(k, tail):
    """The test-next-position behind the first match meets a word that is the block's first word but for byte k, in an empty bucket:
    the candidate is "position 0", and differs in that byte alone.  (Two words of one bucket that differ in a single byte do not exist
    for bytes 0 and 1 -- the hash is a multiplication by the golden ratio, and one byte's difference always moves its upper bits -- so the
    empty bucket is how such a candidate comes about.)"""
    def body(b, s):
        assert s == 1
        s2, y_at, Y, _, _ = opener(b, s)
        first = bytearray(b.b[:4])
        b.b.pop()
        for _ in range(400):
            c = int(b.rng.integers(1, 256))
            first[k] = c
            if c != b.b[k] and b._key(le(first)) not in b.used and first[0] != b.b[s + 1 + Y_LEN]:
                break
        else:
            raise Retry("no such word")
        b.put(bytes(first))
        b.fresh(tail)
        return _exactly(s, [(y_at, Y_OFF, Y_LEN)])
    return body


def c_after_search(delta):
    """a search won at ip with ip + 4 + 256 = matchlimit + delta"""
    def body(b, s):
        s2, y_at, Y, _, _ = opener(b, s)
        m = _copy_y(b, s2 + 7, Y, y_at)
        b.goto(s2 + 7 + 4 + 256 - delta + 5)
        return _has(m)
    return body


def c_search_to_limit(b, s):
    """R (300 fresh bytes) from s on, and its first 264 bytes again at a probe of the first search, where the block ends: the search wins
    at ip with ip + 4 + 256 = matchlimit + 1 and the match runs into matchlimit, 259 bytes.  Counted in one unguarded round it would be 260."""
    r_at, R = _long_source(b, s, 300)
    at = next(probe(s, i) for i in range(100, 400) if probe(s, i) >= b.pos + 12)
    b.goto(at, avoid_last=(b.b[r_at - 1],))
    b.put(R[:264])
    return _exactly(s, [(at, at - r_at, 259)])


def c_long_back(b, s):
    """A catch-up of more than 64 bytes below 64 KiB.  Where the first search's stride is 8 it inserts every eighth position.  A (200
    fresh bytes) lies there, and A again 204 bytes on: the probes inside the copy stand four bytes off the positions inserted in A, so
    none of them finds anything -- until the stride becomes 9, 512 bytes on, and the fifth probe from there lands on
    one.  The match is found 94 bytes into the copy and caught up to its start."""
    z = probe(s, 512 - 67)                                                 # the first probe with stride 8 (attempts = 512)
    assert probe(s, 512 - 67 + 1) - z == 8 and probe(s, 576 - 67) == z + 512 and probe(s, 576 - 67 + 1) == z + 521
    a_at = z + 250
    b.goto(a_at)
    b.fresh(200)
    A = bytes(b.b[a_at:a_at + 200])
    at = a_at + 204
    b.goto(at, avoid_last=(b.b[a_at - 1],))
    b.put(A)
    b.fresh(1, avoid=(b.b[a_at + 200],))
    b.fresh(300)
    return _exactly(s, [(at, 204, 200)])


def c_back_to_start_64(R):
    """A catch-up of 64 bytes and more that ends at the block's first byte: bound = ref = R, 64 or 65.  Position R must be in the table
    and the 64 bytes in front of it equal on both sides, so the block's first R + 5 bytes stand again at B, where the search's stride is
    33: one probe falls in front of B, one on B + R - 33 and the next on B + R.  The word at position R - 33 is in the table, so a word
    C of its bucket stands under an earlier probe and takes the entry: the probe at B + R - 33 meets C and misses, the one at B + R
    finds R.  R = 64: the first search inserts position 64 (lane 62), nothing before B matches, bound == 64.  R = 65: no search from 1
    probes position 65, so Y stands at 10 and again at 61, a match of 4 that ends at 65, and the test of the next position there
    inserts it; the search from 66 is the long one.  back == 64 && bound == 65 is where `bound > 64` decides: the 65th byte is equal."""
    def make(seed):
        for attempt in range(60):
            rng = np.random.default_rng(seed + 7919 * attempt)
            s0 = 1 if R == 64 else 66
            i = next(i for i in range(2, 4000) if probe(s0, i) - probe(s0, i - 1) == 33 and probe(s0, i - 1) - probe(s0, i - 2) == 33) + 5
            hit = probe(s0, i)
            B = hit - R
            n = hit + 5 + 300
            a = rng.integers(1, 256, n).astype(np.uint8)
            if R == 65:
                a[61:65] = a[10:14]
                if a[65] == a[14] or a[60] == a[9]:
                    continue
            a[B:B + R + 5] = a[:R + 5]
            if a[B + R + 5] == a[R + 5]:
                continue
            w = _words(a)
            h = bucket(w)
            # C: another word of the bucket of the word at R - 33, under a probe between the head and B
            ci = probe(s0, 900)
            c = rng.integers(1, 256, (1 << 18, 4)).astype(np.uint64)
            cw = c[:, 0] | c[:, 1] << np.uint64(8) | c[:, 2] << np.uint64(16) | c[:, 3] << np.uint64(24)
            cw = cw[(bucket(cw) == h[R - 33]) & (cw != w[R - 33])]
            if not len(cw):
                continue
            x = int(cw[0])
            a[ci:ci + 4] = [x & 255, x >> 8 & 255, x >> 16 & 255, x >> 24]
            w = _words(a)
            h = bucket(w)
            probes = [probe(s0, k) for k in range(i)]
            assert probes[-1] == hit - 33 == B + R - 33 and probes[-2] < B and ci in probes
            # nothing else may take the entries of R and of C, and no probe before the hit may find its word: the walk below is the serial search
            table, ok = {}, True
            head = (list(range(1, 62)) + [62, 64, 66]) if R == 64 else (list(range(1, 62)) + [63, 65])
            for q in head:
                table[int(h[q])] = q
            for q in probes[67 if R == 64 else 0:]:
                r = table.get(int(h[q]), 0)
                if w[r] == w[q]:
                    ok = False
                table[int(h[q])] = q
            if not ok or table.get(int(h[hit])) != R:
                continue
            first = [(61, 51, 4)] if R == 65 else []
            return a, _exactly(1, first + [(B, B, R + 5)])
        raise AssertionError("no seed gives this block")
    return make


def c_back(back):
    """Y (12 bytes) again where the search's stride is back + 1, its first probe `back` bytes into the copy: the catch-up takes `back` bytes"""
    def body(b, s):
        b.goto(s)
        Y = bytes(bytearray(int(x) for x in b.rng.permutation(254)[:12] + 1))
        y_at = b.put(Y)
        i = 64 * back + 20                                                 # a probe of step back + 1
        at = probe(s, i) - back
        assert probe(s, i - 1) < at
        b.goto(at, avoid_last=(b.b[y_at - 1],))
        b.put(Y)
        b.fresh(1, avoid=(b.b[y_at + 12],))
        b.fresh(300)
        return _has((at, at - y_at, 12))
    return body


def c_back_to_start(b, s):
    """the block's first bytes again, met two bytes in (stride 3): the catch-up reaches the block's first byte (bound = ref)"""
    if s != 1:
        raise AssertionError("64k variant only")
    b.put(bytes(bytearray(int(x) for x in b.rng.permutation(254)[:11] + 1)))
    first = bytes(b.b[:12])
    i = 128 + 20
    at = probe(s, i) - 2
    b.goto(at)
    b.put(first)
    b.fresh(1, avoid=(b.b[12],))
    b.fresh(300)
    return _has((at, at, 12))


def c_back_room(b, s):
    """q T (T = 8 bytes) where the stride is 2 and T's first position is no probe; then Y again, whose match ends in q, then T: the test
    of the next position misses (T's first word was never inserted), the search finds T one byte in, and the catch-up may take ONE byte,
    T's first: the one before it is equal too, and belongs to the match before (bound = room)"""
    Y = bytes(bytearray(int(x) for x in b.rng.permutation(254)[:6] + 1))
    q = Y[5]
    b.goto(s + 1)
    y_at = b.put(Y)
    i = 64 + 10
    t_at = probe(s, i) - 1                                                 # T[1:5] is probed, T[0:4] is not
    b.goto(t_at - 1)
    T = bytes(bytearray(int(x) for x in b.rng.permutation(254)[:8] + 1))
    if q in T:
        raise Retry("q in T")
    b.put(bytes([q]) + T)
    b.fresh(1)
    if T[0] == b.b[y_at + Y_LEN]:
        raise Retry("T would extend the match")
    j = 64 + 40
    at = probe(s, j)
    b.goto(at, avoid_last=(b.b[y_at - 1],))
    b.put(Y)
    t2 = b.put(T)
    b.fresh(1, avoid=(b.b[t_at + 8],))
    b.fresh(300)
    return _exactly(at, [(at, at - y_at, Y_LEN), (t2, t2 - t_at, 8)])


TEST_LENGTHS = (4, 7, 8, 255, 256, 257, 511, 512, 513)


def family_C():
    f = Family("C")
    f.add("test at ip + 256 = matchlimit", *build(c_wide_edge(0), 5000))
    f.add("test at ip + 256 = matchlimit + 1", *build(c_wide_edge(1), 5001))
    for k in range(4):
        f.add(f"candidate differs in byte {k}, wide", *build(c_differs_in(k, 300), 5010 + k))
        f.add(f"candidate differs in byte {k}, byte-wise", *build(c_differs_in(k, 40), 5020 + k))
    for n in TEST_LENGTHS:
        f.add(f"test hits for {n}", *build(c_test_length(n), 5100 + n))
    f.add("test hits up to matchlimit", *build(c_test_length(300, to_limit=True), 5030))
    f.add("test hits up to matchlimit, ip + 256 = matchlimit + 1", *build(c_test_length(255, to_limit=True), 5031))
    f.add("search runs into matchlimit, ip + 4 + 256 = matchlimit + 1", *build(c_search_to_limit, 5032, strict=False))
    f.add("catch-up of 94", *build(c_long_back, 5033, wide=True))
    f.add("catch-up of 64 to the block's first byte, bound 64", *c_back_to_start_64(64)(5070))
    f.add("catch-up of 65 to the block's first byte, bound 65", *c_back_to_start_64(65)(5071))
    f.add("search at ip + 4 + 256 = matchlimit", *build(c_after_search(0), 5040))
    f.add("search at ip + 4 + 256 = matchlimit + 1", *build(c_after_search(1), 5041))
    for back in (0, 1, 2):
        f.add(f"catch-up of {back}", *build(c_back(back), 5050 + back))
    f.add("catch-up to the block's first byte", *build(c_back_to_start, 5060))
    f.add("catch-up bounded by the literals", *build(c_back_room, 5061))
    f.moves = ["TestWide", "TestBytewise", "TestHit", "TestMiss", "TestHit256", "AfterCombined", "AfterGuarded", "Back0", "Back1To63", "Back64", "Back64Continued",
               "WindowRebase"]
    f.pair("catch-up of 2", "catch-up of 94", "Back64Continued")
    f.pair("catch-up of 64 to the block's first byte, bound 64", "catch-up of 65 to the block's first byte, bound 65", "Back64Continued")
    f.pair("catch-up of 65 to the block's first byte, bound 65", "catch-up of 64 to the block's first byte, bound 64", "Back64")
    f.pair("test at ip + 256 = matchlimit + 1", "test at ip + 256 = matchlimit", "TestWide")
    f.pair("test hits for 255", "test hits for 256", "TestHit256")
    f.pair("search at ip + 4 + 256 = matchlimit + 1", "search at ip + 4 + 256 = matchlimit", "AfterCombined")
    f.pair("search at ip + 4 + 256 = matchlimit", "search at ip + 4 + 256 = matchlimit + 1", "AfterGuarded")
    f.pair("catch-up of 0", "catch-up of 1", "Back1To63")
    return f


# ---- Z: position 0 (64k variant) -----------------------------------------------------------------------------------------------------------
def z_search(equal, shared=False):
    """the block's first `equal` bytes again at lane 20 of the first search: its bucket is empty, "position 0"; shared: another word of
    that bucket at lane 30"""
    def body(b, s):
        assert s == 1
        b.fresh(equal)
        first = bytes(b.b[:equal])
        at = probe(s, 20)
        b.goto(at)
        b.put(first)
        b.fresh(1, avoid=(b.b[equal],))
        if shared:
            A, = b.colliders(1, like=first[:4])
            _put_word(b, probe(s, 30), A)
        _tail(b)
        return _has((at, at, equal))
    return body


def z_test(equal, tail=40):
    """the block's first bytes again directly behind the first match: the test of the next position meets the empty bucket"""
    def body(b, s):
        assert s == 1
        s2, y_at, Y, _, _ = opener(b, s)
        first = bytes(b.b[:equal])
        b.b.pop()
        if first[0] == b.b[s + 1 + Y_LEN]:
            raise Retry("the first byte would extend the match")
        at = b.put(first)
        b.fresh(1, avoid=(b.b[equal],))
        _tail(b, tail)
        return _has((y_at, Y_OFF, Y_LEN), (at, at, equal))
    return body


def family_Z():
    f = Family("Z")
    f.add("search, four bytes", *build(z_search(4), 6000))
    f.add("search, nine bytes", *build(z_search(9), 6001))
    f.add("test-next-position, four bytes", *build(z_test(4), 6002))
    f.add("test-next-position, nine bytes", *build(z_test(9), 6003))
    f.add("search, in a shared bucket", *build(z_search(4, shared=True), 6004))
    f.add("test-next-position, wide", *build(z_test(9, tail=300), 6005))
    f.moves = ["Pos0Search", "Pos0Test", "WinHasHigher", "CandGathered", "TestWide", "TestBytewise"]
    return f


# ---- E: the one-store emit -------------------------------------------------------------------------------------------------------------------
E_LL, E_EXTRA = (0, 1, 13, 14, 15), (0, 1, 14, 15)


def e_case(ll, extra):
    """a source of 24 bytes; Y again (a first match); ll fresh bytes; the source's first 4 + extra bytes again.  ll = 0: the hit of a
    test-next-position; otherwise the search behind it, won at lane ll - 1"""
    def body(b, s):
        src_at, F = _source(b, s, 24)
        b.fresh(2)
        Y = b.word() + _b(b.rng.permutation(200)[:2] + 1)
        y_at = b.put(Y)
        b.fresh(5)
        b.fresh(1, avoid=(b.b[y_at - 1],))
        at = b.put(Y)
        if ll:
            b.fresh(1, avoid=(b.b[y_at + Y_LEN],))
            b.goto(at + Y_LEN + ll, avoid_last=(b.b[src_at - 1],))
            if ll == 1 and (b.b[-1] == b.b[src_at - 1] or b.b[-1] == b.b[y_at + Y_LEN]):
                raise Retry("the one literal")
        elif F[0] == b.b[y_at + Y_LEN]:
            raise Retry("the source would extend the match")
        t = b.put(F[:4 + extra])
        b.fresh(1, avoid=(F[4 + extra],))
        _tail(b, max(5, 8 - extra))                                        # (as near the end as a match may start: the capacity sweep reaches the sequence)
        return _exactly(at, [(at, at - y_at, Y_LEN), (t, t - src_at, 4 + extra)])
    return body


def family_E():
    f = Family("E")
    for ll in E_LL:
        for extra in E_EXTRA:
            f.add(f"ll={ll} extra={extra}", *build(e_case(ll, extra), 7000 + 16 * ll + extra))
    f.moves = ["EmitOne", "EmitGeneral", "TestHit", "StepMatchAllv"]
    f.pair("ll=15 extra=0", "ll=14 extra=0", "EmitOne")
    f.pair("ll=14 extra=15", "ll=14 extra=14", "EmitOne")
    f.pair("ll=14 extra=14", "ll=15 extra=14", "EmitGeneral")
    f.pair("ll=0 extra=14", "ll=0 extra=15", "EmitGeneral")
    return f


def limited_cases(oracle, cases):
    """family D's sweep for family E: [(name, block, cap, oracle's return value, oracle's bytes)] at every capacity from 12 below to 4 above"""
    out = []
    for name, block, want, _ in cases:
        for delta in CAP_DELTAS:
            cap = len(want) + delta
            out.append((f"{name} cap={delta:+d}", block, cap, oracle.compress_raw(block, cap)[0], want))
    assert {r > 0 for _, _, _, r, _ in out} == {False, True}
    return out


# ---- H: the hand-over rule ---------------------------------------------------------------------------------------------------------------
def h_case(ends):
    """sequences of one match each, 16 per entry of `ends`: the 16th match of group g ends at ends[g] (the rule compares that position
    with the last check's)"""
    def body(b, s):
        src_at, F = _source(b, s, 56)
        ms, behind = [], ()
        first = next(probe(s, i) for i in range(60, 200) if probe(s, i) >= b.pos + 3)   # the first copy stands at a probe: no catch-up
        for end in ends:
            # 16 matches of 8 bytes that end at `end`, the literal runs between them as equal as they come; every piece of the source
            # starts at a place of its own, so its first word is in the table once, where the first search put it
            room = end - (first if not ms else b.pos) - 16 * 8
            assert room >= 16 * 3, room
            for k in range(16):
                gap = room // 16 + (1 if k < room % 16 else 0) + (first - b.pos if not ms else 0)
                start = 1 + 7 * len(ms) % 45
                b.fresh(1, avoid=behind)
                b.fresh(gap - 2)
                b.fresh(1, avoid=(F[start - 1],))
                at = b.put(F[start:start + 8])
                behind = (F[start + 8],)
                ms.append((at, at - (src_at + start), 8))
            assert b.pos == end, (b.pos, end)
        b.fresh(1, avoid=behind)
        b.fresh(60)
        return _exactly(s, ms)
    return body


def family_H():
    f = Family("H")
    f.add("16th sequence at 1023", *build(h_case([1023]), 8000, wide=True))
    f.add("16th sequence at 1024", *build(h_case([1024]), 8001, wide=True))
    f.add("32nd sequence at 1023 behind the check", *build(h_case([1100, 1100 + 1023]), 8002, wide=True))
    f.add("32nd sequence at 1024 behind the check", *build(h_case([1100, 1100 + 1024]), 8003, wide=True))
    f.handed_over = [True, False, True, False]
    f.moves = ["Deferred", "DeferPassed"]
    f.pair("16th sequence at 1024", "16th sequence at 1023", "Deferred")
    f.pair("16th sequence at 1023", "16th sequence at 1024", "DeferPassed")
    f.pair("32nd sequence at 1024 behind the check", "32nd sequence at 1023 behind the check", "Deferred")
    f.pair("32nd sequence at 1023 behind the check", "32nd sequence at 1024 behind the check", "DeferPassed")
    return f


# ---- the sets ----------------------------------------------------------------------------------------------------------------------------
BUILDERS = {"S": family_S, "X": family_X, "F": family_F, "W": family_W, "C": family_C, "Z": family_Z, "E": family_E, "H": family_H}
NAMES = tuple(BUILDERS)
DESCENDING = ("S", "X", "Z")           # the families that also run with the emulator's lanes in descending order
DICT = ("S", "Z")                      # ... and through the dictionary encoder
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
    return [c for name in NAMES for c in checked(oracle, name)]


# what the capacity sweep of family E must reach, and what the generic blocks of S and X must reach in the generic variant's steps
LIMITED_MOVES = ("EmitOneRefused", "EmitOne", "EmitGeneral")
GENERIC_MOVES = ("Bucket2", "Bucket3", "Bucket4", "Rounds2", "CandLower", "WinHasHigher", "RestoreLiveKept", "BucketSplitByWinner", "StepOutMasked",
                 "StepMatchMasked", "WinStep3")


# ---- the dictionary encoder (families S and Z) ------------------------------------------------------------------------------------------
DICT_KINDS = ("disjoint", "shared-buckets")


def dict_cases(oracle, name):
    """the family's blocks of the 64k variant's size (the dictionary encoder has one variant)"""
    return [c for c in checked(oracle, name) if len(c[1]) < LIMIT_64K]


def _words(a):
    a = np.asarray(a, np.uint8).astype(np.uint64)
    return a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)


def dictionary(kind, blocks):
    """disjoint: 600 bytes that share no four bytes with any of the blocks.  shared-buckets: zeros, and for every bucket of the generic
    hash that two positions of a block share -- with two words or with one -- a word of that bucket which no block holds (the blocks
    hold no zero byte, so nothing of this dictionary matches): the primed table's entry of such a bucket points into the dictionary.
    (The bucket of a block's first word is the exception: the generic variant inserts the block's first position there.)"""
    have = set(int(w) for b in blocks for w in _words(b))
    rng = np.random.default_rng(9100)
    if kind == "disjoint":
        while True:
            d = rng.integers(1, 256, 600).astype(np.uint8)
            if not have & set(int(w) for w in _words(d)):
                return d
    parts = [np.zeros(64, np.uint8)]
    taken = set()
    for b in blocks:
        w = _words(b)
        h = bucket(w, generic=True)
        hs, counts = np.unique(h, return_counts=True)
        for target in hs[counts >= 2]:
            if int(target) in taken:
                continue
            taken.add(int(target))
            while True:
                c = rng.integers(1, 256, (1 << 16, 4)).astype(np.uint64)
                cw = c[:, 0] | c[:, 1] << np.uint64(8) | c[:, 2] << np.uint64(16) | c[:, 3] << np.uint64(24)
                hit = [int(x) for x in cw[bucket(cw, generic=True) == target] if int(x) not in have]
                if hit:
                    x = hit[0]
                    parts += [np.array([x & 255, x >> 8 & 255, x >> 16 & 255, x >> 24], np.uint8), np.zeros(5, np.uint8)]
                    break
    assert taken
    return np.concatenate(parts)


def check_dict(encode, cases, want, what):
    """encode(blocks) -> (results, rows); want: [(result, bytes)] of the twin: result, bytes, guard bytes behind the bound"""
    res, dst = encode([c[1] for c in cases])
    for i, ((name, block, *_), (wr, wb)) in enumerate(zip(cases, want)):
        assert int(res[i]) == wr, (what, name, int(res[i]), wr)
        assert bytes(dst[i, :wr]) == wb, (what, name)
        assert (dst[i, max(wr, 0):] == 0xA5).all(), (what, name, "wrote past the result")


def assert_moves(f, st, slots=S):
    """slots: slot name -> index, of the kernel the counters st are of"""
    for slot in f.moves:
        assert st[slots[slot]] > 0, (f.name, "counter never moved", slot)


def assert_pairs(f, alone, slots=S):
    """alone: case index -> counters of that case encoded alone"""
    for a, b, slot in f.pairs:
        x, y = alone[a][slots[slot]], alone[b][slots[slot]]
        assert x < y, (f.name, "pair not in the declared direction", f.cases[a][0], f.cases[b][0], slot, x, y)
