"""TEST INFRASTRUCTURE for tests/test_simt_wave_decode_cases.py and tests/test_gpu_wave_decode_cases.py, which are one design: LZ4 blocks
BUILT sequence by sequence (lane_flush_cases.emit) so that the wavefront decoder (lz4hip_decode.hpp, one wavefront per block) meets both
sides of every threshold of its paths -- bursts, the five-byte short path, the general path and its three source kinds, long copies by
distance doubling with their register fill, the 512-byte register window, the LDS mirror and its ring_from floor -- and the comparison
with the CPU codec.  Every valid block is asserted against both CPU decoders before a kernel sees it; damaged ones expect the CPU codec's
result code.  Every block decodes to at most 12 KiB.

A family is a list of (stream, expected bytes or None, output size) plus what the emulator's counters (LZ4HIP_STAT, slots 20 .. 34) must
show for it: the slots that must move, and pairs (a, b, slot, known) of items on the two sides of one threshold, for which the slot's
count of item a alone must be BELOW that of item b alone."""
import numpy as np

from lane_flush_cases import TAIL, emit

RING = 4096                  # kWaveRingBytes
SHORT_MAX = 2 + 18           # the short path's longest sequence: RING - SHORT_MAX is kWaveRingShortServed
WINDOW = 512                 # SrcWindow: [base, base + 512)
EXTRA = 5                    # spare capacity of the unknown-size decodes (a family may bring its own)
MAX_OUT = 12 * 1024
HOLE = 0xA5                  # what every output buffer is filled with: the bytes an offset-0 match "copies"; no built byte has this value

# LZ4HIP_STAT (20 .. 25) and LZ4HIP_STAT_PATH (26 .. 34) slots of lz4hip_decode.hpp
BURSTS, BURST_SEQS, BURST_ROUNDS, BURST_FAILED, SHORT, GENERAL = 20, 21, 22, 23, 24, 25
SHORT_MIRROR, SHORT_MEMORY, GEN_LIT, GEN_MIRROR, GEN_MEMORY, LONG, FILL, REBASE, BURST_BEHIND = 26, 27, 28, 29, 30, 31, 32, 33, 34
N_SLOTS = 40


class Family:
    def __init__(self, extra=EXTRA):
        self.items, self.moves, self.pairs, self.extra, self.edges = [], [], [], extra, []
        self.moves_unknown = []      # slots that only the unknown-size decodes of the family move
        self.valid_for = {}          # item -> the one decoder kind (known?) that accepts it; the other's expectation is the CPU codec's code
        # item -> (built bytes, how many of them precede the cut) of a cut stream whose known-size decode is given the stream's OWN length: the
        # kernel never reads past it and refuses at the cut, the CPU codec has no such argument and refuses further on (the one deliberate
        # difference, lz4hip_decode.hpp), so what is compared is that both refuse, and the bytes in front of the cut
        self.exact_len = {}

    def add(self, seqs, tail, edge=None, min_tail=TAIL, garbage=0):
        """a valid block; edge: index of the sequence the family is about (where its damaged copies are cut); returns the item's index"""
        c, raw = emit(seqs, tail, min_tail)
        if garbage:
            c = np.concatenate([c, np.full(garbage, 0x11, np.uint8)])
        self.items.append((c, raw, raw.size))
        if garbage:
            self.valid_for[len(self.items) - 1] = True
        elif len(tail) < TAIL:
            self.valid_for[len(self.items) - 1] = False
        if edge is not None:
            self.edges.append((len(self.items) - 1, _pos(seqs, edge), _pos(seqs, edge) + 1 + _nlen(len(seqs[edge][0])) + len(seqs[edge][0])))
        return len(self.items) - 1

    def add_corrupt(self, seqs, tail, zero_offset_of):
        """the block with the offset of one sequence set to 0: the oracle says what it decodes to"""
        c, raw = emit(seqs, tail)
        at = _pos(seqs, zero_offset_of) + 1 + _nlen(len(seqs[zero_offset_of][0])) + len(seqs[zero_offset_of][0])
        c[at] = c[at + 1] = 0
        self.items.append((c, None, raw.size))
        return len(self.items) - 1

    def pair(self, a, b, slot, known=True):
        self.pairs.append((a, b, slot, known))

    def damage(self):
        """two blocks cut or corrupted at the family's own edge: cut inside the edge sequence, cut behind its offset, its offset reaching
        before the block, its token changed"""
        edges = self.edges[:1] + self.edges[-1:] if self.edges else []
        for j, (i, tok, off_at) in enumerate(edges):
            c, raw, cap = self.items[i]
            for k in (2 * j, 2 * j + 1):
                d = c.copy()
                if k == 0:
                    d = d[:tok + 2]
                elif k == 1:
                    d = d[:off_at + 2]
                elif k == 2:
                    d[off_at:off_at + 2] = 255                 # 65 535 back: no block here is that long
                else:
                    d[tok] ^= 0x5F
                self.items.append((d, None, cap))
        return self


def _rb(rng, n):
    return bytes(rng.integers(1, HOLE, n, dtype=np.uint8))


def _nlen(n):
    """length bytes behind a nibble for the value n"""
    return 0 if n < 15 else 1 + (n - 15) // 255


def _seq_in(ll, ml):
    return 1 + _nlen(ll) + ll + 2 + _nlen(ml - 4)


def _pos(seqs, k):
    """where sequence k's token is in the stream"""
    return sum(_seq_in(len(lit), ml) for lit, _, ml in seqs[:k])


def _out(seqs):
    return sum(len(lit) + ml for lit, _, ml in seqs)


def _bytes_of(seqs):
    return emit(seqs, b"\x01" * TAIL)[1][:_out(seqs)]


def short_run(rng, n, pos, off=None):
    """sequences that a burst takes (4 literals, a near match of 4), together exactly n bytes (0 or >= 8) behind `pos` existing ones"""
    seqs, left = [], n
    assert n == 0 or n >= 8
    while left:
        ll = 4 if left >= 16 else left - 4
        seqs.append((_rb(rng, ll), int(rng.integers(1, min(pos + ll, 40) + 1)) if off is None else off, 4))
        pos += ll + 4
        left -= ll + 4
    return seqs


def other(rng):
    """a sequence no burst takes (15 literals: a length byte) and the short path neither: 19 bytes through the general path"""
    return (_rb(rng, 15), int(rng.integers(1, 9)), 4)


def isolated(rng, pre):
    """`pre` bytes of short sequences, then two sequences for the general path: a burst ends at the first (burst_skip = 1), the next attempt
    fails at the second (tok_m == 0, burst_skip = 1), so the sequence BEHIND them is decoded with the burst skipped: by the short path if
    it qualifies, else by the general path"""
    return short_run(rng, pre, 0) + [other(rng), other(rng)]


# ---- the mirror's old edge -------------------------------------------------------------------------------------------------------------
PLACEMENTS = ("first", "inside", "skip", "end")
MIRROR_LL = (0, 1, 2, 3, 14, 40)


def _mirror_seqs(rng, ll, x, ml, placement, pre):
    """(sequences, tail, index of S): S = ll literals, a match of ml whose first source byte is output byte op - RING + x (op: S's first
    output byte), i.e. offset RING + ll - x.  For 0 <= x < ll that byte shares its mirror slot with S's own literal x; the literals are
    chosen to differ from the bytes whose slots they take."""
    head = short_run(rng, pre, 0)
    if placement == "first":                                  # behind a sequence that ends a burst: S starts the next one
        head.append(other(rng))
    elif placement == "inside":                               # ... one short sequence further in (where S does not fit behind it, S starts the burst after)
        head += [other(rng)] + short_run(rng, 8, pre)
    elif placement == "skip":
        head += [other(rng), other(rng)]
    op = _out(head)
    old = _bytes_of(head)[op - RING:op - RING + ll]
    lit = bytes((int(b) % (HOLE - 1)) + 1 if (int(b) % (HOLE - 1)) + 1 != int(b) else 7 for b in old)
    assert len(lit) == ll and all(a != b for a, b in zip(lit, old))
    seqs = head + [(lit, RING + ll - x, ml)]
    if placement == "end":                                    # S's first byte at oend - 95: past o_burst, inside o_safe
        return seqs, _rb(rng, 95 - ll - ml), len(head)
    return seqs + short_run(rng, 128, op + ll + ml), _rb(rng, TAIL), len(head)


def mirror_edge():
    f = Family()
    f.moves = [BURSTS, BURST_BEHIND, SHORT_MIRROR, SHORT_MEMORY, GEN_MIRROR, GEN_MEMORY]
    n = 0
    for ll in MIRROR_LL:
        for x in range(-2, ll + 2):
            for ml in (4, 18, 19, 64 - ll):
                rng = np.random.default_rng(7000 + n)
                seqs, tail, k = _mirror_seqs(rng, ll, x, ml, PLACEMENTS[(n + n // 4) % 4], 4100 + n % 9)     # (every ml meets every placement)
                f.add(seqs, tail, edge=k)
                n += 1
    # the short path itself (at most 2 literals, a match of at most 18) at every x, where no burst takes the sequence first
    for ll in (0, 1, 2):
        for x in range(-2, ll + 2):
            for ml in (4, 12, 18):
                for placement in ("skip", "end"):
                    rng = np.random.default_rng(7000 + n)
                    seqs, tail, k = _mirror_seqs(rng, ll, x, ml, placement, 4100 + n % 9)
                    f.add(seqs, tail, edge=k)
                    n += 1
    # both sides of what the one-sequence paths serve from the mirror: the bytes it still holds after the step -- for the general path
    # from op + ll + ml - RING on (first source byte one before that: one lane from memory; at it; one behind it), for the short path from
    # op + SHORT_MAX - RING on whatever the sequence's length (one byte before that: the match comes from memory)
    at = {}
    for ll in MIRROR_LL:
        for ml in (4, 64 - ll):
            for placement in ("skip", "end"):
                for x in sorted({ll + ml - 1, ll + ml, ll + ml + 1, SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1}):
                    rng = np.random.default_rng(7900 + 10 * ll + ml)     # (the three differ in S's offset alone)
                    seqs, tail, k = _mirror_seqs(rng, ll, x, ml, placement, 4100)
                    at[ll, ml, placement, x] = f.add(seqs, tail, edge=k)
                    n += 1
    for known in (True, False):
        for placement in ("skip", "end"):
            f.pair(at[1, 4, placement, SHORT_MAX - 1], at[1, 4, placement, SHORT_MAX], SHORT_MIRROR, known)
            f.pair(at[1, 4, placement, SHORT_MAX], at[1, 4, placement, SHORT_MAX - 1], SHORT_MEMORY, known)
            f.pair(at[2, 62, placement, 64], at[2, 62, placement, 63], GEN_MEMORY, known)
            f.pair(at[14, 50, placement, 64], at[14, 50, placement, 63], GEN_MEMORY, known)
            f.pair(at[40, 24, placement, 63], at[40, 24, placement, 64], GEN_MIRROR, known)
    return f.damage()


# ---- ring_from ---------------------------------------------------------------------------------------------------------------------------
def _followers(rng, seqs, E, first):
    """twelve short sequences behind match_end E (2 literals, a match of 6) whose sources start at E - 1, E, E + 1 and E + 64 in turn"""
    targets = (E - 1, E, E + 1, E + 64)
    op = E
    for i in range(12):
        t = targets[(first + i) % 4]
        if t >= op + 2:                                       # not written yet
            t = E - 1
        seqs.append((_rb(rng, 2), op + 2 - t, 6))
        op += 8
    return seqs


def _stale_shows(out, E):
    """every byte the followers read or write, E - 8 .. E + 96, differs from the byte 4 096 before it: whatever a follower took from a
    mirror slot that was not rewritten would be a wrong byte"""
    return all(out[b] != out[b - RING] for b in range(E - 8, E + 96))


def ring_from():
    f = Family()
    f.moves = [LONG, BURST_BEHIND, SHORT_MEMORY, GEN_LIT]
    at = {}
    for ml in (64, 65, 100, 700):                            # ll + ml <= 64: the general path's one store, the mirror stays whole
        for first in range(4):
            pre, E = 4200 + first, 4200 + first + ml
            for seed in range(8000 + ml * 4 + first, 1 << 30, 5000):         # (the first seed with which a stale mirror shows)
                rng = np.random.default_rng(seed)
                seqs = short_run(rng, pre, 0) + [(b"", 37, ml)]
                k = len(seqs) - 1
                seqs = _followers(rng, seqs, E, first)
                if _stale_shows(_bytes_of(seqs), E):
                    break
            at[ml, first] = f.add(seqs + short_run(rng, 128, E + 96), _rb(rng, TAIL), edge=k)
    for first in range(4):                                   # an offset-0 hole: a short sequence by its lengths, decoded by the long path
        for ml in (6, 20, 70):
            pre, E = 4200 + first, 4200 + first + 2 + ml
            for seed in range(8500 + ml * 4 + first, 1 << 30, 5000):
                rng = np.random.default_rng(seed)
                seqs = short_run(rng, pre, 0) + [(_rb(rng, 2), 9, ml)]
                k = len(seqs) - 1
                seqs = _followers(rng, seqs, E, first) + short_run(rng, 128, E + 96)
                i = f.add_corrupt(seqs, _rb(rng, TAIL), k)
                c, _, cap = f.items[i]
                if _stale_shows(replay(c, np.full(cap, HOLE, np.uint8), cap), E):
                    break
                f.items.pop()
    for known in (True, False):
        f.pair(at[64, 0], at[65, 0], LONG, known)
        f.pair(at[64, 0], at[65, 0], BURST_BEHIND, known)
        f.pair(at[64, 0], at[65, 0], SHORT_MEMORY, known)
    return f.damage()


# ---- burst eligibility and size --------------------------------------------------------------------------------------------------------
def _burst_block(rng, middle, pre=40):
    """short sequences, a sequence that ends their burst, `middle` (the next burst attempt starts at its first sequence), the same again"""
    head = short_run(rng, pre, 0) + [other(rng)]
    seqs = head + middle(_out(head))
    return seqs + [other(rng)] + short_run(rng, 160, _out(seqs) + 19), len(head)


def bursts():
    f = Family()
    f.moves = [BURSTS, BURST_SEQS, BURST_ROUNDS, BURST_FAILED, GENERAL]
    rng = np.random.default_rng(9000)
    at = {}

    def one(key, middle, corrupt=None):
        seqs, k = _burst_block(rng, middle)
        if corrupt is None:
            at[key] = f.add(seqs, _rb(rng, TAIL), edge=k)
        else:
            at[key] = f.add_corrupt(seqs, _rb(rng, TAIL), k + corrupt)

    # `simple`: ll <= 14, and a match code of 15 only with ll <= 13 and an extension byte below 255
    for ll in (13, 14, 15):
        for ml in (18, 19, 19 + 254, 19 + 255):              # match code 14; 15 with extension byte 0, 254, 255 (and a second one)
            one(("elig", ll, ml), lambda pos: [(_rb(rng, ll), 5, ml)] + short_run(rng, 24, pos + ll + ml))
    # (an extension byte of 254 or 255 makes a sequence too long for any burst; what differs is how the burst in front of it ends: at
    #  a sequence it could take but for its length, so that the next attempt starts there and fails, or at one it leaves to the general path)
    for ml in (19 + 254, 19 + 255):
        one(("elig2", ml), lambda pos: short_run(rng, 8, pos) + [(_rb(rng, 13), 5, ml)] + short_run(rng, 24, pos + 21 + ml, off=4))
    one(("elig", "offset0"), lambda pos: [(_rb(rng, 3), 5, 6)] + short_run(rng, 24, pos + 9), corrupt=0)
    for known in (True, False):
        f.pair(at["elig", 14, 18], at["elig", 15, 18], GENERAL, known)
        f.pair(at["elig2", 19 + 255], at["elig2", 19 + 254], BURST_FAILED, known)
        f.pair(at["elig", 13, 19], at["elig", 14, 19], GENERAL, known)
        f.pair(at["elig", 15, 18], at["elig", 14, 18], BURST_SEQS, known)
    # a burst's output: 63, 64 and 65 bytes of sequences between two that end a burst -- 64 are one burst, 65 are two
    for total in (63, 64, 65):
        one(("tot4", total), lambda pos: [(b"", 3, 4)] * (15 if total > 63 else 14) + [(_rb(rng, total - 60 - 4 if total > 63 else 3), 3, 4)])
        one(("tot18", total), lambda pos: [(b"", 7, 18)] * 3 + [(b"", 7, total - 54)])
    for known in (True, False):
        for kind in ("tot4", "tot18"):
            f.pair(at[kind, 64], at[kind, 65], BURSTS, known)
            f.pair(at[kind, 63], at[kind, 65], BURSTS, known)
    # a first sequence the burst could take but for its length (tok_m == 0): 13 literals and 19 + 100 bytes of match
    one(("first", 132), lambda pos: [(_rb(rng, 13), 5, 119)] + short_run(rng, 24, pos + 132))
    one(("first", 64), lambda pos: [(_rb(rng, 13), 5, 51)] + short_run(rng, 24, pos + 64))
    for known in (True, False):
        f.pair(at["first", 64], at["first", 132], BURST_FAILED, known)
    # burst_fail: a block that BEGINS with r sequences no burst takes meets a failing attempt at sequence 0, 2, 5, 10, 19 and, the
    # backoff having reached its ceiling of 16, at 36: r = 36 fails five times, r = 37 six times; short sequences follow and recover
    for r in (1, 2, 3, 5, 6, 10, 11, 19, 20, 36, 37, 60):
        seqs = [other(rng) for _ in range(r)]
        at["backoff", r] = f.add(seqs + short_run(rng, 400, 19 * r), _rb(rng, TAIL), edge=r - 1)
    for known in (True, False):
        for r in (2, 5, 10, 19, 36):
            f.pair(at["backoff", r], at["backoff", r + 1], BURST_FAILED, known)
    # sources inside the burst: offset 1 (one round per byte), the previous sequence of the burst, this sequence's own literals
    one(("src", "chain"), lambda pos: [(_rb(rng, 1), 1, 59)])
    one(("src", "previous"), lambda pos: [(_rb(rng, 6), 3, 4), (_rb(rng, 2), 9, 12), (_rb(rng, 1), 13, 18)])
    one(("src", "literals"), lambda pos: [(_rb(rng, 9), 6, 18), (_rb(rng, 14), 14, 5)])
    for known in (True, False):
        f.pair(at["src", "previous"], at["src", "chain"], BURST_ROUNDS, known)
    return f.damage()


# ---- the short path ----------------------------------------------------------------------------------------------------------------------
def short_path():
    f = Family()
    f.moves = [SHORT, SHORT_MIRROR, GENERAL, BURSTS]
    rng = np.random.default_rng(9100)
    at = {}
    # t_off == t_ml + tll is the nearest source the short path takes; one less overlaps the match
    for tll in (0, 1, 2):
        for ml in (4, 18):
            for less in (0, 1):
                seqs = isolated(rng, 200)
                seqs.append((_rb(rng, tll), ml + tll - less, ml))
                at["off", tll, ml, less] = f.add(seqs + short_run(rng, 128, _out(seqs)), _rb(rng, TAIL), edge=len(seqs) - 1)
            f.pair(at["off", tll, ml, 1], at["off", tll, ml, 0], SHORT)
            f.pair(at["off", tll, ml, 1], at["off", tll, ml, 0], SHORT, False)
    # op at o_safe = oend - 28 (known) / oend - 32 (unknown, oend = size + EXTRA) and one past it: S = 2 literals + 4 at size - d, no
    # burst that late (o_burst = oend - 96)
    for d in (26, 27, 28, 29):
        seqs = short_run(rng, 200 - d, 0)
        seqs.append((_rb(rng, 2), 11, 4))
        at["o_safe", d] = f.add(seqs, _rb(rng, d - 6), edge=len(seqs) - 1)
    f.pair(at["o_safe", 27], at["o_safe", 28], SHORT, True)
    f.pair(at["o_safe", 32 - EXTRA - 1], at["o_safe", 32 - EXTRA], SHORT, False)
    # o_burst = oend - 96: bytes the known-size decoder never reads behind the block keep ip <= i_burst, so that op decides
    for d in (95, 96, 97, 95 - EXTRA, 96 - EXTRA):
        seqs = short_run(rng, 200, 0) + [other(rng)]          # the sequence behind `other` starts a burst attempt at op = size - d
        k = len(seqs)
        seqs += short_run(rng, 48, 219)
        at["o_burst", d] = f.add(seqs, _rb(rng, d - 48), edge=k, garbage=64)
    f.pair(at["o_burst", 95], at["o_burst", 96], BURSTS, True)
    f.pair(at["o_burst", 95 - EXTRA], at["o_burst", 96 - EXTRA], BURSTS, False)
    return f, at, rng


def _finish_short(f, at, rng):
    # ip at i_safe = iend - 5 (known): only a stream cut short gets there -- five and four bytes from the token of a one-literal sequence
    # on (that sequence is whole in both: token, literal, offset)
    for cut in (5, 4):
        seqs = isolated(rng, 100)
        seqs.append((_rb(rng, 1), 30, 6))
        k = len(seqs) - 1
        c, raw = emit(seqs + short_run(rng, 64, _out(seqs)), _rb(rng, TAIL))
        f.items.append((c[:_pos(seqs, k) + cut].copy(), None, raw.size))
        at["i_safe", cut] = len(f.items) - 1
        f.exact_len[len(f.items) - 1] = (raw, _out(seqs))
    f.pair(at["i_safe", 4], at["i_safe", 5], SHORT, True)
    return f.damage()


def short_input_edges():
    """the unknown-size decoder's i_safe = iend - 11 and both decoders' i_burst = iend - 112, with spare capacity enough that the output
    side never decides"""
    f = Family(extra=120)
    f.moves, f.moves_unknown = [GENERAL, BURSTS], [SHORT]
    rng = np.random.default_rng(9200)
    at = {}
    # token at iend - 11: two literals, offset, then the last sequence's token and five literals; at iend - 10: one literal
    for tll in (2, 1):
        seqs = isolated(rng, 100)
        seqs.append((_rb(rng, tll), 30, 6))
        at["i_safe", tll] = f.add(seqs, _rb(rng, 5), min_tail=5)      # (five last literals: only the unknown-size decoder accepts the block)
    f.pair(at["i_safe", 1], at["i_safe", 2], SHORT, False)
    # a burst attempt with exactly 112 and 111 bytes of input left: thirty sequences of 3 bytes and a last run of 20 / 19 literals
    for tail in (20, 19, 21):
        seqs = short_run(rng, 100, 0) + [other(rng)]
        k = len(seqs)
        seqs += [(b"", 7, 10)] * 30
        at["i_burst", tail] = f.add(seqs, _rb(rng, tail), edge=k)
    for known in (True, False):
        f.pair(at["i_burst", 19], at["i_burst", 20], BURSTS, known)
    return f.damage()


# ---- the general path --------------------------------------------------------------------------------------------------------------------
def general_path():
    f = Family()
    f.moves = [GENERAL, GEN_LIT, GEN_MIRROR, GEN_MEMORY, LONG]
    rng = np.random.default_rng(9300)
    at = {}

    def one(key, s, pre=300):
        seqs = isolated(rng, pre)
        seqs.append(s(_out(seqs)) if callable(s) else s)
        at[key] = f.add(seqs + short_run(rng, 128, _out(seqs)), _rb(rng, TAIL), edge=len(seqs) - 1)

    for ll in (63, 64, 65):                                   # short_lit: literals out of the register window up to 64
        one(("ll", ll), (_rb(rng, ll), 21, 4))
    for ll, ml in ((0, 64), (0, 65), (20, 44), (20, 45), (60, 4), (61, 4)):       # ll + ml <= 64: one store; else the long path
        one(("sum", ll, ml), (_rb(rng, ll), 90, ml))
    for known in (True, False):
        f.pair(at["sum", 0, 64], at["sum", 0, 65], LONG, known)
        f.pair(at["sum", 20, 44], at["sum", 20, 45], LONG, known)
        f.pair(at["sum", 60, 4], at["sum", 61, 4], LONG, known)
        f.pair(at["sum", 20, 45], at["sum", 20, 44], GEN_MIRROR, known)
    for off in range(1, 18):                                  # off < ml: the modulo on the lane index
        one(("overlap", off), (_rb(rng, off % 3), off, 18))
        one(("overlap64", off), (b"", off, 64))
    for ll, off in ((5, 3), (5, 5), (5, 6), (30, 1), (30, 29), (14, 7)):          # the source inside this sequence's literals (and one byte before them)
        one(("own", ll, off), (_rb(rng, ll), off, 20))
    for known in (True, False):
        f.pair(at["own", 5, 6], at["own", 5, 5], GEN_LIT, known)
    # per-lane mixes: a match of 30 that starts d bytes before the end E of a long match: d lanes from memory, the others from the mirror
    for d in (0, 1, 5, 29, 30):
        seqs = isolated(rng, 300)
        seqs.append((b"", 50, 80))
        E = _out(seqs)
        seqs += short_run(rng, 16, E, off=4)                 # (their sources are their own literals)
        seqs.append((_rb(rng, 3), 16 + 3 + d, 30))
        at["mix", d] = f.add(seqs + short_run(rng, 128, _out(seqs)), _rb(rng, TAIL), edge=len(seqs) - 1)
    for known in (True, False):
        f.pair(at["mix", 0], at["mix", 1], GEN_MEMORY, known)
        f.pair(at["mix", 30], at["mix", 29], GEN_MIRROR, known)
    for ll in (255, 256, 257, 600, 14 + 255, 15 + 255, 15 + 2 * 255):             # length bytes of 255 and the run sizes around them
        one(("run", ll), (_rb(rng, ll), 100, 9))
    return f.damage()


# ---- the register window -----------------------------------------------------------------------------------------------------------------
def window():
    """one sequence -- token, a length byte, 64 literals, the offset pair, a match-length byte -- whose token lies at stream position T
    behind a leading literal run of chosen length: each of its parts ends 0, 1 and 2 bytes past base + 512 for some T, and the offset's two
    bytes fall on either side of the re-base"""
    f = Family()
    f.moves = [REBASE, GENERAL]
    at = {}
    for T in list(range(WINDOW - 72, WINDOW + 3)) + list(range(WINDOW + 256 - 72, WINDOW + 256 + 3, 3)):
        rng = np.random.default_rng(9400 + T)
        L0 = next(n for n in range(15, T) if 1 + _nlen(n) + n + 2 == T)
        seqs = [(_rb(rng, L0), 11, 4), (_rb(rng, 64), 77, 19 + 33)]
        assert _pos(seqs, 1) == T
        at[T] = f.add(seqs + short_run(rng, 64, _out(seqs)), _rb(rng, TAIL), edge=1)
    # a stream that ends inside the first window never re-bases
    rng = np.random.default_rng(9399)
    small = f.add([(_rb(rng, 200), 11, 4)] + short_run(rng, 64, 204), _rb(rng, TAIL), edge=0)
    for known in (True, False):
        f.pair(small, at[WINDOW], REBASE, known)
    return f.damage()


# ---- long copies -------------------------------------------------------------------------------------------------------------------------
LONG_OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 2048, 3000)
LONG_LENGTHS = (65, 1023, 1024, 1025, 2047, 2048, 2049, 3077, 5000)


def long_copies():
    f = Family()
    f.moves = [LONG, FILL]
    at = {}
    for off in LONG_OFFSETS:
        for ml in LONG_LENGTHS:
            rng = np.random.default_rng(9500 + off * 7 + ml)
            seqs = [(_rb(rng, off + 3), off, ml)]
            at[off, ml] = f.add(seqs + short_run(rng, 16, off + 3 + ml), _rb(rng, TAIL), edge=0)
    for known in (True, False):                               # the register fill: the distance has doubled to exactly 1 KiB and 1 KiB is left
        f.pair(at[1024, 2047], at[1024, 2048], FILL, known)
        f.pair(at[1025, 5000], at[1024, 5000], FILL, known)
        f.pair(at[3, 5000], at[4, 5000], FILL, known)
    return f.damage()


def _short_path_family():
    return _finish_short(*short_path())


BUILDERS = {"mirror_edge": mirror_edge, "ring_from": ring_from, "bursts": bursts, "short_path": _short_path_family,
            "short_input_edges": short_input_edges, "general_path": general_path, "window": window, "long_copies": long_copies}
NAMES = tuple(BUILDERS)
_families, _expected = {}, {}


def family(name):
    if name not in _families:
        f = BUILDERS[name]()
        assert all(cap <= MAX_OUT for _, _, cap in f.items), name
        _families[name] = f
    return _families[name]


def plain(oracle, name):
    """the family's shape with plain encoder output in place of its inputs (what the reach assertions must NOT accept)"""
    f = family(name)
    g = Family(f.extra)
    g.moves, g.moves_unknown, g.pairs = f.moves, f.moves_unknown, f.pairs
    rng = np.random.default_rng(1)
    for c, raw, cap in f.items:
        data = np.repeat(rng.integers(1, HOLE, cap // 8 + 1, dtype=np.uint8), 8)[:cap] if cap >= 64 else rng.integers(1, HOLE, cap, dtype=np.uint8)
        g.items.append((oracle.compress(data), data, cap))
    return g


def expected(oracle, name, known, fam=None):
    """(family, CPU codec's result per block, its bytes per block): computed once per family and decoder kind"""
    key = (name, known, fam is None)
    if fam is not None or key not in _expected:
        f = family(name) if fam is None else fam
        res, outs = [], []
        for c, raw, cap in f.items:
            if known:
                r, o = oracle.uncompress_raw(c, cap)
            else:
                r, o = oracle.uncompress_unknown_raw(c, len(c), cap + f.extra)
            if raw is not None and f.valid_for.get(len(res), known) == known:   # a block built here is a valid one, and decodes to what emit() said
                assert (0 < r <= len(c) if known else r == raw.size) and np.array_equal(o[:raw.size], raw), (name, known, len(res), r)
            res.append(r)
            outs.append(o)
        if fam is not None:
            return f, res, outs
        _expected[key] = (f, res, outs)
    return _expected[key]


def _more(c, n, ip):
    while True:
        n += c[ip]; ip += 1
        if c[ip - 1] != 255:
            return n, ip


def replay(c, row, n):
    """the n bytes a stream the CPU codec accepts decodes to when the output starts out as `row`: the bytes of an offset-0 match are the
    ones that were there"""
    c, out, ip, op = bytes(c), row[:n].copy(), 0, 0
    while True:
        tok = c[ip]; ip += 1
        ll = tok >> 4
        if ll == 15:
            ll, ip = _more(c, ll, ip)
        out[op:op + ll] = np.frombuffer(c[ip:ip + ll], np.uint8)
        ip += ll; op += ll
        if op >= n:
            return out
        off = c[ip] | c[ip + 1] << 8; ip += 2
        ml = tok & 15
        if ml == 15:
            ml, ip = _more(c, ml, ip)
        for k in range(op, op + ml + 4 if off else op):
            out[k] = out[k - off]
        op += ml + 4


def check(oracle, name, known, decode, only=None, fam=None, holes_keep=False):
    """decode(streams, capacities, known, stream lengths) -> (results, rows with 64 guard bytes of 0xA5 behind the capacity); only: indices to decode.
    Bytes are compared wherever the CPU codec succeeds -- a block with an offset-0 hole included: every buffer starts out as HOLE, and
    where the decoder works on a staged copy of the row (holes_keep: the bytes of a hole are whatever that copy held) the row is compared
    with replay() of the stream over itself."""
    f, want, outs = expected(oracle, name, known, fam)
    idx = list(range(len(f.items))) if only is None else list(only)
    # (the known-size codec takes no input length: a damaged stream runs on into the zeros the oracle's wrapper puts behind it, so here too)
    comps = [np.concatenate([f.items[j][0], np.zeros(f.items[j][2] + 1024, np.uint8)]) if known and f.items[j][1] is None else f.items[j][0] for j in idx]
    caps = [f.items[j][2] + (0 if known else f.extra) for j in idx]
    lens = [len(f.items[j][0]) if j in f.exact_len else len(c) for j, c in zip(idx, comps)]
    res, dst = decode(comps, caps, known, lens)
    for i, j in enumerate(idx):
        if known and j in f.exact_len:
            raw, n = f.exact_len[j]
            # (a staged row that was refused is not copied back: there only the refusal is seen)
            assert res[i] < 0 and want[j] < 0 and (holes_keep or np.array_equal(dst[i, :n], raw[:n])), (name, j, int(res[i]), want[j])
            continue
        assert res[i] == want[j], (name, known, j, int(res[i]), want[j])
        if want[j] >= 0:
            n = f.items[j][2] if known else want[j]
            model = replay(f.items[j][0], dst[i], n) if holes_keep and f.items[j][1] is None else outs[j]
            bad = np.flatnonzero(dst[i, :n] != model[:n])
            assert bad.size == 0, (name, known, j, "first wrong byte", int(bad[0]), "of", n)
        assert (dst[i, caps[i]:caps[i] + 64] == 0xA5).all(), (name, known, j, "wrote past the block")
