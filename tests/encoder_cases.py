"""Blocks BUILT for single rules of the encoders (shared by tests/test_simt_encoder_edges.py and tests/test_gpu_encoder_edges.py), and a
parser for what an encoder emitted.  Generator data reaches these rules by luck or not at all (a fast-encoder hash entry never survives
65 535 positions of it); a built block reaches them by construction, and says so: every builder returns (block, expectation), and the
expectation is asserted against the ORACLE's output before any kernel is asked -- a case that misses its target fails there.

Family A  distance limit        P | zeros | J | P at distance d | 40 fresh bytes, d around MAX_DISTANCE = 65 535
Family B  length bytes          literal runs of 14..16 / 269..271 / 524..526 and matches of 18..20 / 273..275 / 528..530 bytes
Family C  end of the block      a copy of the block's first bytes that runs into the last s bytes
Family D  output limit          every capacity from 12 below to 4 above the compressed size, for the B and C blocks with long lengths

All random content comes from np.random.default_rng(fixed seed)."""
import contextlib

import numpy as np

from oracle.oracle import compress_bound

LIMIT_64K = 65547                 # blocks of this size and more take the generic variant of the fast encoder (lz4.c:783)
MAX_DISTANCE = 65535
DISTANCES = (65534, 65535, 65536, 65537)
LITERALS = (14, 15, 16, 269, 270, 271, 524, 525, 526)
MATCHES = (18, 19, 20, 273, 274, 275, 528, 529, 530)
# every L with two M values and every M with two L values
LENGTH_PAIRS = tuple((L, MATCHES[i]) for i, L in enumerate(LITERALS)) + tuple((L, MATCHES[(i + 4) % 9]) for i, L in enumerate(LITERALS))
TAILS = (10, 11, 12, 13, 14, 20)
CAP_DELTAS = tuple(range(-12, 5))


def parse_sequences(comp):
    """[(literals, offset, match_len), ..., (literals, None, None)] of one well-formed LZ4 block."""
    comp = bytes(bytearray(comp))
    seqs, i, n = [], 0, len(comp)
    while True:
        token = comp[i]; i += 1
        lit = token >> 4
        if lit == 15:
            while True:
                b = comp[i]; i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        if i >= n:
            assert i == n, "the last literals run past the block"
            seqs.append((lit, None, None))
            return seqs
        off = comp[i] | (comp[i + 1] << 8); i += 2
        ml = token & 15
        if ml == 15:
            while True:
                b = comp[i]; i += 1
                ml += b
                if b != 255:
                    break
        seqs.append((lit, off, ml + 4))


def placed(seqs):
    """[(match position, literals, offset, match_len)] of the sequences that carry a match."""
    out, pos = [], 0
    for lit, off, ml in seqs:
        pos += lit
        if off is not None:
            out.append((pos, lit, off, ml))
            pos += ml
    return out


def _nonzero(rng, n):
    return rng.integers(1, 256, n).astype(np.uint8)


# ---- family A ------------------------------------------------------------------------------------------------------------------------
def distance_case(d, junk, seed, echo=False):
    """P (24 random bytes 1..255) | zeros | J (`junk` fresh bytes) | P again at distance d | 40 fresh bytes.  The zeros are one long match
    that inserts almost nothing, so P's table entries are still there when its second copy arrives.  J empty: the copy is met right after
    the zero match (lz4.c:538); J of three bytes: in the search loop (lz4.c:427).  LZ4HC finds the first copy as the head of its bucket.
    echo (d <= MAX_DISTANCE only): P[5:9] = P[1:5].  Without it an encoder that refuses the copy at lz4.c:538 finds P[1:] one position later,
    catch-up walks back over P[0], and the bytes are the same; with it the bucket of P[1:5] holds position 5, and such an encoder emits
    another match."""
    rng = np.random.default_rng(seed)
    p = _nonzero(rng, 24)
    if echo:
        p[5:9] = p[1:5]
    block = np.zeros(d + 64, np.uint8)
    block[:24] = p
    block[d - junk:d] = _nonzero(rng, junk)
    block[d:d + 24] = p
    block[d + 24:] = _nonzero(rng, 40)

    def expect(seqs):
        at_d = [(off, ml) for pos, _, off, ml in placed(seqs) if pos + ml > d]
        if d <= MAX_DISTANCE:
            assert at_d == [(d, 24)], (d, junk, seed, at_d)
        else:
            assert at_d == [], (d, junk, seed, at_d)
    return block, expect


HOP_GAP = 300
HOPS = ("hop", "two-hops", "wider", "wider-hop", "collision")


def hash15(word):
    """LZ4HC's bucket of a little-endian 4-byte word (lz4hc.c:245)"""
    return ((np.asarray(word, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(17)


def _colliding_lead(p):
    """Three bytes x y z (1..255, the first found in order) for which the word x y z P[2] falls into the bucket of P[2:6], and the two words
    after it do not."""
    le = lambda b: int(b[0]) | int(b[1]) << 8 | int(b[2]) << 16 | int(b[3]) << 24
    target = int(hash15(le(p[2:6])))
    v = np.arange(1, 256, dtype=np.uint64)
    words = v[:, None, None] | v[None, :, None] << np.uint64(8) | v[None, None, :] << np.uint64(16) | np.uint64(int(p[2]) << 24)
    for x, y, z in np.argwhere(hash15(words) == target) + 1:
        if int(hash15(le([y, z, p[2], p[3]]))) != target and int(hash15(le([z, p[2], p[3], p[4]]))) != target:
            return np.array([x, y, z], np.uint8)
    raise AssertionError("no colliding lead for this P")


def hop_case(d, seed, kind="hop"):
    """LZ4HC, the candidate at distance d reached otherwise than as the head of the first search's bucket.  All: P | zeros | ... | zeros | R at
    position d | 40 fresh bytes, every planted piece behind a fresh non-zero byte (or the zeros before it, with its first bytes, are a longer
    match for the zeros before R).
    hop        Q = P[:4] + 20 other bytes, HOP_GAP before R = P: the head is Q (four bytes), the hop from this MATCHING candidate lands on P.
    two-hops   Q twice, 2 x HOP_GAP and HOP_GAP before R = P: the nearer Q matches, the farther one then FAILS the byte test, the hop from it lands on P.
    wider      S = a b P[2:4] + 20 other bytes, R = a b P[2:]: the first search finds S (four bytes), the search for a wider match two bytes on
               finds P[2:] as the head of ITS bucket, at distance d.
    wider-hop  S = a b P[2:6] + others, T = P[4:8] + others half way, R = a b P[2:]: the first search finds S (six bytes), the wider search four
               bytes on finds T (no gain), and the hop from it lands on P[4:] at distance d.
    collision  R = x y z P[2:], where the word x y z P[2] shares the bucket of P[2:6]: at the search for P[2:6] the head is three positions
               back (the repeat test, lz4hc.c:411-421), its word FAILS, and its link -- to the bucket's previous entry, P[2:6] in the first
               P -- lands at distance d."""
    rng = np.random.default_rng(seed)
    p = _nonzero(rng, 24)
    other = (p.astype(np.int32) % 255 + 1).astype(np.uint8)              # 1..255, never the byte of P at that place
    ab = (p[:2].astype(np.int32) + 7) % 255 + 1
    block = np.zeros(d + 64, np.uint8)
    block[:24] = p

    def plant(at, piece):
        block[at - 1] = _nonzero(rng, 1)[0]
        block[at:at + len(piece)] = piece
    r = p.copy()
    if kind in ("hop", "two-hops"):
        q = np.concatenate([p[:4], other[4:]])
        if kind == "two-hops":
            plant(d - 2 * HOP_GAP, q)
        plant(d - HOP_GAP, q)
        near, found = (HOP_GAP, 4), (d, 24)
    elif kind == "collision":
        block[d - 1:d + 2] = _colliding_lead(p)
        near, found = None, (d, 22)
    else:
        r[:2] = ab
        keep = 4 if kind == "wider" else 6
        plant(d - HOP_GAP, np.concatenate([ab, p[2:keep], other[keep:]]).astype(np.uint8))
        if kind == "wider-hop":
            plant(d - HOP_GAP // 2, np.concatenate([p[4:8], other[8:]]))
        near, found = (HOP_GAP, keep), (d, 22)
    block[d + 2 if kind == "collision" else d:d + 24] = r[2:] if kind == "collision" else r
    block[d + 24:] = _nonzero(rng, 40)

    def expect(seqs):
        at_d = [(off, ml) for pos, _, off, ml in placed(seqs) if pos + ml > d]
        assert at_d == ([found] if d <= MAX_DISTANCE else [near] if near else []), (kind, d, seed, at_d)
    return block, expect


# ---- family B ------------------------------------------------------------------------------------------------------------------------
def _search_step(start):
    """The fast encoder's search loop visits 1, 2, ... and widens its step after every 64 probes (lz4.c:636-647).  Returns (v, step): the first
    position >= start that a search begun at position 1 visits, and the step it leaves that position with."""
    pos, attempts = 1, 67
    while True:
        step = attempts >> 6
        attempts += 1
        if pos >= start:
            return pos, step
        pos += step


def _prefix(rng, total, body):
    """24 random non-zero bytes, then zeros, in front of `body`: `total` bytes in all.  One long match covers the zeros, and the search
    restarts behind it exactly as it starts at the head of a block."""
    lead = np.zeros(total - len(body), np.uint8)
    lead[:24] = _nonzero(rng, 24)
    return np.concatenate([lead, body])


def length_case(L, M, seed, hc=False, prefixed=False):
    """A literal run of exactly L and a match of exactly M: random bytes, then a run of one byte b, then 5 fresh bytes
    (five last literals: the least a block can end with, so nothing but the limit checks' own slack covers what follows a sequence).  The byte before the
    run is not b, so catch-up stops there.  LZ4HC looks at every position, finds the run at its second byte and emits (run start + 1, offset 1,
    run - 1).  The fast encoder only looks at the positions its widening step visits: the first visited position v inside the run fills the
    bucket, the next one, v + step, finds it, catch-up walks both back to the run's start, and it emits (run start + step, offset step,
    run - step).  So the run starts at L - step and is M + step long; up to 61 literals step is 1 and the block is rand(L - 1) + run."""
    rng = np.random.default_rng(seed)
    step = 1
    if not hc:
        step = next(s for s in range(1, 9) if _search_step(L - s)[1] == s)
    start, run = L - step, M + step
    body = _nonzero(rng, start + run + 5)
    b = body[start - 1] % 255 + 1                                        # 1..255, not the byte before the run
    body[start:start + run] = b
    if body[start + run] == b:
        body[start + run] = b % 255 + 1
    base = 0
    if prefixed:
        base = LIMIT_64K - len(body)
        body = _prefix(rng, LIMIT_64K, body)

    def expect(seqs):
        mine = [(lit, ml) for pos, lit, off, ml in placed(seqs) if pos >= base]
        assert (L, M) in mine, (L, M, seed, hc, prefixed, mine)
    return body, expect


# ---- family C ------------------------------------------------------------------------------------------------------------------------
def tail_case(s, seed, prefixed=False, k=9):
    """rand(64) | k fresh bytes | a copy of the block's first s bytes, which ends the block.  A match may start at iend - 13 at the latest
    (mflimit) and ends at iend - 5 at the latest (matchlimit): s >= 13 gives a last match that ends exactly at iend - 5 and five last
    literals, a smaller s no match in the tail.  The fresh part ends with eight equal bytes and three more: after 64 literals the fast
    encoder's step is 2 and it would leave at iend - 13 without looking; the short match of the run puts the step back to 1."""
    rng = np.random.default_rng(seed)
    head = _nonzero(rng, 64)
    fresh = _nonzero(rng, k + 11)
    c = fresh[k - 1] % 255 + 1
    fresh[k:k + 8] = c
    if fresh[k + 8] == c:
        fresh[k + 8] = c % 255 + 1
    body = np.concatenate([head, fresh, head[:s]])
    n = len(body)
    base = 0
    if prefixed:
        base = LIMIT_64K + 3 - n
        body = _prefix(rng, LIMIT_64K + 3, body)
        n = len(body)

    def tail_match(seqs):
        return [(pos, off, ml) for pos, _, off, ml in placed(seqs) if pos + ml > n - s]

    def expect(seqs):
        if s >= 13:
            assert tail_match(seqs) == [(n - s, n - s - base, s - 5)] and seqs[-1][0] == 5, (s, seed, prefixed, tail_match(seqs), seqs[-1])
        else:
            assert tail_match(seqs) == [], (s, seed, prefixed, tail_match(seqs))
    expect.tail_match = tail_match
    return body, expect


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
def distance_cases():
    """[(name, block, expectation)] for the fast encoders AND LZ4HC."""
    return [(f"A d={d} J={j}", *distance_case(d, j, 4100 + d % 16 * 4 + j)) for d in DISTANCES for j in (0, 3)] + \
           [(f"A d={d} J=0 echo", *distance_case(d, 0, 4150 + d % 16, echo=True)) for d in DISTANCES if d <= MAX_DISTANCE]


def hop_cases():
    """[(name, block, expectation)] for LZ4HC."""
    return [(f"A {kind} d={d}", *hop_case(d, 4200 + d % 16, kind)) for kind in HOPS for d in DISTANCES]


def length_cases(hc):
    """[(name, block, expectation or None)]: the blocks built for the fast encoder and, where they differ (L > 61), the ones built for LZ4HC.
    Both encoders take all of them; an expectation is set where the block was built for the encoder asked about."""
    out = []
    for prefixed in (False, True):
        for i, (L, M) in enumerate(LENGTH_PAIRS):
            for built_hc in (False, True):
                if built_hc and L <= 61:
                    continue                                              # the same block
                block, expect = length_case(L, M, 4300 + i, hc=built_hc, prefixed=prefixed)
                mine = built_hc == hc or L <= 61
                out.append((f"B L={L} M={M}{' hc' if built_hc else ''}{' prefixed' if prefixed else ''}", block, expect if mine else None))
    return out


def tail_cases():
    """[(name, block, expectation)]; the expectation is the fast encoders' (LZ4HC: expectation.tail_match tells what it did)."""
    return [(f"C s={s}{' prefixed' if prefixed else ''}", *tail_case(s, 4400 + s, prefixed)) for prefixed in (False, True) for s in TAILS]


def has_long_length(seqs):
    return any(lit >= 269 or (ml or 0) >= 273 for lit, _, ml in seqs)


class Reference:
    """The oracle's answers for one set of cases, computed once: its bytes, its parse, every expectation asserted, and for family D its
    return value at every capacity of the sweep."""

    def __init__(self, oracle, hc):
        self.hc = hc
        self.distance = self._checked(oracle, distance_cases() + (hop_cases() if hc else []))
        self.lengths = self._checked(oracle, length_cases(hc))
        tails = tail_cases()
        self.tails = self._checked(oracle, tails, expectations=not hc)
        if hc:
            # LZ4HC parses these blocks its own way: every target length has to occur somewhere in the set, and both outcomes at the end of a block
            seen = [s for _, _, _, seqs in self.lengths for s in seqs]
            assert {lit for lit, _, _ in seen} >= set(LITERALS), sorted({lit for lit, _, _ in seen})
            assert {ml for _, _, ml in seen} >= set(MATCHES), sorted({ml for _, _, ml in seen if ml})
            ends = {bool(expect.tail_match(seqs)) for (_, _, expect), (_, _, _, seqs) in zip(tails, self.tails)}
            assert ends == {False, True}, ends
        # family D
        self.limited = []
        for name, block, want, seqs in self.lengths + self.tails:
            if has_long_length(seqs):
                for delta in CAP_DELTAS:
                    cap = len(want) + delta
                    self.limited.append((f"D {name} cap={delta:+d}", block, cap, oracle.compress_raw(block, cap, hc=hc)[0], want))
        assert {r > 0 for _, _, _, r, _ in self.limited} == {False, True}

    def _checked(self, oracle, cases, expectations=True):
        out = []
        for name, block, expect in cases:
            want = oracle.compress(block, hc=self.hc)
            seqs = parse_sequences(want)
            assert sum(lit + (ml or 0) for lit, _, ml in seqs) == len(block), name
            if expect is not None and expectations:
                expect(seqs)
            out.append((name, block, want, seqs))
        return out

    def everything(self):
        return self.distance + self.lengths + self.tails


_references = {}


def reference(oracle, hc):
    """The shared, unchanged Reference of a session."""
    if hc not in _references:
        _references[hc] = Reference(oracle, hc)
    return _references[hc]


# ---- what both test files do with a set -----------------------------------------------------------------------------------------------
ANY, SMALL, LARGE = (0, 1 << 30), (0, 65536), (65537, 1 << 30)      # block sizes a form takes (inclusive)


def fits(block, sizes):
    return sizes[0] <= len(block) <= sizes[1]


def check_bit_exact(encode, cases, what):
    """cases: [(name, block, oracle's bytes, ...)] in one batch: result, bytes, guard bytes behind the bound"""
    assert cases, what
    res, dst = encode([c[1] for c in cases], None)
    for i, (name, block, want, *_) in enumerate(cases):
        assert res[i] == len(want), (what, name, res[i], len(want))
        assert np.array_equal(dst[i, :res[i]], want), (what, name)
        assert (dst[i, compress_bound(len(block)):] == 0xA5).all(), (what, name, "wrote past the bound")


def check_limited(encode, limited, what):
    """limited: [(name, block, cap, oracle's return value, oracle's bytes)] in one batch: return value, bytes when positive, guard bytes from cap on"""
    assert limited, what
    res, dst = encode([c[1] for c in limited], [c[2] for c in limited])
    for i, (name, block, cap, ret, want) in enumerate(limited):
        assert res[i] == ret, (what, name, res[i], ret)
        if ret > 0:
            assert np.array_equal(dst[i, :ret], want), (what, name)
        assert (dst[i, cap:] == 0xA5).all(), (what, name, "wrote past the capacity")


# ---- the encoder forms (tests and tools take them from here) ---------------------------------------------------------------------------
#            name                                   LZ4HC  block sizes  emu_helpers.encode arguments (None: emu_helpers.encode_two_launches)
EMU_FORMS = [("fast-wave", False, ANY, dict()),
             ("fast-wave-five-per-workgroup", False, ANY, dict(wg5=True)),
             ("fast-lane", False, ANY, dict(lane=True)),
             ("fast-two-launches", False, ANY, None),
             ("hc-wave-heads16", True, SMALL, dict(hc=True)),
             ("hc-wave-heads32", True, LARGE, dict(hc=True)),
             ("hc-lane-large-blocks", True, LARGE, dict(hc=True, lane=True, conv=True)),
             ("hc-lane-natural-chains", True, SMALL, dict(hc=True, nat=True)),
             ("hc-lane-chains-with-shared-lengths", True, SMALL, dict(hc=True, lcp=True))]


def emu_encode(kwargs, blocks, caps=None):
    import emu_helpers as emu
    if kwargs is None:
        return emu.encode_two_launches(blocks, caps=caps)[:2]
    return emu.encode(blocks, caps=caps, **kwargs)


#            name                     LZ4HC  forced mapping (conftest.ForcedMapping)   tuning knobs
GPU_FORMS = [("fast-wave", False, ("LZ4HIP_ENCODER", "wave"), dict()),
             ("fast-wave-one-per-workgroup", False, ("LZ4HIP_ENCODER", "wave"), dict(encoder_wg5=1)),
             ("fast-wave-five-per-workgroup", False, ("LZ4HIP_ENCODER", "wave"), dict(encoder_wg5=2)),
             ("fast-lane", False, ("LZ4HIP_ENCODER", "lane"), dict()),
             ("fast-default", False, None, dict()),
             ("hc-wave", True, ("LZ4HIP_HC", "wave"), dict()),
             ("hc-lane", True, ("LZ4HIP_HC", "lane"), dict()),
             ("hc-default", True, None, dict())]


@contextlib.contextmanager
def forced(form):
    """The mapping and knobs of a GPU form for the calls inside; on exit ForcedMapping asserts that the mapping named ran and its sibling did not"""
    from conftest import ForcedMapping
    from lz4net_amd import _lib
    _, _, mapping, knobs = form
    with contextlib.ExitStack() as stack:
        if mapping is not None:
            stack.enter_context(ForcedMapping(*mapping))
        stack.enter_context(_lib.tuning(**knobs))
        yield


def gpu_size_classes(hc):
    # LZ4HC picks its kernels by the largest block of a batch (16- or 32-bit heads; the lane mapping: precomputed tables up to 64 KiB, the
    # large-block kernel above), so the two classes go in batches of their own; a fast encoder picks its variant block by block
    return (SMALL, LARGE) if hc else (ANY,)
