"""Blocks BUILT for the thresholds of the LZ4HC lane encoder over chains with shared lengths (lz4net_amd/csrc/lz4hip_hc_lcp.hpp) and its two
table builders, shared by tests/test_simt_hc_lane_cases.py and tests/test_gpu_hc_lane_cases.py.  Conventions of tests/encoder_cases.py and
tests/wave_decode_cases.py: every builder returns (block, expectation), the expectation is about the ORACLE's own parse -- which match, at
which offset and length -- and is asserted before any kernel is asked; a family also names the emulator counters (lz4hip::HcStat,
LZ4HIP_STAT_HC) that must move for it, and pairs of blocks on the two sides of a threshold: each encoded alone, the slot named is
smaller for the first than for the second.  A block that misses its threshold fails on the CPU.

Table   the builders' table  chain | lcp << 16 | y << 24  against a plain reference, entry by entry (table_reference, table_blocks)
E  equal case        W M b1 | W M b2 | W m' | W M x: the walk meets F(c) == lcp[c] and decides by one byte of the register window
K  the 255 cap       occurrences sharing 253..257 and 300 bytes: the cap at the head, in the walk, inside one repeat fill
L  matchlimit        candidates whose common bytes with the search position run to the end of the block
R  repeat            period 1..4 runs of every short and two long lengths, at every table alignment; colliding heads; a run walked again
W  wider search      the filter byte inside the common region, at its end, beyond it; the search position's byte cached and reloaded
B  backward          extensions of 0..9 bytes, stopped by the limit, by a mismatch, by the block's first byte
T  attempts          the long match as attempt number 255, 256 and 257: no near head, a repeat head, a head five bytes back
P  parse             small seeded blocks chosen for one branch of the lazy parse each, and the output limit around their size

All random content comes from np.random.default_rng(fixed seed)."""
import numpy as np

from encoder_cases import hash15, parse_sequences, placed

MINMATCH, LAST_LITERALS, CAP, ATTEMPTS = 4, 5, 255, 256

# lz4hip::HcStat (lz4net_amd/csrc/lz4hip_hc_conv.hpp), in its order
SLOTS = ["P_Ml2EqMl", "P_Start0Restore", "P_Start2Near", "P_S3CorrOptimal", "P_S3CorrFit", "P_S3NoSearch", "P_Ml3EqMl2Short", "P_Ml3EqMl2Plain",
         "P_Start3Near", "P_Start3Far", "P_Start3Behind", "P_Start3Inside", "P_Ml2Replaced", "P_Lt15", "P_Ge15", "P_Phase4",
         "P_EmitRefuseLiterals", "P_EmitRefuseMatch", "P_EmitRefuseBytes",
         "W_Less", "W_Greater", "W_EqLimit", "W_EqWinDiff", "W_EqWinSame", "W_EqWinMiss", "W_BothCap", "W_EndDistance", "W_EndStart", "W_EndAttempts",
         "H_Cap", "H_Below", "R_Taken1", "R_Taken2", "R_Taken3", "R_Taken4", "R_Short1", "R_Short2", "R_Short3", "R_Short4",
         "C_WinHit", "C_Fill", "C_MissNoFill", "C_Bytes", "F_Pass", "F_Fail", "F_ReadCached", "F_ReadLoaded", "F_Improved", "F_NotImproved",
         "B_Four4", "B_FourLess", "B_Byte", "B_StopLimit", "B_StopStart", "B_StopMismatch", "L_Store16", "L_Store1", "L_EntryCap", "L_EntryBelow",
         "T_Leader", "T_Follower", "T_Late", "T_LeaderPast255", "N_PrevLane", "N_PrevHead"]
S = {name: i for i, name in enumerate(SLOTS)}
PARSE_SLOTS = [s for s in SLOTS if s.startswith("P_") and not s.startswith("P_EmitRefuse")]
REFUSALS = ["P_EmitRefuseLiterals", "P_EmitRefuseMatch", "P_EmitRefuseBytes"]
POISON = 0x5A5A5A5A


def _rnd(rng, n):
    return rng.integers(1, 256, n).astype(np.uint8)


def _not(*taken):
    """a byte 1..255 that is none of `taken`"""
    return next(b for b in range(1, 256) if b not in {int(t) for t in taken})


def _cat(*parts):
    return np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(p, np.uint8).reshape(-1) for p in parts]).astype(np.uint8)


def _words(a):
    a = np.asarray(a, np.uint64)
    return a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)


# ---- the table against a plain reference ----------------------------------------------------------------------------------------------
def table_reference(a):
    """(chain, len, y, y_valid) for p in 1 .. n - 4 (index 0 unused), by the definitions of lz4hip_hc_lcp.hpp: prev = the latest q in [1, p)
    in the bucket of p, else 0; len = the common bytes of a[p:] and a[prev:], no further than matchlimit - p, at most 255, never negative;
    y = a[prev + len], compared only where len is below both caps."""
    a = np.asarray(a, np.uint8)
    n = len(a)
    last = n - 4
    if last < 1:
        return (np.zeros(1, np.int64),) * 3 + (np.zeros(1, bool),)
    h = hash15(_words(a)).astype(np.int64)
    prev = np.zeros(last + 1, np.int64)
    latest = {}
    for p in range(1, last + 1):
        prev[p] = latest.get(h[p], 0)
        latest[h[p]] = p
    p = np.arange(last + 1)
    room = np.clip(n - LAST_LITERALS - p, 0, CAP)
    length = np.zeros(last + 1, np.int64)
    alive = np.ones(last + 1, bool)
    padded = np.concatenate([a.astype(np.int64), np.full(CAP + 1, -1)])
    for k in range(CAP):
        alive &= (k < room) & (padded[p + k] == padded[prev + k])
        if not alive.any():
            break
        length += alive
    y = a[np.minimum(prev + length, n - 1)]
    return p - prev, length, y, (length < CAP) & (length < n - LAST_LITERALS - p)


def check_table(block, table, what):
    """every entry of the table the builders left for `block` (65536 entries, poisoned before)"""
    n = len(block)
    last = n - 4
    assert (table[max(last, 0) + 1:] == POISON).all(), (what, "an entry past the last position was written")
    if last < 1:
        if n <= 65536:
            assert table[0] & 0xFFFF == 0xFFFF, (what, hex(table[0]))
        return
    assert table[0] & 0xFFFF == 0xFFFF, (what, hex(table[0]))
    chain, length, y, y_valid = table_reference(block)
    t = table[:last + 1].astype(np.int64)
    for name, got, want, where in (("chain", t & 0xFFFF, chain, np.ones(last + 1, bool)), ("len", (t >> 16) & 255, length, np.ones(last + 1, bool)),
                                   ("y", t >> 24, y, y_valid)):
        bad = np.flatnonzero((got != want) & where & (np.arange(last + 1) >= 1))
        assert bad.size == 0, (what, name, "first wrong position", int(bad[0]), "got", int(got[bad[0]]), "want", int(want[bad[0]]), "of", bad.size)


TABLE_SMALL = tuple(range(21))
TABLE_EDGES = tuple(m + 4 for m in (63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097))
TABLE_CONTENTS = ("two-symbols", "periods", "broken-followers", "shared-lengths", "into-matchlimit")
SHARED_LENGTHS = (253, 254, 255, 256, 257, 317, 318, 319, 320)


def table_content(kind, n, seed):
    """n bytes of one of the contents the builders go wrong on:
    two-symbols       buckets shared inside a step of 64 positions, across the four wavefronts' turns and across rounds
    periods           period 1..5 runs of 330 bytes and more (longer than 255 + 64): leaders count past the cap, followers are served
    broken-followers  a copy of 300 random bytes whose words at lanes 0 and 63 of every row have a nearer occurrence, so that the run of
                      consecutive predecessors breaks there
    shared-lengths    copies that share exactly 253..257 and 317..320 bytes with their predecessor
    into-matchlimit   the block ends in a copy of earlier bytes: the common bytes of its positions run into matchlimit"""
    rng = np.random.default_rng(seed)
    parts, have = [], 0

    def add(x):
        nonlocal have
        parts.append(np.asarray(x, np.uint8))
        have += len(x)
    while have < n:
        if kind == "two-symbols":
            add(rng.integers(0, 2, min(n - have, 8192)).astype(np.uint8) + 97)
        elif kind == "periods":
            q = len(parts) % 5 + 1
            add(np.tile(_rnd(rng, q), (330 + int(rng.integers(0, 70))) // q + 1))
            add(_rnd(rng, 3))
        elif kind == "broken-followers":
            src = _rnd(rng, 300)
            add(_rnd(rng, 5))
            add(src)
            at = have + 7 * 6 + 5                                         # where the copy will start
            for j in range(300 - 8):                                      # its positions at lanes 63 and 0: (p - 1) & 63
                if (at + j - 1) & 63 in (63, 0) and len(parts) < 40:
                    add(_cat(src[j:j + 5], [_not(src[j + 5])]))
            while have < at:
                add(_rnd(rng, 1))
            add(src)
        elif kind == "shared-lengths":
            for L in SHARED_LENGTHS:
                src = _rnd(rng, L)
                add(_cat(src, [1], src, [2]))
        else:
            add(_rnd(rng, max(n - have - 40, 64)))
    a = _cat(*parts)[:n].copy()
    if kind == "into-matchlimit" and n >= 16:
        k = min(n // 2, 300)
        a[n - k:] = a[:k]
    return a


def table_blocks():
    """[(name, block)]: every n in 0..20, the steps of 64, the rows of 256 and the rounds of 2048 positions with every content, one of 65 536 bytes"""
    out = [(f"n={n} {kind}", table_content(kind, n, 5000 + n)) for n in TABLE_SMALL for kind in ("two-symbols", "periods", "into-matchlimit")]
    out += [(f"n={n} {kind}", table_content(kind, n, 5100 + i)) for n in TABLE_EDGES for i, kind in enumerate(TABLE_CONTENTS)]
    big = _cat(*[table_content(kind, 13107 + (i == 0), 5200 + i) for i, kind in enumerate(TABLE_CONTENTS)])
    assert len(big) == 65536
    return out + [("n=65536 all contents", big)]


TABLE_MOVES = ["T_Leader", "T_Follower", "T_Late", "T_LeaderPast255", "N_PrevLane", "N_PrevHead"]
# (a, b, slot): the builders alone over block a move the slot less often than over block b
TABLE_PAIRS = [("n=261 broken-followers", "n=261 periods", "T_Follower"), ("n=261 periods", "n=261 broken-followers", "T_Leader"),
               ("n=261 broken-followers", "n=261 two-symbols", "T_Late"), ("n=2051 two-symbols", "n=2051 periods", "T_LeaderPast255"),
               ("n=261 broken-followers", "n=261 periods", "N_PrevLane"), ("n=261 periods", "n=261 broken-followers", "N_PrevHead")]


# ---- families -------------------------------------------------------------------------------------------------------------------------
class Family:
    """cases: [(name, block, expectation)]; moves: slots that must move over the family in one launch; pairs: [(a, b, slot)], cases a and b
    each encoded alone, counter[a][slot] < counter[b][slot]; zero: [(a, slot)], case a alone leaves the slot at 0"""

    def __init__(self, name):
        self.name, self.cases, self.moves, self.pairs, self.zero = name, [], [], [], []

    def add(self, name, block, expect):
        self.cases.append((f"{self.name} {name}", np.asarray(block, np.uint8), expect))
        return len(self.cases) - 1


def _has(pos, off, ml):
    def expect(seqs):
        assert (pos, off, ml) in [(p, o, m) for p, _, o, m in placed(seqs)], ("expected match", (pos, off, ml), "oracle's", placed(seqs))
    expect.want = (pos, off, ml)
    return expect


def _layout(rng, pieces, lead=8, gap=6, tail=40):
    """random bytes | piece | random bytes | piece ...: returns (block, positions of the pieces).  The byte in front of a piece never equals the
    byte in front of another piece (no backward extension across a gap)."""
    parts, at, have = [_rnd(rng, lead)], [], lead
    for i, piece in enumerate(pieces):
        if i:
            g = _rnd(rng, gap)
            parts.append(g)
            have += gap
        parts[-1][-1] = 1 + (7 * i + int(parts[-1][-1])) % 13 + 13 * (i % 19)       # distinct for up to 19 pieces
        at.append(have)
        parts.append(np.asarray(piece, np.uint8))
        have += len(piece)
    parts.append(_rnd(rng, tail))
    return _cat(*parts), at


# ---- E: the equal case --------------------------------------------------------------------------------------------------------------
E_K, E_M = (4, 5, 8, 20), (1, 15, 16, 31, 32, 40)


def equal_case(k, m, same, seed, tail=40):
    """W M b1 t | W M b2 t | W m' t | W M x t: the search at the fourth meets the third (F = k), whose entry says it shares k bytes with the
    second: equal, the byte is not in the window, the compare (which refills the window at s_ip + k) gives F(second) = k + m; the second's
    entry says k + m shared with the first: equal again, and the byte is in the window now.  x == b1: the first occurrence is k + m + 1 long;
    x another byte: the walk knows without a compare that it is k + m too, and the nearer second one stays."""
    rng = np.random.default_rng(seed)
    W, M = _rnd(rng, k), _rnd(rng, m)
    b1 = int(rng.integers(1, 256)); b2 = _not(b1); x = b1 if same else _not(b1, b2)
    t = [_rnd(rng, 3) for _ in range(4)]
    t[3][0] = _not(t[0][0])
    block, at = _layout(rng, [_cat(W, M, [b1], t[0]), _cat(W, M, [b2], t[1]), _cat(W, [_not(M[0])], t[2]), _cat(W, M, [x], t[3])], tail=tail)
    return block, _has(at[3], at[3] - at[0], k + m + 1) if same else _has(at[3], at[3] - at[1], k + m)


def equal_end_case(k, d, seed):
    """W s1 | W s2 | W ...end: the third occurrence starts d bytes in front of matchlimit.  d = k + 1: the deciding byte is the last one a match
    may hold; d = k: there is none (pos >= matchlimit); d < k: the head's length is capped below the entry's, no equal case"""
    rng = np.random.default_rng(seed)
    W = _rnd(rng, k)
    s1 = int(rng.integers(1, 256)); s2 = _not(s1)
    last = _cat(W, [_not(s1, s2)], _rnd(rng, 24))[:d + LAST_LITERALS]
    block, at = _layout(rng, [_cat(W, [s1], _rnd(rng, 3)), _cat(W, [s2], _rnd(rng, 3)), last], tail=0)
    assert len(block) - LAST_LITERALS - at[2] == d
    return block, _has(at[2], at[2] - at[1], min(k, d))


def family_E():
    f = Family("E")
    idx = {}
    for k in E_K:
        for m in E_M:
            for same in (True, False):
                idx[k, m, same] = f.add(f"k={k} m={m} {'same' if same else 'different'}", *equal_case(k, m, same, 6000 + 64 * k + m))
            f.pairs.append((idx[k, m, True], idx[k, m, False], "W_EqWinDiff"))
            f.pairs.append((idx[k, m, False], idx[k, m, True], "W_EqWinSame"))
        f.pairs.append((idx[k, 1, False], idx[k, 16, False], "C_WinHit"))
    # the window's upper edge.  With room behind it the compare that finds F(second) = k + m refills the window on its way, and the deciding
    # byte of m = 32 and 40 lies inside the new one.  Nine bytes behind x the block ends: the third compare step is the byte loop, the
    # window stays at [s_ip + k, s_ip + k + 32), and the deciding byte of m = 32 is the first one past it, of m = 31 the last one in it
    edge = {(m, same): f.add(f"k=8 m={m} {'same' if same else 'different'} at the end of the block", *equal_case(8, m, same, 6400, tail=6))
            for m in (31, 32) for same in (True, False)}
    f.pairs += [(edge[31, True], edge[32, True], "W_EqWinMiss"), (edge[32, True], edge[31, True], "W_EqWinSame"),
                (edge[32, False], edge[31, False], "W_EqWinDiff")]
    for k in (9, 12):
        e = {d: f.add(f"end k={k} d={d}", *equal_end_case(k, d, 6500 + k)) for d in (k + 1, k, k - 1)}
        f.pairs += [(e[k + 1], e[k], "W_EqLimit"), (e[k - 1], e[k], "W_EqLimit"), (e[k], e[k - 1], "W_Less"), (e[k], e[k + 1], "C_Bytes"), (e[k], e[k + 1], "W_EqWinMiss")]
    f.moves = ["W_EqWinDiff", "W_EqWinSame", "W_EqWinMiss", "W_EqLimit", "W_Less", "H_Below", "C_Fill", "C_WinHit", "C_Bytes", "W_EndStart", "W_EndDistance"]
    return f


# ---- K: the 255 cap ------------------------------------------------------------------------------------------------------------------
K_SHARED = (253, 254, 255, 256, 257, 300)


def cap_head_case(L, seed):
    """X c1 | X c2, X of L bytes: the head of the search at the second shares L bytes, the entry says min(L, 255): from 255 on it is compared"""
    rng = np.random.default_rng(seed)
    X, Y, Z = _rnd(rng, 302), _rnd(rng, 302), _rnd(rng, 302)           # (every L: the same number of searches)
    Y[L], Z[L] = _not(X[L]), _not(X[L], _not(X[L]))
    block, at = _layout(rng, [_cat(X[:L], Y[L:]), _cat(X[:L], Z[L:])])
    return block, _has(at[1], at[1] - at[0], L)


def cap_walk_case(L, F, seed, G=300):
    """X[:L] c1 | X[:G] c2 | X[:F] c3, L <= G: the second's entry says min(L, 255); the search at the third has min(F, G) bytes in common with
    it -- below, at and above the entry's length, and the entry's length below and at the cap.  The nearer occurrence wins a tie."""
    rng = np.random.default_rng(seed)
    X = _rnd(rng, 321)
    c = [_not(X[L], X[G], X[F]), 0, 0]
    c[1] = _not(X[L], X[G], X[F], c[0]); c[2] = _not(X[L], X[G], X[F], c[0], c[1])
    block, at = _layout(rng, [_cat(X[:L], [c[0]]), _cat(X[:G], [c[1]]), _cat(X[:F], [c[2]])])
    return block, _has(at[2], at[2] - at[1], min(G, F))


def family_K():
    f = Family("K")
    head = {L: f.add(f"head L={L}", *cap_head_case(L, 6600 + L)) for L in K_SHARED}
    f.pairs += [(head[254], head[255], "H_Cap"), (head[255], head[254], "H_Below")]
    walk = {(L, F): f.add(f"walk L={L} F={F}", *cap_walk_case(L, F, 6700))
            for L, F in ((300, 254), (300, 255), (300, 256), (300, 300), (254, 300), (254, 254), (255, 300), (255, 255), (256, 300), (253, 257))}
    f.pairs += [(walk[300, 254], walk[300, 255], "W_BothCap"), (walk[300, 255], walk[300, 254], "W_Less"),
                (walk[256, 300], walk[254, 300], "W_Greater"), (walk[254, 300], walk[256, 300], "W_BothCap")]
    for delta in (1, 3):
        for repl in (254, 255, 256, 300):
            f.add(f"fill delta={delta} repl={repl}", *repeat_case(delta, repl, 0, 6800 + repl))
    f.moves = ["H_Cap", "H_Below", "W_BothCap", "W_Less", "W_Greater", "L_EntryCap", "L_EntryBelow", "C_Fill"]
    return f


# ---- L: matchlimit -------------------------------------------------------------------------------------------------------------------
L_D = tuple(range(8, 41))


def limit_case(d, three, seed):
    """T | T[:4] o | (T[:6] o |) ... T to the end of the block, the last occurrence d bytes in front of matchlimit: the walk from the short
    candidates meets the equal case and compares on towards the end of the block -- 16 bytes at a time while they fit under matchlimit
    (d >= 20), refilling the window only while 32 bytes fit into the block (d >= 31), byte by byte otherwise"""
    rng = np.random.default_rng(seed)
    T = _rnd(rng, 64)
    pieces = [_cat(T, [1]), _cat(T[:4], [_not(T[4])], _rnd(rng, 2))]
    if three:
        pieces.append(_cat(T[:6], [_not(T[6])], _rnd(rng, 2)))
    pieces.append(T[:d + LAST_LITERALS])
    block, at = _layout(rng, pieces, tail=0)
    assert len(block) - LAST_LITERALS - at[-1] == d
    return block, _has(at[-1], at[-1] - at[0], d)


def limit_wider_case(seed):
    """The wider search's filter index at a length that is only CAPPED (the M-cap shape).  U[6:] to the end 9 9 | a U[1:] to the end |
    U[0:8] q | U, which ends the block 14 bytes behind the wider search's position.  The best match at the last U is U[0:8]; the wider
    search six bytes on meets the copy of U[1:] first -- backwards to its limit, forwards to matchlimit -- and then U[6:], which
    shares the same capped length: fj == s_f == matchlimit - s_ip is no mismatch, the byte behind has to be READ (and agrees)."""
    rng = np.random.default_rng(seed)
    U = _rnd(rng, 40)
    n_u = 6 + 14 + LAST_LITERALS                                          # bytes of U at the block's end
    block, at = _layout(rng, [_cat(U[6:n_u], [9, 9]), _cat([_not(U[0])], U[1:n_u]), _cat(U[:8], [_not(U[8])], _rnd(rng, 2)), U[:n_u]], tail=0)
    ip = at[3]
    return block, _has(ip + 1, ip + 1 - (at[1] + 1), n_u - 1 - LAST_LITERALS)


def family_L():
    f = Family("L")
    idx = {(d, three): f.add(f"d={d} {'three' if three else 'two'} candidates", *limit_case(d, three, 6900 + three)) for d in L_D for three in (False, True)}
    f.pairs += [(idx[19, False], idx[20, False], "C_MissNoFill"), (idx[31, False], idx[30, False], "C_MissNoFill"),
                (idx[30, False], idx[31, False], "C_Fill")]
    w = f.add("wider capped", *limit_wider_case(6990))
    f.zero.append((w, "F_Fail"))
    f.moves = ["C_Bytes", "C_MissNoFill", "C_Fill", "W_EqWinMiss", "F_ReadLoaded"]
    return f


# ---- R: repeat ------------------------------------------------------------------------------------------------------------------------
R_REPL = (3, 4, 5, 6, 7, 8, 259, 260)


def repeat_case(delta, repl, align, seed):
    """lead | a run of period delta whose second period shares exactly `repl` bytes with the first | a breaker.  The run's second period starts
    at a position = align mod 4, where the repeat fill starts too.  repl >= 4: the head of the search there is delta bytes back and the
    match is (delta, repl); repl = 3: no match at all."""
    rng = np.random.default_rng(seed)
    P = _rnd(rng, delta)
    while len(set(P.tolist())) < delta:
        P = _rnd(rng, delta)
    run = np.tile(P, (delta + repl) // delta + 1)[:delta + repl]
    lead = 12 + (align - 12 - delta) % 4
    block = _cat(_rnd(rng, lead - 1), [_not(run[-1 % delta], P[-1])], run, [_not(run[repl % delta if delta else 0], np.tile(P, repl + 8)[repl + delta])], _rnd(rng, 30))
    ip = lead + delta
    assert ip % 4 == align
    if repl < MINMATCH:
        def expect(seqs):
            assert not [x for x in placed(seqs) if x[0] < lead + delta + repl + 4], placed(seqs)
        return block, expect
    return block, _has(ip, delta, repl)


def colliding_head(delta, seed):
    """8 bytes whose words at 0 and at delta differ and share a bucket: a head within 4 bytes that shares fewer than 4 bytes"""
    rng = np.random.default_rng(seed)
    while True:
        c = rng.integers(1, 256, (1 << 18, 8)).astype(np.uint64)
        w = lambda o: c[:, o] | c[:, o + 1] << np.uint64(8) | c[:, o + 2] << np.uint64(16) | c[:, o + 3] << np.uint64(24)
        hit = np.flatnonzero((hash15(w(0)) == hash15(w(delta))) & (w(0) != w(delta)) & (c[:, 0] != c[:, delta]))
        if hit.size:
            return c[hit[0]].astype(np.uint8)


def short_head_case(delta, seed):
    rng = np.random.default_rng(seed)
    block = _cat(_rnd(rng, 9), colliding_head(delta, seed), _rnd(rng, 30))

    def expect(seqs):
        assert not placed(seqs), placed(seqs)
    return block, expect


def distance5_case(seed):
    """period 5: the head is five bytes back -- not a repeat, an attempt like any other"""
    rng = np.random.default_rng(seed)
    P = np.array([3, 1, 4, 15, 9], np.uint8)
    block = _cat(_rnd(rng, 11), [7], np.tile(P, 5), [8], _rnd(rng, 30))
    return block, _has(12 + 5, 5, 20)


RERUN_L = 20


def rerun_case(delta, brk, seed, L=RERUN_L):
    """a run of period delta, `brk` other bytes, the run again for L bytes, another byte.  The search at the second run walks the first
    one backwards, delta at a time, through the entries its repeat fill wrote: each candidate shares with the search position exactly what
    its entry says it shares with its predecessor (up to the first run's end) -- the equal case -- and whether the predecessor shares more
    is decided by the entry's y, the byte behind the first run on the predecessor's side.  The first such step finds the byte outside the
    register window and compares (which refills the window); from the second step on y decides: equal while the second run goes on (the
    walk compares on and ends at the candidate that shares all L bytes), different where it has ended.  L = what the second candidate
    shares: y only ever says "different".  A wrong y ends the walk early: a shorter match."""
    rng = np.random.default_rng(seed)
    P = _rnd(rng, delta)
    while len(set(P.tolist())) < delta:
        P = _rnd(rng, delta)
    R = 40 + delta
    run = np.tile(P, R)[:R]
    b = _not(*P)
    head = max(p for p in range(0, R - 3, delta))                         # the latest position of the first run that holds the second run's first word
    shares = [R - c for c in range(head, delta - 1, -delta)]              # ... and what the walk's candidates share at the most, the head first
    L = shares[1] if L is None else L
    shares = [min(k, L) for k in shares]
    x = _not(*P, b)
    block = _cat(_rnd(rng, 11), [_not(*P, b, x)], run, [b] * brk, np.tile(P, L)[:L], [x], _rnd(rng, 40))
    start, again = 12, 12 + R + brk
    winner = head - delta * shares.index(L)
    return block, _has(again, again - (start + winner), L)


def fill_extent_case(delta, repl, align, seed):
    """X LONG | a run of period delta that ends in X = its last three bytes and the breaker | X LONG again.  The fill of the run's search
    ends three entries in front of the run's end: the entry of the X inside the run keeps its natural link to the first X, and the search
    at the last X, whose head is the X inside the run, reaches the first one and its 15 bytes.  A fill that writes one entry more sends
    that walk into the run."""
    rng = np.random.default_rng(seed)
    P = _rnd(rng, delta)
    while len(set(P.tolist())) < delta:
        P = _rnd(rng, delta)
    run = np.tile(P, (delta + repl) // delta + 1)[:delta + repl]
    b = _not(*P)
    X, LONG = _cat(run[-3:], [b]), rng.integers(100, 200, 11).astype(np.uint8)
    lead = _rnd(rng, 8 + (align - 8 - 1 - 4 - 11 - 6 - 1 - delta) % 4)
    block = _cat(lead, [_not(*P, b)], X, LONG, _rnd(rng, 6) % 90 + 1, [_not(*P, b, _not(*P, b))], run, [b, _not(LONG[0])], _rnd(rng, 5) % 90 + 1,
                 [_not(*P, b, _not(*P, b), _not(*P, b, _not(*P, b)))], X, LONG[:-1], [_not(LONG[-1])], _rnd(rng, 20) % 90 + 1)
    first = len(lead) + 1
    ip = first + 4 + 11 + 6 + 1 + delta
    last = ip + repl + 2 + 5 + 1
    assert ip % 4 == align and np.array_equal(block[last:last + 4], X) and np.array_equal(block[first:first + 4], X)
    return block, _has(last, last - first, 14)


def family_R():
    f = Family("R")
    idx = {}
    for delta in (1, 2, 3, 4):
        for repl in R_REPL:
            for align in range(4):
                idx[delta, repl, align] = f.add(f"delta={delta} repl={repl} align={align}", *repeat_case(delta, repl, align, 7000 + 16 * repl + delta))
        f.pairs += [(idx[delta, 3, 0], idx[delta, 4, 0], f"R_Taken{delta}")]
        sh = f.add(f"colliding head delta={delta}", *short_head_case(delta, 7900 + delta))
        f.pairs += [(idx[delta, 3, 0], sh, f"R_Short{delta}")]
    f.pairs += [(idx[1, 6, 1], idx[1, 7, 0], "L_Store16"), (idx[1, 7, 0], idx[1, 7, 1], "L_Store1"), (idx[1, 8, 0], idx[1, 259, 0], "L_EntryCap"),
                (idx[1, 4, 0], idx[1, 8, 0], "L_EntryBelow")]
    for delta in (1, 2, 3, 4):
        for repl in (5, 6, 7, 8, 9, 10):
            for align in range(4):
                f.add(f"fill extent delta={delta} repl={repl} align={align}", *fill_extent_case(delta, repl, align, 7800 + repl))
    f.add("distance 5", *distance5_case(7950))
    for delta in (1, 2, 3, 4):
        for brk in (1, 2, 3):
            long = f.add(f"run again delta={delta} break={brk}", *rerun_case(delta, brk, 7960 + 4 * delta + brk))
            short = f.add(f"run again delta={delta} break={brk}, two candidates long", *rerun_case(delta, brk, 7960 + 4 * delta + brk, L=None))
            f.pairs += [(short, long, "W_EqWinSame")]
    f.moves = [f"R_Taken{d}" for d in (1, 2, 3, 4)] + [f"R_Short{d}" for d in (1, 2, 3, 4)] + ["L_Store16", "L_Store1", "L_EntryCap", "L_EntryBelow", "H_Cap", "W_EqWinSame", "W_EqWinDiff"]
    return f


# ---- W and B: the wider search ------------------------------------------------------------------------------------------------------
def wider_case(cands, seed, ml=8, at_start=None):
    """U[0:ml] q | candidates | ... | U.  The best match at the last U is U[0:ml] (ml bytes); the wider search at ip + ml - 2 (start limit ip + 1)
    walks the occurrences of U[ml - 2:ml + 2], the latest first: `cands` in the order of the walk, each (back, fwd, behind) = the piece
    U[ml - 2 - back : ml - 2 + fwd] between a byte that differs in front and `behind` (None: a byte that differs) after it.  at_start: the LAST
    candidate of the walk sits at that position of the block (0..5), nothing but its `back` bytes in front of it."""
    rng = np.random.default_rng(seed)
    U = _rnd(rng, 100)
    s = ml - 2
    pieces = []
    for back, fwd, behind in reversed(cands):
        pieces.append(_cat([_not(U[s - back - 1])], U[s - back:s + fwd], [_not(U[s + fwd]) if behind is None else behind], _rnd(rng, 2)))
    pieces = [_cat(U[:ml], [_not(U[ml])], _rnd(rng, 2))] + pieces + [U[:90]]
    if at_start is not None:
        back, fwd, behind = cands[-1]
        assert back == at_start
        first = _cat(U[s - back:s + fwd], [_not(U[s + fwd])], _rnd(rng, 2))
        block, at = _layout(rng, [pieces[0]] + pieces[2:], lead=len(first) + 6)
        block[:len(first)] = first
        where = [(at[len(cands) - 1 - i] + 1, at[len(cands) - 1 - i] + 1 + cands[i][0] + cands[i][1]) for i in range(len(cands) - 1)] + [(0, back + fwd)]
    else:
        block, at = _layout(rng, pieces)
        where = [(at[len(cands) - i] + 1, at[len(cands) - i] + 1 + cands[i][0] + cands[i][1]) for i in range(len(cands))]
    return block, at[-1], where


def _wider_expect(ip, where, winner):
    """after ip the parse holds a match out of candidate `winner` (its position in `where`) and none out of the others; winner None: the first
    match is the best search's own"""
    def expect(seqs):
        src = {k for p, _, o, m in placed(seqs) if p >= ip for k, (w, e) in enumerate(where) if w <= p - o < e}
        assert src == (set() if winner is None else {winner}), ("expected a match out of candidate", winner, "at", where, "oracle's", [x for x in placed(seqs) if x[0] >= ip])
    return expect


def family_W():
    """ml = 8: s_back = 5, the filter index fj = longest - 5.  A = (5, 10): the whole way back, 15 bytes, fj = 10.  A candidate that shares
    fewer bytes than fj can never win (it extends backwards by 5 at the most): the reference reads its filter byte all the same, and so
    does the kernel -- what that byte decides is only whether a backward extension runs, which the counters see and the bytes do not."""
    f = Family("W")

    def add(name, cands, winner, seed):
        block, ip, where = wider_case(cands, seed)
        return f.add(name, block, _wider_expect(ip, where, winner))
    A = (5, 10, None)
    inside = add("filter byte inside the common region", [A, (0, 12, None)], 0, 8001)          # fj = 10 < 12: pass, no gain
    at_end = add("filter byte at the end of the common region", [A, (0, 10, None)], 0, 8001)   # fj = 10 == F: fail
    beyond = add("filter byte beyond the common region", [A, (0, 6, None)], 0, 8001)           # fj = 10 > 6: read
    cached = add("two reads, the longest unchanged", [A, (0, 6, None), (0, 5, None)], 0, 8001)
    # the M-probe shape: read (probe loaded) | a pass that improves (15 -> 17, fj = 12) | read: the search position's byte at the NEW
    # length must be loaded again
    reload = add("read, improved, read again", [A, (0, 6, None), (5, 12, None), (0, 7, None)], 2, 8001)
    add("read, not improved, read again", [A, (0, 6, None), (4, 11, None), (0, 7, None)], 0, 8001)
    f.pairs += [(at_end, inside, "F_Pass"), (inside, at_end, "F_Fail"), (inside, beyond, "F_ReadLoaded"), (beyond, cached, "F_ReadCached"),
                (cached, reload, "F_ReadLoaded"), (reload, cached, "F_ReadCached"), (at_end, inside, "F_NotImproved"), (beyond, reload, "F_Improved")]
    f.zero += [(reload, "F_ReadCached"), (cached, "F_Fail")]
    f.moves = ["F_Pass", "F_Fail", "F_ReadCached", "F_ReadLoaded", "F_Improved", "F_NotImproved", "B_StopLimit"]
    return f


B_ML, B_FWD = 32, 40


def back_case(back, seed, at_start=None):
    """the best match is B_ML = 32 bytes, the wider search at ip + 30 finds a candidate that shares 40 bytes forwards and `back` backwards:
    longer, and starting 18 bytes or more behind ip, so the parse cuts the first match where the second starts -- the bytes show `back`"""
    block, ip, where = wider_case([(back, B_FWD, None)], seed, ml=B_ML, at_start=at_start)
    start2 = ip + B_ML - 2 - back
    if start2 - ip < 3:
        e = _has(start2, start2 - where[0][0], back + B_FWD)
        e.ip = ip
        return block, e

    def expect(seqs):
        got = [(p, o, m) for p, _, o, m in placed(seqs) if p >= ip]
        assert got[:2] == [(ip, got[0][1], start2 - ip), (start2, start2 - where[0][0], back + B_FWD)], ("expected", (ip, start2 - ip), (start2, back + B_FWD), "oracle's", got)
    expect.ip = ip
    return block, expect


def family_B():
    """s_back = 29.  (A backward extension that stops at its limit with the byte in front of it still matching cannot be built: such a
    candidate holds the best search's word too, and the best search would have found it -- the limit stops the extension of 29 bytes.)"""
    f = Family("B")
    idx = {back: f.add(f"back={back}", *back_case(back, 8100)) for back in tuple(range(10)) + (28, 29)}
    f.pairs += [(idx[3], idx[4], "B_Four4"), (idx[28], idx[29], "B_StopLimit"), (idx[29], idx[28], "B_StopMismatch"), (idx[28], idx[29], "B_Byte"),
                (idx[29], idx[4], "B_FourLess")]
    f.start = {c: f.add(f"candidate at position {c}", *back_case(c, 8140, at_start=c)) for c in range(6)}
    # the M-back4 shape: the candidate at position 3 extends three bytes backwards, to the block's first byte; a row that ENDS with the byte
    # that would continue the match (the search position's byte four in front of its start), directly in front of the block, must not
    # be looked at.  With a row stride equal to that row's length its last byte is the byte in front of the block.
    block = f.cases[f.start[3]][1]
    ip = f.cases[f.start[3]][2].ip
    f.front_byte = int(block[ip + B_ML - 2 - 4])
    f.front_row = _cat(_rnd(np.random.default_rng(8150), len(block) + 50), [block[ip + B_ML - 2 - 4]])
    f.pairs += [(idx[2], f.start[2], "B_StopStart")]
    f.moves = ["B_Four4", "B_FourLess", "B_Byte", "B_StopLimit", "B_StopStart", "B_StopMismatch", "F_Improved"]
    return f


# ---- T: attempts --------------------------------------------------------------------------------------------------------------------
def attempts_case(shorts, head, seed):
    """Wd LONG | `shorts` times Wd and three other bytes | Wd LONG: the walk of the search at the last occurrence meets the short ones, the
    latest first, and then the long one; it has 256 attempts.
    head None  the long one is candidate number shorts + 1.
    head 2     Wd = a b a b, and in front of the last occurrence stands Z a b, a copy of an earlier Z a b q: that match ends where the last
               occurrence starts, and the search there finds its head two bytes back -- the repeat test, not one of the attempts: the long
               one is attempt number shorts + 1 again, with one candidate more in front of it.
    head 5     in front of the last occurrence stands Z Wd q, a copy of an earlier Z Wd q r: the head is five bytes back, one byte too far for
               the repeat test, and IS an attempt; with the Wd of the earlier copy the long one is attempt number shorts + 3."""
    rng = np.random.default_rng(seed)
    Wd = np.array([201, 202, 201, 202] if head == 2 else [201, 202, 203, 204], np.uint8)
    LONG = _cat([150], rng.integers(100, 200, 15).astype(np.uint8))
    Z = rng.integers(210, 256, 10).astype(np.uint8)
    lead = {None: [201, 202], 2: [201, 202], 5: _cat(Wd, [96])}[head]
    parts = [_rnd(rng, 6) % 90 + 1, Wd, LONG, [90], Z, lead, [99]]
    first_short = sum(len(p) for p in parts)
    for i in range(shorts):
        parts += [Wd, [1 + i % 89, 1 + (i // 89) % 89], [91 + i % 7]]
    parts += [[98]] if head is None else [[98], Z, lead]
    last = sum(len(p) for p in parts)
    block = _cat(*parts, Wd, LONG[:-1], [_not(LONG[-1])], _rnd(rng, 20) % 90 + 1)
    # a stray word in Wd's bucket would move the boundary: the walk from `last` is the near head (if any), the short ones, the earlier copy's
    # Wd (head 5), position 6, position 0
    chain = table_reference(block)[0]
    walk, c = [], last
    while c > 0:
        c -= int(chain[c])
        walk.append(c)
    want = ([] if head is None else [last - head]) + [first_short + 7 * i for i in reversed(range(shorts))] + ([37] if head == 5 else []) + [6, 0]
    if walk != want:
        assert seed < 20000, (walk, want)
        return attempts_case(shorts, head, seed + 1000)
    attempt = walk.index(6) + (0 if head == 2 else 1)                     # which attempt the long one is
    # not found: the wider search two bytes on finds the long one without its first byte
    return block, (_has(last, last - 6, 4 + 15) if attempt <= ATTEMPTS else _has(last + 1, last - 6, 4 + 14))


T_SHORTS = {None: (254, 255, 256), 2: (254, 255, 256), 5: (252, 253, 254)}


def family_T():
    f = Family("T")
    idx = {(n, head): f.add(f"shorts={n}" + ("" if head is None else f" head {head} bytes back"), *attempts_case(n, head, 8200))
           for head in (None, 2, 5) for n in T_SHORTS[head]}
    # (the long one as the LAST attempt ends the walk by its attempts too, with the block's first position still to come)
    f.pairs += [(idx[T_SHORTS[head][0], head], idx[T_SHORTS[head][1], head], "W_EndAttempts") for head in (None, 2, 5)]
    f.moves = ["W_EndAttempts", "R_Taken2"]
    return f


# ---- P: parse branches ------------------------------------------------------------------------------------------------------------
def parse_block(seed):
    """at most 600 bytes of a 2-, 3-, 4- or 8-symbol alphabet (by seed) with copies of earlier pieces planted: many overlapping matches of
    similar lengths, the lazy parse's food"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(120, 601))
    a = rng.integers(0, (2, 3, 4, 8)[seed % 4], n).astype(np.uint8) + 65
    for _ in range(int(rng.integers(2, 20))):
        ln = int(rng.integers(5, 60))
        src = int(rng.integers(0, n - ln))
        dst = int(rng.integers(0, n - ln))
        a[dst:dst + ln] = a[src:src + ln].copy()
    return a


# slot -> the seeds of parse_block chosen for it, offline, by choose_parse_seeds below over seeds from 9000 on (the rare ones further out)
PARSE_SEEDS = {"P_Ml2EqMl": [9000, 9001],
               "P_Start0Restore": [9000, 9004],
               "P_Start2Near": [9000, 9001],
               "P_S3CorrOptimal": [9000, 9001],
               "P_S3CorrFit": [9884, 11104],
               "P_S3NoSearch": [9000, 9004],
               "P_Ml3EqMl2Short": [9005, 9009],
               "P_Ml3EqMl2Plain": [9000, 9001],
               "P_Start3Near": [9000, 9001],
               "P_Start3Far": [9004, 9005],
               "P_Start3Behind": [9000, 9001],
               "P_Start3Inside": [9110, 9154],
               "P_Ml2Replaced": [12373, 12952],
               "P_Lt15": [],
               "P_Ge15": [9005, 9040],
               "P_Phase4": [9001, 9002]}


def choose_parse_seeds(stats_of, seeds=range(9000, 9400), per=2):
    """offline: for every parse slot the first `per` seeds whose block moves it, rarest slot first; stats_of(block) -> counters"""
    moved = {seed: stats_of(parse_block(seed)) for seed in seeds}
    out = {}
    for slot in sorted(PARSE_SLOTS, key=lambda s: sum(m[S[s]] > 0 for m in moved.values())):
        out[slot] = [seed for seed in seeds if moved[seed][S[slot]] > 0][:per]
    return out


def long_match_case(seed):
    """20 fresh bytes, 1700 zeros, 5 fresh bytes: one match of 1699 bytes, seven length bytes -- more than the six bytes the second check of the
    sequence emit (lz4hc.c:541) asks for, so at the capacity that just passes it the length bytes themselves do not fit"""
    rng = np.random.default_rng(seed)
    return _cat(_rnd(rng, 20), np.zeros(1700, np.uint8), _rnd(rng, 5)), _has(21, 1, 1699)


# (a, b, slot): the block of seed a moves the slot less often than the block of seed b, each encoded alone (counted offline, like PARSE_SEEDS)
PARSE_PAIRS = [(9002, 9000, "P_Start3Near"), (9000, 11104, "P_Start3Far"), (9154, 9000, "P_Start3Behind"), (9000, 9110, "P_Start3Inside"),
               (9000, 9110, "P_Ml3EqMl2Short"), (9154, 9004, "P_Ml3EqMl2Plain"), (9002, 9004, "P_S3CorrOptimal"), (9000, 9884, "P_S3CorrFit")]


def family_P():
    f = Family("P")
    f.slot_of = []
    for slot in PARSE_SLOTS:
        if slot in UNREACHED:
            continue
        seeds = PARSE_SEEDS.get(slot, [])
        assert len(seeds) >= 2, ("no two blocks chosen for", slot)
        for seed in seeds:
            f.slot_of.append((f.add(f"seed={seed} for {slot}", parse_block(seed), lambda seqs: None), slot))
    f.long_literals = f.add("40 literals and a match", *long_literals_case(9990))
    f.long_match = f.add("a match of 1699 bytes", *long_match_case(9991))
    of_seed = {}
    for i, (name, _, _) in enumerate(f.cases):
        if "seed=" in name:
            of_seed.setdefault(int(name.split("seed=")[1].split()[0]), i)
    f.pairs += [(of_seed[a], of_seed[b], slot) for a, b, slot in PARSE_PAIRS]
    f.moves = [s for s in PARSE_SLOTS if s not in UNREACHED]
    return f


P_CAP_DELTAS = tuple(range(-8, 3))


def long_literals_case(seed):
    """40 fresh bytes, a copy of the first 12, 6 fresh bytes: the one match has 40 literals in front of it -- a length byte, which the second
    check of the sequence emit (lz4hc.c:541) counts and the first (lz4hc.c:529) does not: at a capacity of 49 bytes only the second refuses"""
    rng = np.random.default_rng(seed)
    head = _rnd(rng, 40)
    return _cat(head, head[:12], [_not(head[12])], _rnd(rng, 5)), _has(40, 40, 12)


def limited_cases(oracle, f_P):
    """[(name, block, cap, oracle's return value, oracle's bytes)]: every capacity from 8 below to 2 above the compressed size for the first
    block of every parse slot"""
    out = []
    for i in [i for i, _ in f_P.slot_of[::2]] + [f_P.long_literals, f_P.long_match]:
        name, block, _ = f_P.cases[i]
        want = oracle.compress(block, hc=True)
        for delta in P_CAP_DELTAS:
            cap = len(want) + delta
            out.append((f"{name} cap={delta:+d}", block, cap, oracle.compress_raw(block, cap, hc=True)[0], want))
    assert {r > 0 for _, _, _, r, _ in out} == {False, True}
    return out


# slots with two sides: each stands in a threshold pair of some family (what ends a walk by distance or at the block's start has none: every
# walk that is not cut short ends so; the parse slots are asserted block by block, family P)
TWO_SIDED = [s for s in SLOTS if s[0] in "WHRCFBLTN" and s[1] == "_" and s not in ("W_EndDistance", "W_EndStart")] + [s for _, _, s in PARSE_PAIRS]
# the families whose named counters plain generator output moves too (gated by their pairs alone)
PLAIN_MOVES_ALL = ("E", "L", "W", "B")
# The one slot that no block can reach, asserted to stay at 0 over every block.  P_Lt15 (lz4hc.c:694) needs start2 < ip + ml and
# start2 - ip < 15 behind a third match with start3 >= ip + ml + 3 (P_Start3Far).  _Search3 (lz4hc.c:624-641) has moved start2 before:
#   no second rule   start2 = ip + min(ml, 18): not below ip + ml, or 18 bytes behind ip;
#   corr <= 0        start2 - ip >= min(ml, 18) already: the same;
#   second rule      ml2 = 4 and start2 < ip + ml.  The third search starts at start2 + ml2 - 3 = start2 + 1 with start2 as its limit, so
#                    start3 <= start2 + 1 <= ip + ml < ip + ml + 3: P_Start3Near; without a third search ml3 == ml2.
# (profiles/hc_lane_cases/README.md)
UNREACHED = ("P_Lt15",)


# ---- the sets ---------------------------------------------------------------------------------------------------------------------------
BUILDERS = {"E": family_E, "K": family_K, "L": family_L, "R": family_R, "W": family_W, "B": family_B, "T": family_T, "P": family_P}
NAMES = tuple(BUILDERS)
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
            want = oracle.compress(block, hc=True)
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


def assert_moves(f, st):
    for slot in f.moves:
        assert st[S[slot]] > 0, (f.name, "counter never moved", slot)


def assert_pairs(f, alone):
    """alone: case index -> counters of that case encoded alone"""
    for a, b, slot in f.pairs:
        x, y = alone[a][S[slot]], alone[b][S[slot]]
        assert x < y, (f.name, "pair not in the declared direction", f.cases[a][0], f.cases[b][0], slot, x, y)
    for a, slot in f.zero:
        assert alone[a][S[slot]] == 0, (f.name, "counter moved", f.cases[a][0], slot, alone[a][S[slot]])
