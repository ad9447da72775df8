"""TEST INFRASTRUCTURE for tests/test_gpu_lane_window.py and tests/test_simt_lane_window.py, which are one design: small LZ4 blocks BUILT
sequence by sequence (lane_flush_cases.emit) so that the lane decoder's input window (lz4hip_decode_lane4.hpp, T1a / T1b / B3) meets the
positions at which a conditional assignment done as a MOVE UNDER A LANE MASK can go wrong where a select cannot: a move that runs under the
wrong lanes, in the wrong order inside its region, or between registers the compiler paired differently.

The window W holds 48 bytes of the 64-byte-aligned source: 16 of the previous 32-byte piece and one piece, the low or the high half of the
sector in L.  The cursor sits at byte d of W; at d >= 32 the next piece is taken in (W[0..3] <- W[8..11], W[4..11] <- a half of L), and the
16 bytes at d come out of W through a tree over the bits of d / 4 and a byte rotation by d % 4.  Where the cursor rests follows from the
block alone (cursor_trace below: a model of the CURSOR, not of the decoder), so the families can say what they reach:
  * skew: the same block with its source at every byte alignment 0 .. 63 of a sector;
  * refill: runs of sequences of one encoded size, and streamed literal runs, that make the cursor leave a piece at every d in 32 .. 47, for
    the low and for the high half of the sector, each block a second time with one more sequence in front (the other iteration parity);
  * cursor: literal runs of 0, 1, 11, 12, 15, 16, 270 and 300 bytes and matches of 4, 18, 19, 274 and 529 bytes in changing order: every dword
    index 0 .. 7 and byte phase 0 .. 3 of the cursor, the first streamed run, one and two length bytes, length bytes of 255;
  * ends: sources that end 1 .. 64 bytes into a sector, and blocks of one and of two pieces;
  * identical: 64 times the same block at the same alignment (every lane mask is all ones or all zeros), and last_wave: 66 blocks, whose second
    wavefront is mostly inactive lanes.  In the other batches block i lies at alignment i % 64: 64 lanes of pairwise different phases.
Two blocks of every batch are also truncated and corrupted; the result codes are the CPU codec's.  Every block produces at most 2 KiB."""
import numpy as np

import lane_flush_cases as flush

EXTRA = flush.EXTRA
TAIL = flush.TAIL
LITS = (0, 1, 11, 12, 15, 16, 270, 300)
MATCHES = (4, 18, 19, 274, 529)


def lay_out(comps, step, first=0):
    """(buffer, offset of row 0 in it, stride): row i at alignment (first + i * step) % 64 of a 64-byte sector, 64 spare bytes on both sides"""
    longest = max([len(c) for c in comps] + [1]) + 16
    stride = longest + (step - longest) % 64
    raw = np.zeros(len(comps) * stride + 256, np.uint8)
    at = 64 + (first - (raw.ctypes.data + 64)) % 64
    for i, c in enumerate(comps):
        raw[at + i * stride:at + i * stride + len(c)] = c
    return raw, at, stride


def cursor_trace(block, skew):
    """where the decoder's input cursor rests while it decodes `block` from alignment `skew`: (views, crossings) -- the offsets d < 32 in the
    window at which it looks at the stream, and (d, half of the sector that comes in) of every refill.  The cursor rests at each token, behind
    the length bytes of a streamed literal run (12 bytes and more) and every 16 bytes of it, and at the offset field behind such a run."""
    b = bytes(block)
    stops, p = [], 0
    while p < len(b):
        stops.append(p)
        tok = b[p]
        p += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                ll += b[p]
                p += 1
                if b[p - 1] != 255:
                    break
        if (tok >> 4) >= 12:
            stops += list(range(p, p + ll, 16)) + [p + ll]
        p += ll
        if p >= len(b):
            break
        p += 2
        if (tok & 15) == 15:
            while True:
                p += 1
                if b[p - 1] != 255:
                    break
    views, crossings, wb = [], [], -48
    for c in stops:
        while c + skew - wb >= 32:
            crossings.append((c + skew - wb, ((wb + 48) & 32) != 0))
            wb += 32
        views.append(c + skew - wb)
    return views, crossings


def sequence_lengths(block):
    """(literal run lengths, match lengths) of a block"""
    b, p, lits, matches = bytes(block), 0, [], []
    while p < len(b):
        tok = b[p]
        p += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                ll += b[p]
                p += 1
                if b[p - 1] != 255:
                    break
        lits.append(ll)
        p += ll
        if p >= len(b):
            break
        p += 2
        ml = (tok & 15) + 4
        if ml == 19:
            while True:
                ml += b[p]
                p += 1
                if b[p - 1] != 255:
                    break
        matches.append(ml)
    return lits, matches


def _finish(rng, seqs, pending=b""):
    """the block of the sequences, closed by a short near match and the last literals"""
    return flush.emit(seqs + [(pending + flush._bytes(rng, 3), 2, 5)], flush._bytes(rng, TAIL))


def uniform_block(lit, ml, count, lead, seed):
    """`count` sequences of one encoded size (lit literals, match length ml), `lead` short ones in front"""
    rng = np.random.default_rng(seed)
    seqs = [(flush._bytes(rng, 6), 2, 4) for _ in range(1 + lead)]
    seqs += [(flush._bytes(rng, lit), int(rng.integers(1, 7)), ml) for _ in range(count)]
    return _finish(rng, seqs)


def mixed_block(seed, budget=2000):
    """literal runs and match lengths of LITS and MATCHES in an order of the seed's, up to `budget` bytes of output"""
    rng = np.random.default_rng(seed)
    seqs, out = [(flush._bytes(rng, 8), 3, 4)], 12
    while True:
        lit, ml = LITS[int(rng.integers(len(LITS)))], MATCHES[int(rng.integers(len(MATCHES)))]
        if out + lit + ml > budget - 40:
            if out > budget - 400:
                break
            lit, ml = LITS[int(rng.integers(5))], MATCHES[int(rng.integers(3))]
        seqs.append((flush._bytes(rng, lit), int(rng.integers(1, min(out + lit, 60) + 1)), ml))
        out += lit + ml
    return _finish(rng, seqs)


def end_block(i, target, seed):
    """a block for row i (alignment i % 64) whose source ends `target` bytes into a sector: the last literals make up the difference"""
    rng = np.random.default_rng(seed)
    seqs = [(flush._bytes(rng, int(rng.integers(0, 14))), int(rng.integers(1, 5)), int(rng.integers(4, 24))) for _ in range(int(rng.integers(1, 9)))]
    seqs[0] = (flush._bytes(rng, 9), 4, 6)
    for tail in range(TAIL, TAIL + 140):
        block, raw = flush.emit(seqs, flush._bytes(rng, tail))
        if (i % 64 + block.size - target) % 64 == 0:
            return block, raw
    raise AssertionError((i, target))


def small_block(n_lit, with_match, seed):
    """one or two pieces of source: literals only, or one short match and the last literals"""
    rng = np.random.default_rng(seed)
    return flush.emit([(flush._bytes(rng, max(n_lit, 1)), 1, 4)] if with_match else [], flush._bytes(rng, TAIL + (0 if with_match else n_lit)))


def _with_damage(items):
    extra = []
    for j, i in enumerate((1, len(items) - 2)):
        for k in (2 * j, 2 * j + 1):
            c, cap = flush.damaged(items[i][0], items[i][1], k)
            extra.append((c, None, cap))
    return [(c, raw, raw.size) for c, raw in items] + extra


def batches():
    """name -> (items, step, first): items as in lane_flush_cases.batches(); row i lies at alignment (first + i * step) % 64"""
    out = {}
    out["skew"] = (_with_damage([mixed_block(11, 700)] * 64), 1, 0)
    # token + literals + offset (+ one length byte from match length 19 on): encoded sizes 3 .. 15; streamed runs move the cursor by 16
    shapes = [(0, 4), (2, 4), (4, 5), (6, 18), (8, 4), (10, 19), (11, 18), (11, 19)]
    refill = [uniform_block(lit, ml, 1900 // (lit + ml), lead, 100 * lit + ml + lead) for lit, ml in shapes for lead in (0, 1) for _ in range(3)]
    refill += [_finish(np.random.default_rng(900 + i), [(flush._bytes(np.random.default_rng(i), n), 3, 4) for n in runs])
               for i, runs in enumerate([(40, 75, 300, 33), (16, 270, 17, 290), (12, 13, 14, 15, 31, 47, 63, 500), (600, 19, 700),
                                         (41, 76, 301, 34), (17, 271, 18, 291), (13, 14, 15, 16, 32, 48, 64, 501), (601, 20, 701)] * 2)]
    out["refill"] = (_with_damage(refill), 1, 0)                                                   # 48 + 16 + 4
    out["cursor"] = (_with_damage([mixed_block(2000 + i) for i in range(64)]), 1, 5)
    ends = [end_block(i, 1 + (i * 27) % 64, 3000 + i) for i in range(64)]                          # (27 is odd: every target 1 .. 64 once)
    ends += [small_block(n, m, 3100 + n) for n in (0, 1, 3, 7, 12, 19, 30, 44) for m in (False, True)]
    out["ends"] = (_with_damage(ends), 1, 0)                                                       # 64 + 16 + 4
    out["identical"] = (_with_damage([mixed_block(12, 900)] * 64), 0, 37)
    out["last_wave"] = (_with_damage([mixed_block(4000 + i, 500 + 20 * i) for i in range(66)]), 1, 21)   # 66 + 4: the second wavefront has six lanes
    for name, (items, step, first) in out.items():
        assert 64 <= len(items) <= 130 and all(cap <= 2048 for _, _, cap in items), name
    return out


def reach(name):
    """(views, crossings) of the valid blocks of a batch at the alignments its rows lie at"""
    items, step, first = _cached()[name]
    views, crossings = set(), set()
    for i, (c, raw, _) in enumerate(items):
        if raw is not None:
            v, x = cursor_trace(c, (first + i * step) % 64)
            views.update(v)
            crossings.update(x)
    return views, crossings


_expected = {}


def _cached():
    if "batches" not in _expected:
        _expected["batches"] = batches()
    return _expected["batches"]


def expected(oracle, name, known):
    """(items, step, first, CPU codec's result per block, its bytes per block): computed once per batch and decoder kind, shared by every form"""
    key = (name, known)
    if key not in _expected:
        items, step, first = _cached()[name]
        res, outs = [], []
        for c, raw, cap in items:
            r, o = oracle.uncompress_raw(c, cap) if known else oracle.uncompress_unknown_raw(c, len(c), cap + EXTRA)
            if raw is not None:                                    # a block built here is a valid one, and decodes to what emit() said
                assert r == (len(c) if known else raw.size) and np.array_equal(o[:raw.size], raw), (name, known)
            res.append(r)
            outs.append(o)
        _expected[key] = (items, step, first, res, outs)
    return _expected[key]


def check(oracle, name, known, decode, repeat=1):
    """decode(streams, capacities, known, step, first) -> (results, rows with 64 guard bytes of 0xA5 behind the capacity), the streams laid out
    by lay_out(streams, step, first); repeat: the batch is decoded `repeat` times over in one call (a form that only larger batches reach)"""
    items, step, first, want, outs = expected(oracle, name, known)
    # (the known-size codec takes no input length: a damaged stream runs on into the zeros the oracle's wrapper puts behind it, so here too)
    comps = [np.concatenate([c, np.zeros(cap + 1024, np.uint8)]) if known and raw is None else c for c, raw, cap in items] * repeat
    caps = [cap + (0 if known else EXTRA) for _, _, cap in items] * repeat
    res, dst = decode(comps, caps, known, step, first)
    for i in range(len(comps)):
        j = i % len(items)
        assert res[i] == want[j], (name, known, i, int(res[i]), want[j])
        if items[j][1] is not None:
            n = items[j][1].size
            assert np.array_equal(dst[i, :n], outs[j][:n]), (name, known, i)
        assert (dst[i, caps[i]:caps[i] + 64] == 0xA5).all(), (name, known, i, "wrote past the block")
