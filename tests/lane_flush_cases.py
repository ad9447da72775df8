"""TEST INFRASTRUCTURE for tests/test_gpu_lane_flush_order.py and tests/test_simt_lane_flush_order.py, which are one design: small LZ4
blocks BUILT sequence by sequence so that the lane decoder's cooperative flush (lz4hip_decode_lane4.hpp, T2a .. T2d) meets the positions
at which a reordering of its stages could go wrong, batches of 64 to 130 of them, and the comparison with the CPU codec.

The flush moves finished output from a lane's 192-byte ring to memory in units of 128 bytes, in every second iteration, and a far match
(offset > ring - 20 = 172) is fetched back from memory one and a half iterations ahead of its use.  So the shapes are
  * blocks of 127 .. 385 bytes: one unit, two units and the first wrap of the ring, each one byte short, exact, and one byte over;
  * a far match whose first 16 source bytes END one byte before, at, and one byte after a multiple of 128 of the output: the unit that holds
    them was flushed in the same iteration as the fetch or in the one before, or is not flushed yet;
  * the same with an overlapping near match (offset 1 .. 16) directly in front: the ring rows a helper lane reads while their owner appends;
  * 64 identical blocks (every lane wants to flush in the same iteration: more units than records) and 64 blocks of pairwise different
    lengths (flushing and idle lanes mixed in every iteration);
  * two blocks of every batch also truncated and corrupted: the result codes are the CPU codec's.
Every block produces at most 1 KiB."""
import numpy as np

LENGTHS = (127, 128, 129, 255, 256, 257, 383, 384, 385)
FAR_OFFSETS = (173, 174, 188, 192, 193, 256, 300)
NEAR_OFFSETS = (1, 2, 3, 4, 15, 16)
DELTAS = (-1, 0, 1)
UNIT = 128
TAIL = 12                # literals of the last sequence: the last match ends 12 bytes before the block does (lz4.c MFLIMIT)
EXTRA = 5                # spare capacity of the unknown-size decodes


def _length_bytes(n):
    out = []
    n -= 15
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def emit(seqs, tail, min_tail=TAIL):
    """the LZ4 block of the sequences (literals, offset, match length >= 4) and the last literals; returns (block, bytes it decodes to)"""
    b, out = bytearray(), bytearray()
    for lit, off, ml in seqs:
        assert ml >= 4 and 1 <= off <= len(out) + len(lit), (off, ml, len(out), len(lit))
        b.append((min(len(lit), 15) << 4) | min(ml - 4, 15))
        if len(lit) >= 15:
            b += _length_bytes(len(lit))
        b += lit
        b += bytes((off & 255, off >> 8))
        if ml - 4 >= 15:
            b += _length_bytes(ml - 4)
        out += lit
        for _ in range(ml):
            out.append(out[-off])
    assert len(tail) >= min_tail
    b.append(min(len(tail), 15) << 4)
    if len(tail) >= 15:
        b += _length_bytes(len(tail))
    b += tail
    out += tail
    return np.frombuffer(bytes(b), np.uint8).copy(), np.frombuffer(bytes(out), np.uint8).copy()


def _bytes(rng, n):
    return bytes(rng.integers(1, 256, n, dtype=np.uint8))


def prefix(rng, p):
    """(sequences, pending literals) that together produce exactly p bytes: short literal runs and near matches of mixed lengths"""
    seqs, pos = [], 0
    lit = _bytes(rng, min(p, int(rng.integers(16, 25))))
    while True:
        pos_lit = pos + len(lit)
        ml = int(rng.integers(4, 21))
        if pos_lit + ml + 4 > p:                                   # no room for another match: the rest is literals
            return seqs, lit + _bytes(rng, p - pos_lit)
        off = int(rng.integers(1, min(pos_lit, 40) + 1))
        seqs.append((lit, off, ml))
        pos = pos_lit + ml
        lit = _bytes(rng, min(p - pos, int(rng.integers(0, 10))))


def length_block(L, seed):
    """a block of exactly L bytes that ends with a short near match and the last literals"""
    rng = np.random.default_rng(seed)
    seqs, lit = prefix(rng, L - TAIL - 8)
    return emit(seqs + [(lit, 3, 8)], _bytes(rng, TAIL))


def far_block(off, delta, m, seed, near=None, far_len=18):
    """a far match of offset `off` whose first 16 source bytes end at output byte UNIT * m + delta; near: offset of an overlapping match
    of 24 bytes that ends where the far match begins"""
    rng = np.random.default_rng(seed)
    p = UNIT * m + delta - 16 + off                                # where the far match goes
    if near is None:
        seqs, lit = prefix(rng, p)
        seqs = seqs + [(lit, off, far_len)]
    else:
        seqs, lit = prefix(rng, p - 24)
        seqs = seqs + [(lit, near, 24), (b"", off, far_len)]
    return emit(seqs, _bytes(rng, TAIL))


def damaged(block, raw, k):
    """(stream, capacity) of four damaged copies: cut inside the last literals, cut in the middle, an offset that reaches before the
    block, a changed token"""
    c = block.copy()
    if k == 0:
        c = c[:c.size - 7]
    elif k == 1:
        c = c[:c.size // 2]
    elif k == 2:
        ll = int(c[0] >> 4)                                          # (the first literal run has 16 .. 24 bytes: one length byte)
        at = 1 + ll if ll < 15 else 2 + 15 + int(c[1])
        c[at:at + 2] = 255
    else:
        c[0] ^= 0x5F
    return c, raw.size


def batches():
    """name -> list of (stream, decoded bytes or None for a damaged one, output size)"""
    out = {}

    def with_damage(items):
        extra = []
        for j, i in enumerate((1, len(items) - 2)):
            for k in (2 * j, 2 * j + 1):
                c, cap = damaged(items[i][0], items[i][1], k)
                extra.append((c, None, cap))
        return [(c, raw, raw.size) for c, raw in items] + extra

    far = [far_block(o, d, m, 1000 + 10 * o + m) for o in FAR_OFFSETS for d in DELTAS for m in (1, 2)]
    far += [far_block(o, d, 3, 2000 + o, far_len=35) for o in (173, 192, 300) for d in DELTAS]
    out["lengths_and_far"] = with_damage([length_block(L, L) for L in LENGTHS] + far)                        # 9 + 42 + 9 + 4 = 64
    out["near_then_far"] = with_damage([far_block(o, d, 2, 3000 + 20 * o + n, near=n) for n in NEAR_OFFSETS for o in FAR_OFFSETS for d in DELTAS])   # 126 + 4
    out["identical"] = with_damage([far_block(192, 0, 2, 77, near=1)] * 64)                                   # 64 + 4
    out["different_lengths"] = with_damage([length_block(127 + 13 * i, 500 + i) for i in range(64)])          # 64 + 4
    for name, items in out.items():
        assert 64 <= len(items) <= 130 and all(cap <= 1024 for _, _, cap in items), name
    return out


_expected = {}


def expected(oracle, name, known):
    """(items, CPU codec's result per block, its bytes per block): computed once per batch and decoder kind, shared by every form"""
    key = (name, known)
    if key not in _expected:
        if "batches" not in _expected:
            _expected["batches"] = batches()
        items = _expected["batches"][name]
        res, outs = [], []
        for c, raw, cap in items:
            if known:
                r, o = oracle.uncompress_raw(c, cap)
            else:
                r, o = oracle.uncompress_unknown_raw(c, len(c), cap + EXTRA)
            if raw is not None:                                    # a block built here is a valid one, and decodes to what emit() said
                assert r == (len(c) if known else raw.size) and np.array_equal(o[:raw.size], raw), (name, known)
            res.append(r)
            outs.append(o)
        _expected[key] = (items, res, outs)
    return _expected[key]


def check(oracle, name, known, decode, repeat=1):
    """decode(streams, capacities, known) -> (results, rows with 64 guard bytes of 0xA5 behind the capacity); repeat: the batch is decoded
    `repeat` times over in one call (a form that only larger batches reach)"""
    items, want, outs = expected(oracle, name, known)
    # (the known-size codec takes no input length: a damaged stream runs on into the zeros the oracle's wrapper puts behind it, so here too)
    comps = [np.concatenate([c, np.zeros(cap + 1024, np.uint8)]) if known and raw is None else c for c, raw, cap in items] * repeat
    caps = [cap + (0 if known else EXTRA) for _, _, cap in items] * repeat
    res, dst = decode(comps, caps, known)
    for i in range(len(comps)):
        j = i % len(items)
        assert res[i] == want[j], (name, known, i, int(res[i]), want[j])
        if items[j][1] is not None:
            n = items[j][1].size
            assert np.array_equal(dst[i, :n], outs[j][:n]), (name, known, i)
        assert (dst[i, caps[i]:caps[i] + 64] == 0xA5).all(), (name, known, i, "wrote past the block")
