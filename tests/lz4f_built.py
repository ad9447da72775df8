"""Hand-made LZ4 blocks and frames for the tests of the ordered decode (frames with linked blocks, frames with a dictionary): a builder
of sequences and blocks that knows what they decode to, and the two sets of smallest shapes at which such a decode can go wrong.  The
model of what the decode calls make of them is tests/lz4f_ref.py.  Nothing here is shipped, and nothing here looks at the code under
test."""
import lz4f_ref as ref

DICT_LENGTHS = (1, 13, 4095, 4097, 65535, 70000)


def _length(n):
    """the bytes that extend a token's nibble of 15 by n"""
    return bytes([255] * (n // 255) + [n % 255])


def sequence(literals=b"", offset=None, match=None):
    """token, literal length bytes, literals [, offset, match length bytes]; without offset: a block's last sequence"""
    ll = len(literals)
    ml = 0 if offset is None else match - 4
    assert offset is None or (match >= 4 and 0 <= offset <= 65535)
    out = bytes([(min(ll, 15) << 4) | min(ml, 15)])
    if ll >= 15:
        out += _length(ll - 15)
    out += bytes(literals)
    if offset is not None:
        out += int(offset).to_bytes(2, "little")
        if ml >= 15:
            out += _length(ml - 15)
    return out


class Content:
    """the bytes a frame under construction decodes to: blocks are appended as they are built.  What a block may copy from is the
    dictionary and, in a linked frame, the frame's bytes so far; in an independent frame the dictionary alone"""
    def __init__(self, dictionary=b"", linked=True):
        self.dict, self.linked, self.out = bytes(dictionary), linked, bytearray()

    def raw(self, data):
        self.out += data
        return bytes(data), True

    def block(self, parts, tail):
        """a compressed block of the sequences parts = [(literals, offset, match length)] that ends in the literals `tail`, at least 12
        of them so that the format's end rules hold whatever the matches are"""
        assert len(tail) >= ref.MF_LIMIT
        window = bytearray(self.dict + (bytes(self.out) if self.linked else b""))
        base, data = len(window), b""
        for literals, offset, match in parts:
            data += sequence(literals, offset, match)
            window += literals
            assert 1 <= offset <= len(window), "a built match starts in the dictionary or the frame (the broken cases patch the bytes afterwards)"
            for _ in range(match):
                window.append(window[-offset])
        window += tail
        self.out += window[base:]
        return data + sequence(tail), False


def frame_of(blocks, linked=True, block_id=4, flags=0, content=b"", dict_id=None):
    """descriptor, the blocks [(stored bytes, raw)] behind their size fields (and in front of their checksums), EndMark, content checksum"""
    out = [ref.descriptor(block_id, flags, len(content), linked=linked, dict_id=dict_id)]
    for data, raw in blocks:
        out.append(ref.le32(len(data) | (0x80000000 if raw else 0)) + data)
        if flags & ref.F_BLOCK_CHECKSUM:
            out.append(ref.le32(ref.xxh32(data)))
    out.append(ref.le32(0))
    if flags & ref.F_CONTENT_CHECKSUM:
        out.append(ref.le32(ref.xxh32(content)))
    return b"".join(out)


def noise(n, seed):
    """n bytes without repeats worth a match (a 32-bit LCG's high bytes)"""
    out, x = bytearray(), seed * 2654435761 + 1 & 0xFFFFFFFF
    for _ in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(x >> 24)
    return bytes(out)


def _patched_offset(block, at, old, new):
    data = bytearray(block[0])
    assert int.from_bytes(data[at:at + 2], "little") == old and new <= 65535
    data[at:at + 2] = new.to_bytes(2, "little")
    return bytes(data), False


# ---- linked frames without a dictionary ------------------------------------------------------------------------------------------------
def hand_built_linked():
    """The smallest shapes at which an ordered decode can go wrong -> {name: (frame, content or None for a frame that is refused,
    index of the block that is refused or None)}"""
    cases = {}
    tail = bytes(range(100, 112))

    c = Content()                                                      # (a) a match that starts at the frame's first byte, in a raw block
    blocks = [c.raw(noise(1000, 1)), c.block([(b"", 1000, 20)], tail)]
    cases["a_first_byte"] = (frame_of(blocks), bytes(c.out), None)
    cases["a_before_the_frame"] = (frame_of([blocks[0], _patched_offset(blocks[1], 1, 1000, 1001)]), None, 1)   # (a') one byte further back

    def full_block(c, seed):                                           # 65 536 bytes: half of them literals, the other half their copy
        return c.block([(noise(32762, seed), 32762, 32762)], tail)

    c = Content()                                                      # (b) the furthest a match reaches: 65 535 back, at a block's first byte
    blocks = [full_block(c, 2), c.block([(b"", 65535, 8)], tail)]
    cases["b_offset_65535"] = (frame_of(blocks), bytes(c.out), None)

    c = Content()                                                      # (c) a source that starts in block 1, crosses raw block 2 and overlaps itself
    blocks = [full_block(c, 3), c.raw(noise(10, 4)), c.block([(b"", 20, 40), (b"xy", 65535, 5)], tail)]
    cases["c_across_a_raw_block"] = (frame_of(blocks), bytes(c.out), None)

    c = Content()                                                      # (d) the run fill out of the history
    blocks = [c.block([], noise(50, 5)), c.block([(b"", 1, 1000)], tail)]
    cases["d_run_fill"] = (frame_of(blocks), bytes(c.out), None)

    c = Content()                                                      # (e) 40 short sequences out of block 1, then a long copy
    first = c.block([], noise(4096, 6))
    parts, at = [], 0                                                  # at: the bytes of block 2 in front of the match
    for j in range(40):
        literals = bytes([65 + j % 26] * (j % 3))
        at += len(literals)
        parts.append((literals, at + 100 + 13 * j, 4 + j % 15))        # (the source: 100 + 13 j bytes before block 1's end, wholly inside it)
        at += 4 + j % 15
    parts.append((b"", 3000, 200))
    blocks = [first, c.block(parts, noise(150, 7))]
    cases["e_short_sequences"] = (frame_of(blocks), bytes(c.out), None)

    c = Content()                                                      # (f) three blocks with checksums, a byte flipped in the second
    blocks = [c.block([(b"abcdefgh", 8, 100)], tail), c.block([(b"", 50, 30)], tail), c.block([(b"", 130, 60)], tail)]
    good = frame_of(blocks, flags=ref.F_BLOCK_CHECKSUM, content=bytes(c.out))
    at = 7 + 4 + len(blocks[0][0]) + 4 + 4 + 5
    cases["f_bad_checksum"] = (good[:at] + bytes([good[at] ^ 0x40]) + good[at + 1:], None, 1)
    cases["f_good_checksums"] = (good, bytes(c.out), None)
    return cases


FRONT = b"an item in front of the case: 37 bytes"[:37]


def front_item():
    """an independent one-block frame (stored raw) that decodes to FRONT"""
    return frame_of([(FRONT, True)], linked=False)


# ---- frames whose matches start in a dictionary ----------------------------------------------------------------------------------------
def dictionary(n, seed=77):
    """n bytes without repeats worth a match, whose last byte is not the byte in front of it"""
    d = bytearray(noise(n, seed))
    if n >= 2 and d[-1] == d[-2]:
        d[-1] ^= 0x55
    return bytes(d)


def hand_built_dict(dictionary, dict_id=None):
    """The smallest shapes at which a decode with this dictionary can go wrong -> {name: (frame, content or None for a frame with a
    block that is refused, index of that block or None)}; a case the dictionary's length does not allow is left out.  Names starting
    with "i" are independent frames, with "l" linked ones."""
    d = bytes(dictionary)
    L, reach = len(d), min(len(d), ref.HISTORY)
    cases = {}
    tail = bytes(range(100, 112))

    def add(name, blocks, c, linked, refused=None):
        cases[name] = (frame_of(blocks, linked=linked, dict_id=dict_id), None if refused is not None else bytes(c.out), refused)

    # ---- independent frames: every block sees the dictionary, and only the dictionary
    c = Content(d, False)                                              # a match in block 2 that starts at the dictionary's first reachable byte
    blocks = [c.block([], noise(100, 1)), c.block([(b"", reach, 20)], tail)]
    add("i_first_byte", blocks, c, False)
    if reach < ref.HISTORY:                                            # ... and one byte further back
        add("i_before_the_dictionary", [blocks[0], _patched_offset(blocks[1], 1, reach, reach + 1)], c, False, 1)
    c = Content(d, False)                                              # from the dictionary on into the block's own bytes, overlapping itself
    k = min(reach, 3)
    add("i_into_the_block", [c.block([], noise(30, 2)), c.block([(b"xy", k + 2, 40)], tail)], c, False)
    if L >= 30:                                                        # an offset that hits block 1 in a linked frame reads the dictionary here
        c, cl = Content(d, False), Content(d, True)
        blocks = [c.block([], noise(50, 3)), c.block([(b"", 30, 20)], tail)]
        cl.block([], noise(50, 3)), cl.block([(b"", 30, 20)], tail)
        assert bytes(c.out) != bytes(cl.out), "the linked reading of the same blocks differs"
        add("i_not_the_block_before", blocks, c, False)

    # ---- linked frames
    c = Content(d, True)                                               # offset 1 at item offset 0: a run of the dictionary's last byte
    add("l_run_fill", [c.block([(b"", 1, 1000)], tail)], c, True)
    c = Content(d, True)                                               # behind a raw block, to the dictionary's first reachable byte
    far = min(1000 + L, ref.HISTORY)
    blocks = [c.raw(noise(1000, 4)), c.block([(b"", far, 20)], tail)]
    add("l_behind_a_raw_block", blocks, c, True)
    if 1000 + L < ref.HISTORY:                                         # ... and one byte further back: refused, and it keeps its place
        add("l_before_the_dictionary", [blocks[0], _patched_offset(blocks[1], 1, far, far + 1)], c, True, 1)
    c = Content(d, True)                                               # from the dictionary across a 10-byte raw block into the block itself
    blocks = [c.raw(noise(10, 5)), c.block([(b"xy", 12 + k, 40)], tail), c.block([(b"", 64 + k, 80)], tail)]
    assert len(c.out) == 64 + 92, "block 3's source starts in the dictionary too, and runs on into block 3"
    add("l_across_a_raw_block", blocks, c, True)
    c = Content(d, True)                                               # 65 000 literals, then as far back as an offset goes
    add("l_65000_literals", [c.block([(noise(65000, 6), min(65000 + L, ref.HISTORY), 8)], tail)], c, True)
    c = Content(d, True)                                               # a full block in front: the dictionary is out of reach
    blocks = [c.block([(noise(32762, 7), 32762, 32762)], tail), c.block([(b"", ref.HISTORY, 8)], tail)]
    assert len(c.out) == 65536 + 20
    add("l_out_of_reach", blocks, c, True)
    c = Content(d, True)                                               # 40 short sequences out of the dictionary, then a long copy
    parts, at, span = [], 0, min(L, 3000)
    for j in range(40):
        literals = bytes([65 + j % 26] * (j % 3))
        at += len(literals)
        parts.append((literals, at + 1 + 13 * j % span, 4 + j % 15))
        at += 4 + j % 15
    parts.append((b"", at + span, 200))
    add("l_short_sequences", [c.block(parts, noise(150, 8))], c, True)
    return cases
