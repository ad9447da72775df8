"""Test-side twin of the decode of LZ4 frames WITH A DICTIONARY (lz4hip_lz4f_decode_dict_* and lz4hip_lz4f_batch_decode_dict_*,
include/lz4hip.h), on top of tests/lz4f_linked_ref.py and tests/lz4f_ref.py: the from-the-spec block decoder there already takes bytes
in front of the output.  The model is LZ4F_decompress_usingDict's: ONE dictionary per call, in front of every frame's first byte;
history = (dictionary + output)[-65535:] for the blocks of a linked frame, dictionary[-65535:] for every block of an independent one.
A builder of hand-made frames whose matches start in a dictionary.  Nothing here is shipped, and nothing here looks at the code under
test."""
import lz4f_linked_ref as lk
import lz4f_ref as ref

REACH = 65535
DICT_ID_MISMATCH = 14
DICT_LENGTHS = (1, 13, 4095, 4097, 65535, 70000)


def dictionary(n, seed=77):
    """n bytes without repeats worth a match, whose last byte is not the byte in front of it"""
    d = bytearray(lk.noise(n, seed))
    if n >= 2 and d[-1] == d[-2]:
        d[-1] ^= 0x55
    return bytes(d)


class _DictCodec:
    """the block decoder of an independent frame's rows for lz4f_ref.read_frame: every block behind the dictionary's reachable bytes"""
    def __init__(self, tail):
        self.tail = tail

    def uncompress_unknown_raw(self, data, size, cap):
        res, out = lk.decode_block(bytes(data[:size]), cap, self.tail)
        return res, out


def _without_id(frame, h):
    """the same frame with FLG.0 clear, the ID gone and HC recomputed: the readers of the plain calls walk it, four bytes early"""
    d = bytearray(frame[4:h["pos"] - 5])
    d[0] &= 0xFE
    return frame[:4] + bytes(d) + bytes([(ref.xxh32(d) >> 8) & 0xFF]) + frame[h["pos"]:]


def _linked(frame, tail, slot_bytes, max_blocks, verify, room):
    """lz4f_linked_ref.read_frame_linked's model of a linked frame, with `tail` in front of the frame's first byte"""
    walk, _, wrows = ref.read_frame(lk._NoCodec, lk._unlinked(frame), slot_bytes, max_blocks, 0)
    info = dict(walk, flg=frame[4], decoded_bytes=0, good_bytes=0)
    flg, block_max = frame[4], walk["block_max"]
    info["checks"] = ((ref.SKIPPED if not verify & ref.V_BLOCKS else ref.VERIFIED) if flg & 0x10 else ref.ABSENT) | \
        ((ref.SKIPPED if flg & 0x04 else ref.ABSENT) << 2)
    if walk["error"] == ref.SLOT_TOO_SMALL:
        return info, b"", False
    walk_ok = walk["error"] in (ref.OK, ref.CONTENT_SIZE)
    if walk["error"] == ref.CONTENT_SIZE:
        info.update(error=ref.OK, error_offset=-1)
    sum_bytes = 4 if flg & 0x10 else 0
    plan, badsums, bad = [], [], None
    for k, (at, size, raw, _, _, _) in enumerate(wrows):
        data = frame[at:at + size]
        badsum = bool(sum_bytes and verify & ref.V_BLOCKS and ref.xxh32(data) != int.from_bytes(frame[at + size:at + size + 4], "little"))
        n = -1 if badsum else (size if raw else lk.size_block(data))
        if bad is None and (n < 0 or n > block_max):
            bad = k
        plan.append(0 if bad is not None else n)
        badsums.append(badsum)
    total = sum(plan)
    if room is None:
        room = total
    out = bytearray()
    refused = False
    for k, (at, size, raw, _, _, _) in enumerate(wrows):
        if k == bad or len(out) + plan[k] > room:
            break
        data = frame[at:at + size]
        if raw:
            out += data
            continue
        res, got = lk.decode_block(data, plan[k], (tail + bytes(out))[-REACH:])
        if res != plan[k]:
            bad, refused = k, True
            break
        out += got
    info.update(decoded_bytes=total, good_bytes=total)
    if walk["error"] == ref.TABLE_FULL:
        pass
    elif bad is not None:
        info.update(error=ref.BLOCK_CHECKSUM if badsums[bad] else ref.CORRUPT_BLOCK, error_offset=wrows[bad][0] - 4, good_bytes=sum(plan[:bad]))
    elif walk_ok and walk["content_size"] >= 0 and walk["content_size"] != total:
        info.update(error=ref.CONTENT_SIZE, error_offset=6)
    if info["error"] == ref.OK and flg & 0x04 and verify & ref.V_CONTENT and total <= room:
        info["checks"] = (info["checks"] & 3) | (ref.VERIFIED << 2)
        trailer = walk["frame_bytes"] - 4
        if ref.xxh32(bytes(out)) != int.from_bytes(frame[trailer:trailer + 4], "little"):
            info.update(error=ref.CONTENT_CHECKSUM, error_offset=trailer)
    return info, bytes(out), refused


def read_frame_dict(frame, dictionary, dict_id=0, slot_bytes=65536, max_blocks=1 << 30, verify=3, accept_linked=True, room=None):
    """What ONE frame at the start of `frame` is to the dictionary calls with a dictionary of at least one byte, `room` bytes of dst_cap
    being left at the item's first byte (None: all it needs; may be negative) -> (info dict, the item's bytes that are written and
    specified, whether the item's bytes behind them are unspecified)."""
    frame, tail = bytes(frame), bytes(dictionary)[-REACH:]
    assert tail, "without a dictionary the call is the plain call"
    cap = None if room is None else max(room, -1)
    framed = len(frame) >= 7 and int.from_bytes(frame[:4], "little") == ref.MAGIC
    h = ref.parse_header(frame) if framed else None
    if not framed or h["error"] != ref.OK:                             # what comes before the dictionary check is the plain calls'
        info, out, _ = ref.read_frame(None, frame, slot_bytes, max_blocks, verify, cap)
        return info, out, False
    with_id = bool(frame[4] & 0x01)
    if with_id and dict_id and int.from_bytes(frame[h["pos"] - 5:h["pos"] - 1], "little") != dict_id:
        info, _, _ = ref.read_frame(None, frame, slot_bytes, max_blocks, verify, cap)
        assert info["error"] == ref.UNSUPPORTED_DICT
        return dict(info, error=DICT_ID_MISMATCH, error_offset=h["pos"] - 5), b"", False
    plain = _without_id(frame, h) if with_id else frame
    if frame[4] & 0x20 or not accept_linked:
        info, out, _ = ref.read_frame(_DictCodec(tail), plain, slot_bytes, max_blocks, verify, cap)
        out, unspecified = (b"" if cap == -1 else out), False
    else:
        info, out, unspecified = _linked(plain, tail, slot_bytes, max_blocks, verify, room)
    if with_id:                                                        # the four bytes of the ID lie behind offset 6 (or 14)
        info = dict(info, flg=frame[4], frame_bytes=info["frame_bytes"] + 4,
                    error_offset=info["error_offset"] + 4 if info["error_offset"] >= 7 else info["error_offset"])
    return info, out, unspecified


# ---- hand-made frames ------------------------------------------------------------------------------------------------------------------
class Content:
    """lz4f_linked_ref.Content with a dictionary in front: what a block under construction may copy from is the dictionary and, in a
    linked frame, the frame's bytes so far; in an independent frame the dictionary alone"""
    def __init__(self, dictionary, linked):
        self.dict, self.linked, self.out = bytes(dictionary), linked, bytearray()

    def raw(self, data):
        self.out += data
        return bytes(data), True

    def block(self, parts, tail):
        assert len(tail) >= lk.MF_LIMIT
        window = bytearray(self.dict + (bytes(self.out) if self.linked else b""))
        base, data = len(window), b""
        for literals, offset, match in parts:
            data += lk.sequence(literals, offset, match)
            window += literals
            assert 1 <= offset <= min(len(window), REACH), "a built match starts in the dictionary or behind it"
            for _ in range(match):
                window.append(window[-offset])
        window += tail
        self.out += window[base:]
        return data + lk.sequence(tail), False


def _patched_offset(block, at, old, new):
    data = bytearray(block[0])
    assert int.from_bytes(data[at:at + 2], "little") == old and new <= 65535
    data[at:at + 2] = new.to_bytes(2, "little")
    return bytes(data), False


def hand_built(dictionary, dict_id=None):
    """The smallest shapes at which a decode with this dictionary can go wrong -> {name: (frame, content or None for a frame with a
    block that is refused, index of that block or None)}; a case the dictionary's length does not allow is left out.  Names starting
    with "i" are independent frames, with "l" linked ones."""
    d = bytes(dictionary)
    L, reach = len(d), min(len(d), REACH)
    cases = {}
    tail = bytes(range(100, 112))

    def add(name, blocks, c, linked, refused=None):
        cases[name] = (lk.frame_of(blocks, linked=linked, dict_id=dict_id), None if refused is not None else bytes(c.out), refused)

    # ---- independent frames: every block sees the dictionary, and only the dictionary
    c = Content(d, False)                                              # a match in block 2 that starts at the dictionary's first reachable byte
    blocks = [c.block([], lk.noise(100, 1)), c.block([(b"", reach, 20)], tail)]
    add("i_first_byte", blocks, c, False)
    if reach < REACH:                                                  # ... and one byte further back
        add("i_before_the_dictionary", [blocks[0], _patched_offset(blocks[1], 1, reach, reach + 1)], c, False, 1)
    c = Content(d, False)                                              # from the dictionary on into the block's own bytes, overlapping itself
    k = min(reach, 3)
    add("i_into_the_block", [c.block([], lk.noise(30, 2)), c.block([(b"xy", k + 2, 40)], tail)], c, False)
    if L >= 30:                                                        # an offset that hits block 1 in a linked frame reads the dictionary here
        c, cl = Content(d, False), Content(d, True)
        blocks = [c.block([], lk.noise(50, 3)), c.block([(b"", 30, 20)], tail)]
        cl.block([], lk.noise(50, 3)), cl.block([(b"", 30, 20)], tail)
        assert bytes(c.out) != bytes(cl.out), "the linked reading of the same blocks differs"
        add("i_not_the_block_before", blocks, c, False)

    # ---- linked frames
    c = Content(d, True)                                               # offset 1 at item offset 0: a run of the dictionary's last byte
    add("l_run_fill", [c.block([(b"", 1, 1000)], tail)], c, True)
    c = Content(d, True)                                               # behind a raw block, to the dictionary's first reachable byte
    far = min(1000 + L, REACH)
    blocks = [c.raw(lk.noise(1000, 4)), c.block([(b"", far, 20)], tail)]
    add("l_behind_a_raw_block", blocks, c, True)
    if 1000 + L < REACH:                                               # ... and one byte further back: refused, and it keeps its place
        add("l_before_the_dictionary", [blocks[0], _patched_offset(blocks[1], 1, far, far + 1)], c, True, 1)
    c = Content(d, True)                                               # from the dictionary across a 10-byte raw block into the block itself
    blocks = [c.raw(lk.noise(10, 5)), c.block([(b"xy", 12 + k, 40)], tail), c.block([(b"", 64 + k, 80)], tail)]
    assert len(c.out) == 64 + 92, "block 3's source starts in the dictionary too, and runs on into block 3"
    add("l_across_a_raw_block", blocks, c, True)
    c = Content(d, True)                                               # 65 000 literals, then as far back as an offset goes
    add("l_65000_literals", [c.block([(lk.noise(65000, 6), min(65000 + L, REACH), 8)], tail)], c, True)
    c = Content(d, True)                                               # a full block in front: the dictionary is out of reach
    blocks = [c.block([(lk.noise(32762, 7), 32762, 32762)], tail), c.block([(b"", REACH, 8)], tail)]
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
    add("l_short_sequences", [c.block(parts, lk.noise(150, 8))], c, True)
    return cases


FRONT = lk.FRONT


def front_item():
    return lk.front_item()
