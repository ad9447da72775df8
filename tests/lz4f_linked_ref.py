"""Test-side twin of the decode of LZ4 frames with LINKED blocks (LZ4HIP_LZ4F_ACCEPT_LINKED, include/lz4hip.h), on top of
tests/lz4f_ref.py: a from-the-spec LZ4 block decoder and size walk with a history argument, a reader that models what the flag
promises (the outcomes, good_bytes, bad blocks that end an item, the clip at a block boundary), and a builder of hand-made blocks and
frames.  Nothing here is shipped, and nothing here looks at the code under test."""
import lz4f_ref as ref

HISTORY = 65535
ACCEPT_LINKED = 8
MF_LIMIT, LAST_LITERALS = 12, 5


# ---- blocks: the reference's LZ4_uncompress_unknownOutputSize with bytes in front of the output ------------------------------------------
def _at(data, i):
    return data[i] if i < len(data) else 0


def size_block(data, history=HISTORY):
    """What the block decodes to when its output limit never binds and `history` bytes lie in front of it, or -(error position)."""
    data = bytes(data)
    iend, ip, produced = len(data), 0, 0
    if iend == 0:
        return 0
    while True:
        token = data[ip]
        ip += 1
        ll = token >> 4
        if ll == 15:
            b = 255
            while ip < iend and b == 255:
                b = data[ip]
                ip += 1
                ll += b
        if ip + ll > iend - 8:
            return produced + ll if ip + ll == iend else -ip
        produced += ll
        ip += ll
        off = _at(data, ip) | _at(data, ip + 1) << 8
        ip += 2
        if off > produced + history:
            return -ip
        ml = token & 15
        if ml == 15:
            while ip < iend - 6:
                b = data[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        produced += ml + 4


def decode_block(data, cap, history=b""):
    """The block decoded into `cap` bytes of room behind the bytes `history` -> (bytes produced or -(error position), the bytes).
    A match may start in the history; one that starts before it is an error, and so is a block that breaks the end rules at cap."""
    data, hist = bytes(data), len(history)
    out = bytearray(history)
    iend, ip = len(data), 0
    if iend == 0:
        return 0, b""
    while True:
        token = data[ip]
        ip += 1
        ll = token >> 4
        if ll == 15:
            b = 255
            while ip < iend and b == 255:
                b = data[ip]
                ip += 1
                ll += b
        lit_end = len(out) - hist + ll
        if lit_end > cap - MF_LIMIT or ip + ll > iend - 8:
            if lit_end > cap or ip + ll != iend:
                return -ip, bytes(out[hist:])
            out += data[ip:ip + ll]
            return lit_end, bytes(out[hist:])
        out += data[ip:ip + ll]
        ip += ll
        off = _at(data, ip) | _at(data, ip + 1) << 8
        ip += 2
        if off > len(out):
            return -ip, bytes(out[hist:])
        ml = token & 15
        if ml == 15:
            while ip < iend - 6:
                b = data[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if lit_end + ml > cap - LAST_LITERALS:
            return -ip, bytes(out[hist:])
        if off == 0:                                                   # (only in corrupt streams: the bytes are whatever dst held)
            out += bytes(ml)
        elif off >= ml:
            start = len(out) - off
            out += out[start:start + ml]
        else:
            for _ in range(ml):
                out.append(out[-off])


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
class _NoCodec:
    """the walk of lz4f_ref.read_frame alone: every compressed row decodes to nothing"""
    @staticmethod
    def uncompress_unknown_raw(data, size, cap):
        return 0, b""


def is_linked(frame):
    """a frame (not a skippable one) whose descriptor parses, with FLG.5 clear and no dictionary ID"""
    frame = bytes(frame)
    if len(frame) < 7 or int.from_bytes(frame[:4], "little") != ref.MAGIC:
        return False
    h = ref.parse_header(frame)
    return h["error"] == ref.OK and not h["flg"] & 0x20 and not h["flg"] & 0x01


def _unlinked(frame):
    """the same frame with FLG.5 set and HC recomputed: lz4f_ref.read_frame walks it"""
    h = ref.parse_header(frame)
    d = bytearray(frame[4:h["pos"] - 1])
    d[0] |= 0x20
    return frame[:4] + bytes(d) + bytes([(ref.xxh32(d) >> 8) & 0xFF]) + frame[h["pos"]:]


def read_frame_linked(oracle, frame, slot_bytes=4 << 20, max_blocks=1 << 30, verify=ref.V_BLOCKS | ref.V_CONTENT, room=None):
    """What ONE frame at the start of `frame` is to the decode calls with LZ4HIP_LZ4F_ACCEPT_LINKED, `room` bytes of dst_cap being left
    at the item's first byte (None: all it needs; may be negative) -> (info dict, the item's bytes that are written and specified,
    whether the item's bytes behind them are unspecified, rows as lz4f_ref.read_frame's).  A frame that is not linked is
    lz4f_ref.read_frame's, clipped byte-exact; the rows of a linked one are empty rows to the ring decoder."""
    frame = bytes(frame)
    if not is_linked(frame):
        cap = None if room is None else max(room, -1)                 # (-1: no byte of the item lies inside dst_cap)
        info, out, rows = ref.read_frame(oracle, frame, slot_bytes, max_blocks, verify, cap)
        return info, b"" if cap == -1 else out, False, rows
    # the walk: descriptor, size fields, table
    walk, _, wrows = ref.read_frame(_NoCodec, _unlinked(frame), slot_bytes, max_blocks, 0)
    info = dict(walk, flg=frame[4], decoded_bytes=0, good_bytes=0)
    flg, block_max = frame[4], walk["block_max"]
    info["checks"] = ((ref.SKIPPED if not verify & ref.V_BLOCKS else ref.VERIFIED) if flg & 0x10 else ref.ABSENT) | \
        ((ref.SKIPPED if flg & 0x04 else ref.ABSENT) << 2)
    if walk["error"] == ref.SLOT_TOO_SMALL:
        return info, b"", False, []
    walk_ok = walk["error"] in (ref.OK, ref.CONTENT_SIZE)              # (CONTENT_SIZE: the stand-in's sizes, looked at again below)
    if walk["error"] == ref.CONTENT_SIZE:
        info.update(error=ref.OK, error_offset=-1)
    sum_bytes = 4 if flg & 0x10 else 0
    # the plan: every row's size before anything is decoded; the first bad row ends the item
    rows, plan, badsums, bad = [], [], [], None
    for k, (at, size, raw, _, _, _) in enumerate(wrows):
        data = frame[at:at + size]
        badsum = bool(sum_bytes and verify & ref.V_BLOCKS and ref.xxh32(data) != int.from_bytes(frame[at + size:at + size + 4], "little"))
        n = -1 if badsum else (size if raw else size_block(data))
        if bad is None and (n < 0 or n > block_max):
            bad = k
        plan.append(0 if bad is not None else n)
        badsums.append(badsum)
        rows.append((at, size, True, badsum, 0, b""))                  # (raw or not, the ring decoder is handed an empty row)
    total = sum(plan)
    if room is None:
        room = total
    # the decode: live rows in order, each wholly inside the room or not at all
    out = bytearray()
    refused = False
    for k, (at, size, raw, _, _, _) in enumerate(wrows):
        if k == bad or len(out) + plan[k] > room:
            break
        data = frame[at:at + size]
        if raw:
            out += data
            continue
        res, got = decode_block(data, plan[k], bytes(out[-HISTORY:]))
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
    return info, bytes(out), refused, rows


# ---- hand-made blocks and frames -------------------------------------------------------------------------------------------------------
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
    """the bytes a frame under construction decodes to: blocks are appended as they are built"""
    def __init__(self):
        self.out = bytearray()

    def raw(self, data):
        self.out += data
        return bytes(data), True

    def block(self, parts, tail):
        """a compressed block of the sequences parts = [(literals, offset, match length)] that ends in the literals `tail`, at least 12
        of them so that the format's end rules hold whatever the matches are"""
        assert len(tail) >= MF_LIMIT
        data = b""
        for literals, offset, match in parts:
            data += sequence(literals, offset, match)
            self.out += literals
            assert 1 <= offset <= len(self.out), "a built match starts inside the frame (the broken cases patch the bytes afterwards)"
            for _ in range(match):
                self.out.append(self.out[-offset])
        self.out += tail
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


def hand_built():
    """The smallest shapes at which an ordered decode can go wrong -> {name: (frame, content or None for a frame that is refused,
    index of the block that is refused or None)}"""
    cases = {}
    tail = bytes(range(100, 112))

    c = Content()                                                      # (a) a match that starts at the frame's first byte, in a raw block
    blocks = [c.raw(noise(1000, 1)), c.block([(b"", 1000, 20)], tail)]
    cases["a_first_byte"] = (frame_of(blocks), bytes(c.out), None)
    data = bytearray(blocks[1][0])                                     # (a') one byte further back: before the frame
    assert int.from_bytes(data[1:3], "little") == 1000
    data[1:3] = (1001).to_bytes(2, "little")
    cases["a_before_the_frame"] = (frame_of([blocks[0], (bytes(data), False)]), None, 1)

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
