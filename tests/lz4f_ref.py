"""Test-side twin of the LZ4 frame path (LZ4 Frame format v1.6.x): a from-the-spec xxHash32, a frame writer over the oracle's block
encoder, a from-the-spec LZ4 block decoder and size walk with a history argument, and ONE frame reader.  The reader models what the
decode calls promise of one frame (lz4hip_lz4f_decode_* and lz4hip_lz4f_batch_decode_*, with and without LZ4HIP_LZ4F_ACCEPT_LINKED, and
their _dict_ forms, include/lz4hip.h): the outcomes, their precedence, bad blocks, clipping.  The dictionary's model is
LZ4F_decompress_usingDict's: ONE dictionary per call, in front of every frame's first byte.  Nothing here is shipped, and nothing here
looks at the code under test."""
import struct

import numpy as np

MAGIC = 0x184D2204
SKIPPABLE = 0x184D2A50
P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
M = 0xFFFFFFFF

(OK, BAD_MAGIC, BAD_HEADER, HEADER_CHECKSUM, UNSUPPORTED_LINKED, UNSUPPORTED_DICT, SLOT_TOO_SMALL, TRUNCATED, BAD_BLOCK_SIZE, CORRUPT_BLOCK,
 BLOCK_CHECKSUM, CONTENT_SIZE, CONTENT_CHECKSUM, TABLE_FULL, DICT_ID_MISMATCH) = range(15)
F_BLOCK_CHECKSUM, F_CONTENT_CHECKSUM, F_CONTENT_SIZE = 1, 2, 4
V_BLOCKS, V_CONTENT, ACCEPT_LINKED = 1, 2, 8
ABSENT, VERIFIED, SKIPPED = 0, 1, 2
HISTORY = 65535                                                        # the bytes in front of a block that a match may reach
MF_LIMIT, LAST_LITERALS = 12, 5


def xxh32(data, seed=0):
    data = bytes(data)
    n = len(data)
    words = struct.unpack("<%dI" % (n // 4), data[:n // 4 * 4])
    i = 0
    if n >= 16:
        v1, v2, v3, v4 = (seed + P1 + P2) & M, (seed + P2) & M, seed & M, (seed - P1) & M
        for i in range(0, n // 16 * 4, 4):
            v1 = (v1 + words[i] * P2) & M
            v1 = (((v1 << 13) | (v1 >> 19)) & M) * P1 & M
            v2 = (v2 + words[i + 1] * P2) & M
            v2 = (((v2 << 13) | (v2 >> 19)) & M) * P1 & M
            v3 = (v3 + words[i + 2] * P2) & M
            v3 = (((v3 << 13) | (v3 >> 19)) & M) * P1 & M
            v4 = (v4 + words[i + 3] * P2) & M
            v4 = (((v4 << 13) | (v4 >> 19)) & M) * P1 & M
        h = (((v1 << 1) | (v1 >> 31)) + ((v2 << 7) | (v2 >> 25)) + ((v3 << 12) | (v3 >> 20)) + ((v4 << 18) | (v4 >> 14))) & M
        i = n // 16 * 4
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    for w in words[i:]:
        h = (h + w * P3) & M
        h = (((h << 17) | (h >> 15)) & M) * P4 & M
    for b in data[n // 4 * 4:]:
        h = (h + b * P5) & M
        h = (((h << 11) | (h >> 21)) & M) * P1 & M
    h ^= h >> 15
    h = h * P2 & M
    h ^= h >> 13
    h = h * P3 & M
    h ^= h >> 16
    return h


def block_bytes(block_id):
    return 1 << (8 + 2 * block_id)


def le32(v):
    return int(v).to_bytes(4, "little")


def descriptor(block_id=4, flags=0, content_size=0, linked=False, dict_id=None):
    """magic + FLG + BD [+ content size] [+ dictID] + HC; the content size is written only for a non-empty source"""
    flg = 0x40 | (0 if linked else 0x20) | (0x10 if flags & F_BLOCK_CHECKSUM else 0) | (0x04 if flags & F_CONTENT_CHECKSUM else 0)
    body = b""
    if flags & F_CONTENT_SIZE and content_size > 0:
        flg |= 0x08
        body += int(content_size).to_bytes(8, "little")
    if dict_id is not None:
        flg |= 0x01
        body += le32(dict_id)
    d = bytes([flg, block_id << 4]) + body
    return le32(MAGIC) + d + bytes([(xxh32(d) >> 8) & 0xFF])


def cut(src, block_id):
    bs = block_bytes(block_id)
    src = bytes(src)
    return [src[i:i + bs] for i in range(0, len(src), bs)]


def encode_block(oracle, block, hc):
    """the format library's rule: the encoder gets len - 1 bytes of room, a block that does not fit is stored raw -> (ret, bytes)"""
    a = np.frombuffer(block, np.uint8)
    ret, out = oracle.compress_raw(a, len(block) - 1, hc)
    ret = ret if 0 < ret < len(block) else 0
    return ret, bytes(out[:ret])


def write_frame(oracle, src, block_id=4, hc=False, flags=0):
    """-> (frame, [per block: the encoder's result (0: stored raw)], [its bytes])"""
    src = bytes(src)
    out = [descriptor(block_id, flags, len(src))]
    rets, datas = [], []
    for block in cut(src, block_id):
        ret, comp = encode_block(oracle, block, hc)
        rets.append(ret)
        datas.append(comp)
        stored = comp if ret else block
        out.append(le32(len(stored) | (0 if ret else 0x80000000)) + stored)
        if flags & F_BLOCK_CHECKSUM:
            out.append(le32(xxh32(stored)))
    out.append(le32(0))
    if flags & F_CONTENT_CHECKSUM:
        out.append(le32(xxh32(src)))
    return b"".join(out), rets, datas


def skippable(payload, nibble=0):
    return le32(SKIPPABLE + nibble) + le32(len(payload)) + bytes(payload)


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
def parse_header(frame):
    """-> dict(error, error_offset, flg, bd, block_max, content_size, dict_id (None: the descriptor has none), pos) for a frame that
    starts with the frame magic; the dictionary ID's own offset is pos - 5"""
    h = dict(error=OK, error_offset=-1, flg=0, bd=0, block_max=0, content_size=-1, dict_id=None, pos=0)
    n = len(frame)
    if n < 7:
        return dict(h, error=TRUNCATED, error_offset=4)
    flg, bd = frame[4], frame[5]
    h.update(flg=flg, bd=bd)
    bid = (bd >> 4) & 7
    dlen = 3 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
    if (flg >> 6) != 1 or flg & 0x02 or bd & 0x8F or bid < 4:
        return dict(h, error=BAD_HEADER, error_offset=4)
    if 4 + dlen > n:
        return dict(h, error=TRUNCATED, error_offset=4)
    if frame[4 + dlen - 1] != (xxh32(frame[4:4 + dlen - 1]) >> 8) & 0xFF:
        return dict(h, error=HEADER_CHECKSUM, error_offset=4 + dlen - 1)
    h["block_max"] = block_bytes(bid)
    if flg & 0x08:
        h["content_size"] = int.from_bytes(frame[6:14], "little")
    if flg & 0x01:
        h["dict_id"] = int.from_bytes(frame[dlen - 1:dlen + 3], "little")
    h["pos"] = 4 + dlen
    return h


def is_linked(frame):
    """a frame (not a skippable one) whose descriptor parses, with FLG.5 clear and no dictionary ID"""
    frame = bytes(frame)
    if len(frame) < 7 or int.from_bytes(frame[:4], "little") != MAGIC:
        return False
    h = parse_header(frame)
    return h["error"] == OK and not h["flg"] & 0x20 and not h["flg"] & 0x01


def read_frame(codec, frame, slot_bytes=4 << 20, max_blocks=1 << 30, verify=V_BLOCKS | V_CONTENT, room=None, accept_linked=False, dictionary=b"",
               dict_id=0):
    """What ONE frame at the start of `frame` is to the decode calls, `room` bytes of dst_cap being left at the item's first byte (None:
    all it needs; may be negative) -> (info dict, the item's bytes that are written and specified, whether the item's bytes behind them
    are unspecified, rows).  accept_linked: the call's LZ4HIP_LZ4F_ACCEPT_LINKED; dictionary, dict_id: those of the _dict_ calls, b"" for
    the plain calls.  Every offset is the offset in `frame`.
      An independent frame's blocks decode each behind dictionary[-65535:], into slot_bytes; a bad block takes no bytes, the blocks
    behind it are decoded all the same, and the output is clipped byte-exact at the room.  `codec` decodes them where there is no
    dictionary (the oracle); behind a dictionary it is decode_block above.
      A linked frame's blocks decode in order behind (dictionary + output)[-65535:], each wholly inside the room or not at all; the first
    bad block ends the item, and one that only the decoder refuses keeps its place (decoded_bytes against good_bytes), its bytes
    unspecified.
      rows: per table row (stored offset, stored length, raw, bad checksum, the decoder's result at slot_bytes, its bytes) -- what the
    emulator's stand-in codec hands out; a linked frame's rows are empty rows to it."""
    frame, tail = bytes(frame), bytes(dictionary)[-HISTORY:]
    n = len(frame)
    info = dict(blocks=0, decoded_bytes=0, good_bytes=0, error_offset=-1, content_size=-1, frame_bytes=0, error=OK, kind=0, block_max=0,
                flg=0, bd=0, checks=0)

    def refused(error, error_offset):
        return dict(info, error=error, error_offset=error_offset), b"", False, []

    if n < 4:
        return refused(BAD_MAGIC, 0)
    magic = int.from_bytes(frame[:4], "little")
    if magic & 0xFFFFFFF0 == SKIPPABLE:
        info["kind"] = 1
        if n < 8:
            return refused(TRUNCATED, 4)
        end = 8 + int.from_bytes(frame[4:8], "little")
        info["frame_bytes"] = end
        return refused(TRUNCATED, 4) if end > n else (info, b"", False, [])
    if magic != MAGIC:
        return refused(BAD_MAGIC, 0)
    h = parse_header(frame)
    info.update(flg=h["flg"], bd=h["bd"], block_max=h["block_max"], content_size=h["content_size"])
    if h["error"] != OK:
        return refused(h["error"], h["error_offset"])
    flg, block_max = h["flg"], h["block_max"]
    pos = h["pos"]
    linked = not flg & 0x20
    info["frame_bytes"] = pos
    info["checks"] = ((SKIPPED if not verify & V_BLOCKS else VERIFIED) if flg & 0x10 else ABSENT) | ((SKIPPED if flg & 0x04 else ABSENT) << 2)
    if flg & 0x01 and not tail:
        return refused(UNSUPPORTED_DICT, 4)
    if flg & 0x01 and dict_id and h["dict_id"] != dict_id:
        return refused(DICT_ID_MISMATCH, pos - 5)
    if linked and not accept_linked:
        return refused(UNSUPPORTED_LINKED, 4)
    if block_max > slot_bytes:
        return refused(SLOT_TOO_SMALL, 5)
    # the walk: size fields, table
    sum_bytes = 4 if flg & 0x10 else 0
    blocks, walk_err, walk_off, full_off, trailer = [], OK, -1, -1, -1
    while True:
        if pos + 4 > n:
            walk_err, walk_off = TRUNCATED, pos
            break
        field = int.from_bytes(frame[pos:pos + 4], "little")
        if field == 0:
            pos += 4
            if flg & 0x04:
                if pos + 4 > n:
                    walk_err, walk_off = TRUNCATED, pos
                    break
                trailer = pos
                pos += 4
            break
        size = field & 0x7FFFFFFF
        if size > block_max:
            walk_err, walk_off = BAD_BLOCK_SIZE, pos
            break
        if pos + 4 + size + sum_bytes > n:
            walk_err, walk_off = TRUNCATED, pos
            break
        if len(blocks) == max_blocks and full_off < 0:
            full_off = pos
        blocks.append((pos, size, bool(field >> 31)))
        pos += 4 + size + sum_bytes
    info.update(blocks=len(blocks), frame_bytes=pos, error=walk_err, error_offset=walk_off)
    # the plan: every row's size before a linked block is decoded; the first bad row ends a linked item, and takes no bytes of any
    rows, plan, parts, bad = [], [], [], None
    for k, (at, size, raw) in enumerate(blocks[:max_blocks]):
        data = frame[at + 4:at + 4 + size]
        badsum = bool(sum_bytes and verify & V_BLOCKS and xxh32(data) != int.from_bytes(frame[at + 4 + size:at + 8 + size], "little"))
        res, got = 0, b""
        if linked:
            sized = size if raw else size_block(data)
            rows.append((at + 4, size, True, badsum, 0, b""))          # (raw or not, the ring decoder is handed an empty row)
        else:
            if not raw and not badsum:
                res, got = decode_block(data, slot_bytes, tail) if tail else codec.uncompress_unknown_raw(np.frombuffer(data, np.uint8), size, slot_bytes)
                got = bytes(got[:max(res, 0)])
            sized = size if raw else res
            rows.append((at + 4, size, raw, badsum, res, got))
        good = not badsum and 0 <= sized <= block_max
        if not good and bad is None:
            bad = k
        live = good and not (linked and bad is not None)
        plan.append(sized if live else 0)
        if live and not linked:
            parts.append(data if raw else got)
    total = sum(plan)
    if room is None:
        room = total
    # the decode: an independent frame's bytes are there, to be clipped; a linked frame's live rows go in order, each wholly inside the
    # room or not at all
    out, unspecified = bytearray(b"".join(parts)[:max(room, 0)]), False
    assert linked or total == sum(len(p) for p in parts), "a block decoder's result is the number of its bytes"
    for k, (at, size, raw) in enumerate(blocks[:max_blocks] if linked else ()):
        if k == bad or len(out) + plan[k] > room:
            break
        data = frame[at + 4:at + 4 + size]
        if raw:
            out += data
            continue
        res, got = decode_block(data, plan[k], (tail + bytes(out))[-HISTORY:])
        if res != plan[k]:
            bad, unspecified = k, True
            break
        out += got
    info.update(decoded_bytes=total, good_bytes=total)
    if len(blocks) > max_blocks:
        info.update(error=TABLE_FULL, error_offset=full_off)
    elif bad is not None:
        info.update(error=BLOCK_CHECKSUM if rows[bad][3] else CORRUPT_BLOCK, error_offset=blocks[bad][0], good_bytes=sum(plan[:bad]))
    elif walk_err == OK and h["content_size"] >= 0 and h["content_size"] != total:
        info.update(error=CONTENT_SIZE, error_offset=6)
    if info["error"] == OK and flg & 0x04 and verify & V_CONTENT and total <= room:
        info["checks"] = (info["checks"] & 3) | (VERIFIED << 2)
        if xxh32(bytes(out)) != int.from_bytes(frame[trailer:trailer + 4], "little"):
            info.update(error=CONTENT_CHECKSUM, error_offset=trailer)
    return info, bytes(out), unspecified, rows


# ---- the sources of tests/golden/lz4f_frames.json (only the frames are stored) ---------------------------------------------------------
def golden_source(oracle, kind, n):
    """"formula": in[i] = (u8)((i * 2654435761u) >> 24); "d2" / "d3": the oracle's generators, seed 11, from block 0"""
    if kind == "formula":
        i = np.arange(n, dtype=np.uint64)
        return (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.uint8).tobytes()
    return oracle.gen({"d2": 2, "d3": 3}[kind], 11, 0, (n + 65535) // 65536 or 1).reshape(-1)[:n].tobytes()
