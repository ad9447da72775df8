"""Test-side twin of the LZ4 frame path (LZ4 Frame format v1.6.x): a from-the-spec xxHash32, a frame writer and a frame reader over
the oracle's block codec.  The reader models what lz4hip_lz4f_decode_device promises (include/lz4hip.h): the outcomes, their
precedence, bad blocks that take no bytes, clipping.  Nothing here is shipped, and nothing here looks at the code under test."""
import struct

import numpy as np

MAGIC = 0x184D2204
SKIPPABLE = 0x184D2A50
P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
M = 0xFFFFFFFF

(OK, BAD_MAGIC, BAD_HEADER, HEADER_CHECKSUM, UNSUPPORTED_LINKED, UNSUPPORTED_DICT, SLOT_TOO_SMALL, TRUNCATED, BAD_BLOCK_SIZE, CORRUPT_BLOCK,
 BLOCK_CHECKSUM, CONTENT_SIZE, CONTENT_CHECKSUM, TABLE_FULL) = range(14)
F_BLOCK_CHECKSUM, F_CONTENT_CHECKSUM, F_CONTENT_SIZE = 1, 2, 4
V_BLOCKS, V_CONTENT = 1, 2
ABSENT, VERIFIED, SKIPPED = 0, 1, 2


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


def parse_header(frame):
    """-> dict(error, error_offset, flg, bd, block_max, content_size, pos) for a frame that starts with the frame magic"""
    h = dict(error=OK, error_offset=-1, flg=0, bd=0, block_max=0, content_size=-1, pos=0)
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
    h["pos"] = 4 + dlen
    return h


def read_frame(oracle, frame, slot_bytes=4 << 20, max_blocks=1 << 30, verify=V_BLOCKS | V_CONTENT, dst_cap=None):
    """What ONE frame at the start of `frame` is to lz4hip_lz4f_decode_device -> (info dict, output bytes clipped at dst_cap, rows).
    rows: per table row (stored offset, stored length, raw, bad checksum, the decoder's result at slot_bytes, its bytes) -- what the
    emulator's stand-in codec hands out."""
    frame = bytes(frame)
    n = len(frame)
    info = dict(blocks=0, decoded_bytes=0, good_bytes=0, error_offset=-1, content_size=-1, frame_bytes=0, error=OK, kind=0, block_max=0,
                flg=0, bd=0, checks=0)
    if n < 4:
        return dict(info, error=BAD_MAGIC, error_offset=0), b"", []
    magic = int.from_bytes(frame[:4], "little")
    if magic & 0xFFFFFFF0 == SKIPPABLE:
        info["kind"] = 1
        if n < 8:
            return dict(info, error=TRUNCATED, error_offset=4), b"", []
        end = 8 + int.from_bytes(frame[4:8], "little")
        info["frame_bytes"] = end
        if end > n:
            return dict(info, error=TRUNCATED, error_offset=4), b"", []
        return info, b"", []
    if magic != MAGIC:
        return dict(info, error=BAD_MAGIC, error_offset=0), b"", []
    h = parse_header(frame)
    info.update(flg=h["flg"], bd=h["bd"], block_max=h["block_max"], content_size=h["content_size"], error=h["error"], error_offset=h["error_offset"])
    if h["error"] != OK:
        return info, b"", []
    flg, block_max = h["flg"], h["block_max"]
    pos = h["pos"]
    info["frame_bytes"] = pos
    info["checks"] = ((SKIPPED if not verify & V_BLOCKS else VERIFIED) if flg & 0x10 else ABSENT) | ((SKIPPED if flg & 0x04 else ABSENT) << 2)
    if flg & 0x01:
        return dict(info, error=UNSUPPORTED_DICT, error_offset=4), b"", []
    if not flg & 0x20:
        return dict(info, error=UNSUPPORTED_LINKED, error_offset=4), b"", []
    if block_max > slot_bytes:
        return dict(info, error=SLOT_TOO_SMALL, error_offset=5), b"", []
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
    rows, parts, bad, before_bad = [], [], None, 0
    for k, (at, size, raw) in enumerate(blocks[:max_blocks]):
        data = frame[at + 4:at + 4 + size]
        badsum = bool(sum_bytes and verify & V_BLOCKS and xxh32(data) != int.from_bytes(frame[at + 4 + size:at + 8 + size], "little"))
        res, out = 0, b""
        if not raw and not badsum:
            res, buf = oracle.uncompress_unknown_raw(np.frombuffer(data, np.uint8), size, slot_bytes)
            out = bytes(buf[:max(res, 0)])
        rows.append((at + 4, size, raw, badsum, res, out))
        good = not badsum and (raw or 0 <= res <= block_max)
        if not good and bad is None:
            bad, before_bad = k, sum(len(p) for p in parts)
        parts.append((data if raw else out) if good else b"")
    content = b"".join(parts)
    info["decoded_bytes"] = info["good_bytes"] = len(content)
    cap = len(content) if dst_cap is None else dst_cap
    if len(blocks) > max_blocks:
        info.update(error=TABLE_FULL, error_offset=full_off)
    elif bad is not None:
        info.update(error=BLOCK_CHECKSUM if rows[bad][3] else CORRUPT_BLOCK, error_offset=blocks[bad][0], good_bytes=before_bad)
    elif walk_err == OK and h["content_size"] >= 0 and h["content_size"] != len(content):
        info.update(error=CONTENT_SIZE, error_offset=6)
    if info["error"] == OK and flg & 0x04 and verify & V_CONTENT and len(content) <= cap:
        info["checks"] = (info["checks"] & 3) | (VERIFIED << 2)
        if xxh32(content) != int.from_bytes(frame[trailer:trailer + 4], "little"):
            info.update(error=CONTENT_CHECKSUM, error_offset=trailer)
    return info, content[:cap], rows


# ---- the sources of tests/golden/lz4f_frames.json (only the frames are stored) ---------------------------------------------------------
def golden_source(oracle, kind, n):
    """"formula": in[i] = (u8)((i * 2654435761u) >> 24); "d2" / "d3": the oracle's generators, seed 11, from block 0"""
    if kind == "formula":
        i = np.arange(n, dtype=np.uint64)
        return (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.uint8).tobytes()
    return oracle.gen({"d2": 2, "d3": 3}[kind], 11, 0, (n + 65535) // 65536 or 1).reshape(-1)[:n].tobytes()
