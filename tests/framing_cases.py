"""TEST INFRASTRUCTURE for the LZ4Stream / Wrap framing tests under the SIMT emulator (tests/test_simt_framing.py, test_simt_into.py,
test_simt_spans.py): the statuses, the byte pattern and the noise the buffers are made of, and the references the kernels are held
against -- the stream header walk written to the rules of LZ4Stream.cs, and Unwrap's checks."""
import struct

import numpy as np

from lz4net_amd import stream as st
from stream_cases import frame

OK, EOS, PASSES, CORRUPT_BLOCK, TABLE_FULL = 0, 1, 2, 3, 4          # LZ4HIP_STREAM_* (include/lz4hip.h)
WRAP_OK, WRAP_SIZE_INVALID, WRAP_CORRUPT_HEADER, WRAP_CORRUPT_BLOCK = 0, 1, 2, 3


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 17) & 0xFF).astype(np.uint8)


def header_stream(flags, original, clen=None):
    return st.write_varint(flags) + st.write_varint(original) + (st.write_varint(clen) if flags & 1 else b"")


def header_wrap(original, payload):
    return struct.pack("<ii", original, payload)


RNG = np.random.default_rng(20240607)
NOISE = RNG.integers(0, 256, 1 << 18, dtype=np.uint8)


def noise(n, salt=0):
    o = (salt * 7919) % (NOISE.size - n - 1) if n < NOISE.size else 0
    return NOISE[o:o + n].copy() if n <= NOISE.size else np.resize(NOISE, n)


# ---- the header reader ------------------------------------------------------------------------------------------------------------
# The reference walk, written to the rules of LZ4Stream.cs: TryReadVarInt sums (b & 0x7F) << count into a ulong (modulo 2^64; the
# tenth byte's shift is 63, so only its bit 0 survives) and stops at a clear continuation bit or after ten bytes (:167-187);
# AcquireNextChunk casts the lengths to int and the flags to an int-based enum, and tests (int)flags >> 2 (:274-312).
MASK64 = (1 << 64) - 1


def cs_varint(buf, pos):
    """-> (value, new pos); value None: clean end of data, "eos": the data ends inside the varint"""
    result = count = 0
    while True:
        if pos >= len(buf):
            return (None if count == 0 else "eos"), pos
        b = buf[pos]
        pos += 1
        result = (result + ((b & 0x7F) << count)) & MASK64
        count += 7
        if (b & 0x80) == 0 or count >= 64:
            return result, pos


def s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def ref_walk(buf, max_chunks=None):
    """-> dict: rows [(compressed, header offset, payload offset, payload length, original, output offset)] of the non-empty
    chunks, status, error_offset, chunks, compressed_chunks, decoded_bytes -- what lz4hip_stream_index_device documents."""
    buf = bytes(buf)
    pos, out, rows, status = 0, 0, [], OK
    while pos < len(buf):
        flags, p = cs_varint(buf, pos)
        original, p = cs_varint(buf, p) if flags != "eos" else ("eos", p)
        bad = flags == "eos" or original in (None, "eos")
        compressed = (not bad) and (flags & 1) != 0
        clen = original
        if compressed:
            clen, p = cs_varint(buf, p)
            bad = clen in (None, "eos")
        if not bad:
            original, clen = s32(original), s32(clen)
            bad = clen > original or clen < 0 or p + clen > len(buf)
        if bad:
            status = EOS
            break
        if compressed and (s32(flags) >> 2) != 0:
            status = PASSES
            break
        if original != 0:
            rows.append((compressed, pos, p, clen, original, out))
            out += original
        pos = p + clen
    w = dict(rows=rows, status=status, error_offset=pos if status != OK else -1, chunks=len(rows),
             compressed_chunks=sum(1 for r in rows if r[0]), decoded_bytes=out)
    if max_chunks is not None and len(rows) > max_chunks:                 # a full table wins over a later header error
        w.update(status=TABLE_FULL, error_offset=rows[max_chunks][1])
    return w


TAIL = frame([(0, 3, b"abc")] * 12)                                       # behind every buffer: bytes that parse as more chunks


def mixed(oracle, size, salt):
    """compressible and incompressible stretches"""
    if size == 0:
        return np.zeros(0, np.uint8)
    a = oracle.gen(2, 21 + salt, 3, -(-size // 65536)).reshape(-1)[:size].copy()
    a[size // 3:size // 2] = noise(size // 2 - size // 3, salt)
    return a


def ref_unwrap(m):
    """Unwrap's checks in its order with signed fields -> (status, "raw" / "comp" / None, output size, payload length)"""
    if len(m) < 8:
        return WRAP_SIZE_INVALID, None, 0, 0
    original, payload = struct.unpack("<ii", bytes(m[:8]))
    if payload < 0 or payload > len(m) - 8:
        return WRAP_CORRUPT_HEADER, None, 0, 0
    if payload >= original:
        return WRAP_OK, "raw", payload, payload
    return WRAP_OK, "comp", original, payload
