"""TEST INFRASTRUCTURE for the LZ4Stream tests, on the device and under the SIMT emulator: a stream framed HERE from chunks, the
stream the oracle's blocks give for a source, the sources, and streams and chunks with something odd about them."""
import glob
import os

import numpy as np

from lz4net_amd import stream as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [16, 4096, 65536, 100003, 1 << 20]


def frame(chunks):
    """chunks: (flags, original, payload bytes[, clen override]) -> stream bytes."""
    out = bytearray()
    for c in chunks:
        flags, original, payload = c[0], c[1], bytes(c[2])
        out += st.write_varint(flags) + st.write_varint(original)
        if flags & st.FLAG_COMPRESSED:
            out += st.write_varint(c[3] if len(c) > 3 else len(payload))
        out += payload
    return bytes(out)


def expected_stream(oracle, data, B, hc):
    chunks = []
    for o in range(0, len(data), B):
        chunk = data[o:o + B]
        r, buf = oracle.compress_raw(chunk, len(chunk), hc=hc)
        compressed = 0 < r < len(chunk)
        flags = (st.FLAG_COMPRESSED if compressed else 0) | (st.FLAG_HIGH_COMPRESSION if hc else 0)
        chunks.append((flags, len(chunk), buf[:r] if compressed else chunk))
    return frame(chunks)


_REAL = None


def real_bytes():
    """The repository's own text and sources."""
    global _REAL
    if _REAL is None:
        files = sorted(glob.glob(os.path.join(ROOT, "*.md")) + glob.glob(os.path.join(ROOT, "lz4net_amd", "**", "*.hip"), recursive=True) +
                       glob.glob(os.path.join(ROOT, "lz4net_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py")))
        _REAL = np.frombuffer(b"".join(open(f, "rb").read() for f in files), dtype=np.uint8)
    return _REAL


def data_of(oracle, kind, size):
    if kind in (0, 1, 2, 3):
        rows = -(-size // 65536)
        return oracle.gen(kind, 11 + kind, 3, max(rows, 1)).reshape(-1)[:size].copy()
    if kind == "random":
        return np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(size, np.uint8)
    r = real_bytes()
    return np.resize(r, size) if size > r.size else r[:size].copy()


KINDS = [0, 1, 2, 3, "random", "zeros", "real"]


def _nonminimal(v):
    b = bytearray(st.write_varint(v))
    b[-1] |= 0x80
    return bytes(b) + b"\x00"


def wide_flags_streams(oracle):
    a = data_of(oracle, 2, 5000)
    r, buf = oracle.compress_raw(a, 5000)
    rest = st.write_varint(5000) + st.write_varint(r) + buf[:r].tobytes() + frame([(0, 7, b"1234567")])
    return [bytes.fromhex("818080808001") + rest, bytes.fromhex("8180808080808080807e") + rest]


def _bad_block(original=100):
    """A compressed payload the decoder must reject: one literal, then a match 65 535 bytes back."""
    return (st.FLAG_COMPRESSED, original, bytes([0x1F, 0x41, 0xFF, 0xFF]) + bytes(6))


def _offsets(chunks):
    offs, pos = [], 0
    for c in chunks:
        offs.append(pos)
        pos += len(frame([c]))
    return offs
