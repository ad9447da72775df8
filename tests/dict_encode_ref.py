"""The twin of the dictionary encode (lz4hip_encode_batch_dict_*): a serial restatement of its parse, which IS the definition
of the bytes -- the reference's generic encoder (LZ4_compressCtx) over V = tail || block with a primed table.  Nothing here is shared with
the kernels.  encode() gives the result and bytes of one block, primed_table() the table a call starts from, and a trace of the sequences
for the tests that build a block around one edge (tests/dict_encode_cases.py)."""
import numpy as np

REACH = 65535
MIN_LENGTH, MF_LIMIT, LAST_LITERALS, MIN_MATCH = 13, 12, 5, 4
GOLDEN = 2654435761
TABLE = 4096


def tail_of(dictionary):
    d = bytes(dictionary)
    return d[len(d) - REACH:] if len(d) > REACH else d


def _hash(w):
    return ((w * GOLDEN) & 0xFFFFFFFF) >> 20


def _r32(v, p):
    return v[p] | v[p + 1] << 8 | v[p + 2] << 16 | v[p + 3] << 24


def primed_table(dictionary):
    """U32[4096]: bucket h = the highest p in [0, T - 4] with hash(read32(tail, p)) == h, 0 where there is none"""
    tail = np.frombuffer(tail_of(dictionary), np.uint8).astype(np.uint64)
    table = np.zeros(TABLE, np.int64)
    if tail.size >= 4:
        w = tail[:-3] | tail[1:-2] << np.uint64(8) | tail[2:-1] << np.uint64(16) | tail[3:] << np.uint64(24)
        h = ((w * np.uint64(GOLDEN)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)
        np.maximum.at(table, h.astype(np.int64), np.arange(w.size, dtype=np.int64))
    return table.astype(np.uint32)


def _common(v, a, b, limit):
    """equal bytes v[a + i] == v[b + i] with a + i < limit"""
    n, step = 0, 32
    while a + n < limit:
        k = min(step, limit - a - n)
        if v[a + n:a + n + k] == v[b + n:b + n + k]:
            n += k
            step = min(step * 2, 1 << 16)
            continue
        while v[a + n] == v[b + n]:
            n += 1
        break
    return n


def _length_bytes(rest):
    return bytes([255] * (rest // 255) + [rest % 255])


def bound(n):
    return n + n // 255 + 16


def encode(block, dictionary=b"", cap=None, trace=None):
    """-> (result, bytes): the size and the bytes of `block` encoded against `dictionary` into `cap` bytes of room (0 and nothing: it
    does not fit).  trace: a list that receives (literals from, match at, candidate, match length, backward steps) per sequence, in V."""
    block = bytes(block)
    tail = tail_of(dictionary)
    T, n = len(tail), len(block)
    v = tail + block
    N = T + n
    cap = bound(n) if cap is None else cap
    out = bytearray()
    mflimit, matchlimit = N - MF_LIMIT, N - LAST_LITERALS
    ip = anchor = T

    def sequence_parse():
        nonlocal ip, anchor
        table = primed_table(dictionary).tolist()
        table[_hash(_r32(v, T))] = T
        ip = T + 1
        while True:
            # the search: the skip schedule starts at 67 attempts
            attempts, forward = 67, ip
            while True:
                step = attempts >> 6
                attempts += 1
                ip = forward
                forward = ip + step
                if forward > mflimit:
                    return True
                h = _hash(_r32(v, ip))
                ref = table[h]
                table[h] = ip
                if ref >= ip - REACH and v[ref:ref + 4] == v[ip:ip + 4]:
                    break
            back = 0
            while ip > anchor and ref > 0 and v[ip - 1] == v[ref - 1]:
                ip -= 1
                ref -= 1
                back += 1
            ll = ip - anchor
            token_at = len(out)
            out.append(0)
            if len(out) + ll + (ll >> 8) > cap - 8:
                return False
            if ll >= 15 and len(out) + (ll - 15) // 255 + 1 + ll > cap:
                return False
            token = 0xF0 if ll >= 15 else ll << 4
            if ll >= 15:
                out.extend(_length_bytes(ll - 15))
            out.extend(v[anchor:ip])
            while True:
                off = ip - ref
                assert 0 < off <= REACH and anchor >= T
                if len(out) + 2 > cap:
                    return False
                out.extend((off & 255, off >> 8))
                at = ip
                ip += MIN_MATCH
                ref += MIN_MATCH
                anchor = ip
                ip += _common(v, ip, ref, matchlimit)
                extra = ip - anchor
                if trace is not None:
                    trace.append((at - ll, at, at - off, extra + MIN_MATCH, back))
                if len(out) + (extra >> 8) > cap - 6:
                    return False
                if extra >= 15 and len(out) + (extra - 15) // 255 + 1 > cap:
                    return False
                out[token_at] = token | min(extra, 15)
                if extra >= 15:
                    out.extend(_length_bytes(extra - 15))
                if ip > mflimit:
                    anchor = ip
                    return True
                table[_hash(_r32(v, ip - 2))] = ip - 2
                h = _hash(_r32(v, ip))
                ref = table[h]
                table[h] = ip
                if not (ref > ip - (REACH + 1) and v[ref:ref + 4] == v[ip:ip + 4]):
                    break
                token_at = len(out)
                out.append(0)
                token, ll, back = 0, 0, 0
            anchor = ip
            ip += 1

    if n >= MIN_LENGTH and not sequence_parse():
        return 0, b""
    run = N - anchor
    if len(out) + run + 1 + (run - 15 + 255) // 255 > cap:
        return 0, b""
    out.append(0xF0 if run >= 15 else run << 4)
    if run >= 15:
        out.extend(_length_bytes(run - 15))
    out.extend(v[anchor:])
    return len(out), bytes(out)
