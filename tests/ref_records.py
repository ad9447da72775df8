"""The calls tests/test_oracle_vs_ref.py and tests/test_legacy_frame.py make of the reference, as records any codec can
answer: tests/golden/make_golden.py records the reference's own answers (oracle/_ref) in tests/golden/ref_records.json,
and the tests compare the oracle's answers with those, so they need nothing outside the repository.

A walker yields (group, return code, bytes the comparison looks at or None, self-check or None); summarise() folds a walk
into {group: {"ret": [return codes], "sha": digest of the compared bytes}}.  The self-check is a property the tests
assert of the oracle itself (output canary untouched, well-formed stream decoded to its source)."""
import hashlib
import json
import os

import numpy as np

from oracle.oracle import compress_bound

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_records.json")

SIZES = (0, 1, 5, 12, 13, 14, 64, 255, 1000, 4096, 32768, 65535, 65536, 65546, 65547, 70000, 200000)
ALIGN_OFFSETS = (0, 1, 7, 65535, 65536, 65537, 40000)
STREAM_SEEDS = (2026, 7)
# legacy frames written by the reference CLI: (bytes, distribution, LZ4HC), original/lz4demo.c
FRAME_PARSE_CASE = (300000, 3, False)
FRAME_INTEROP_CASES = [(n, d, hc) for hc in (False, True) for n, d in ((1000, 2), (70000, 2), (300000, 3), ((8 << 20) + 123457, 3))
                       if not (hc and n > (1 << 20))]          # HC over 8 MiB chunks: covered by the fast path only (time)


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def inputs(oracle):
    rng = np.random.default_rng(1)
    for dist in range(4):
        for seed in range(2):
            for n in SIZES:
                yield f"d{dist}s{seed}n{n}", oracle.gen(dist, seed, n, 1, max(n, 1))[0][:n]
    for n in (100, 5000, 65536, 150000):
        for k in (2, 3, 16):
            yield f"alpha{k}n{n}", rng.integers(0, k, n, dtype=np.uint8)


def frame_sample(oracle, n_bytes, dist=3):
    blocks = (n_bytes + 65535) // 65536
    return oracle.gen(dist, 11, 0, blocks).reshape(-1)[:n_bytes].tobytes()


def frame_key(n_bytes, dist, hc) -> str:
    return f"{n_bytes}/{dist}/{'hc' if hc else 'fast'}"


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()[:16]


def summarise(records):
    """-> ({group: {"ret": [...], "sha": ...}}, [groups whose self-check failed])"""
    out, hashers, failed = {}, {}, []
    for group, ret, data, ok in records:
        e = out.setdefault(group, {"ret": [], "sha": None})
        e["ret"].append(int(ret))
        h = hashers.setdefault(group, hashlib.sha256())
        if data is not None:
            data = bytes(data)
            h.update(len(data).to_bytes(8, "little") + data)
        else:
            h.update(b"-")
        if ok is False:
            failed.append(group)
    for group, h in hashers.items():
        out[group]["sha"] = h.hexdigest()[:16]
    return out, failed


def encoders(codec, oracle):
    for name, a in inputs(oracle):
        bound = compress_bound(a.size)
        for hc in (False, True):
            g = f"{name}/{'hc' if hc else 'fast'}"
            r, b = codec.compress_raw(a, bound, hc)
            yield g, r, b[:max(r, 0)], bool((b[bound:] == 0xA5).all())
            for cap in (r, r - 1, r // 2, 0, 1, 12):           # original/fuzzer.c:212-227
                q, x = codec.compress_raw(a, cap, hc)
                # (the reference's HC emitter can overrun a too-small cap: lz4hc.c:541)
                yield g, q, None, None if hc else bool((x[max(cap, 0):] == 0xA5).all())


def decoders(codec, oracle):
    rng = np.random.default_rng(2)
    for name, a in inputs(oracle):
        n = a.size
        for hc in (False, True):
            g = f"{name}/{'hc' if hc else 'fast'}"
            c = codec.compress(a, hc)
            yield g, len(c), c, None
            for osize in (n, n - 1, n + 1, n // 2):           # original/fuzzer.c:185-194
                if osize < 0:
                    continue
                d, o = codec.uncompress_raw(c, osize)
                yield g, d, o[:osize] if d >= 0 else None, bool((o[osize:] == 0xA5).all())
            r1 = len(c)
            for isz, mo in ((r1, n), (r1, n + 1), (r1, n - 1), (r1 - 1, n), (r1 + 1, n), (r1, n + 100),
                            (0, n), (r1, n // 2)):             # original/fuzzer.c:196-210
                if mo < 0 or isz < 0:
                    continue
                d, o = codec.uncompress_unknown_raw(c, isz, mo)
                yield g, d, o[:d] if d >= 0 else None, bool((o[mo:] == 0xA5).all())
            if r1 > 20:                                        # corrupted streams: same error position
                for _ in range(8):
                    cc = c.copy()
                    cc[rng.integers(0, r1)] = rng.integers(0, 256)
                    yield g, codec.uncompress_raw(cc, n)[0], None, None
                    yield g, codec.uncompress_unknown_raw(cc, r1, n)[0], None, None


def alignment(codec, oracle):
    """HC chain slots are address & 0xFFFF in the reference; the same block placed at several offsets."""
    a = oracle.gen(2, 9, 0, 1, 65536)[0]
    big = np.zeros(65536 * 3 + 64, dtype=np.uint8)
    for off in ALIGN_OFFSETS:
        big[off:off + 65536] = a
        out = np.zeros(compress_bound(65536), dtype=np.uint8)
        ret = codec._hc(big.ctypes.data + off, out.ctypes.data, 65536, out.size)
        yield f"off{off}", ret, out[:max(ret, 0)], None


def streams(codec):
    """Streams no encoder produced (tests/stream_fuzz.py).  Bytes of offset-0 matches are unspecified in the reference
    (see stream_fuzz.has_zero_offset): for those streams only the return codes are recorded."""
    import stream_fuzz
    for seed in STREAM_SEEDS:
        for i, ((c, raw), t) in enumerate(stream_fuzz.cases(seed, 400)):
            g = f"s{seed}i{i}"
            d, o = codec.uncompress_raw(c, t)
            holes = stream_fuzz.has_zero_offset(c, t + 3)
            well_formed = None if raw is None else bool(d == len(c) and np.array_equal(o[:t], raw))
            yield g, d, o[:t] if d >= 0 and not holes else None, well_formed
            for cap in (t, t + 3, t - 1):
                u, p = codec.uncompress_unknown_raw(c, len(c), cap)
                yield g, u, p[:u] if u >= 0 and not holes else None, None
