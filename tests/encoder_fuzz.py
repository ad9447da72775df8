"""Differential fuzz of the encoder forms against the CPU oracle (shared by tests/test_simt_encoder_edges.py::test_encoder_fuzz_slice,
tests/test_gpu_encoder_edges.py::test_encoder_fuzz_slice, tools/fuzz_gpu_encoders.py and tools/emu_fuzz_hc.py): rows that stress the
exactness arguments of the kernels -- tiny alphabets, runs of period 1-5 between junk, copies of earlier content, fuzzer-style and
record-like rows, long runs with single disturbed bytes, random rows with islands of copies, and repeats planted at distances
65 520 .. 65 550 behind a run of zeros (the distance limit, tests/encoder_cases.py family A) -- of 13 bytes to 70 000: six rows in eight
are small, one is 30 000 .. 65 560 (around LZ4_64KLIMIT) and one 65 536 .. 70 000 (the generic fast variant, LZ4HC's large-block kernels).
The fast encoders against o.compress(a), LZ4HC against o.compress(a, hc=True); with the full bound and with too-small output limits:
return value, bytes, guard bytes.  How a form encodes is the caller's business (emulator or C ABI): see Form."""
import os

import numpy as np

import encoder_cases as ec

MODES = 8
PLANT_DISTANCES = (65520, 65551)


def row(o, rng, seed, rnd, i):
    mode = int(rng.integers(0, MODES))
    pick = int(rng.integers(0, 8))
    sz = int(rng.integers(65536, 70001)) if pick == 0 else int(rng.integers(30000, 65560)) if pick == 1 else int(rng.integers(13, 6000))
    if mode == 0:        # tiny alphabet
        return rng.integers(0, int(rng.integers(2, 4)), sz).astype(np.uint8)
    if mode == 1:        # runs of periods 1..5 with random junk
        a = rng.integers(0, 256, sz).astype(np.uint8); pos = 0
        while pos < sz:
            per = int(rng.integers(1, 6)); ln = int(rng.integers(4, 700))
            pat = rng.integers(0, 3, per).astype(np.uint8)
            seg = np.tile(pat, ln // per + 2)[:ln]; e = min(sz, pos + ln); a[pos:e] = seg[:e - pos]; pos = e + int(rng.integers(0, 12))
        return a
    if mode == 2:        # markov-ish repeats of earlier content
        a = rng.integers(0, 8, sz).astype(np.uint8); pos = 64
        while pos < sz - 8:
            ln = int(rng.integers(4, 400)); src = int(rng.integers(0, pos)); e = min(sz, pos + ln)
            for j in range(pos, e):
                a[j] = a[src + (j - pos)] if src + (j - pos) < j else a[j]
            pos = e + int(rng.integers(0, 6))
        return a
    if mode == 3:        # fuzzer-style
        return o.gen(2, seed * 131 + rnd, i, 1, max(sz, 16))[0][:sz].copy()
    if mode == 4:        # record-like, sometimes behind a long run
        a = o.gen(3, seed * 131 + rnd, i, 1, max(sz, 16))[0][:sz].copy()
        if rng.integers(0, 2):
            a[:sz // 3] = a[0]
        return a
    if mode == 5:        # long runs with single-byte disturbances
        a = np.full(sz, int(rng.integers(0, 256)), np.uint8)
        for _ in range(int(rng.integers(0, 40))):
            a[int(rng.integers(0, sz))] = int(rng.integers(0, 256))
        return a
    if mode == 6:        # incompressible with islands of copies
        a = rng.integers(0, 256, sz).astype(np.uint8)
        for _ in range(sz // 150):
            src, ln, dstp = int(rng.integers(0, max(sz - 40, 1))), int(rng.integers(4, 40)), int(rng.integers(0, max(sz - 40, 1)))
            if dstp > src and dstp + ln <= sz:
                a[dstp:dstp + ln] = a[src:src + ln]
        return a
    # mode 7: patterns, a run of zeros that keeps their table entries alive, then the patterns again at distances around MAX_DISTANCE
    a = np.zeros(int(rng.integers(66000, 70001)), np.uint8)
    lead = int(rng.integers(30, 400))
    a[:lead] = rng.integers(1, 256, lead)
    pos = int(rng.integers(*PLANT_DISTANCES))
    while pos + 80 < a.size:
        junk, d, ln = int(rng.integers(0, 4)), int(rng.integers(*PLANT_DISTANCES)), int(rng.integers(5, 40))
        a[pos:pos + junk] = rng.integers(1, 256, junk)
        pos += junk
        src = pos - d                                     # inside the lead, or before the block: then only junk, and on
        if src >= lead - 4:
            break
        if src >= 0:
            ln = min(ln, lead - src)
            a[pos:pos + ln] = a[src:src + ln]
            pos += ln
        else:
            a[pos] = int(rng.integers(1, 256)); pos += 1
    a[pos:] = rng.integers(1, 256, a.size - pos)
    return a


def rows(o, seed, rnd, per):
    """Round `rnd` of `seed`: `per` rows (every round of a seed draws from its own generator, so a round can be rebuilt alone)."""
    rng = np.random.default_rng([seed, rnd])
    return [row(o, rng, seed, rnd, i) for i in range(per)]


class Form:
    """One encoder form: `encode(blocks, caps or None) -> (result, dst)` with 0xA5 guard bytes behind every row; it takes the blocks whose
    size lies in `sizes` (inclusive); `deltas`: the output limits, None for the full bound, else the oracle's compressed size + delta."""

    def __init__(self, name, hc, sizes, encode, deltas=(None, 0, -1, -5)):
        self.name, self.hc, self.sizes, self.encode, self.deltas = name, hc, sizes, encode, deltas
        self.compared = 0              # comparisons made so far


def emu_forms(limits=None):
    """The emulator's forms (encoder_cases.EMU_FORMS); limits: {form name: deltas} where a caller cannot afford all four"""
    limits = limits or {}
    return [Form(name, hc, sizes, lambda b, c, k=kwargs: ec.emu_encode(k, b, c), **({"deltas": limits[name]} if name in limits else {}))
            for name, hc, sizes, kwargs in ec.EMU_FORMS]


def gpu_forms():
    """The C ABI's forms (encoder_cases.GPU_FORMS), LZ4HC's once per size class"""
    import gpu_helpers as gpu

    def encoder(form):
        def encode(blocks, caps):
            with ec.forced(form):
                return gpu.encode(blocks, caps=caps, hc=form[1])
        return encode
    return [Form(f"{form[0]} {sizes}", form[1], sizes, encoder(form)) for form in ec.GPU_FORMS for sizes in ec.gpu_size_classes(form[1])]


def run_round(o, forms, seed, rnd, per, report=print, save_dir=None):
    """One round's rows through every form; returns (comparisons, mismatches).  Every row is compared by every form that takes its size."""
    blocks = rows(o, seed, rnd, per)
    want = {hc: [o.compress(a, hc=hc) for a in blocks] for hc in {f.hc for f in forms}}
    limited = {}
    total = bad = 0
    for f in forms:
        idx = [i for i, a in enumerate(blocks) if f.sizes[0] <= a.size <= f.sizes[1]]
        if not idx:
            continue
        for delta in f.deltas:
            caps = None if delta is None else [max(len(want[f.hc][i]) + delta, 0) for i in idx]
            res, dst = f.encode([blocks[i] for i in idx], caps)
            for k, i in enumerate(idx):
                a, w = blocks[i], want[f.hc][i]
                cap = (a.size + a.size // 255 + 16) if caps is None else caps[k]
                if caps is None:
                    exp = len(w)
                else:
                    if (f.hc, i, cap) not in limited:
                        limited[f.hc, i, cap] = o.compress_raw(a, cap, hc=f.hc)[0]
                    exp = limited[f.hc, i, cap]
                ok = res[k] == exp and (exp <= 0 or np.array_equal(dst[k, :exp], w)) and (dst[k, cap:] == 0xA5).all()
                total += 1
                f.compared += 1
                if not ok:
                    bad += 1
                    saved = ""
                    if save_dir is not None and bad < 8:
                        saved = os.path.join(save_dir, f"enc_fuzz_bad_{seed}_{rnd}_{i}.npy")
                        np.save(saved, a)
                    report(f"MISMATCH {f.name} seed {seed} round {rnd} block {i} size {a.size} limit {delta} result {res[k]} want {exp} {saved}")
    return total, bad


def run_seed(o, forms, seed, per, rounds=1, report=print, save_dir=None):
    total = bad = 0
    for rnd in range(rounds):
        t, b = run_round(o, forms, seed, rnd, per, report, save_dir)
        total += t; bad += b
    return total, bad


def run(o, forms, first_seed, seeds, per, rounds=1, report=print, save_dir=None):
    """Seeds first_seed .. first_seed + seeds - 1, a fixed number: no time budget."""
    total = bad = 0
    for seed in range(first_seed, first_seed + seeds):
        t, b = run_seed(o, forms, seed, per, rounds, report, save_dir)
        total += t; bad += b
    return total, bad
