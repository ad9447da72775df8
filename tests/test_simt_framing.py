"""The framing kernels (lz4net_amd/csrc/lz4hip_stream.hpp, lz4hip_wrap.hpp, lz4hip_streams.hpp) under the CPU SIMT emulator
(tests/simt/emu_stream.inc): the int64 scan, the position-driven copy routine behind its five layouts, the header reader, and the
library's own host code for the framing paths (lz4net_amd/csrc/lz4hip_framing.hpp: scratch layouts, grids, kernel sequences), once
from the kernels' argument structs over arrays made here and once whole, from the C ABI's arguments over a scratch buffer of exactly
the size the library asks for, with the block codec step replaced by arrays handed in here; and the six host-pointer calls on top of
them, over a device image in host memory (at the end of this file).  Every reference is plain Python /
numpy written from the wire formats (LZ4Stream: src/LZ4/LZ4Stream.cs:162-312, Wrap: src/LZ4/LZ4Codec.cs:471-599), never from the
kernels.  Every output buffer has guard bytes on both sides and is pre-filled with a pattern; bytes that belong to no segment must
still hold it.  Every case runs with a grid of one workgroup, a small odd grid and the product's grid formula.  The `-m gpu` tests
of test_stream_device.py, test_wrap_device.py and test_streams_device.py repeat the end-to-end comparisons through the C ABI."""
import struct

import numpy as np
import pytest

import emu_helpers as emu
from emu_helpers import addr, ref
from emu_lib import E_ARGUMENT
from framing_cases import (CORRUPT_BLOCK, EOS, OK, PASSES, TABLE_FULL, TAIL, WRAP_CORRUPT_BLOCK, WRAP_CORRUPT_HEADER, WRAP_OK, header_stream, header_wrap,
                           mixed, noise, pattern, ref_unwrap, ref_walk)
from lz4net_amd import stream as st
from stream_cases import expected_stream, frame

GUARD = 64
SPAN = 65536                                                            # kCopySpan (checked in test_constants)
NONE64 = 0xFFFFFFFFFFFFFFFF


def guarded(size):
    """(array of GUARD + size + GUARD pattern bytes, address of byte GUARD)"""
    buf = pattern(size + 2 * GUARD)
    return buf, addr(buf, GUARD)


def ref_copy(size, segs, end):
    """What a copy over the segments (start, bytes) leaves of a guarded buffer: nothing at or past `end`, nothing in the gaps."""
    want = pattern(size + 2 * GUARD)
    for start, data in segs:
        data = np.frombuffer(bytes(data), np.uint8)[:max(0, end - start)]
        want[GUARD + start:GUARD + start + data.size] = data
    return want


def same(got, want, what):
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at byte {i - GUARD} (got {got[i]}, want {want[i]})")


def copy_grids(product_bytes):
    return sorted({1, 3, emu.framing().emu_copy_grid(product_bytes)})


def item_grids(items):
    return sorted({1, 3, emu.framing().emu_items_grid(items)})


def at_residue(backing, residue, size):
    """A `size`-byte view of `backing` whose address is `residue` mod 16."""
    shift = (residue - backing.ctypes.data) % 16
    return backing[shift:shift + size]


def test_constants():
    assert emu.scan_tile() == 4096 and emu.copy_span() == SPAN


# ---- the scan -------------------------------------------------------------------------------------------------------------------
TILE = 4096
SCAN_N = [1, 255, 256, 257, 4095, 4096, 4097, 8192, 256 * TILE - 1, 256 * TILE, 256 * TILE + 1, 2 * 256 * TILE + 5]


@pytest.mark.parametrize("n", SCAN_N)
def test_scan(n):
    """reduce -> partials -> apply against np.cumsum on int64.  More than 256 tiles (n > 1 048 576) is the second round of the
    partials kernel's loop, with its carry."""
    L = emu.framing()
    tiles = -(-n // TILE)
    rng = np.random.default_rng(n)
    for kind in ("random", "zeros", "ones"):
        v = {"random": rng.integers(0, 1 << 40, n, dtype=np.int64), "zeros": np.zeros(n, np.int64), "ones": np.ones(n, np.int64)}[kind]
        x = np.full(n + 8, -99, np.int64)
        x[:n] = v
        partial = np.full(tiles + 8, -98, np.int64)
        total = np.full(3, -97, np.int64)
        L.emu_scan(addr(x), n, addr(partial), addr(total, 1))
        want = np.cumsum(v) - v
        assert np.array_equal(x[:n], want), (n, kind, int(np.flatnonzero(x[:n] != want)[0]))
        assert total.tolist() == [-97, int(v.sum()), -97], (n, kind)
        assert (x[n:] == -99).all() and (partial[tiles:] == -98).all(), (n, kind)
        tile_sums = np.add.reduceat(v, np.arange(0, n, TILE))
        assert np.array_equal(partial[:tiles], np.cumsum(tile_sums) - tile_sums), (n, kind)


# ---- the copy routine, once per layout, on synthetic segment tables ------------------------------------------------------------------
# A case is (run(dst_address, end, grid), segments [(start, bytes)], total, bytes the product would size the grid by).  `ends` are
# the cut positions every case runs with: the total, and cuts in the middle of a piece and exactly at a piece edge.

def ends_for(total):
    c = {total, total - 1, total - 15, total - 16, total - 17, total // 2, (total // 2) & ~15, ((total // 2) & ~15) + 7, 16, 1, 0}
    for k in (SPAN, 2 * SPAN):
        c |= {k - 16, k - 1, k, k + 1, k + 16}
    return sorted(e for e in c if 0 <= e <= total)


def check_copy(name, case, ends=None, grids=None):
    run, segs, total, product_bytes = case
    starts = [s for s, _ in segs]
    assert starts == sorted(starts), name
    for end in (ends_for(total) if ends is None else ends):
        want = ref_copy(total, segs, end)
        for grid in (copy_grids(product_bytes) if grids is None else grids):
            buf, ptr = guarded(total)
            run(ptr, end, grid)
            same(buf, want, f"{name}: end {end} of {total}, grid {grid}")


# -- RawLayout: (gap before, length, source residue) per segment; gaps, zero lengths, any source alignment
def raw_case(spec, first=0):
    L = emu.framing()
    n = len(spec)
    src_size = sum(ln for _, ln, _ in spec) + 16 * n + 64
    backing = noise(src_size + 16, 1)
    src = at_residue(backing, 0, src_size)
    t, arr = emu.stream_tables(n)
    segs, pos, spos = [], first, 0
    for k, (gap, ln, res) in enumerate(spec):
        pos += gap
        spos += (res - spos) % 16
        arr["r_dst_off"][k], arr["r_src_off"][k], arr["r_len"][k] = pos, spos, ln
        segs.append((pos, src[spos:spos + ln]))
        pos += ln
        spos += ln
    total = pos + 40                                                   # `end` may lie past the last segment

    def run(dst, end, grid):
        L.emu_copy_raw(addr(src), ref(t), n, dst, end, grid)
    run.keep = (backing, arr)
    return run, segs, total, total


GAPS = (0, 1, 15, 16, 17, 33)


def sweep_spec():
    """payload lengths 0..48 with every gap, at source residues that cycle through all 16; the starts hit every residue too"""
    spec = []
    for ln in range(49):
        for g, gap in enumerate(GAPS):
            spec.append((gap, ln, (ln * 5 + g * 3) % 16))
    return spec


def test_copy_raw_layout():
    spec = sweep_spec()
    case = raw_case(spec)
    assert {s % 16 for s, _ in case[1]} == set(range(16)) and {r for _, _, r in spec} == set(range(16))
    check_copy("raw sweep", case)
    for first in (1, 16, 37):                                           # the first segment not at 0
        check_copy(f"raw sweep from {first}", raw_case(spec[:60], first), ends=None, grids=[1, 3])
    # long segments: a piece wholly inside, a second and third span of one workgroup with a live cursor
    long_spec = [(5, 4095, 3), (0, 4096, 0), (17, 4097, 9), (1, 65539, 13), (33, 40, 1), (0, 65536 + 4096, 7), (16, 3, 2)]
    check_copy("raw long", raw_case(long_spec))
    # several zero-length segments in a row with equal starts, at the front, in the middle and at the end
    zeros = [(7, 0, 0)] + [(0, 0, 0)] * 4 + [(0, 20, 5)] + [(0, 0, 0)] * 3 + [(3, 0, 0)] * 2 + [(0, 31, 11)] + [(0, 0, 0)] * 5
    check_copy("raw zero-length runs", raw_case(zeros))
    check_copy("raw zero-length only", raw_case([(9, 0, 0)] * 7))
    check_copy("raw no segment", raw_case([]))
    # a few thousand 3-byte segments: every piece holds several, the cursor gallops and bisects from every position
    tiny = [(0, 3, k % 16) for k in range(6000)]
    check_copy("raw tiny", raw_case(tiny), ends=[18000, 17999, 9008, 16, 0])
    tiny_gaps = [(k % 3, 3, (k * 7) % 16) for k in range(50000)]      # > 2 spans of tiny segments with gaps
    case = raw_case(tiny_gaps)
    check_copy("raw tiny with gaps", case, ends=[case[2], SPAN, SPAN + 5, 2 * SPAN - 16])


# -- EncodeLayout: chunks of `block` bytes (the last one shorter), result r per chunk; compressed iff 0 < r < len
def encode_case(src_len, block, results, hc=False, src_res=0, comp_res=0, total_cut=None):
    L = emu.framing()
    n = -(-src_len // block)
    assert n == len(results)
    real = src_len if total_cut is None else min(src_len, total_cut + 64)      # bytes that really exist behind the pointers
    b1, b2 = noise(real + 32, 2), noise(real + 32, 3)
    src, comp = at_residue(b1, src_res, real), at_residue(b2, comp_res, real)
    res = np.array(results, np.int32)
    offs = np.zeros(n + 1, np.int64)
    segs, pos = [], 0
    for k, r in enumerate(results):
        ln = min(block, src_len - k * block)
        c = 0 < r < ln
        flags = (1 if c else 0) | (2 if hc else 0)
        plen = r if c else ln
        head = header_stream(flags, ln, r)
        have = max(0, min(plen, real - k * block))                          # (a cut total never reaches what is not there)
        payload = (comp if c else src)[k * block:k * block + have]
        offs[k] = pos
        segs.append((pos, head + payload.tobytes()))
        pos += len(head) + plen
    offs[n] = pos
    total = pos if total_cut is None else total_cut
    a = emu.StreamEncodeArgs(src=addr(src), comp=addr(comp), src_len=src_len, n=n, block=block, hc_flag=2 if hc else 0,
                             result=addr(res), offs=addr(offs))
    tot = np.zeros(1, np.int64)

    def run(dst, end, grid):
        tot[0] = end
        L.emu_copy_encode(ref(a), dst, addr(tot), grid)
    run.keep = (b1, b2, res, offs, a, tot)
    return run, segs, total, src_len + n * (1 + 2 * len(st.write_varint(block)))


def test_copy_encode_layout():
    # payloads 1..48 and the forced results (0, -1, len, len - 1, len + 5, 1) at block sizes around the varint edges
    for block in (17, 49, 127, 128):
        results = []
        for r in range(1, 49):
            results += [r, (0, -1, block, block - 1, block + 5, 1)[r % 6]]
        src_len = block * len(results) - (block - 7)                        # the last chunk: 7 bytes (result 1 or raw)
        case = encode_case(src_len, block, results, hc=bool(block & 1))
        if block == 17:
            assert {s % 16 for s, _ in case[1]} == set(range(16))
        check_copy(f"encode block {block}", case)
    for res in range(16):                                                   # payload source addresses at every residue
        check_copy(f"encode residue {res}", encode_case(49 * 40 - 3, 49, [(k % 48) + 1 if k % 3 else 0 for k in range(40)], src_res=res,
                                                       comp_res=(res * 7 + 3) % 16), ends=None, grids=[1])
    for block in (16383, 16384):
        check_copy(f"encode block {block}", encode_case(block * 5 + 128, block, [127, 128, block - 1, 0, 16383 if block > 16383 else 16382, 127]))
    for block in (2097151, 2097152):
        check_copy(f"encode block {block}", encode_case(block + 200, block, [16384, 128]), ends=[16384 + 400, 16384 + 9, 16, 9, 8, 0])
    # lengths of five varint bytes: one chunk, the total cut short behind the header (the payload's tail does not exist)
    for ln, r in ((1 << 28, (1 << 21) + 3), ((1 << 28) + 5, 1 << 28), ((1 << 28) - 1, 2097151)):
        case = encode_case(ln, 1 << 29, [r], total_cut=300)
        check_copy(f"encode original {ln} clen {r}", case, ends=[300, 17, 16, 12, 11, 10, 5], grids=[1, 3])
    # several spans per workgroup
    check_copy("encode long", encode_case(4096 * 40 + 5, 4096, [(4095, 0, 1, 4000, 129)[k % 5] for k in range(41)]))
    # tiny chunks: block 16 with results 1..2: segments of 4 or 5 bytes for two spans and more
    n = 30000
    check_copy("encode tiny", encode_case(16 * n, 16, [1 + (k % 2) for k in range(n)]), ends=[4 * n + n // 2, SPAN, SPAN + 3, 20])


# -- WrapLayout: message k is src[off[k], off[k + 1]); 8 header bytes, then the encoder's bytes (0 < enc < len) or the message
def wrap_case(lens, enc, bad=(), cap_extra=0, src_res=0):
    L = emu.framing()
    n = len(lens)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    src_len = int(off[n])
    off_k = off.copy()
    for k in bad:                                                           # message k ends before it starts: no bytes at all
        off_k[k + 1] = off_k[k] - 1
    b1, b2 = noise(src_len + 32, 4), noise(src_len + 32, 5)
    src, comp = at_residue(b1, src_res, src_len), at_residue(b2, (src_res + 5) % 16, src_len)
    dst_off = np.zeros(n + 1, np.int64)
    segs, pos = [], 0
    for k in range(n):
        a, b = int(off_k[k]), int(off_k[k + 1])
        dst_off[k] = pos
        if a < 0 or b < a or b > src_len:
            segs.append((pos, b""))
            continue
        ln, r = b - a, int(enc[k])
        c = 0 < r < ln
        plen = r if c else ln
        segs.append((pos, header_wrap(ln, plen) + (comp if c else src)[a:a + plen].tobytes()))
        pos += 8 + plen
    dst_off[n] = pos
    e = np.array(enc, np.int32)
    a = emu.WrapArgs(src=addr(src), comp=addr(comp), off=addr(off_k), src_len=src_len, n=n, enc=addr(e), dst_off=addr(dst_off))

    def run(dst, end, grid):
        L.emu_copy_wrap(ref(a), dst, end, grid)                             # (cap cuts like a total does: end = min(total, cap))
    run.keep = (b1, b2, off_k, dst_off, e, a)
    return run, segs, pos + cap_extra, src_len + 8 * n


def test_copy_wrap_layout():
    lens, enc = [], []
    for ln in range(49):
        for j in range(3):
            lens.append(ln)
            enc.append((0, max(ln - 1, 0), 1 + (ln * 7 + j) % max(ln, 1))[j])
    case = wrap_case(lens, enc)
    assert {s % 16 for s, _ in case[1]} >= set(range(0, 16))
    check_copy("wrap sweep", case)
    check_copy("wrap sweep, cap past the total", wrap_case(lens, enc, cap_extra=40), ends=[case[2] + 40, case[2] + 1])
    check_copy("wrap with bad offsets", wrap_case(lens[:90], enc[:90], bad=(0, 1, 2, 30, 31, 50, 88)))
    for res in range(16):
        check_copy(f"wrap residue {res}", wrap_case(lens[20:80], enc[20:80], src_res=res), grids=[1])
    big = [4095, 4096, 4097, 65539, 0, 0, 0, 9, 65536, 70000]
    check_copy("wrap long", wrap_case(big, [0, 4000, 4096, 65000, 0, 5, -3, 8, 1, 69999]))
    check_copy("wrap tiny", wrap_case([3] * 20000, [k % 3 for k in range(20000)]), ends=[20000 * 11 - 5000, SPAN, 2 * SPAN + 1, 24])


# -- UnwrapRawLayout: per message ("raw", payload length) / ("comp", decoded length: a gap) / ("bad",): no bytes
def unwrap_raw_case(msgs, src_res=0):
    L = emu.framing()
    n = len(msgs)
    sizes = [8 + (m[1] if m[0] == "raw" else 5) for m in msgs]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    src_len = int(off[n])
    b1 = noise(src_len + 32, 6)
    src = at_residue(b1, src_res, src_len)
    dst_off = np.zeros(n + 1, np.int64)
    raw_len = np.zeros(n, np.int32)
    status = np.zeros(n, np.int32)
    segs, pos = [], 0
    for k, m in enumerate(msgs):
        dst_off[k] = pos
        if m[0] == "raw":
            raw_len[k] = m[1]
            a = int(off[k]) + 8
            segs.append((pos, src[a:a + m[1]]))
            pos += m[1]
        elif m[0] == "comp":
            raw_len[k] = -1
            pos += m[1]
    dst_off[n] = pos
    a = emu.UnwrapArgs(src=addr(src), off=addr(off), src_len=src_len, n=n, dst_off=addr(dst_off), status=addr(status))
    t = emu.UnwrapTables(n=n, raw_len=addr(raw_len))

    def run(dst, end, grid):
        L.emu_copy_unwrap_raw(ref(a), ref(t), dst, end, grid)
    run.keep = (b1, off, dst_off, raw_len, status, a, t)
    return run, segs, pos + 40, pos


def test_copy_unwrap_raw_layout():
    msgs = []
    for ln in range(49):
        for g, gap in enumerate(GAPS):
            if gap:
                msgs.append(("comp", gap))
            msgs.append(("raw", ln))
            if g == 2:
                msgs += [("bad",)] * (ln % 4)
    case = unwrap_raw_case(msgs)
    assert {s % 16 for s, _ in case[1]} == set(range(16))
    check_copy("unwrap sweep", case)
    for res in range(16):
        check_copy(f"unwrap residue {res}", unwrap_raw_case(msgs[40:140], src_res=res), grids=[1])
    check_copy("unwrap leading gap", unwrap_raw_case([("comp", 37), ("bad",), ("raw", 0), ("raw", 0), ("raw", 21), ("bad",), ("bad",), ("comp", 1)]))
    check_copy("unwrap nothing raw", unwrap_raw_case([("comp", 100), ("bad",), ("comp", 3)]))
    check_copy("unwrap long", unwrap_raw_case([("raw", 4095), ("comp", 4097), ("raw", 4096), ("raw", 65539), ("comp", 70000), ("raw", 4097), ("raw", 2)]))
    tiny = [("raw", 3) if k % 5 else ("comp", 2) for k in range(50000)]
    case = unwrap_raw_case(tiny)
    check_copy("unwrap tiny", case, ends=[case[2] - 40, SPAN, SPAN + 9, 2 * SPAN - 16, 32])


# -- StreamsEncodeLayout: chunk table entries (source position, length, result), `pad` empty entries behind them
def streams_copy_case(entries, pad, hc=False, total_cut=None):
    L = emu.framing()
    K, cap = len(entries), len(entries) + pad
    need = max([at + (0 if total_cut is not None else ln) for at, ln, _ in entries] + [0]) + 512
    b1, b2 = noise(need + 32, 7), noise(need + 32, 8)
    src, comp = at_residue(b1, 0, need), at_residue(b2, 0, need)
    c_at, c_len, res = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.full(cap, 5, np.int32)   # (a padding entry's result is ignored)
    offs = np.zeros(cap + 1, np.int64)
    segs, pos = [], 0
    for k, (at, ln, r) in enumerate(entries):
        c_at[k], c_len[k], res[k] = at, ln, r
        c = 0 < r < ln
        plen = r if c else ln
        head = header_stream((1 if c else 0) | (2 if hc else 0), ln, r)
        offs[k] = pos
        segs.append((pos, head + (comp if c else src)[at:at + min(plen, 400 if total_cut is not None else plen)].tobytes()))
        pos += len(head) + plen
    offs[K:] = pos
    total = pos if total_cut is None else total_cut
    a = emu.StreamsEncodeArgs(src=addr(src), comp=addr(comp), cap=cap, hc_flag=2 if hc else 0, c_at=addr(c_at), c_len=addr(c_len),
                              result=addr(res), offs=addr(offs))

    def run(dst, end, grid):
        if total_cut is not None:
            offs[cap] = end                                                 # the kernel reads its total from offs[cap]
        L.emu_copy_streams(ref(a), dst, end, grid)
    run.keep = (b1, b2, c_at, c_len, res, offs, a)
    return run, segs, total, total


def test_copy_streams_layout():
    entries = []
    for ln in range(1, 50):
        for j, r in enumerate((0, ln - 1, 1, ln, -1, (ln * 5) % ln if ln > 1 else 0)):
            entries.append(((ln * 6 + j) * 3 % 1000, ln, r))            # source positions at every residue
    assert {at % 16 for at, _, _ in entries} == set(range(16))
    for pad in (0, 1, 17, len(entries)):
        case = streams_copy_case(entries, pad, hc=bool(pad & 1))
        assert {s % 16 for s, _ in case[1]} == set(range(16))
        check_copy(f"streams sweep, {pad} padding entries", case)
    check_copy("streams only padding", streams_copy_case([], 9))
    # total > cap: the pack stops at cap (offsets that decrease can make the total exceed the bound)
    case = streams_copy_case(entries[:80], 5)
    check_copy("streams cap below the total", case, ends=[case[2] - 1, case[2] - 16, case[2] // 2, 33])
    # header lengths 1 + 1..5 + 0..5: originals and compressed lengths at the varint edges; the total is cut short behind the headers
    edges = [127, 128, 16383, 16384, 2097151, 2097152, (1 << 28) - 1, 1 << 28]
    for original in edges:
        for r in [0] + [e for e in edges if e < original]:
            case = streams_copy_case([(3, original, r), (40, 20, 7)], 2, total_cut=250)
            check_copy(f"streams original {original} result {r}", case, ends=[250, 16, 12, 11, 7, 3], grids=[1, 3])
    check_copy("streams long", streams_copy_case([(5, 4095, 0), (9000, 4097, 4096), (100, 65539, 65000), (11, 70000, 0), (7, 16, 3)], 3))
    tiny = [(k % 97, 16, 1 + k % 2) for k in range(30000)]
    check_copy("streams tiny", streams_copy_case(tiny, 1000), ends=[4 * 30000 + 15000, SPAN, SPAN + 3, 2 * SPAN, 20])


# ---- the header reader ------------------------------------------------------------------------------------------------------------
def host_outcome(buf):
    """stream.parse_chunks as (status, non-empty chunks)"""
    try:
        chunks = st.parse_chunks(bytes(buf))
    except NotImplementedError:
        return PASSES, None
    except st.EndOfStreamException:
        return EOS, None
    return OK, [c for c in chunks if c[1] != 0]


FILL = -77


def check_index(name, data, max_chunks=None, host=True):
    """stream_index_kernel on `data` against the reference walk (and stream.parse_chunks), tables included"""
    L = emu.framing()
    data = bytes(data)
    w = ref_walk(data, max_chunks)
    full = ref_walk(data)
    mc = full["chunks"] + 3 if max_chunks is None else max_chunks
    src = np.frombuffer(data + TAIL, np.uint8).copy()
    t, arr = emu.stream_tables(mc, fill=FILL)
    info = emu.StreamInfo(chunks=-5, compressed_chunks=-5, decoded_bytes=-5, error_offset=-5, error=-5, reserved=-5)
    L.emu_stream_index(addr(src), len(data), ref(t), ref(info))
    got = (info.error, info.error_offset, info.chunks, info.compressed_chunks, info.decoded_bytes, info.reserved)
    want = (w["status"], w["error_offset"], w["chunks"], w["compressed_chunks"], w["decoded_bytes"], 0)
    assert got == want, f"{name}: (status, error_offset, chunks, compressed, decoded, reserved) = {got}, want {want}; data {data[:48].hex()}"
    tabled = full["rows"][:mc]
    comp, raw = [r for r in tabled if r[0]], [r for r in tabled if not r[0]]
    exp = {k: np.full(mc + 4, FILL, np.int64) for k in ("c_src_off", "c_dst_off", "c_hdr_off", "r_dst_off", "r_src_off", "c_src_len", "c_dst_cap", "c_result", "r_len")}
    for j, r in enumerate(comp):
        exp["c_src_off"][j], exp["c_dst_off"][j], exp["c_hdr_off"][j], exp["c_src_len"][j], exp["c_dst_cap"][j] = r[2], r[5], r[1], r[3], r[4]
    for j, r in enumerate(raw):
        exp["r_dst_off"][j], exp["r_src_off"][j], exp["r_len"][j] = r[5], r[2], r[4]
    for k, v in exp.items():
        assert np.array_equal(arr[k].astype(np.int64), v), f"{name}: table {k} = {arr[k].tolist()}, want {v.tolist()}"
    assert arr["min_bad"][0] == NONE64, name
    if host and max_chunks is None:
        status, chunks = host_outcome(data)
        assert status == full["status"], f"{name}: stream.parse_chunks ends with {status}, the reference walk with {full['status']}; data {data[:48].hex()}"
        if status == OK:
            assert chunks == [(r[0], r[4], r[2], r[3]) for r in full["rows"]], name
    return w


def check_streams_index(name, streams, spare=3):
    """The same inputs as items of one batch, behind a prefix (so that no item starts at 0): the count pass, the three scans, the
    fill pass and the info, for a grid of 1, 3 and one wavefront per item"""
    L = emu.framing()
    prefix = TAIL[:37]
    n = len(streams)
    off = np.zeros(n + 1, np.int64)
    off[0] = len(prefix)
    off[1:] = len(prefix) + np.cumsum([len(s) for s in streams])
    src = np.frombuffer(prefix + b"".join(bytes(s) for s in streams) + TAIL, np.uint8).copy()
    walks = [ref_walk(s) for s in streams]
    chunks, ncomp = sum(w["chunks"] for w in walks), sum(w["compressed_chunks"] for w in walks)
    mc = chunks + spare
    exp = {k: np.full(mc + 4, FILL, np.int64) for k in ("c_src_off", "c_dst_off", "c_hdr_off", "r_dst_off", "r_src_off", "c_src_len", "c_dst_cap", "r_len", "c_item")}
    jc = jr = out = 0
    dst_off, status, err_off = [], [], []
    for i, w in enumerate(walks):
        dst_off.append(out)
        status.append(w["status"])
        err_off.append(w["error_offset"])
        at = int(off[i])
        for r in w["rows"]:
            if r[0]:
                exp["c_src_off"][jc], exp["c_dst_off"][jc], exp["c_hdr_off"][jc], exp["c_src_len"][jc], exp["c_dst_cap"][jc], exp["c_item"][jc] = at + r[2], out + r[5], r[1], r[3], r[4], i
                jc += 1
            else:
                exp["r_dst_off"][jr], exp["r_src_off"][jr], exp["r_len"][jr] = out + r[5], at + r[2], r[4]
                jr += 1
        out += w["decoded_bytes"]
    dst_off.append(out)
    bad = [i for i in range(n) if status[i] != OK]
    want_info = (n, chunks, ncomp, out, bad[0] if bad else -1, err_off[bad[0]] if bad else -1, status[bad[0]] if bad else OK, 0)
    for grid in sorted({1, 3, L.emu_walk_grid(n)}):
        for max_chunks in ((mc, chunks - 1) if chunks > 0 and grid == 3 else (mc,)):
            r = run_streams_index(src, off, n, max_chunks)
            info = r["info"]
            got = (info.items, info.chunks, info.compressed_chunks, info.decoded_bytes, info.first_error, info.error_offset, info.error, info.reserved)
            if max_chunks < chunks:                                        # the tables are too small: nothing is written to them
                assert got == want_info[:4] + (-1, -1, TABLE_FULL, 0), (name, grid, got)
                for k in exp:
                    assert (r["tables"][k] == FILL).all(), (name, grid, k)
                continue
            assert got == want_info, f"{name}: grid {grid}: info {got}, want {want_info}"
            assert r["dst_off"].tolist() == dst_off + [FILL] and r["status"].tolist() == status + [FILL] and r["error_offset"].tolist() == err_off + [FILL], \
                f"{name}: grid {grid}: first differing item {[i for i in range(n) if (r['status'][i], r['error_offset'][i], r['dst_off'][i]) != (status[i], err_off[i], dst_off[i])][:3]}"
            for k, v in exp.items():
                assert np.array_equal(r["tables"][k].astype(np.int64), v), f"{name}: grid {grid}: table {k}"
    return walks


def run_streams_index(src, off, n, max_chunks, grid=0):
    L = emu.framing()
    t, arr = emu.stream_tables(max_chunks, fill=FILL)
    arr["c_item"] = np.full(max_chunks + 4, FILL, np.int32)
    head = np.zeros(3, np.int64)                                            # [min_bad, totals[0], totals[1]]
    per_item = {k: np.full(n + 1, FILL, np.int64) for k in ("chunk_base", "comp_base", "item_bad", "dst_off", "error_offset")}
    per_item["dst_off"] = np.full(n + 2, FILL, np.int64)
    status = np.full(n + 1, FILL, np.int32)
    partial = np.full(-(-n // TILE) + 1, FILL, np.int64)
    t.min_bad = addr(head)
    ts = emu.StreamsTables(t=t, totals=addr(head, 1), chunk_base=addr(per_item["chunk_base"]), comp_base=addr(per_item["comp_base"]),
                           item_bad=addr(per_item["item_bad"]), partial=addr(partial), c_item=addr(arr["c_item"]))
    a = emu.StreamsDecodeArgs(src=addr(src), off=addr(off), src_len=src.size - len(TAIL), n=n, dst_off=addr(per_item["dst_off"]),
                              status=addr(status), error_offset=addr(per_item["error_offset"]))
    info = emu.StreamsInfo()
    L.emu_streams_index(ref(a), ref(ts), ref(info), grid)
    assert partial[-1] == FILL
    return dict(info=info, tables=arr, dst_off=per_item["dst_off"], status=status, error_offset=per_item["error_offset"], a=a, ts=ts,
                keep=(head, per_item, partial, src, off))


def enc(value, k, cont_last=False):
    """`value` as a varint of exactly k bytes (non-minimal when its high groups are zero); cont_last: the continuation bit is set
    on the last byte too (only a tenth byte ends a varint that way)"""
    out = bytearray(((value >> (7 * j)) & 0x7F) | 0x80 for j in range(k))
    if not cont_last:
        out[-1] &= 0x7F
    return bytes(out)


def top(k, group):
    """`group` as the 7-bit group of the k-th byte of a varint"""
    return group << (7 * (k - 1))


def header_cases():
    cases = []
    nxt = frame([(0, 3, b"xyz")])
    raw_payload, comp_payload = b"hello", b"\x40abc"
    # each field as a varint of every length 1..10: non-minimal, with bits in its last group, and with the tenth byte's continuation bit
    for k in range(1, 11):
        groups = [0] if k > 1 else []
        groups += [0x01, 0x10, 0x7E, 0x7F] if k > 1 else []
        variants = [(g, False) for g in groups] + ([(0, True), (0x01, True), (0x7E, True)] if k == 10 else [])
        if k == 1:
            variants = [(None, False)]
        for g, cont in variants:
            hi = top(k, g) if g is not None else 0
            tag = f"{k} bytes, last group {g}, cont {cont}"
            cases.append((f"flags raw: {tag}", enc(0 | hi, k, cont) + enc(5, 1) + raw_payload + nxt))
            cases.append((f"flags compressed: {tag}", enc(1 | hi, k, cont) + enc(9, 1) + enc(4, 1) + comp_payload + nxt))
            cases.append((f"original raw: {tag}", enc(0, 1) + enc(5 | hi, k, cont) + raw_payload + nxt))
            cases.append((f"original compressed: {tag}", enc(1, 1) + enc(9 | hi, k, cont) + enc(4, 1) + comp_payload + nxt))
            cases.append((f"clen: {tag}", enc(1, 1) + enc(9, 1) + enc(4 | hi, k, cont) + comp_payload + nxt))
            cases.append((f"all three: {tag}", enc(1 | (hi if k > 5 else 0), k, cont) + enc(9 | (hi if k > 5 else 0), k, cont) + enc(4 | (hi if k > 5 else 0), k, cont) + comp_payload + nxt))
    # values
    v = st.write_varint
    for name, data in [
        ("original with bit 31 raw", v(0) + v(1 << 31) + raw_payload),
        ("original with bit 31 compressed", v(1) + v(1 << 31) + v(4) + comp_payload),
        ("original 0xFFFFFFFF raw", v(0) + v(0xFFFFFFFF) + raw_payload),
        ("original 2^32 + 5 raw", v(0) + v((1 << 32) + 5) + raw_payload + nxt),
        ("original 2^32 + 9 compressed", v(1) + v((1 << 32) + 9) + v(4) + comp_payload + nxt),
        ("clen 2^32 + 4", v(1) + v(9) + v((1 << 32) + 4) + comp_payload + nxt),
        ("clen with bit 31", v(1) + v(9) + v((1 << 31) + 4) + comp_payload + nxt),
        ("clen 0xFFFFFFFF, original 0xFFFFFFFF", v(1) + v(0xFFFFFFFF) + v(0xFFFFFFFF) + comp_payload + nxt),
        ("clen == original", v(1) + v(4) + v(4) + comp_payload + nxt),
        ("clen == original + 1", v(1) + v(3) + v(4) + comp_payload + nxt),
        ("original 0 raw", v(0) + v(0) + nxt),
        ("original 0 compressed", v(1) + v(0) + v(0) + nxt),
        ("original 0 compressed with a passes bit", v(5) + v(0) + v(0) + nxt),
        ("original 0 raw, twice, then the end", v(0) + v(0) + v(2) + v(0)),
        ("clen 0, original 7", v(1) + v(7) + v(0) + nxt),
        ("payload ends with the buffer", v(0) + v(5) + raw_payload),
        ("payload one byte short", v(0) + v(6) + raw_payload),
        ("compressed payload ends with the buffer", nxt + v(1) + v(9) + v(4) + comp_payload),
        ("compressed payload one byte short", nxt + v(1) + v(9) + v(5) + comp_payload),
        ("nothing", b""),
    ]:
        cases.append((name, data))
    # passes bits: in the first byte, the second, at bits 31, 32, 35, 63 and in the tenth byte's bits 1..6; raw (accepted) and compressed
    passes = [("bit 2", 4), ("bits 2..6", 0x7C), ("bit 7", 1 << 7), ("bit 13", 1 << 13), ("bit 28", 1 << 28), ("bit 31", 1 << 31), ("bit 32", 1 << 32),
              ("bit 35", 1 << 35), ("bits 32..62", ((1 << 63) - 1) ^ 0xFFFFFFFF), ("bit 63", 1 << 63)]
    for name, bits in passes:
        for hc in (0, 2):
            cases.append((f"passes {name} raw hc {hc}", v(bits | hc) + v(5) + raw_payload + nxt))
            cases.append((f"passes {name} compressed hc {hc}", v(bits | hc | 1) + v(9) + v(4) + comp_payload + nxt))
    for g in (0x02, 0x40, 0x7E, 0x7F):
        cases.append((f"tenth byte {g:#x} raw", enc(0 | top(10, g), 10) + v(5) + raw_payload + nxt))
        cases.append((f"tenth byte {g:#x} compressed", enc(1 | top(10, g), 10) + v(9) + v(4) + comp_payload + nxt))
    # the two streams of the issue: flags 81 80 80 80 80 01 (bit 35, low 32 bits = 1) and a tenth byte of 0x7E
    cases.append(("flags 81 80 80 80 80 01", bytes.fromhex("818080808001") + v(9) + v(4) + comp_payload + nxt))
    cases.append(("flags 81 80 x 8 7e", bytes.fromhex("8180808080808080807e") + v(9) + v(4) + comp_payload + nxt))
    # a header in the last 1..30 bytes of the buffer
    for j in range(2, 31):
        cases.append((f"raw chunk in the last {j} bytes", nxt + v(0) + v(j - 2) + bytes(range(j - 2))))
    long_header = enc(1, 10) + enc(0, 10) + enc(0, 10)                      # 30 header bytes, no payload
    for cut in range(0, 31):
        cases.append((f"30-byte header cut to {cut}", nxt + long_header[:cut]))
    cases.append(("30-byte header, twice", long_header + long_header + nxt))
    cases.append(("29-byte header with a 3-byte payload", nxt + enc(1, 10) + enc(7, 10) + enc(3, 9) + b"abc"))
    return cases


FIVE = frame([(1, 300, bytes(range(40))), (0, 7, b"7 bytes"), (0, 0, b""), (3, 1000, bytes(200), 200), (2, 130, bytes(130)), (1, 20, b"\x11" * 19)])


def test_header_cases():
    cases = header_cases()
    for name, data in cases:
        check_index(name, data)
    check_streams_index("header cases", [d for _, d in cases])


def test_header_every_prefix():
    """a valid stream of five non-empty chunks (and an empty one) cut at every byte"""
    assert ref_walk(FIVE)["chunks"] == 5 and ref_walk(FIVE)["status"] == OK
    for cut in range(len(FIVE) + 1):
        check_index(f"prefix {cut}", FIVE[:cut])
    check_streams_index("prefixes", [FIVE[:cut] for cut in range(len(FIVE) + 1)])


def test_header_table_full():
    n = ref_walk(FIVE)["chunks"]
    for data, name in ((FIVE, "valid"), (FIVE + b"\x81", "with a truncated header behind it"), (FIVE + b"\x05\x03\x01", "with passes behind it")):
        for mc in (0, 1, n - 1, n, n + 1):
            w = check_index(f"{name}, max_chunks {mc}", data, max_chunks=mc)
            assert w["chunks"] == n and (w["status"] == TABLE_FULL) == (mc < n), (name, mc)


def fuzz_stream(rng):
    """a valid stream of 2..6 chunks, the byte ranges of its headers"""
    out, heads = bytearray(), []
    for _ in range(int(rng.integers(2, 7))):
        compressed = bool(rng.integers(0, 2))
        original = int(rng.integers(1, 300)) if compressed or rng.integers(0, 8) else 0
        clen = int(rng.integers(1, original + 1)) if compressed else original
        flags = (1 if compressed else 0) | (2 if rng.integers(0, 2) else 0)
        fields = [flags, original] + ([clen] if compressed else [])
        head = b"".join(enc(f, max(len(st.write_varint(f)), int(rng.integers(1, 4)))) if rng.integers(0, 4) == 0 else st.write_varint(f) for f in fields)
        heads.append((len(out), len(out) + len(head)))
        out += head + rng.integers(0, 256, clen, dtype=np.uint8).tobytes()
    return out, heads


FUZZ_SEEDS = (11, 12, 13, 14, 15, 16, 17, 18)
FUZZ_PER_SEED = 256


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_header_fuzz(seed):
    """valid streams with 1..3 random byte edits inside header regions: kernel, reference walk and stream.parse_chunks agree"""
    assert len(FUZZ_SEEDS) * FUZZ_PER_SEED >= 2000
    rng = np.random.default_rng(seed)
    streams = []
    for index in range(FUZZ_PER_SEED):
        data, heads = fuzz_stream(rng)
        for _ in range(int(rng.integers(1, 4))):
            lo, hi = heads[int(rng.integers(0, len(heads)))]
            p = int(rng.integers(lo, hi))
            data[p] = int(rng.integers(0, 256)) if rng.integers(0, 2) else data[p] ^ (1 << int(rng.integers(0, 8)))
        check_index(f"fuzz seed {seed} index {index}", bytes(data))
        streams.append(bytes(data))
    check_streams_index(f"fuzz seed {seed}", streams)


# ---- the kernel sequences of lz4hip_framing.hpp around a block codec that is the test's ----------------------------------------------
PIPE_BLOCKS = (16, 17, 127, 128, 4096)
MODE_FAST, MODE_HC = 0, 1


def lib_scratch(which, *args):
    """(guarded buffer of exactly the bytes lz4hip_framing.hpp's size function `which` returns, address, size)"""
    size = emu.framing().emu_scratch_bytes(which, *(list(args) + [0, 0])[:3])
    buf, ptr = guarded(size)
    return buf, ptr, size


def untouched(buf):
    return np.array_equal(buf, pattern(buf.size))


def guards_intact(buf):
    want = pattern(buf.size)
    return np.array_equal(buf[:GUARD], want[:GUARD]) and np.array_equal(buf[-GUARD:], want[-GUARD:])


def filled(n, dtype=np.int64):
    return np.full(n, FILL, dtype)


def lib_stream_encode(name, data, B, results, comp, hc, gi, gc, want):
    """the whole stream_encode (front, layout, sequence) on a scratch buffer of exactly the size asked for, then on one a byte short"""
    L = emu.framing()
    n = -(-data.size // B)
    bound = data.size + n * (1 + 2 * len(st.write_varint(B))) if data.size else 0
    src = np.ascontiguousarray(np.concatenate([data, np.zeros(1, np.uint8)]))
    res = np.array(list(results) + [0], np.int32)
    for short in (0, 1):
        scratch, sptr, size = lib_scratch(0, data.size, B)
        dst_len = filled(3)
        buf, ptr = guarded(bound)
        rc = L.emu_lib_stream_encode(addr(src), data.size, B, MODE_HC if hc else MODE_FAST, ptr, bound, addr(dst_len, 1), sptr, size - short,
                                     addr(res), addr(comp), gi, gc)
        if short:
            assert rc == E_ARGUMENT and untouched(buf) and untouched(scratch) and (dst_len == FILL).all(), (name, rc)
            continue
        assert rc == 0 and dst_len.tolist() == [FILL, len(want), FILL] and guards_intact(scratch), (name, rc, dst_len.tolist())
        same(buf, ref_copy(bound, [(0, want)], len(want)), f"{name}: whole, grids {gi}, {gc}")
        if data.size == 0:
            assert size == 0 and untouched(buf), name                       # src_len == 0: *dst_len = 0 and nothing else


def pipe_lengths(B):
    return [0, 1, B - 1, B, B + 1, 5 * B + 3]


def run_stream_encode(data, B, results, comp, hc, grid_items, grid_copy):
    L = emu.framing()
    n = -(-data.size // B)
    bound = data.size + n * (1 + 2 * len(st.write_varint(B))) if data.size else 0
    res = np.array(results, np.int32).reshape(n)
    offs = np.full(n + 2, FILL, np.int64)
    lens = np.full(n + 2, FILL, np.int32)
    partial = np.full(-(-n // TILE) + 2, FILL, np.int64)
    dst_len = np.full(1, FILL, np.int64)
    src = np.ascontiguousarray(data)
    a = emu.StreamEncodeArgs(src=addr(src), comp=addr(comp), src_len=data.size, n=n, block=B, hc_flag=2 if hc else 0, result=addr(res), offs=addr(offs))
    buf, ptr = guarded(bound)
    L.emu_stream_encode(ref(a), addr(lens), addr(partial), ptr, addr(dst_len), bound, grid_items, grid_copy)
    assert lens[:n].tolist() == [min(B, data.size - k * B) for k in range(n)] and (lens[n:] == FILL).all() and (offs[n:] == FILL).all()
    return buf, int(dst_len[0]), bound


def check_stream_encode(name, data, B, results, comp, hc, want):
    n = -(-data.size // B)
    for gi in item_grids(n):
        for gc in copy_grids(data.size + n * (1 + 2 * len(st.write_varint(B)))):
            buf, total, bound = run_stream_encode(data, B, results, comp, hc, gi, gc)
            assert total == len(want) <= bound, (name, total, len(want))
            same(buf, ref_copy(bound, [(0, want)], len(want)), f"{name}: grids {gi}, {gc}")
            lib_stream_encode(name, data, B, results, comp, hc, gi, gc, want)


@pytest.mark.parametrize("B", PIPE_BLOCKS)
def test_pipeline_stream_encode(oracle, B):
    for hc in (False, True):
        for size in pipe_lengths(B):
            data = mixed(oracle, size, B)
            n = -(-size // B)
            comp = noise(size + 16, 9)
            results = []
            for k in range(n):
                chunk = data[k * B:(k + 1) * B]
                r, buf = oracle.compress_raw(chunk, chunk.size, hc=hc)
                results.append(r)
                if r > 0:
                    comp[k * B:k * B + r] = buf[:r]
            check_stream_encode(f"block {B}, {size} bytes, hc {hc}", data, B, results, comp, hc, expected_stream(oracle, data, B, hc))
            if hc:
                continue
            # results no encoder would return: the rule is "compressed iff 0 < r < length", whatever the bytes
            forced = {"0": lambda ln, k: 0, "-1": lambda ln, k: -1, "len": lambda ln, k: ln, "len - 1": lambda ln, k: ln - 1, "1": lambda ln, k: 1,
                      "mixed": lambda ln, k: (0, -1, ln, ln - 1, 1, ln + 1)[k % 6]}
            for fname, f in forced.items():
                comp = noise(size + 16, 10)
                results, chunks = [], []
                for k in range(n):
                    chunk = data[k * B:(k + 1) * B]
                    r = f(chunk.size, k)
                    results.append(r)
                    c = 0 < r < chunk.size
                    chunks.append((1 if c else 0, chunk.size, comp[k * B:k * B + r] if c else chunk))
                check_stream_encode(f"block {B}, {size} bytes, forced {fname}", data, B, results, comp, False, frame(chunks))


def run_stream_decode(stream, results, decoded, grid_items, grid_copy, spare=2):
    """-> (index info, final info, guarded output, capacity)"""
    L = emu.framing()
    w = ref_walk(stream)
    src = np.frombuffer(bytes(stream) + TAIL, np.uint8).copy()
    t, arr = emu.stream_tables(w["chunks"] + spare, fill=FILL)
    res = np.array(list(results) + [0], np.int32)
    dec = np.ascontiguousarray(np.concatenate([decoded, np.zeros(8, np.uint8)]))
    cap = w["decoded_bytes"] + 24
    buf, ptr = guarded(cap)
    index_info, info = emu.StreamInfo(), emu.StreamInfo()
    assert L.emu_stream_decode(addr(src), len(stream), ref(t), addr(res), addr(dec), ptr, ref(index_info), ref(info), grid_items, grid_copy) == 0
    assert (index_info.error, index_info.error_offset, index_info.chunks) == (w["status"], w["error_offset"], w["chunks"])
    return index_info, info, buf, cap


def lib_stream_decode(stream, results, decoded, grid_items, grid_copy, spare=2):
    """run_stream_decode through the whole stream_index and stream_decode, tables in a scratch buffer of exactly the size asked for"""
    L = emu.framing()
    w = ref_walk(stream)
    src = np.frombuffer(bytes(stream) + TAIL, np.uint8).copy()
    mc = w["chunks"] + spare
    res = np.array(list(results) + [0], np.int32)
    dec = np.ascontiguousarray(np.concatenate([decoded, np.zeros(8, np.uint8)]))
    cap = w["decoded_bytes"] + 24
    for short in (1, 0):
        scratch, sptr, size = lib_scratch(1, mc)
        buf, ptr = guarded(cap)
        index_info, info = emu.StreamInfo(chunks=FILL), emu.StreamInfo(chunks=FILL)
        rc = L.emu_lib_stream_index(addr(src), len(stream), mc, sptr, size - short, ref(index_info))
        if short:
            good = emu.StreamInfo(chunks=w["chunks"], compressed_chunks=w["compressed_chunks"], decoded_bytes=w["decoded_bytes"], error_offset=-1)
            rc2 = L.emu_lib_stream_decode(addr(src), ref(good), mc, sptr, size - 1, ptr, cap, ref(info), addr(res), addr(dec), grid_items, grid_copy)
            assert rc == rc2 == E_ARGUMENT and index_info.chunks == info.chunks == FILL and untouched(scratch) and untouched(buf)
            continue
        assert rc == 0 and (index_info.error, index_info.error_offset, index_info.chunks) == (w["status"], w["error_offset"], w["chunks"])
        assert L.emu_lib_stream_decode(addr(src), ref(index_info), mc, sptr, size, ptr, cap, ref(info), addr(res), addr(dec), grid_items, grid_copy) == 0
        assert guards_intact(scratch)
    return index_info, info, buf, cap


def both_stream_decodes(*args):
    """the sequences over the test's tables, then the whole functions over a scratch buffer: the same outcome is expected of both"""
    yield run_stream_decode(*args)
    yield lib_stream_decode(*args)


@pytest.mark.parametrize("B", PIPE_BLOCKS)
def test_pipeline_stream_decode(oracle, B):
    for size in pipe_lengths(B):
        data = mixed(oracle, size, B + 1)
        stream = expected_stream(oracle, data, B, False)
        rows = ref_walk(stream)["rows"]
        good = [r[3] for r in rows if r[0]]
        for gi in item_grids(len(good)):
            for gc in copy_grids(size):
                for _, info, buf, cap in both_stream_decodes(stream, good, data, gi, gc):
                    assert (info.error, info.error_offset, info.chunks, info.decoded_bytes) == (OK, -1, len(rows), size), (B, size)
                    same(buf, ref_copy(cap, [(0, data)], size), f"block {B}, {size} bytes, grids {gi}, {gc}")


def test_pipeline_stream_decode_errors(oracle):
    """the corrupt block FIRST in stream order is reported, before any later header error, whatever the grid and the order of arrival"""
    parts = [mixed(oracle, 700, k) if k % 3 != 1 else noise(90, k) for k in range(9)]
    chunks = []
    for k, p in enumerate(parts):
        r, buf = oracle.compress_raw(p, p.size)
        chunks.append((1, p.size, buf[:r]) if 0 < r < p.size and k % 3 != 1 else (0, p.size, p))
    assert [c[0] for c in chunks] == [1, 0, 1, 1, 0, 1, 1, 0, 1]
    data = np.concatenate(parts)
    for tail, n_tabled in ((b"", 9), (b"\x81", 9)):
        stream = frame(chunks[:5]) + tail + (frame(chunks[5:]) if not tail else b"")
        w = ref_walk(stream)
        assert w["status"] == (EOS if tail else OK) and w["chunks"] == (5 if tail else 9)
        comp_rows = [r for r in w["rows"] if r[0]]
        hdr = [r[1] for r in comp_rows]
        assert hdr[1] == len(frame(chunks[:2]))                            # chunk 2 is the second compressed chunk
        for bad in ([1], [1, 2], [2, 1], list(range(len(comp_rows)))[::-1], [len(comp_rows) - 1], []):
            results = [r[3] - (1 if j in bad else 0) for j, r in enumerate(comp_rows)]
            for gi in (1, 3, 0):
                for index_info, info, buf, cap in both_stream_decodes(stream, results, data, gi, 0):
                    if bad:
                        want = (CORRUPT_BLOCK, hdr[min(bad)])
                    else:
                        want = (w["status"], w["error_offset"])
                    assert (info.error, info.error_offset) == want, (tail, bad, gi, info.error, info.error_offset)
                    assert (info.chunks, info.compressed_chunks, info.decoded_bytes) == (w["chunks"], len(comp_rows), w["decoded_bytes"])
                    same(buf, ref_copy(cap, [(0, data[:w["decoded_bytes"]])], w["decoded_bytes"]), f"errors {tail} {bad} {gi}")


def test_stream_check_kernel_takes_the_minimum():
    """corrupt rows whose header offsets DESCEND with the row index, one workgroup: the lowest offset must win"""
    L = emu.framing()
    n = 700
    t, arr = emu.stream_tables(n)
    arr["c_hdr_off"][:n] = np.arange(n, 0, -1) * 10
    arr["c_src_len"][:n] = 5
    arr["c_result"][:n] = 5
    for bad in ([3, 400, 699], [0], [699, 1], list(range(n))):
        for grid in (1, 3, 0):
            arr["c_result"][:n] = 5
            arr["c_result"][bad] = 4
            arr["min_bad"][0] = NONE64
            L.emu_stream_check(ref(t), n, grid)
            assert arr["min_bad"][0] == min(int(arr["c_hdr_off"][j]) for j in bad), (bad, grid)


# -- wrap
def wrap_messages(oracle):
    msgs = [np.zeros(0, np.uint8), mixed(oracle, 300, 1), noise(50, 2), np.zeros(0, np.uint8), np.zeros(0, np.uint8), mixed(oracle, 5000, 3), noise(1, 4),
            np.zeros(4096, np.uint8), noise(4097, 5), mixed(oracle, 70000, 6), np.zeros(13, np.uint8), noise(12, 7), np.zeros(0, np.uint8)]
    return msgs + [mixed(oracle, 40 + 3 * k, k) for k in range(300)]


def run_wrap(msgs, off, enc, comp, grid_items, grid_copy):
    L = emu.framing()
    n = len(off) - 1
    src = np.ascontiguousarray(np.concatenate(msgs + [np.zeros(1, np.uint8)]))
    src_len = src.size - 1
    bound = src_len + 8 * n
    dst_off = np.full(n + 2, FILL, np.int64)
    at, lens, result = np.full(n + 1, FILL, np.int64), np.full(n + 1, FILL, np.int32), np.full(n + 1, FILL, np.int32)
    partial = np.full(-(-n // TILE) + 1, FILL, np.int64)
    e = np.array(enc, np.int32)
    a = emu.WrapArgs(src=addr(src), comp=addr(comp), off=addr(off), src_len=src_len, n=n, enc=addr(e), dst_off=addr(dst_off))
    buf, ptr = guarded(bound)
    L.emu_wrap(ref(a), addr(at), addr(lens), addr(result), addr(partial), ptr, bound, bound, grid_items, grid_copy)
    assert dst_off[n + 1] == FILL and at[n] == FILL and lens[n] == FILL and result[n] == FILL and partial[-1] == FILL
    return buf, bound, dst_off[:n + 1], at[:n], lens[:n], result[:n]


def lib_wrap(msgs, off, enc, comp, grid_items, grid_copy, short=0):
    """run_wrap through the whole wrap_encode: the encoder's results and bytes are handed in, the scratch has exactly the size asked for"""
    L = emu.framing()
    n = len(off) - 1
    src = np.ascontiguousarray(np.concatenate(msgs + [np.zeros(1, np.uint8)]))
    src_len = src.size - 1
    bound = src_len + 8 * n
    dst_off, result = filled(n + 2), filled(n + 1, np.int32)
    e = np.array(list(enc) + [0], np.int32)
    scratch, sptr, size = lib_scratch(2, n, src_len)
    buf, ptr = guarded(bound)
    rc = L.emu_lib_wrap(addr(src), src_len, addr(off), n, MODE_FAST, ptr, bound, addr(dst_off), addr(result), sptr, size - short, addr(e), addr(comp),
                        grid_items, grid_copy)
    if short:
        assert rc == E_ARGUMENT and untouched(buf) and untouched(scratch) and (dst_off == FILL).all() and (result == FILL).all()
        return None
    assert rc == 0 and dst_off[n + 1] == FILL and result[n] == FILL and guards_intact(scratch)
    return buf, bound, dst_off[:n + 1], result[:n]


def test_pipeline_wrap(oracle):
    msgs = wrap_messages(oracle)
    n = len(msgs)
    good_off = np.zeros(n + 1, np.int64)
    good_off[1:] = np.cumsum([m.size for m in msgs])
    src_len = int(good_off[n])
    for variant in ("oracle", "forced", "bad offsets"):
        off = good_off.copy()
        if variant == "bad offsets":
            off[3] = off[2] - 7                                             # message 2 ends before it starts, message 3 starts there
            off[20] = src_len + 5                                           # messages 19 and 20 reach outside the buffer
            off[40] = -1                                                    # messages 39 and 40 start or end below 0
        comp = noise(src_len + 16, 11)
        enc, want, want_off, want_result, want_at, want_len = [], b"", [], [], [], []
        for k in range(n):
            a, b = int(off[k]), int(off[k + 1])
            want_off.append(len(want))
            if a < 0 or b < a or b > src_len:
                enc.append(3)
                want_result.append(E_ARGUMENT)
                want_at.append(0)
                want_len.append(0)
                continue
            m = np.concatenate(msgs)[a:b]
            if variant == "forced":
                r = (0, -1, m.size, m.size - 1, 1, m.size + 1)[k % 6]
            else:
                r, buf = oracle.compress_raw(m, m.size)
                if r > 0:
                    comp[a:a + r] = buf[:r]
            enc.append(r)
            c = 0 < r < m.size
            want += header_wrap(m.size, r if c else m.size) + (comp[a:a + r] if c else m).tobytes()
            want_result.append(r if c else 0)
            want_at.append(a)
            want_len.append(m.size)
        want_off.append(len(want))
        for gi in item_grids(n):
            for gc in copy_grids(src_len + 8 * n):
                buf, bound, dst_off, at, lens, result = run_wrap(msgs, off, enc, comp, gi, gc)
                what = f"wrap {variant}: grids {gi}, {gc}"
                assert dst_off.tolist() == want_off and result.tolist() == want_result and at.tolist() == want_at and lens.tolist() == want_len, what
                same(buf, ref_copy(bound, [(0, want)], len(want)), what)
                buf, bound, dst_off, result = lib_wrap(msgs, off, enc, comp, gi, gc)
                assert dst_off.tolist() == want_off and result.tolist() == want_result, what
                same(buf, ref_copy(bound, [(0, want)], len(want)), what + ", whole")
        lib_wrap(msgs, off, enc, comp, 0, 0, short=1)


def lib_unwrap(src, off, src_len, n, results, decoded, total, grid_items, grid_copy):
    """the whole unwrap_index and unwrap_decode on a scratch buffer of exactly the size asked for (and refused on one a byte short)
    -> (index info, final info, output offsets, statuses after the index, final statuses, guarded output)"""
    L = emu.framing()
    res = np.array(list(results) + [0], np.int32)
    for short in (1, 0):
        scratch, sptr, size = lib_scratch(3, n)
        dst_off, st_arr = filled(n + 2), filled(n + 1, np.int32)
        buf, ptr = guarded(total + 24)
        index_info, info = emu.UnwrapInfo(messages=FILL), emu.UnwrapInfo(messages=FILL)
        rc = L.emu_lib_unwrap_index(addr(src), src_len, addr(off), n, addr(dst_off), addr(st_arr), sptr, size - short, ref(index_info), grid_items)
        if short:
            good = emu.UnwrapInfo(messages=n)
            rc2 = L.emu_lib_unwrap_decode(addr(src), src_len, addr(off), n, ref(good), sptr, size - 1, ptr, total + 24, addr(dst_off), addr(st_arr),
                                          ref(info), addr(res), addr(decoded), grid_items, grid_copy)
            assert rc == rc2 == E_ARGUMENT and index_info.messages == info.messages == FILL
            assert untouched(scratch) and untouched(buf) and (dst_off == FILL).all() and (st_arr == FILL).all()
            continue
        assert rc == 0
        index_status = st_arr.copy()
        assert L.emu_lib_unwrap_decode(addr(src), src_len, addr(off), n, ref(index_info), sptr, size, ptr, total + 24, addr(dst_off), addr(st_arr),
                                       ref(info), addr(res), addr(decoded), grid_items, grid_copy) == 0
        assert guards_intact(scratch)
    return index_info, info, dst_off, index_status, st_arr, buf


def test_pipeline_unwrap(oracle):
    L = emu.framing()
    plain = [mixed(oracle, 300, 1), noise(33, 2), mixed(oracle, 5000, 3), np.zeros(100, np.uint8), noise(4100, 4)]
    wrapped, truth = [], []

    def add(m, data=b""):
        wrapped.append(np.frombuffer(bytes(m), np.uint8))
        truth.append(bytes(data))
    for p in plain:
        c = oracle.compress(p)
        if c.size < p.size:
            add(header_wrap(p.size, c.size) + c.tobytes(), p.tobytes())
        add(header_wrap(p.size, p.size) + p.tobytes(), p.tobytes())                    # stored raw
    add(header_wrap(0, 0))                                                             # an empty message
    add(b"")                                                                            # too short: 0 .. 7 bytes
    add(b"\x01\x00\x00\x00\x00\x00\x00")
    add(header_wrap(10, 3) + b"ab")                                                     # payloadLength past the end
    add(header_wrap(10, -1) + b"abc")                                                   # negative payloadLength
    add(header_wrap(-5, 3) + b"abcd", b"abc")                                           # negative originalLength: the payload as it is, the 4th byte ignored
    add(header_wrap(2, 5) + b"abcde", b"abcde")                                         # compressed > original: the payload as it is
    add(header_wrap(-2147483648, 0), b"")
    add(header_wrap(2147483647, 2147483647) + b"x")                                     # corrupt header: far past the end
    add(header_wrap(40, 4) + b"\x40abc", bytes(40))                                     # compressed (the test supplies the decoder's bytes)
    add(header_wrap(1, 0), b"\x07")                                                     # compressed from an empty payload
    for k in range(600):
        add(header_wrap(k % 50, k % 50) + bytes([k & 0xFF]) * (k % 50), bytes([k & 0xFF]) * (k % 50))
    n = len(wrapped)
    src = np.ascontiguousarray(np.concatenate(wrapped + [np.frombuffer(header_wrap(3, 3) + b"abc", np.uint8)]))
    good_off = np.zeros(n + 1, np.int64)
    good_off[1:] = np.cumsum([m.size for m in wrapped])
    src_len = int(good_off[n])
    for variant in ("good offsets", "bad offsets", "corrupt blocks"):
        off = good_off.copy()
        if variant == "bad offsets":
            off[5] = off[4] - 1
            off[30] = src_len + 1
            off[0] = 0
            off[60] = -3
        refs = []
        for k in range(n):
            a, b = int(off[k]), int(off[k + 1])
            refs.append((E_ARGUMENT, None, 0, 0) if a < 0 or b < a or b > src_len else ref_unwrap(src[a:b]))
        comp = [k for k in range(n) if refs[k][1] == "comp"]
        sizes = [r[2] for r in refs]
        want_off = [0] + np.cumsum(sizes).tolist()
        total = want_off[-1]
        bad_rows = [1, len(comp) - 1] if variant == "corrupt blocks" else []
        results = [refs[k][3] - (1 if j in bad_rows else 0) for j, k in enumerate(comp)]
        status = [r[0] for r in refs]
        decoded = pattern(total + 8) ^ 0xFF                                 # what the decoder "writes": recognisable, not the prefill
        segs = []
        for k in range(n):
            if refs[k][1] == "raw":
                a = int(off[k]) + 8
                segs.append((want_off[k], src[a:a + refs[k][3]]))
                if variant == "good offsets":
                    assert src[a:a + refs[k][3]].tobytes() == truth[k], k
            elif refs[k][1] == "comp":
                segs.append((want_off[k], decoded[want_off[k]:want_off[k + 1]]))
        final_status = list(status)
        for j in bad_rows:
            final_status[comp[j]] = WRAP_CORRUPT_BLOCK
        for gi in item_grids(n):
            for gc in copy_grids(total):
                dst_off = np.full(n + 2, FILL, np.int64)
                st_arr = np.full(n + 1, FILL, np.int32)
                tabs = {k: np.full(n + 1, FILL, np.int64) for k in ("cidx", "c_src_off", "c_dst_off", "c_msg")}
                tabs.update({k: np.full(n + 1, FILL, np.int32) for k in ("c_src_len", "c_dst_cap", "c_result", "raw_len")})
                head = np.full(2, 12345, np.int64)
                partial = np.full(-(-n // TILE) + 1, FILL, np.int64)
                t = emu.UnwrapTables(n=n, min_bad=addr(head), ncomp=addr(head, 1), partial=addr(partial), **{k: addr(v) for k, v in tabs.items()})
                a = emu.UnwrapArgs(src=addr(src), off=addr(off), src_len=src_len, n=n, dst_off=addr(dst_off), status=addr(st_arr))
                index_info, info = emu.UnwrapInfo(), emu.UnwrapInfo()
                L.emu_unwrap_index(ref(a), ref(t), ref(index_info), gi)
                what = f"unwrap {variant}: grids {gi}, {gc}"
                first = min([k for k in range(n) if status[k] != WRAP_OK], default=-1)
                got = (index_info.messages, index_info.compressed, index_info.decoded_bytes, index_info.first_error, index_info.error, index_info.reserved)
                assert got == (n, len(comp), total, first, status[first] if first >= 0 else WRAP_OK, 0), (what, got)
                assert dst_off.tolist() == want_off + [FILL] and st_arr.tolist() == status + [FILL], what
                m = len(comp)
                assert tabs["c_msg"][:m].tolist() == comp and (tabs["c_msg"][m:] == FILL).all(), what
                assert tabs["c_src_off"][:m].tolist() == [int(off[k]) + 8 for k in comp] and tabs["c_src_len"][:m].tolist() == [refs[k][3] for k in comp], what
                assert tabs["c_dst_off"][:m].tolist() == [want_off[k] for k in comp] and tabs["c_dst_cap"][:m].tolist() == [sizes[k] for k in comp], what
                assert tabs["raw_len"][:n].tolist() == [r[3] if r[1] == "raw" else (-1 if r[1] == "comp" else 0) for r in refs], what
                buf, ptr = guarded(total + 24)
                res = np.array(results + [0], np.int32)
                L.emu_unwrap_decode(ref(a), ref(t), ref(index_info), addr(res), addr(decoded), ptr, ref(info), gi, gc)
                first = min([k for k in range(n) if final_status[k] != WRAP_OK], default=-1)
                got = (info.messages, info.compressed, info.decoded_bytes, info.first_error, info.error)
                assert got == (n, len(comp), total, first, final_status[first] if first >= 0 else WRAP_OK), (what, got)
                assert st_arr.tolist() == final_status + [FILL] and dst_off.tolist() == want_off + [FILL], what
                same(buf, ref_copy(total + 24, segs, total), what)
                index_info, info, dst_off, index_status, st_arr, buf = lib_unwrap(src, off, src_len, n, results, decoded, total, gi, gc)
                first = min([k for k in range(n) if status[k] != WRAP_OK], default=-1)
                got = (index_info.messages, index_info.compressed, index_info.decoded_bytes, index_info.first_error, index_info.error, index_info.reserved)
                assert got == (n, len(comp), total, first, status[first] if first >= 0 else WRAP_OK, 0), (what, got)
                first = min([k for k in range(n) if final_status[k] != WRAP_OK], default=-1)
                got = (info.messages, info.compressed, info.decoded_bytes, info.first_error, info.error)
                assert got == (n, len(comp), total, first, final_status[first] if first >= 0 else WRAP_OK), (what, got)
                assert index_status.tolist() == status + [FILL] and st_arr.tolist() == final_status + [FILL] and dst_off.tolist() == want_off + [FILL], what
                same(buf, ref_copy(total + 24, segs, total), what + ", whole")


# -- batches of streams
def streams_items(oracle, B):
    e = np.zeros(0, np.uint8)
    return [e, e, mixed(oracle, 1, 1), mixed(oracle, B - 1, 2), e, mixed(oracle, B, 3), noise(B + 1, 4), e, e, e, mixed(oracle, 5 * B + 3, 5),
            noise(3 * B, 6), mixed(oracle, 2 * B + 1, 7), e]


@pytest.mark.parametrize("B", PIPE_BLOCKS)
def test_pipeline_streams_encode(oracle, B):
    L = emu.framing()
    items = streams_items(oracle, B)
    n = len(items)
    src = np.ascontiguousarray(np.concatenate(items + [np.zeros(1, np.uint8)]))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([m.size for m in items])
    src_len = int(off[n])
    cap = src_len // B + n
    bound = src_len + cap * (1 + 2 * len(st.write_varint(B)))
    table = [(int(off[i]) + o, min(B, items[i].size - o)) for i in range(n) for o in range(0, items[i].size, B)]
    K = len(table)
    assert K < cap
    for hc in (False, True):
        want = [expected_stream(oracle, m, B, hc) for m in items]
        want_off = [0] + np.cumsum([len(w) for w in want]).tolist()
        for gi in item_grids(cap):
            for gc in copy_grids(bound):
                first = np.full(n + 1, FILL, np.int64)
                head = np.full(2, FILL, np.int64)
                c_at, c_len, res = np.full(cap + 1, FILL, np.int64), np.full(cap + 1, FILL, np.int32), np.full(cap + 1, 9, np.int32)
                offs = np.full(cap + 2, FILL, np.int64)
                partial = np.full(-(-cap // TILE) + 1, FILL, np.int64)
                comp = noise(src_len + 16, 12)
                dst_off = np.full(n + 2, FILL, np.int64)
                a = emu.StreamsEncodeArgs(src=addr(src), comp=addr(comp), off=addr(off), src_len=src_len, n=n, cap=cap, block=B, hc_flag=2 if hc else 0,
                                          first=addr(first), total=addr(head), c_at=addr(c_at), c_len=addr(c_len), result=addr(res), offs=addr(offs))
                L.emu_streams_plan(ref(a), addr(partial), gi)
                what = f"streams encode block {B} hc {hc}: grids {gi}, {gc}"
                assert head.tolist() == [K, FILL] and first[n] == FILL and c_at[cap] == FILL and c_len[cap] == FILL, what
                assert list(zip(c_at[:K].tolist(), c_len[:K].tolist())) == table and (c_len[K:cap] == 0).all() and (c_at[K:cap] == 0).all(), what
                for k, (at, ln) in enumerate(table):                            # the block encoder's part, by the oracle
                    r, buf = oracle.compress_raw(src[at:at + ln], ln, hc=hc)
                    res[k] = r
                    if r > 0:
                        comp[at:at + r] = buf[:r]
                out, ptr = guarded(bound)
                L.emu_streams_pack(ref(a), addr(partial), addr(dst_off), ptr, bound, bound, gi, gc)
                assert dst_off.tolist() == want_off + [FILL] and offs[cap] == want_off[-1] and offs[cap + 1] == FILL and partial[-1] == FILL, what
                same(out, ref_copy(bound, [(0, b"".join(want))], want_off[-1]), what)
                # the whole streams_encode: the encoder's results in chunk order (the chunk table follows from the offsets and B), its
                # bytes at each chunk's own position, the scratch of exactly the size asked for -- and refused on one a byte short
                for short in (0, 1):
                    scratch, sptr, size = lib_scratch(4, n, src_len, B)
                    dst_off = filled(n + 2)
                    out, ptr = guarded(bound)
                    rc = L.emu_lib_streams_encode(addr(src), src_len, addr(off), n, B, MODE_HC if hc else MODE_FAST, ptr, bound, addr(dst_off), sptr,
                                                  size - short, addr(res), addr(comp), gi, gc)
                    if short:
                        assert rc == E_ARGUMENT and untouched(out) and untouched(scratch) and (dst_off == FILL).all(), what
                        continue
                    assert rc == 0 and dst_off.tolist() == want_off + [FILL] and guards_intact(scratch), what
                    same(out, ref_copy(bound, [(0, b"".join(want))], want_off[-1]), what + ", whole")


def lib_streams_decode(src, off, n, max_chunks, results, decoded, total, grid_walk, grid_items, grid_copy):
    """the whole streams_index and streams_decode on a scratch buffer of exactly the size asked for (and refused on one a byte short)"""
    L = emu.framing()
    src_len = src.size - len(TAIL)
    res = np.array(list(results) + [0], np.int32)
    for short in (1, 0):
        scratch, sptr, size = lib_scratch(5, n, max_chunks)
        dst_off, status, error_offset = filled(n + 2), filled(n + 1, np.int32), filled(n + 1)
        buf, ptr = guarded(total + 24)
        index_info, info = emu.StreamsInfo(items=FILL), emu.StreamsInfo(items=FILL)
        rc = L.emu_lib_streams_index(addr(src), src_len, addr(off), n, max_chunks, addr(dst_off), addr(status), addr(error_offset), sptr, size - short,
                                     ref(index_info), grid_walk)
        if short:
            good = emu.StreamsInfo(items=n)
            rc2 = L.emu_lib_streams_decode(addr(src), src_len, addr(off), n, ref(good), max_chunks, sptr, size - 1, ptr, total + 24, addr(dst_off),
                                           addr(status), addr(error_offset), ref(info), addr(res), addr(decoded), grid_items, grid_copy)
            assert rc == rc2 == E_ARGUMENT and index_info.items == info.items == FILL and untouched(scratch) and untouched(buf)
            assert (dst_off == FILL).all() and (status == FILL).all() and (error_offset == FILL).all()
            continue
        assert rc == 0
        assert L.emu_lib_streams_decode(addr(src), src_len, addr(off), n, ref(index_info), max_chunks, sptr, size, ptr, total + 24, addr(dst_off),
                                        addr(status), addr(error_offset), ref(info), addr(res), addr(decoded), grid_items, grid_copy) == 0
        assert guards_intact(scratch)
    return dict(index_info=index_info, info=info, dst_off=dst_off, status=status, error_offset=error_offset, buf=buf)


def test_pipeline_streams_decode(oracle):
    """items whose chunk counts differ, empty ones at the start, in the middle and at the end, failing items between good ones: a
    failing item never disturbs another one's bytes or status"""
    L = emu.framing()
    B = 128
    plain = streams_items(oracle, B)
    streams = [expected_stream(oracle, m, B, False) for m in plain]
    n_good = len(streams)
    # item n_good: a header error behind three chunks; n_good + 1: passes; n_good + 2: gets a corrupt block; then good ones again
    extra_plain = mixed(oracle, 3 * B, 8)
    streams += [expected_stream(oracle, extra_plain, B, False) + b"\x80", frame([(0, 4, b"abcd"), (5, 9, b"\x40abc")]),
                expected_stream(oracle, mixed(oracle, 4 * B, 9), B, False), streams[10], b"", streams[3]]
    n = len(streams)
    walks = [ref_walk(s) for s in streams]
    assert [w["status"] for w in walks[n_good:]] == [EOS, PASSES, OK, OK, OK, OK]
    src = np.frombuffer(b"".join(streams) + TAIL, np.uint8).copy()
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in streams])
    sizes = [w["decoded_bytes"] for w in walks]
    want_off = [0] + np.cumsum(sizes).tolist()
    total = want_off[-1]
    truth = pattern(total + 8) ^ 0xFF                                       # the decoder's bytes for compressed chunks: recognisable
    comp_rows = [(i, r) for i, w in enumerate(walks) for r in w["rows"] if r[0]]
    victim = n_good + 2
    victim_rows = [j for j, (i, _) in enumerate(comp_rows) if i == victim]
    assert len(victim_rows) >= 3
    for bad in ([], [victim_rows[1]], [victim_rows[2], victim_rows[0]], [victim_rows[1], 0]):
        results = [r[3] - (1 if j in bad else 0) for j, (i, r) in enumerate(comp_rows)]
        status = [w["status"] for w in walks]
        err_off = [w["error_offset"] for w in walks]
        for i in sorted({comp_rows[j][0] for j in bad}):
            status[i] = CORRUPT_BLOCK
            err_off[i] = min(comp_rows[j][1][1] for j in bad if comp_rows[j][0] == i)
        segs = []
        for i, w in enumerate(walks):
            for r in w["rows"]:
                o = want_off[i] + r[5]
                a = int(off[i]) + r[2]
                segs.append((o, truth[o:o + r[4]] if r[0] else src[a:a + r[3]]))
        first = min(i for i in range(n) if status[i] != OK)
        for gw in (1, 3, 0):
            for gi, gc in ((1, 1), (3, 3), (0, 0)):
                r = run_streams_index(src, off, n, sum(w["chunks"] for w in walks) + 2, gw)
                info = emu.StreamsInfo()
                buf, ptr = guarded(total + 24)
                res = np.array(results + [0], np.int32)
                assert L.emu_streams_decode(ref(r["a"]), ref(r["ts"]), ref(r["info"]), addr(res), addr(truth), ptr, ref(info), gi, gc) == 0
                what = f"streams decode, corrupt rows {bad}: grids {gw}, {gi}, {gc}"
                got = (info.items, info.chunks, info.compressed_chunks, info.decoded_bytes, info.first_error, info.error_offset, info.error)
                assert got == (n, sum(w["chunks"] for w in walks), len(comp_rows), total, first, err_off[first], status[first]), (what, got)
                assert r["status"].tolist() == status + [FILL] and r["error_offset"].tolist() == err_off + [FILL] and r["dst_off"].tolist() == want_off + [FILL], what
                same(buf, ref_copy(total + 24, segs, total), what)
                lr = lib_streams_decode(src, off, n, sum(w["chunks"] for w in walks) + 2, results, truth, total, gw, gi, gc)
                info = lr["info"]
                got = (info.items, info.chunks, info.compressed_chunks, info.decoded_bytes, info.first_error, info.error_offset, info.error)
                assert got == (n, sum(w["chunks"] for w in walks), len(comp_rows), total, first, err_off[first], status[first]), (what, got)
                assert lr["status"].tolist() == status + [FILL] and lr["error_offset"].tolist() == err_off + [FILL] and lr["dst_off"].tolist() == want_off + [FILL], what
                same(lr["buf"], ref_copy(total + 24, segs, total), what + ", whole")
                for i in range(n_good):                                         # every item in front of the failing ones decodes to its full size
                    assert sizes[i] == plain[i].size, (what, i)


def test_whole_calls_without_items():
    """n == 0 (and, for the encoders, src_len == 0) as the library's fronts handle them: the one offset (or all n + 1) set to 0, the info of
    an empty batch, and not a byte of anything else -- destination, scratch, statuses"""
    L = emu.framing()
    src, off = np.zeros(8, np.uint8), np.zeros(4, np.int64)
    res, comp = np.zeros(4, np.int32), np.zeros(8, np.uint8)

    def fresh():
        return guarded(4096) + guarded(64) + (filled(5), filled(3, np.int32), filled(3))

    scratch, sptr, buf, ptr, dst_off, status, error_offset = fresh()
    assert L.emu_lib_wrap(addr(src), 0, addr(off), 0, MODE_FAST, ptr, 64, addr(dst_off, 1), addr(status), sptr, 0, addr(res), addr(comp), 0, 0) == 0
    assert dst_off.tolist() == [FILL, 0, FILL, FILL, FILL] and untouched(buf) and untouched(scratch) and (status == FILL).all()

    for n, src_len in ((0, 0), (0, 8), (3, 0)):
        scratch, sptr, buf, ptr, dst_off, status, error_offset = fresh()
        assert L.emu_lib_streams_encode(addr(src), src_len, addr(off), n, 16, MODE_FAST, ptr, 64, addr(dst_off, 1), sptr, 0, addr(res), addr(comp), 0, 0) == 0
        assert dst_off.tolist() == [FILL] + [0] * (n + 1) + [FILL] * (3 - n) and untouched(buf) and untouched(scratch), (n, src_len)

    scratch, sptr, buf, ptr, dst_off, status, error_offset = fresh()
    info = emu.UnwrapInfo(messages=FILL, compressed=FILL, decoded_bytes=FILL, first_error=FILL, error=FILL, reserved=FILL)
    size = L.emu_scratch_bytes(3, 0, 0, 0)
    assert size == 256 and L.emu_lib_unwrap_index(addr(src), 0, addr(off), 0, addr(dst_off, 1), addr(status), sptr, size, ref(info), 0) == 0
    assert (info.messages, info.compressed, info.decoded_bytes, info.first_error, info.error, info.reserved) == (0, 0, 0, -1, WRAP_OK, 0)
    assert dst_off.tolist() == [FILL, 0, FILL, FILL, FILL] and (status == FILL).all() and untouched(buf)
    want = pattern(scratch.size)
    want[GUARD:GUARD + 16] = np.frombuffer(struct.pack("<Qq", NONE64, 0), np.uint8)          # [min_bad = none, ncomp = 0]
    same(scratch, want, "unwrap index of no messages: scratch")

    empty = (0, 0, 0, 0, -1, -1, OK, 0)
    for max_chunks in (0, 5):
        scratch, sptr, buf, ptr, dst_off, status, error_offset = fresh()
        info = emu.StreamsInfo(items=FILL, chunks=FILL, compressed_chunks=FILL, decoded_bytes=FILL, first_error=FILL, error_offset=FILL, error=FILL, reserved=FILL)
        assert L.emu_scratch_bytes(5, 0, max_chunks, 0) == 0
        assert L.emu_lib_streams_index(addr(src), 8, addr(off), 0, max_chunks, addr(dst_off, 1), addr(status), addr(error_offset), sptr, 0, ref(info), 0) == 0
        got = (info.items, info.chunks, info.compressed_chunks, info.decoded_bytes, info.first_error, info.error_offset, info.error, info.reserved)
        assert got == empty and dst_off.tolist() == [FILL, 0, FILL, FILL, FILL], got
        assert untouched(scratch) and untouched(buf) and (status == FILL).all() and (error_offset == FILL).all()
        final = emu.StreamsInfo(items=FILL, chunks=FILL, compressed_chunks=FILL, decoded_bytes=FILL, first_error=FILL, error_offset=FILL, error=FILL, reserved=FILL)
        dst_off[:] = FILL
        assert L.emu_lib_streams_decode(addr(src), 8, addr(off), 0, ref(info), max_chunks, sptr, 0, ptr, 64, addr(dst_off, 1), addr(status),
                                        addr(error_offset), ref(final), addr(res), addr(comp), 0, 0) == 0
        got = (final.items, final.chunks, final.compressed_chunks, final.decoded_bytes, final.first_error, final.error_offset, final.error, final.reserved)
        assert got == empty and (dst_off == FILL).all(), got
        assert untouched(scratch) and untouched(buf) and (status == FILL).all() and (error_offset == FILL).all()


# ---- the host-pointer calls of lz4hip_framing.hpp (*_host) over a device image in host memory -----------------------------------------
# Each call is compared with the device-path functions above (emu_lib_*) on the same input and the same faked codec arrays, and with
# what the emulated backend counted: index passes, reserves and how many of them moved the image, copies in and out, waits.  The
# backend's reserve moves whenever it grows and fills the block it gave up, so `intact` fails a call that wrote to a stale base and the
# comparison one that read from it.
def a256(v):
    return -(-v // 256) * 256


def host_run(results=None, codec_bytes=None, gi=0, gc=0, gw=0):
    r = emu.HostRun(grid_items=gi, grid_copy=gc, grid_walk=gw)
    r.keep = [np.array(list(results) + [0], np.int32) if results is not None else None, codec_bytes]
    r.results = addr(r.keep[0]) if results is not None else None
    r.bytes = addr(codec_bytes) if codec_bytes is not None else None
    return r


def counts(r):
    return dict(passes=r.passes, reserves=r.reserves, moves=r.moves, uploads=r.uploads, downloads=r.downloads, syncs=r.syncs)


def info_tuple(info):
    return tuple(getattr(info, f[0]) for f in info._fields_)


def poisoned(cls):
    return cls(**{f[0]: FILL for f in cls._fields_})


def forced_results(lens):
    """results no encoder returns, of every kind: the rule is "compressed iff 0 < r < length" """
    return [(ln // 2, 0, -1, ln, ln - 1, 1, ln + 1)[k % 7] for k, ln in enumerate(lens)]


HOST_GRIDS = ((0, 0), (1, 1), (3, 3))


@pytest.mark.parametrize("B,size", [(16, 0), (16, 1), (17, 1000), (128, 128 * 40 + 5), (4096, 70000)])
def test_host_stream_encode(B, size):
    L = emu.framing()
    data = noise(size, B)
    src = np.ascontiguousarray(np.concatenate([data, np.zeros(1, np.uint8)]))
    n = -(-size // B)
    bound = size + n * (1 + 2 * len(st.write_varint(B))) if size else 0
    results = forced_results([min(B, size - k * B) for k in range(n)])
    comp = noise(size + 16, 9)
    for hc in (MODE_FAST, MODE_HC):
        for gi, gc in HOST_GRIDS:
            scratch, sptr, sbytes = lib_scratch(0, size, B)
            want_len, want = filled(3), guarded(bound)
            res = np.array(results + [0], np.int32)
            assert L.emu_lib_stream_encode(addr(src), size, B, hc, want[1], bound, addr(want_len, 1), sptr, sbytes, addr(res), addr(comp), gi, gc) == 0
            dst_len, (buf, ptr), r = filled(3), guarded(bound), host_run(results, comp, gi, gc)
            assert L.emu_host_stream_encode(addr(src), size, B, hc, ptr, bound, addr(dst_len, 1), ref(r)) == 0 and r.intact
            assert dst_len.tolist() == want_len.tolist() == [FILL, want_len[1], FILL]
            same(buf, want[0], f"host stream encode {B} {size} {hc}")
            if size == 0:                                                   # the short cut: *dst_len = 0 and no device at all
                assert counts(r) == dict(passes=0, reserves=0, moves=0, uploads=0, downloads=0, syncs=0) and untouched(buf)
                continue
            assert counts(r) == dict(passes=0, reserves=1, moves=1, uploads=1, downloads=2, syncs=2)
            assert r.image_bytes == a256(size) + a256(bound) + sbytes + 256


def wrap_input(n, seed):
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.choice([0, 1, 7, 8, 40, 300, 5000], n)]
    msgs = [noise(ln, k) for k, ln in enumerate(lens)]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    src = np.ascontiguousarray(np.concatenate(msgs + [np.zeros(1, np.uint8)]))
    return src, off, int(off[n]), lens


@pytest.mark.parametrize("n", [1, 13, 300])
def test_host_wrap(n):
    L = emu.framing()
    src, off, src_len, lens = wrap_input(n, n)
    bound = src_len + 8 * n
    enc, comp = forced_results(lens), noise(src_len + 16, 11)
    for bad_offsets in (False, True):
        if bad_offsets and n > 5:
            off = off.copy()
            off[3] = off[2] - 7
            off[5] = src_len + 5
        for gi, gc in HOST_GRIDS:
            for with_result in (True, False):
                scratch, sptr, sbytes = lib_scratch(2, n, src_len)
                want_off, want_res, want = filled(n + 2), filled(n + 1, np.int32), guarded(bound)
                e = np.array(enc + [0], np.int32)
                assert L.emu_lib_wrap(addr(src), src_len, addr(off), n, MODE_FAST, want[1], bound, addr(want_off), addr(want_res), sptr, sbytes,
                                      addr(e), addr(comp), gi, gc) == 0
                dst_off, result, (buf, ptr), r = filled(n + 2), filled(n + 1, np.int32), guarded(bound), host_run(enc, comp, gi, gc)
                assert L.emu_host_wrap(addr(src), src_len, addr(off), n, MODE_FAST, ptr, bound, addr(dst_off), addr(result) if with_result else None,
                                       ref(r)) == 0 and r.intact
                assert dst_off.tolist() == want_off.tolist() and dst_off[n + 1] == FILL
                assert result.tolist() == want_res.tolist() if with_result else (result == FILL).all()
                same(buf, want[0], f"host wrap {n} {bad_offsets}")
                total = int(dst_off[n])
                assert counts(r) == dict(passes=0, reserves=1, moves=1, uploads=1 + (src_len > 0), downloads=1 + with_result + (total > 0), syncs=2)
                assert r.image_bytes == a256(src_len) + 2 * a256(8 * (n + 1)) + a256(bound) + a256(4 * n) + sbytes


@pytest.mark.parametrize("B", [16, 128, 4096])
def test_host_streams_encode(B):
    L = emu.framing()
    lens = [0, 0, 1, B - 1, 0, B, B + 1, 0, 5 * B + 3, 3 * B, 0]
    n = len(lens)
    items = [noise(ln, k) for k, ln in enumerate(lens)]
    src = np.ascontiguousarray(np.concatenate(items + [np.zeros(1, np.uint8)]))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    src_len = int(off[n])
    cap = src_len // B + n
    bound = src_len + cap * (1 + 2 * len(st.write_varint(B)))
    chunk_lens = [min(B, ln - o) for ln in lens for o in range(0, ln, B)]
    results = forced_results(chunk_lens) + [0] * (cap - len(chunk_lens))
    comp = noise(src_len + 16, 12)
    for hc in (MODE_FAST, MODE_HC):
        for gi, gc in HOST_GRIDS:
            scratch, sptr, sbytes = lib_scratch(4, n, src_len, B)
            want_off, want = filled(n + 2), guarded(bound)
            res = np.array(results + [0], np.int32)
            assert L.emu_lib_streams_encode(addr(src), src_len, addr(off), n, B, hc, want[1], bound, addr(want_off), sptr, sbytes, addr(res), addr(comp), gi, gc) == 0
            dst_off, (buf, ptr), r = filled(n + 2), guarded(bound), host_run(results, comp, gi, gc)
            assert L.emu_host_streams_encode(addr(src), src_len, addr(off), n, B, hc, ptr, bound, addr(dst_off), ref(r)) == 0 and r.intact
            assert dst_off.tolist() == want_off.tolist() and dst_off[n + 1] == FILL
            same(buf, want[0], f"host streams encode {B} {hc}")
            assert counts(r) == dict(passes=0, reserves=1, moves=1, uploads=2, downloads=2, syncs=2)
            assert r.image_bytes == a256(src_len) + 2 * a256(8 * (n + 1)) + a256(bound) + sbytes


# -- the decoders: every way the index settles.  A chunk or message (compressed, original size, payload bytes) decodes to `original`
# bytes whatever its payload, the codec being the test's: any ratio, and any number of chunks per source byte.
def decoder_chunks(kind):
    """-> the chunks of one stream: few and modest / more than the table guess holds / larger than the output guess / both"""
    if kind == "at once":
        return [(1, 300, noise(100, 1)), (0, 90, noise(90, 2)), (1, 260, noise(70, 3)), (0, 1, noise(1, 4)), (1, 200, noise(199, 5))]
    if kind == "table":
        return [(k % 2, 4 if k % 2 else 3, noise(3, k)) for k in range(45)]
    if kind == "output":
        return [(1, 5000, noise(100, 6)), (0, 50, noise(50, 7)), (1, 9000, noise(20, 8))]
    if kind == "both":
        return [(1, 500 + k, noise(3, k)) for k in range(45)]
    raise ValueError(kind)


SETTLE = {"at once": 1, "table": 2, "output": 2, "both": 3}


def stream_of(chunks):
    return frame([(c, original, payload.tobytes()) for c, original, payload in chunks])


def stream_image_bytes(src_len, out_bytes, max_chunks):
    return a256(src_len) + 256 + a256(out_bytes) + emu.framing().emu_scratch_bytes(1, max_chunks, 0, 0)


@pytest.mark.parametrize("kind", list(SETTLE))
@pytest.mark.parametrize("outcome", ["good", "corrupt block", "bad header", "size query"])
def test_host_stream_decode(kind, outcome):
    L = emu.framing()
    chunks = decoder_chunks(kind)
    stream = stream_of(chunks) + (b"\x81" if outcome == "bad header" else b"")
    w = ref_walk(stream)
    assert w["chunks"] == len(chunks) and w["status"] == (EOS if outcome == "bad header" else OK)
    src_len, total, passes = len(stream), w["decoded_bytes"], SETTLE[kind]
    assert (w["chunks"] > (src_len + 4095) // 4096 + 16) == (kind in ("table", "both")) and (total > 4 * src_len) == (kind in ("output", "both"))
    comp_rows = [r for r in w["rows"] if r[0]]
    results = [r[3] - (1 if outcome == "corrupt block" and j in (1, 2) else 0) for j, r in enumerate(comp_rows)]
    decoded = pattern(total + 8) ^ 0xFF
    src = np.frombuffer(stream + TAIL, np.uint8).copy()
    for gi, gc in HOST_GRIDS:
        _, want_info, want, cap = lib_stream_decode(stream, results, decoded, gi, gc)
        dec = np.ascontiguousarray(np.concatenate([decoded, np.zeros(8, np.uint8)]))
        info, r = poisoned(emu.StreamInfo), host_run(results, dec, gi, gc)
        what = f"host stream decode, {kind}, {outcome}: grids {gi}, {gc}"
        if outcome == "size query":
            # only *info is filled: the index's, with the size to bring.  A size above dst_cap ends the loop: no pass for the output.
            passes = 2 if kind in ("table", "both") else 1
            assert L.emu_host_stream_decode(addr(src), src_len, None, 0, ref(info), ref(r)) == E_ARGUMENT and r.intact, what
            assert r.error == b"stream decode: dst_cap < decoded_bytes (reported in info->decoded_bytes)"
            assert info_tuple(info) == (w["chunks"], len(comp_rows), total, -1, OK, 0), what
            assert counts(r) == dict(passes=passes, reserves=passes, moves=passes, uploads=passes, downloads=passes, syncs=passes), (what, counts(r))
            assert r.image_bytes == stream_image_bytes(src_len, 0, w["chunks"] if passes == 2 else (src_len + 4095) // 4096 + 16), what
            continue
        buf, ptr = guarded(cap)
        rc = L.emu_host_stream_decode(addr(src), src_len, ptr, cap, ref(info), ref(r))
        assert r.intact and info_tuple(info) == info_tuple(want_info) and rc == info.error, (what, rc, info_tuple(info))
        assert info.error == {"good": OK, "corrupt block": CORRUPT_BLOCK, "bad header": EOS}[outcome], what
        same(buf, want, what)
        assert counts(r) == dict(passes=passes, reserves=passes, moves=passes, uploads=passes, downloads=passes + 2, syncs=passes + 1), (what, counts(r))
        # the last pass: a table of exactly the reported count (or still the guess), an output of exactly the reported size (or the guess)
        max_chunks = w["chunks"] if kind in ("table", "both") else (src_len + 4095) // 4096 + 16
        assert r.image_bytes == stream_image_bytes(src_len, total if kind in ("output", "both") else min(cap, 4 * src_len), max_chunks), what


def test_host_stream_decode_of_nothing():
    """src_len == 0 is no short cut here: one index pass over no bytes, nothing uploaded, an info of zeros"""
    L = emu.framing()
    info, r, (buf, ptr) = poisoned(emu.StreamInfo), host_run([], np.zeros(8, np.uint8)), guarded(64)
    assert L.emu_host_stream_decode(None, 0, ptr, 64, ref(info), ref(r)) == 0 and r.intact and untouched(buf)
    assert info_tuple(info) == (0, 0, 0, -1, OK, 0)
    assert counts(r) == dict(passes=1, reserves=1, moves=1, uploads=0, downloads=2, syncs=2)


def unwrap_input(kind, outcome):
    """-> (src, off, n, src_len, refs, results, total)"""
    msgs = {"at once": [(300, 100), (90, 90), (0, 0), (260, 70), (1, 1), (200, 199)],
            "output": [(5000, 100), (50, 50), (9000, 20), (0, 0)]}[kind]
    wrapped = [header_wrap(original, payload) + noise(payload, k).tobytes() for k, (original, payload) in enumerate(msgs)]
    if outcome == "bad header":
        wrapped.insert(2, header_wrap(50, 60) + bytes(20))                  # a payload longer than the message
        wrapped.insert(4, b"\x01\x02\x03")                                  # shorter than a header
    n = len(wrapped)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in wrapped])
    src = np.frombuffer(b"".join(wrapped) + bytes(16), np.uint8).copy()
    refs = [ref_unwrap(np.frombuffer(m, np.uint8)) for m in wrapped]
    comp = [k for k in range(n) if refs[k][1] == "comp"]
    results = [refs[k][3] - (1 if outcome == "corrupt block" and j in (0, 2) else 0) for j, k in enumerate(comp)]
    return src, off, n, int(off[n]), refs, results, sum(r[2] for r in refs)


def unwrap_image_bytes(src_len, n, out_bytes):
    return a256(src_len) + 2 * a256(8 * (n + 1)) + a256(4 * n) + 256 + emu.framing().emu_scratch_bytes(3, n, 0, 0) + out_bytes


@pytest.mark.parametrize("kind", ["at once", "output"])
@pytest.mark.parametrize("outcome", ["good", "corrupt block", "bad header", "size query"])
def test_host_unwrap(kind, outcome):
    L = emu.framing()
    src, off, n, src_len, refs, results, total = unwrap_input(kind, outcome)
    assert (total > 4 * src_len) == (kind == "output")
    passes = 2 if kind == "output" else 1
    decoded = pattern(total + 8) ^ 0xFF
    for gi, gc in HOST_GRIDS:
        want_index, want_info, want_off, index_status, want_status, want = lib_unwrap(src, off, src_len, n, results, decoded, total, gi, gc)
        info, dst_off, status, r = poisoned(emu.UnwrapInfo), filled(n + 2), filled(n + 1, np.int32), host_run(results, decoded, gi, gc)
        what = f"host unwrap, {kind}, {outcome}: grids {gi}, {gc}"
        if outcome == "size query":
            # the info, the offsets and the statuses of the index are the caller's; one pass, the size being above dst_cap
            assert L.emu_host_unwrap(addr(src), src_len, addr(off), n, None, 0, addr(dst_off), addr(status), ref(info), ref(r)) == E_ARGUMENT and r.intact, what
            assert r.error == b"unwrap: dst_cap < decoded_bytes (reported in info->decoded_bytes)"
            assert info_tuple(info) == info_tuple(want_index) and info.decoded_bytes == total, what
            assert dst_off.tolist() == want_off.tolist() and status.tolist() == index_status.tolist(), what
            assert counts(r) == dict(passes=1, reserves=1, moves=1, uploads=2, downloads=3, syncs=2), (what, counts(r))
            assert r.image_bytes == unwrap_image_bytes(src_len, n, 0), what
            continue
        buf, ptr = guarded(total + 24)
        rc = L.emu_host_unwrap(addr(src), src_len, addr(off), n, ptr, total + 24, addr(dst_off), addr(status), ref(info), ref(r))
        assert r.intact and info_tuple(info) == info_tuple(want_info) and rc == info.error, (what, rc, info_tuple(info))
        assert info.error == {"good": WRAP_OK, "corrupt block": WRAP_CORRUPT_BLOCK, "bad header": WRAP_CORRUPT_HEADER}[outcome], what
        assert dst_off.tolist() == want_off.tolist() and status.tolist() == want_status.tolist() and dst_off[n + 1] == FILL and status[n] == FILL, what
        same(buf, want, what)
        assert counts(r) == dict(passes=passes, reserves=passes, moves=passes, uploads=2 * passes, downloads=passes + 4, syncs=passes + 1), (what, counts(r))
        assert r.image_bytes == unwrap_image_bytes(src_len, n, total if kind == "output" else min(total + 24, 4 * src_len)), what


def test_host_unwrap_of_nothing():
    """n == 0 is no short cut here: the one offset is staged, the index runs, dst_off[0] = 0 and the info of no messages come back"""
    L = emu.framing()
    info, dst_off, status, r, (buf, ptr) = poisoned(emu.UnwrapInfo), filled(3), filled(2, np.int32), host_run([], np.zeros(8, np.uint8)), guarded(64)
    off = np.zeros(1, np.int64)
    assert L.emu_host_unwrap(None, 0, addr(off), 0, ptr, 64, addr(dst_off, 1), addr(status), ref(info), ref(r)) == 0 and r.intact and untouched(buf)
    assert info_tuple(info) == (0, 0, 0, -1, WRAP_OK, 0) and dst_off.tolist() == [FILL, 0, FILL] and (status == FILL).all()
    assert counts(r) == dict(passes=0, reserves=1, moves=1, uploads=1, downloads=3, syncs=2)


def streams_input(kind, outcome):
    """-> (src with TAIL, off, n, walks): the chunks of decoder_chunks(kind) dealt to four items, an empty one between them"""
    chunks = decoder_chunks(kind)
    k = -(-len(chunks) // 4)
    items = [stream_of(chunks[0:k]), b"", stream_of(chunks[k:2 * k]), stream_of(chunks[2 * k:3 * k]), stream_of(chunks[3 * k:])]
    if outcome == "bad header":
        items[2] += b"\x81"
    n = len(items)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in items])
    return np.frombuffer(b"".join(items) + TAIL, np.uint8).copy(), off, n, [ref_walk(s) for s in items]


def streams_image_bytes(src_len, n, out_bytes, max_chunks):
    return a256(src_len) + 2 * a256(8 * (n + 1)) + a256(4 * n) + a256(8 * n) + 256 + a256(out_bytes) + emu.framing().emu_scratch_bytes(5, n, max_chunks, 0)


@pytest.mark.parametrize("kind", list(SETTLE))
@pytest.mark.parametrize("outcome", ["good", "corrupt block", "bad header", "size query"])
def test_host_streams_decode(kind, outcome):
    L = emu.framing()
    src, off, n, walks = streams_input(kind, outcome)
    src_len, chunks, total, passes = int(off[n]), sum(w["chunks"] for w in walks), sum(w["decoded_bytes"] for w in walks), SETTLE[kind]
    guess = src_len // 4096 + n + 16
    assert (chunks > guess) == (kind in ("table", "both")) and (total > 4 * src_len) == (kind in ("output", "both"))
    comp_rows = [r for w in walks for r in w["rows"] if r[0]]
    results = [r[3] - (1 if outcome == "corrupt block" and j in (1, len(comp_rows) - 1) else 0) for j, r in enumerate(comp_rows)]
    decoded = pattern(total + 8) ^ 0xFF
    for gw, gi, gc in ((0, 0, 0), (1, 1, 1), (3, 3, 3)):
        want = lib_streams_decode(src, off, n, chunks + 2, results, decoded, total, gw, gi, gc)
        info, dst_off, status, error_offset = poisoned(emu.StreamsInfo), filled(n + 2), filled(n + 1, np.int32), filled(n + 1)
        r = host_run(results, decoded, gi, gc, gw)
        what = f"host streams decode, {kind}, {outcome}: grids {gw}, {gi}, {gc}"
        if outcome == "size query":
            # the info, the offsets, the statuses and the error offsets of the index are the caller's
            passes = 2 if kind in ("table", "both") else 1
            assert L.emu_host_streams_decode(addr(src), src_len, addr(off), n, None, 0, addr(dst_off), addr(status), addr(error_offset), ref(info),
                                             ref(r)) == E_ARGUMENT and r.intact, what
            assert r.error == b"streams decode: dst_cap < decoded_bytes (reported in info->decoded_bytes)"
            assert info_tuple(info) == info_tuple(want["index_info"]) and info.decoded_bytes == total, what
            assert dst_off.tolist() == want["dst_off"].tolist() and status.tolist() == want["status"].tolist(), what
            assert error_offset.tolist() == want["error_offset"].tolist(), what
            assert counts(r) == dict(passes=passes, reserves=passes, moves=passes, uploads=2 * passes, downloads=passes + 3, syncs=passes + 1), (what, counts(r))
            assert r.image_bytes == streams_image_bytes(src_len, n, 0, chunks if passes == 2 else guess), what
            continue
        buf, ptr = guarded(total + 24)
        rc = L.emu_host_streams_decode(addr(src), src_len, addr(off), n, ptr, total + 24, addr(dst_off), addr(status), addr(error_offset), ref(info), ref(r))
        assert r.intact and info_tuple(info) == info_tuple(want["info"]) and rc == info.error, (what, rc, info_tuple(info))
        assert info.error == {"good": OK, "corrupt block": CORRUPT_BLOCK, "bad header": EOS}[outcome], what
        assert dst_off.tolist() == want["dst_off"].tolist() and status.tolist() == want["status"].tolist(), what
        assert error_offset.tolist() == want["error_offset"].tolist() and dst_off[n + 1] == FILL and status[n] == FILL and error_offset[n] == FILL, what
        same(buf, want["buf"], what)
        assert counts(r) == dict(passes=passes, reserves=passes, moves=passes, uploads=2 * passes, downloads=passes + 5, syncs=passes + 1), (what, counts(r))
        assert r.image_bytes == streams_image_bytes(src_len, n, total if kind in ("output", "both") else min(total + 24, 4 * src_len),
                                                    chunks if kind in ("table", "both") else guess), what


def test_host_argument_checks_and_short_cuts():
    """every argument check of the six, by its message, with no device touched and nothing written (the mode is the device path's to
    check: the source is staged by then, and still nothing is written); then the short cuts, which write the one thing they document
    and nothing else"""
    L = emu.framing()
    src, off3 = np.zeros(64, np.uint8), np.array([0, 10, 20, 30], np.int64)
    none = dict(passes=0, reserves=0, moves=0, uploads=0, downloads=0, syncs=0)
    S, O = addr(src), addr(off3)

    def fresh():
        return guarded(4096) + (filled(6), filled(5, np.int32), filled(5), filled(3))

    def refused(name, message, *args, uploads=0):
        buf, ptr, dst_off, status, error_offset, dst_len = fresh()
        info = {"emu_host_stream_decode": emu.StreamInfo, "emu_host_unwrap": emu.UnwrapInfo, "emu_host_streams_decode": emu.StreamsInfo}.get(name)
        info = poisoned(info) if info else None
        named = dict(dst=ptr, dst_off=addr(dst_off, 1), status=addr(status), error_offset=addr(error_offset), dst_len=addr(dst_len, 1),
                     info=ref(info) if info else None)
        r = host_run([], src)
        rc = getattr(L, name)(*[named[a] if isinstance(a, str) else a for a in args], ref(r))
        staged = dict(none, reserves=1, moves=1, uploads=uploads) if uploads else none
        assert rc == E_ARGUMENT and r.error == message.encode() and counts(r) == staged and r.intact, (name, args, rc, r.error, counts(r))
        assert untouched(buf) and all((a == FILL).all() for a in (dst_off, status, error_offset, dst_len)), (name, args)
        assert info is None or all(v == FILL for v in info_tuple(info)), (name, args)

    m = "stream encode: negative size or NULL pointer"
    refused("emu_host_stream_encode", m, S, -1, 16, MODE_FAST, "dst", 4096, "dst_len")
    refused("emu_host_stream_encode", m, S, 30, 16, MODE_FAST, "dst", 4096, None)
    refused("emu_host_stream_encode", m, None, 30, 16, MODE_FAST, "dst", 4096, "dst_len")
    refused("emu_host_stream_encode", m, S, 30, 16, MODE_FAST, None, 4096, "dst_len")
    refused("emu_host_stream_encode", "stream encode: dst_cap < lz4hip_stream_bound", S, 30, 16, MODE_FAST, "dst", 30 + 2 * 3 - 1, "dst_len")
    refused("emu_host_stream_encode", "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC", S, 30, 16, 7, "dst", 4096, "dst_len", uploads=1)
    m = "stream decode: negative size or NULL pointer"
    refused("emu_host_stream_decode", m, S, -1, "dst", 4096, "info")
    refused("emu_host_stream_decode", m, S, 30, "dst", -1, "info")
    refused("emu_host_stream_decode", m, S, 30, "dst", 4096, None)
    refused("emu_host_stream_decode", m, None, 30, "dst", 4096, "info")
    m = "wrap: negative size or NULL pointer"
    refused("emu_host_wrap", m, S, -1, O, 3, MODE_FAST, "dst", 4096, "dst_off", "status")
    refused("emu_host_wrap", m, S, 30, O, -1, MODE_FAST, "dst", 4096, "dst_off", "status")
    refused("emu_host_wrap", m, S, 30, O, 3, MODE_FAST, "dst", 4096, None, "status")
    refused("emu_host_wrap", m, S, 30, None, 3, MODE_FAST, "dst", 4096, "dst_off", "status")
    refused("emu_host_wrap", m, S, 30, O, 3, MODE_FAST, None, 4096, "dst_off", "status")
    refused("emu_host_wrap", m, None, 30, O, 3, MODE_FAST, "dst", 4096, "dst_off", "status")
    refused("emu_host_wrap", "wrap: dst_cap < lz4hip_wrap_bound", S, 30, O, 3, MODE_FAST, "dst", 30 + 24 - 1, "dst_off", "status")
    refused("emu_host_wrap", "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC", S, 30, O, 3, 7, "dst", 4096, "dst_off", "status", uploads=2)
    m = "unwrap: negative size or NULL pointer"
    refused("emu_host_unwrap", m, S, -1, O, 3, "dst", 4096, "dst_off", "status", "info")
    refused("emu_host_unwrap", m, S, 30, O, -1, "dst", 4096, "dst_off", "status", "info")
    refused("emu_host_unwrap", m, S, 30, O, 3, "dst", -1, "dst_off", "status", "info")
    refused("emu_host_unwrap", m, S, 30, O, 3, "dst", 4096, None, "status", "info")
    refused("emu_host_unwrap", m, S, 30, O, 3, "dst", 4096, "dst_off", "status", None)
    refused("emu_host_unwrap", m, S, 30, None, 3, "dst", 4096, "dst_off", "status", "info")
    refused("emu_host_unwrap", m, S, 30, O, 3, "dst", 4096, "dst_off", None, "info")
    refused("emu_host_unwrap", m, None, 30, O, 3, "dst", 4096, "dst_off", "status", "info")
    m = "streams encode: negative size or NULL pointer"
    refused("emu_host_streams_encode", m, S, -1, O, 3, 16, MODE_FAST, "dst", 4096, "dst_off")
    refused("emu_host_streams_encode", m, S, 30, O, -1, 16, MODE_FAST, "dst", 4096, "dst_off")
    refused("emu_host_streams_encode", m, S, 30, O, 3, 16, MODE_FAST, "dst", 4096, None)
    refused("emu_host_streams_encode", m, S, 30, None, 3, 16, MODE_FAST, "dst", 4096, "dst_off")
    refused("emu_host_streams_encode", m, None, 30, O, 3, 16, MODE_FAST, "dst", 4096, "dst_off")
    refused("emu_host_streams_encode", m, S, 30, O, 3, 16, MODE_FAST, None, 4096, "dst_off")
    m = "streams encode: offsets decrease or fall outside [0, src_len]"
    for bad in ([-1, 10, 20, 30], [0, 10, 9, 30], [0, 10, 20, 31]):
        refused("emu_host_streams_encode", m, S, 30, addr(np.array(bad, np.int64)), 3, 16, MODE_FAST, "dst", 4096, "dst_off")
    refused("emu_host_streams_encode", "streams encode: dst_cap < lz4hip_streams_bound", S, 30, O, 3, 16, MODE_FAST, "dst", 30 + 4 * 3 - 1, "dst_off")
    refused("emu_host_streams_encode", "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC", S, 30, O, 3, 16, 7, "dst", 4096, "dst_off", uploads=2)
    m = "streams decode: negative size or NULL pointer"
    refused("emu_host_streams_decode", m, S, -1, O, 3, "dst", 4096, "dst_off", "status", "error_offset", "info")
    refused("emu_host_streams_decode", m, S, 30, O, -1, "dst", 4096, "dst_off", "status", "error_offset", "info")
    refused("emu_host_streams_decode", m, S, 30, O, 3, "dst", -1, "dst_off", "status", "error_offset", "info")
    refused("emu_host_streams_decode", m, S, 30, O, 3, "dst", 4096, None, "status", "error_offset", "info")
    refused("emu_host_streams_decode", m, S, 30, O, 3, "dst", 4096, "dst_off", "status", "error_offset", None)
    refused("emu_host_streams_decode", m, S, 30, None, 3, "dst", 4096, "dst_off", "status", "error_offset", "info")
    refused("emu_host_streams_decode", m, S, 30, O, 3, "dst", 4096, "dst_off", None, "error_offset", "info")
    refused("emu_host_streams_decode", m, S, 30, O, 3, "dst", 4096, "dst_off", "status", None, "info")
    refused("emu_host_streams_decode", m, None, 30, O, 3, "dst", 4096, "dst_off", "status", "error_offset", "info")

    # the short cuts: no device, NULL buffers welcome
    buf, ptr, dst_off, status, error_offset, dst_len = fresh()
    r = host_run([], src)
    assert L.emu_host_stream_encode(None, 0, 16, MODE_FAST, None, 0, addr(dst_len, 1), ref(r)) == 0 and dst_len.tolist() == [FILL, 0, FILL] and counts(r) == none
    assert L.emu_host_wrap(None, 0, None, 0, MODE_FAST, None, 0, addr(dst_off, 1), None, ref(r)) == 0 and counts(r) == none
    assert dst_off.tolist() == [FILL, 0] + [FILL] * 4
    for n, src_len in ((0, 0), (0, 30), (3, 0)):
        dst_off[:] = FILL
        zeros = np.zeros(4, np.int64)
        assert L.emu_host_streams_encode(None if src_len == 0 else S, src_len, addr(zeros) if n else None, n, 16, MODE_FAST, None, 4096, addr(dst_off, 1), ref(r)) == 0
        assert dst_off.tolist() == [FILL] + [0] * (n + 1) + [FILL] * (4 - n) and counts(r) == none, (n, src_len)
    dst_off[:] = FILL
    info = poisoned(emu.StreamsInfo)
    assert L.emu_host_streams_decode(S, 30, None, 0, None, 0, addr(dst_off, 1), None, None, ref(info), ref(r)) == 0 and counts(r) == none
    assert info_tuple(info) == (0, 0, 0, 0, -1, -1, OK, 0) and dst_off.tolist() == [FILL, 0] + [FILL] * 4
    assert untouched(buf) and (status == FILL).all() and (error_offset == FILL).all()
