"""CPU-only: the one-call decodes of an LZ4Stream buffer, of a batch of them and of wrapped messages (lz4hip_framing.hpp:
stream_decode_into, streams_decode_into, unwrap_into) under the SIMT emulator (tests/simt/emu_into.inc): the real clip, check, copy and
info kernels, the library's fronts and sequences, on a scratch buffer of exactly the size asked for between guard bytes.  The block
decoder is a stand-in fed the oracle's results and bytes that verifies what it is handed: ONE known-size call over the whole table,
every row past the count and every clipped row as (0, 0), every other row with its own offsets, length and capacity.  Every case runs
with the library's grids and with grids of 1 and 3; with a capacity that holds everything the outputs are compared with the two-call
pair's from the same emulator, byte for byte.  (stream.decompress_stream and LZ4Codec.Unwrap decode on the device, which this suite does
without: the good parts are held against the plain bytes the oracle compressed, which is what those two return for them;
tests/test_gpu_decode_into.py repeats the cases against the host paths.)"""
import numpy as np
import pytest

import emu_helpers as emu
import framing_cases as fr
from emu_helpers import addr, ref
from emu_lib import E_ARGUMENT, GRIDS
from framing_cases import CORRUPT_BLOCK, EOS, OK, PASSES, TABLE_FULL
from into_cases import FILL, Buf, info_bytes, lib, run_record
from lz4net_amd._lib import StreamInfo, StreamsInfo, UnwrapInfo
from stream_cases import expected_stream, frame

def cap_values(ends, total):
    """0, 1, the start and the end of each given chunk (item, message), total - 1, total, total + 4096"""
    caps = {0, 1, max(total - 1, 0), total, total + 4096}
    for start, end in ends:
        caps |= {start, end}
    return sorted(caps)


# ---- one stream ------------------------------------------------------------------------------------------------------------------
def stream_chunks(oracle):
    """compressed, raw and empty chunks mixed, 16 .. 4096 bytes -> (chunk list for frame(), the plain bytes)"""
    sizes = [16, 300, 4096, 17, 1000, 64, 2048, 4095, 33, 700, 128, 4096, 90, 1500, 16]
    chunks, parts = [], []
    for k, size in enumerate(sizes):
        p = fr.noise(size, k) if k % 3 == 1 else fr.mixed(oracle, size, k)
        r, buf = oracle.compress_raw(p, p.size)
        chunks.append((1, p.size, buf[:r]) if 0 < r < p.size and k % 3 != 1 else (0, p.size, p))
        parts.append(p)
        if k % 4 == 2:
            chunks.append((0, 0, b""))                                     # an empty chunk: skipped by the walk
    kinds = [c[0] for c in chunks if c[1]]
    assert kinds.count(1) >= 5 and kinds.count(0) >= 5
    return chunks, np.concatenate(parts)


def pair_stream(src, src_len, max_chunks, results, truth, total):
    """lz4hip_stream_index + lz4hip_stream_decode under the same emulator -> (info bytes, dst[0, total))"""
    L = emu.framing()
    size = L.emu_scratch_bytes(1, max_chunks, 0, 0)
    scratch, dst = Buf(size, 0xC3), Buf(total)
    index_info, info = emu.StreamInfo(), emu.StreamInfo()
    res = np.array(list(results) + [0], np.int32)
    dec = np.ascontiguousarray(np.concatenate([truth, np.zeros(8, np.uint8)]))
    assert L.emu_lib_stream_index(addr(src), src_len, max_chunks, scratch.ptr, size, ref(index_info)) == 0
    assert L.emu_lib_stream_decode(addr(src), ref(index_info), max_chunks, scratch.ptr, size, dst.ptr, total, ref(info), addr(res), addr(dec), 0, 0) == 0
    return info_bytes(info), dst.a.copy()


def check_stream(name, stream, results, truth, max_chunks, caps=None, want_written=True):
    """results: the decoder's answer per compressed row of the whole stream; truth: its bytes, by output offset"""
    L = lib()
    stream = bytes(stream)
    full, w = fr.ref_walk(stream), fr.ref_walk(stream, max_chunks)
    rows, is_full = full["rows"], fr.ref_walk(stream, max_chunks)["status"] == TABLE_FULL
    comp = [r for r in rows if r[0]]
    tabled = [r for r in rows[:max_chunks] if r[0]]                         # (a full table still holds the first max_chunks chunks)
    src = np.frombuffer(stream + fr.TAIL, np.uint8).copy()
    total = full["decoded_bytes"]
    size = L.emu_into_scratch_bytes(0, max_chunks, 0)
    assert size == L.emu_into_scratch_bytes(10, max_chunks, 0) + 2 * ((4 * max_chunks + 255) // 256 * 256)
    for dst_cap in (caps if caps is not None else [total + 24]):
        fits = [(not is_full) and r[5] + r[4] <= dst_cap for r in rows]
        written = max([r[5] + r[4] for r, f in zip(rows, fits) if f], default=0)
        cfit = [(not is_full) and r[5] + r[4] <= dst_cap for r in tabled]
        bad = [j for j, r in enumerate(tabled) if cfit[j] and results[j] != r[3]]
        want_info = (w["chunks"], w["compressed_chunks"], w["decoded_bytes"], w["error_offset"], w["status"])
        if bad:
            want_info = want_info[:3] + (tabled[bad[0]][1], CORRUPT_BLOCK)
        want = np.full(dst_cap + 32, FILL, np.uint8)
        for r, f in zip(rows, fits):
            if f:
                want[r[5]:r[5] + r[4]] = truth[r[5]:r[5] + r[4]] if r[0] else src[r[2]:r[2] + r[3]]
        for grid in GRIDS:
            what = f"{name}: max_chunks {max_chunks}, dst_cap {dst_cap}, grid {grid}"
            run, keep = run_record(results, truth, [r[2] for r in tabled], [r[5] for r in tabled], [r[3] if f else 0 for r, f in zip(tabled, cfit)] + [0] * (max_chunks - len(tabled)),
                                   [r[4] if f else 0 for r, f in zip(tabled, cfit)] + [0] * (max_chunks - len(tabled)), max_chunks, len(tabled), grid)
            scratch, dst = Buf(size, 0xC3), Buf(dst_cap + 32)
            info = StreamInfo(chunks=-5, error=-5, reserved=-5)
            out_written = np.full(3, -77, np.int64)
            rc = L.emu_stream_decode_into(addr(src), len(stream), max_chunks, scratch.ptr, size, dst.ptr if dst_cap else None, dst_cap, ref(info),
                                          addr(out_written, 1) if want_written else None, ref(run))
            assert rc == 0 and run.shape_errors == 0 and run.calls == (1 if max_chunks else 0), (what, rc, run.shape_errors, run.calls, run.error)
            assert run.decoded_rows == sum(cfit), what
            assert scratch.guards_intact() and dst.guards_intact(), what
            got = (info.chunks, info.compressed_chunks, info.decoded_bytes, info.error_offset, info.error)
            assert got == want_info and info.reserved == 0, (what, got, want_info)
            assert out_written.tolist() == [-77, written if want_written else -77, -77], (what, out_written.tolist(), written)
            assert np.array_equal(dst.a, want), f"{what}: first difference at byte {int(np.flatnonzero(dst.a != want)[0])}, written {written}"
            assert (dst.a[written:] == FILL).all(), what
        if not is_full and dst_cap >= total:
            pair_info, pair_dst = pair_stream(src, len(stream), max_chunks, results, truth, total)
            assert info_bytes(info) == pair_info and np.array_equal(dst.a[:total], pair_dst), f"{name}: differs from the two-call pair"
    return full


def test_stream_parity_and_table_sizes(oracle):
    chunks, plain = stream_chunks(oracle)
    stream = frame(chunks)
    full = fr.ref_walk(stream)
    count = full["chunks"]
    good = [r[3] for r in full["rows"] if r[0]]
    assert full["decoded_bytes"] == plain.size
    for mc in (count - 1, count, count + 37, 0):
        check_stream("good stream", stream, good, plain, mc)
        # a buffer that holds everything is the source again: what stream.decompress_stream gives for these chunks
    check_stream("no written_bytes", stream, good, plain, count + 37, want_written=False)
    check_stream("empty source", b"", [], np.zeros(0, np.uint8), 5, caps=[0, 7])
    check_stream("empty source, no table", b"", [], np.zeros(0, np.uint8), 0, caps=[0, 7])
    check_stream("only empty chunks", frame([(0, 0, b"")] * 3), [], np.zeros(0, np.uint8), 2, caps=[0, 7])


def test_stream_clipping(oracle):
    chunks, plain = stream_chunks(oracle)
    stream = frame(chunks)
    rows = fr.ref_walk(stream)["rows"]
    ck = [r for r in rows if r[0]][2]                                       # a compressed chunk k and a raw chunk k, neither the first
    rk = [r for r in rows if not r[0]][2]
    caps = cap_values([(r[5], r[5] + r[4]) for r in (ck, rk)], plain.size)
    assert len(caps) == 9
    good = [r[3] for r in rows if r[0]]
    for mc in (len(rows), len(rows) + 37, len(rows) - 1):
        check_stream("clipped stream", stream, good, plain, mc, caps=caps)


def test_stream_errors(oracle):
    chunks, plain = stream_chunks(oracle)
    base = frame(chunks)
    rows = fr.ref_walk(base)["rows"]
    count, ncomp = len(rows), sum(1 for r in rows if r[0])
    good = [r[3] for r in rows if r[0]]
    hurt = lambda bad: [g - (1 if j in bad else 0) for j, g in enumerate(good)]
    passes = frame([(5, 9, b"\x40abc")])
    for tail, status in ((b"", OK), (b"\x81", EOS), (passes + frame(chunks[:2]), PASSES)):
        stream = base + tail
        w = fr.ref_walk(stream)
        assert (w["status"], w["chunks"]) == (status, count)
        for bad in ([], [1], [ncomp - 1, 2], [0]):                          # no corrupt block (the header error alone), one, two (the first wins), the first row
            full = check_stream(f"tail {tail[:1]!r}, corrupt rows {bad}", stream, hurt(bad), plain, count + 3)
            assert full["status"] == status
    # a corrupt block is found only in a chunk that was written: clipped away, the index's outcome stays
    comp = [r for r in rows if r[0]]
    for tail in (b"", b"\x81"):
        check_stream("corrupt row clipped", base + tail, hurt([3]), plain, count + 1, caps=[comp[3][5] + comp[3][4] - 1, comp[3][5] + comp[3][4], comp[2][5]])
    # TABLE_FULL wins over everything, and nothing is decoded
    check_stream("full table, corrupt rows", base + b"\x81", hurt([0, 1]), plain, count - 1)
    check_stream("truncated header", base[:len(base) - 3], good[:-1] if rows[-1][0] else good, plain, count + 2)


# ---- a batch of streams ----------------------------------------------------------------------------------------------------------
def streams_batch(oracle):
    """about 40 items of 0 - 3 chunks of 128 bytes: an empty item, failing items between good ones, an item (two, in fact: the offset
    between them is the bad one) with bad offsets -> (items as bytes, offsets, plain bytes per item)"""
    B = 128
    items, plain = [], []
    for i in range(40):
        size = (0, 1, 100, 128, 129, 300, 384, 256, 17, 383)[i % 10]
        p = fr.noise(size, i) if i % 4 == 3 else fr.mixed(oracle, size, i)
        items.append(expected_stream(oracle, p, B, False))
        plain.append(p)
    items[7] += b"\x80"                                                     # a header error behind its chunks
    items[21] = frame([(0, 4, b"abcd"), (5, 9, b"\x40abc")])               # passes, behind a raw chunk
    plain[21] = np.frombuffer(b"abcd", np.uint8)
    off = np.zeros(41, np.int64)
    off[1:] = np.cumsum([len(s) for s in items])
    off[31] = off[40] + 7                                                   # items 30 and 31: outside the buffer, and ending before its start
    return items, off, plain


def streams_walks(items, off):
    src_len = int(sum(len(s) for s in items))
    walks = []
    for i, s in enumerate(items):
        a, b = int(off[i]), int(off[i + 1])
        if a < 0 or b < a or b > src_len:
            walks.append(dict(rows=[], status=E_ARGUMENT, error_offset=-1, chunks=0, compressed_chunks=0, decoded_bytes=0))
        else:
            walks.append(fr.ref_walk(s))
    return walks


def check_streams(name, items, off, bad_rows, max_chunks, caps=None, want_written=True):
    """bad_rows: rows of the compressed table (all items) whose block is corrupt"""
    L = lib()
    n = len(items)
    src = np.frombuffer(b"".join(items) + fr.TAIL, np.uint8).copy()
    src_len = src.size - len(fr.TAIL)
    walks = streams_walks(items, off)
    sizes = [w["decoded_bytes"] for w in walks]
    want_off = [0] + np.cumsum(sizes).tolist() if n else [0]
    total = want_off[-1]
    truth = fr.pattern(total + 8) ^ 0xFF
    chunks = sum(w["chunks"] for w in walks)
    comp = [(i, r) for i, w in enumerate(walks) for r in w["rows"] if r[0]]
    is_full = chunks > max_chunks
    tabled = [] if is_full else comp                                        # (a full table is not filled at all)
    results = [r[3] - (1 if j in bad_rows else 0) for j, (i, r) in enumerate(comp)]
    size = L.emu_into_scratch_bytes(1, n, max_chunks)
    assert size == (L.emu_into_scratch_bytes(11, n, max_chunks) + 2 * ((4 * max_chunks + 255) // 256 * 256) if n else 0)
    for dst_cap in (caps if caps is not None else [total + 24]):
        w_items = 0 if is_full else sum(1 for i in range(n) if want_off[i + 1] <= dst_cap)
        end = want_off[w_items]
        status, err_off = [w["status"] for w in walks], [w["error_offset"] for w in walks]
        for i in sorted({comp[j][0] for j in bad_rows if comp[j][0] < w_items}):
            status[i] = CORRUPT_BLOCK
            err_off[i] = min(comp[j][1][1] for j in bad_rows if comp[j][0] == i)
        failing = [i for i in range(n) if status[i] != OK]
        want_info = (n, chunks, len(comp), total, failing[0] if failing else -1, err_off[failing[0]] if failing else -1, status[failing[0]] if failing else OK)
        if is_full:
            want_info = want_info[:4] + (-1, -1, TABLE_FULL)
        want = np.full(dst_cap + 32, FILL, np.uint8)
        for i in range(w_items):
            for r in walks[i]["rows"]:
                o, a = want_off[i] + r[5], int(off[i]) + r[2]
                want[o:o + r[4]] = truth[o:o + r[4]] if r[0] else src[a:a + r[3]]
        for grid in GRIDS:
            what = f"{name}: max_chunks {max_chunks}, dst_cap {dst_cap}, grid {grid}"
            pad = [0] * (max_chunks - len(tabled))
            run, keep = run_record(results, truth, [int(off[i]) + r[2] for i, r in tabled], [want_off[i] + r[5] for i, r in tabled],
                                   [r[3] if i < w_items else 0 for i, r in tabled] + pad, [r[4] if i < w_items else 0 for i, r in tabled] + pad,
                                   max_chunks, len(tabled), grid)
            scratch, dst = Buf(size, 0xC3), Buf(dst_cap + 32)
            info = StreamsInfo(items=-5, error=-5, reserved=-5)
            dst_off, st_arr, eo = np.full(n + 3, -77, np.int64), np.full(n + 2, -77, np.int32), np.full(n + 2, -77, np.int64)
            out_written = np.full(3, -77, np.int64)
            rc = L.emu_streams_decode_into(addr(src), src_len, addr(off), n, max_chunks, scratch.ptr if size else None, size, dst.ptr if dst_cap else None,
                                           dst_cap, addr(dst_off, 1), addr(st_arr, 1), addr(eo, 1), ref(info), addr(out_written, 1) if want_written else None,
                                           ref(run))
            assert rc == 0 and run.shape_errors == 0 and run.calls == (1 if n and max_chunks else 0), (what, rc, run.shape_errors, run.calls, run.error)
            assert run.decoded_rows == sum(1 for i, r in tabled if i < w_items), what
            assert scratch.guards_intact() and dst.guards_intact(), what
            got = (info.items, info.chunks, info.compressed_chunks, info.decoded_bytes, info.first_error, info.error_offset, info.error)
            assert got == want_info and info.reserved == 0, (what, got, want_info)
            assert dst_off.tolist() == [-77] + want_off + [-77], what
            assert st_arr.tolist() == [-77] + status + [-77] and eo.tolist() == [-77] + err_off + [-77], what
            assert out_written.tolist() == [-77, w_items if want_written else -77, -77], (what, out_written.tolist(), w_items)
            assert np.array_equal(dst.a, want), f"{what}: first difference at byte {int(np.flatnonzero(dst.a != want)[0])}, end {end}"
            assert (dst.a[end:] == FILL).all(), what
        if not is_full and dst_cap >= total and n:
            E = emu.framing()
            psize = E.emu_scratch_bytes(5, n, max_chunks, 0)
            pscratch, pdst = Buf(psize, 0xC3), Buf(total)
            pinfo, pfinal = emu.StreamsInfo(), emu.StreamsInfo()
            p_off, p_st, p_eo = np.zeros(n + 1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int64)
            res = np.array(results + [0], np.int32)
            assert E.emu_lib_streams_index(addr(src), src_len, addr(off), n, max_chunks, addr(p_off), addr(p_st), addr(p_eo), pscratch.ptr, psize, ref(pinfo), 0) == 0
            assert E.emu_lib_streams_decode(addr(src), src_len, addr(off), n, ref(pinfo), max_chunks, pscratch.ptr, psize, pdst.ptr, total, addr(p_off),
                                            addr(p_st), addr(p_eo), ref(pfinal), addr(res), addr(truth), 0, 0) == 0
            assert info_bytes(info) == info_bytes(pfinal) and np.array_equal(dst.a[:total], pdst.a), f"{name}: differs from the two-call pair"
            assert dst_off[1:n + 2].tolist() == p_off.tolist() and st_arr[1:n + 1].tolist() == p_st.tolist() and eo[1:n + 1].tolist() == p_eo.tolist(), name
    return walks, comp, want_off


def test_streams_parity_and_table_sizes(oracle):
    items, off, plain = streams_batch(oracle)
    walks = streams_walks(items, off)
    count = sum(w["chunks"] for w in walks)
    assert [walks[i]["status"] for i in (7, 21, 30, 31)] == [EOS, PASSES, E_ARGUMENT, E_ARGUMENT] and walks[0]["chunks"] == 0
    for i, w in enumerate(walks):                                           # the good items decode to their source
        assert w["status"] != OK or w["decoded_bytes"] == plain[i].size
    comp = [(i, r) for i, w in enumerate(walks) for r in w["rows"] if r[0]]
    vi = next(i for i in range(8, 40) if walks[i]["compressed_chunks"] >= 2)
    victim = [j for j, (i, r) in enumerate(comp) if i == vi]
    early = [j for j, (i, r) in enumerate(comp) if i < 7]
    assert len(victim) >= 2 and early
    for mc in (count - 1, count, count + 37, 0):
        for bad in ((), (victim[1],), (victim[1], victim[0], early[0])):   # a failing item between good ones; a corrupt block before the header errors
            check_streams(f"batch, corrupt rows {bad}", items, off, bad, mc)
    check_streams("no written_items", items, off, (), count + 1, want_written=False)
    off0 = np.zeros(1, np.int64)
    check_streams("no items", [], off0, (), 5, caps=[0, 9])
    check_streams("no items, no table", [], off0, (), 0, caps=[0])
    check_streams("empty source", [b"", b""], np.zeros(3, np.int64), (), 3, caps=[0, 5])


def test_streams_clipping(oracle):
    items, off, plain = streams_batch(oracle)
    walks = streams_walks(items, off)
    count = sum(w["chunks"] for w in walks)
    sizes = [w["decoded_bytes"] for w in walks]
    want_off = [0] + np.cumsum(sizes).tolist()
    comp = [(i, r) for i, w in enumerate(walks) for r in w["rows"] if r[0]]
    ci = next(i for i in range(8, 40) if walks[i]["compressed_chunks"] >= 2)    # an item with compressed chunks, and one of raw chunks alone
    ri = next(i for i in range(8, 40) if walks[i]["chunks"] and not walks[i]["compressed_chunks"])
    assert walks[ci]["compressed_chunks"] >= 2
    caps = cap_values([(want_off[i], want_off[i + 1]) for i in (ci, ri)], want_off[-1])
    victim = [j for j, (i, r) in enumerate(comp) if i == ci]
    for mc in (count, count + 37, count - 1):
        check_streams("clipped batch", items, off, (), mc, caps=caps)
    # the item's corrupt block counts only once the item is written
    check_streams("clipped corrupt item", items, off, (victim[0],), count + 2, caps=[want_off[ci + 1] - 1, want_off[ci + 1]])


# ---- wrapped messages ----------------------------------------------------------------------------------------------------------------
def wrapped_batch(oracle):
    """about 40 messages: compressed ones, one stored raw, an empty one, one of fewer than 8 bytes, a negative payload length"""
    msgs, plain = [], []
    for k in range(40):
        p = fr.noise(30 + 7 * k, k) if k % 5 == 4 else fr.mixed(oracle, 200 + 97 * k, k)
        c = oracle.compress(p)
        if c.size < p.size and k % 5 != 4:
            msgs.append(fr.header_wrap(p.size, c.size) + c.tobytes())
        else:
            msgs.append(fr.header_wrap(p.size, p.size) + p.tobytes())      # stored raw
        plain.append(p.tobytes())
    msgs[3], plain[3] = fr.header_wrap(0, 0), b""                           # an empty message
    msgs[11], plain[11] = b"\x01\x00\x00\x00\x00\x00\x00", None            # fewer than 8 bytes
    msgs[26], plain[26] = fr.header_wrap(10, -1) + b"abc", None            # a negative payload length
    return msgs, plain


def check_unwrap(name, msgs, bad_rows, caps=None, want_written=True):
    L = lib()
    n = len(msgs)
    src = np.frombuffer(b"".join(msgs) + fr.header_wrap(3, 3) + b"abc", np.uint8).copy()
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    src_len = int(off[n])
    refs = [fr.ref_unwrap(m) for m in msgs]
    want_off = [0] + (np.cumsum([r[2] for r in refs]).tolist() if n else [])
    total = want_off[-1]
    truth = fr.pattern(total + 8) ^ 0xFF
    comp = [k for k in range(n) if refs[k][1] == "comp"]
    results = [refs[k][3] - (1 if j in bad_rows else 0) for j, k in enumerate(comp)]
    size = L.emu_into_scratch_bytes(2, n, 0)
    assert size == L.emu_into_scratch_bytes(12, n, 0) + 2 * ((4 * n + 255) // 256 * 256)
    for dst_cap in (caps if caps is not None else [total + 24]):
        w_msgs = sum(1 for i in range(n) if want_off[i + 1] <= dst_cap)
        end = want_off[w_msgs]
        status = [r[0] for r in refs]
        for j in bad_rows:
            if comp[j] < w_msgs:
                status[comp[j]] = fr.WRAP_CORRUPT_BLOCK
        failing = [i for i in range(n) if status[i] != 0]
        want_info = (n, len(comp), total, failing[0] if failing else -1, status[failing[0]] if failing else 0)
        want = np.full(dst_cap + 32, FILL, np.uint8)
        for k in range(w_msgs):
            o = want_off[k]
            if refs[k][1] == "raw":
                want[o:o + refs[k][3]] = src[int(off[k]) + 8:int(off[k]) + 8 + refs[k][3]]
            elif refs[k][1] == "comp":
                want[o:want_off[k + 1]] = truth[o:want_off[k + 1]]
        for grid in GRIDS:
            what = f"{name}: dst_cap {dst_cap}, grid {grid}"
            pad = [0] * (n - len(comp))
            run, keep = run_record(results, truth, [int(off[k]) + 8 for k in comp], [want_off[k] for k in comp],
                                   [refs[k][3] if k < w_msgs else 0 for k in comp] + pad, [refs[k][2] if k < w_msgs else 0 for k in comp] + pad, n, len(comp), grid)
            scratch, dst = Buf(size, 0xC3), Buf(dst_cap + 32)
            info = UnwrapInfo(messages=-5, error=-5, reserved=-5)
            dst_off, st_arr = np.full(n + 3, -77, np.int64), np.full(n + 2, -77, np.int32)
            out_written = np.full(3, -77, np.int64)
            rc = L.emu_unwrap_into(addr(src), src_len, addr(off), n, scratch.ptr, size, dst.ptr if dst_cap else None, dst_cap, addr(dst_off, 1), addr(st_arr, 1),
                                   ref(info), addr(out_written, 1) if want_written else None, ref(run))
            assert rc == 0 and run.shape_errors == 0 and run.calls == (1 if n else 0), (what, rc, run.shape_errors, run.calls, run.error)
            assert run.decoded_rows == sum(1 for k in comp if k < w_msgs), what
            assert scratch.guards_intact() and dst.guards_intact(), what
            got = (info.messages, info.compressed, info.decoded_bytes, info.first_error, info.error)
            assert got == want_info and info.reserved == 0, (what, got, want_info)
            assert dst_off.tolist() == [-77] + want_off + [-77] and st_arr.tolist() == [-77] + status + [-77], what
            assert out_written.tolist() == [-77, w_msgs if want_written else -77, -77], (what, out_written.tolist(), w_msgs)
            assert np.array_equal(dst.a, want), f"{what}: first difference at byte {int(np.flatnonzero(dst.a != want)[0])}, end {end}"
            assert (dst.a[end:] == FILL).all(), what
        if dst_cap >= total and n:
            E = emu.framing()
            psize = E.emu_scratch_bytes(3, n, 0, 0)
            pscratch, pdst = Buf(psize, 0xC3), Buf(total)
            pinfo, pfinal = emu.UnwrapInfo(), emu.UnwrapInfo()
            p_off, p_st = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
            res = np.array(results + [0], np.int32)
            assert E.emu_lib_unwrap_index(addr(src), src_len, addr(off), n, addr(p_off), addr(p_st), pscratch.ptr, psize, ref(pinfo), 0) == 0
            assert E.emu_lib_unwrap_decode(addr(src), src_len, addr(off), n, ref(pinfo), pscratch.ptr, psize, pdst.ptr, total, addr(p_off), addr(p_st),
                                           ref(pfinal), addr(res), addr(truth), 0, 0) == 0
            assert info_bytes(info) == info_bytes(pfinal) and np.array_equal(dst.a[:total], pdst.a), f"{name}: differs from the two-call pair"
            assert dst_off[1:n + 2].tolist() == p_off.tolist() and st_arr[1:n + 1].tolist() == p_st.tolist(), name
    return refs, comp, want_off


def test_unwrap_parity(oracle):
    msgs, plain = wrapped_batch(oracle)
    refs, comp, want_off = check_unwrap("messages", msgs, ())
    assert [refs[k][0] for k in (3, 11, 26)] == [0, fr.WRAP_SIZE_INVALID, fr.WRAP_CORRUPT_HEADER] and len(comp) >= 20
    assert sum(1 for r in refs if r[1] == "raw") >= 8
    for k, r in enumerate(refs):                                            # the good messages unwrap to their source: LZ4Codec.Unwrap's answer
        assert plain[k] is None or r[2] == len(plain[k])
    check_unwrap("a corrupt block before the header errors", msgs, (2,))
    check_unwrap("corrupt blocks after them too", msgs, (len(comp) - 1, 4))
    good = [m for k, m in enumerate(msgs) if plain[k] is not None]
    check_unwrap("a corrupt block as the only error", good, (5,))
    check_unwrap("no written_messages", msgs, (), want_written=False)
    check_unwrap("no messages", [], (), caps=[0, 9])


def test_unwrap_clipping(oracle):
    msgs, plain = wrapped_batch(oracle)
    refs = [fr.ref_unwrap(m) for m in msgs]
    want_off = [0] + np.cumsum([r[2] for r in refs]).tolist()
    n = len(msgs)
    ck = [k for k in range(n) if refs[k][1] == "comp"][6]
    rk = [k for k in range(n) if refs[k][1] == "raw" and refs[k][2] > 0][3]
    caps = cap_values([(want_off[k], want_off[k + 1]) for k in (ck, rk)], want_off[-1])
    check_unwrap("clipped messages", msgs, (), caps=caps)
    comp = [k for k in range(n) if refs[k][1] == "comp"]
    check_unwrap("clipped corrupt message", msgs, (comp.index(ck),), caps=[want_off[ck + 1] - 1, want_off[ck + 1]])
