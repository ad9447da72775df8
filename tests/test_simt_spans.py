"""CPU-only: the span forms of the one-call decodes (lz4hip_framing.hpp: unwrap_spans_into, streams_decode_spans_into), the selection
kernel (spans_select) and the chunk directory of one stream (stream_directory) under the SIMT emulator (tests/simt/emu_spans.inc): the
real index, walk, clip, check, copy and info kernels, the library's fronts and sequences, on a scratch buffer of exactly the size asked
for between guard bytes, with the library's grids and with grids of 1 and 3.  The block decoder is emu_into.inc's stand-in, which
verifies the table it is handed row by row; it hands out each item's own plain bytes, so what a call leaves in dst is held against the
items' sources.  The identity cases run the consecutive entry points of emu_into.inc and the span entry points on the same arena in
the same library and compare every output byte for byte."""
import ctypes as C
import functools

import numpy as np

import emu_helpers as emu
import framing_cases as fr
import into_cases as into
from emu_helpers import addr, ref
from emu_lib import E_ARGUMENT, GRIDS, I64 as _I64, P as _P
from framing_cases import CORRUPT_BLOCK, EOS, OK, PASSES, TABLE_FULL
from into_cases import FILL, Buf, info_bytes, run_record
from lz4net_amd import stream as st
from lz4net_amd._lib import StreamInfo, StreamsInfo, UnwrapInfo
from stream_cases import expected_stream, frame



@functools.lru_cache(maxsize=None)
def lib():
    L = into.lib()                                                         # the consecutive forms, typed and their records checked
    L.emu_streams_decode_spans_into.argtypes = [_P, _I64, _P, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P]
    L.emu_unwrap_spans_into.argtypes = [_P, _I64, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]
    L.emu_spans_select.argtypes = [_P, _I64, _P, _I64, _P, _P, C.c_int]
    L.emu_stream_directory.argtypes = [_P, _I64, _I64, _P, _P, _P]
    L.emu_spans_stream_index.argtypes = [_P, _I64, _I64, _P, _I64, _P]
    return L


def i64(values):
    return np.array(list(values), np.int64)


def cap_values(offsets):
    """0, 1, each item boundary, total - 1, total, total + 4096"""
    total = int(offsets[-1])
    return sorted({0, 1, max(total - 1, 0), total, total + 4096} | {int(o) for o in offsets})


def valid_span(b, e, src_len):
    return 0 <= b <= e <= src_len


class Arena:
    """items back to back: the bytes (with bytes behind them that parse as more items), the offsets, each item's plain bytes by its
    span, and the begins of the items (wrapped messages) or the absolute header offsets of the chunks (streams) whose block is corrupt"""

    def __init__(self, items, plain, tail, corrupt=()):
        self.items, self.n = items, len(items)
        self.src = np.frombuffer(b"".join(items) + tail, np.uint8).copy()
        self.off = np.zeros(self.n + 1, np.int64)
        self.off[1:] = np.cumsum([len(s) for s in items])
        self.src_len = int(self.off[-1])
        self.plain = {(int(self.off[i]), int(self.off[i + 1])): np.frombuffer(bytes(plain[i]), np.uint8) for i in range(self.n) if plain[i] is not None}
        self.corrupt = set(corrupt)

    def spans_of(self, sel):
        return [(int(self.off[i]), int(self.off[i + 1])) for i in sel]


# ---- arena A: wrapped messages ----------------------------------------------------------------------------------------------------
CORRUPT_MSG, SHORT_MSG, PAST_END_MSG = 17, 23, 29


@functools.lru_cache(maxsize=None)
def arena_a(oracle):
    sizes = [0, 1, 7, 8, 9, 100, 300, 1024, 2500, 4096]
    msgs, plain = [], []
    for k in range(40):
        size = sizes[k % 10]
        if size == 100:
            p = fr.noise(100, k)                                            # incompressible
        elif size == 300:
            p = np.zeros(300, np.uint8)
        elif size >= 1024:
            p = oracle.gen(2 + (k // 10) % 2, 50 + k, 0, 1).reshape(-1)[:size].copy()       # D2 and D3
        else:
            p = fr.noise(size, k)
        c = oracle.compress(p) if size else p
        msgs.append(fr.header_wrap(p.size, c.size) + c.tobytes() if c.size < p.size else fr.header_wrap(p.size, p.size) + p.tobytes())
        plain.append(p.tobytes())
    msgs[SHORT_MSG], plain[SHORT_MSG] = b"\x01\x02\x03\x04\x05", None      # 5 bytes: SIZE_INVALID
    msgs[PAST_END_MSG], plain[PAST_END_MSG] = fr.header_wrap(10, 50) + b"abc", None          # payloadLength runs past its end
    a = Arena(msgs, plain, fr.header_wrap(3, 3) + b"abc")
    assert fr.ref_unwrap(msgs[CORRUPT_MSG])[1] == "comp"
    a.corrupt = {int(a.off[CORRUPT_MSG])}
    kinds = [fr.ref_unwrap(m)[1] for m in msgs]
    assert kinds.count("comp") >= 12 and kinds.count("raw") >= 12
    return a


def unwrap_call(a, spans, dst_cap, grid, consecutive=False, want_written=True):
    """One call on the messages `spans` of the arena -- through the consecutive entry point when the spans ARE the arena's offsets --
    checked against the model; -> every output, as bytes and lists."""
    L = lib()
    m = len(spans)
    refs = [fr.ref_unwrap(bytes(a.src[b:e])) if valid_span(b, e, a.src_len) else (E_ARGUMENT, None, 0, 0) for b, e in spans]
    want_off = [0] + np.cumsum([r[2] for r in refs]).tolist() if m else [0]
    total = want_off[-1]
    truth = np.zeros(total + 8, np.uint8)
    comp = [j for j in range(m) if refs[j][1] == "comp"]
    for j in comp:
        truth[want_off[j]:want_off[j + 1]] = a.plain[spans[j]]
    results = [refs[j][3] - (1 if spans[j][0] in a.corrupt else 0) for j in comp]
    w_msgs = sum(1 for j in range(m) if want_off[j + 1] <= dst_cap)
    end = want_off[w_msgs]
    status = [r[0] for r in refs]
    for j in comp:
        if j < w_msgs and spans[j][0] in a.corrupt:
            status[j] = fr.WRAP_CORRUPT_BLOCK
    failing = [j for j in range(m) if status[j] != 0]
    want_info = (m, len(comp), total, failing[0] if failing else -1, status[failing[0]] if failing else 0)
    want = np.full(dst_cap + 32, FILL, np.uint8)
    for j in range(w_msgs):
        if refs[j][1] == "raw":
            want[want_off[j]:want_off[j + 1]] = a.src[spans[j][0] + 8:spans[j][0] + 8 + refs[j][3]]
        elif refs[j][1] == "comp":
            want[want_off[j]:want_off[j + 1]] = truth[want_off[j]:want_off[j + 1]]
    what = f"{m} messages, dst_cap {dst_cap}, grid {grid}, consecutive {consecutive}"
    pad = [0] * (m - len(comp))
    run, keep = run_record(results, truth, [spans[j][0] + 8 for j in comp], [want_off[j] for j in comp],
                           [refs[j][3] if j < w_msgs else 0 for j in comp] + pad, [refs[j][2] if j < w_msgs else 0 for j in comp] + pad, m, len(comp), grid)
    size = L.emu_into_scratch_bytes(2, m, 0)
    scratch, dst = Buf(size, 0xC3), Buf(dst_cap + 32)
    info = UnwrapInfo(messages=-5, error=-5, reserved=-5)
    dst_off, st_arr = np.full(m + 3, -77, np.int64), np.full(m + 2, -77, np.int32)
    out_written = np.full(3, -77, np.int64)
    begin, stop = i64([s[0] for s in spans] + [-99]), i64([s[1] for s in spans] + [-99])
    tail = (scratch.ptr, size, dst.ptr if dst_cap else None, dst_cap, addr(dst_off, 1), addr(st_arr, 1), ref(info),
            addr(out_written, 1) if want_written else None, ref(run))
    if consecutive:
        assert spans == a.spans_of(range(a.n))
        rc = L.emu_unwrap_into(addr(a.src), a.src_len, addr(a.off), m, *tail)
    else:
        rc = L.emu_unwrap_spans_into(addr(a.src), a.src_len, addr(begin), addr(stop), m, *tail)
    assert rc == 0 and run.shape_errors == 0 and run.calls == (1 if m else 0), (what, rc, run.shape_errors, run.calls, run.error)
    assert run.decoded_rows == sum(1 for j in comp if j < w_msgs), what
    assert scratch.guards_intact() and dst.guards_intact(), what
    got = (info.messages, info.compressed, info.decoded_bytes, info.first_error, info.error)
    assert got == want_info and info.reserved == 0, (what, got, want_info)
    assert dst_off.tolist() == [-77] + want_off + [-77] and st_arr.tolist() == [-77] + status + [-77], what
    assert out_written.tolist() == [-77, w_msgs if want_written else -77, -77], (what, out_written.tolist(), w_msgs)
    assert np.array_equal(dst.a, want), f"{what}: first difference at byte {int(np.flatnonzero(dst.a != want)[0])}, end {end}"
    assert (dst.a[end:] == FILL).all(), what
    return dict(dst=dst.whole.tobytes(), dst_off=dst_off.tolist(), status=st_arr.tolist(), info=info_bytes(info), written=out_written.tolist(),
                off=want_off, total=total, first_error=info.first_error, compressed=info.compressed)


def test_unwrap_identity(oracle):
    a = arena_a(oracle)
    spans = a.spans_of(range(a.n))
    full = unwrap_call(a, spans, 1 << 20, 0)
    assert [full["status"][1 + k] for k in (CORRUPT_MSG, SHORT_MSG, PAST_END_MSG)] == [fr.WRAP_CORRUPT_BLOCK, fr.WRAP_SIZE_INVALID, fr.WRAP_CORRUPT_HEADER]
    for i in range(a.n):                                                    # the good messages unwrap to their source
        if i not in (SHORT_MSG, PAST_END_MSG):
            assert full["off"][i + 1] - full["off"][i] == len(a.plain[spans[i]])
    for dst_cap in cap_values(full["off"]):
        for grid in GRIDS:
            assert unwrap_call(a, spans, dst_cap, grid, consecutive=True) == unwrap_call(a, spans, dst_cap, grid), (dst_cap, grid)
    assert unwrap_call(a, spans, full["total"], 0, consecutive=True, want_written=False) == unwrap_call(a, spans, full["total"], 0, want_written=False)


def selections(n, repeat):
    return {"reversed": list(range(n - 1, -1, -1)), "every second left out": list(range(3, n, 2)), "one item three times": [2, repeat, repeat, repeat, 5]}


def test_unwrap_selection(oracle):
    a = arena_a(oracle)
    full = unwrap_call(a, a.spans_of(range(a.n)), 1 << 20, 0)
    body = full["dst"][64:]
    for name, sel in selections(a.n, CORRUPT_MSG - 8).items():
        for grid in GRIDS:
            got = unwrap_call(a, a.spans_of(sel), full["total"] * 2, grid)
            # the concatenation, in call order, of those messages' outputs from the full decode; a failing message (its bytes are
            # unspecified) leaves its neighbours' intact
            for j, i in enumerate(sel):
                assert got["status"][1 + j] == full["status"][1 + i], (name, j)
                if full["status"][1 + i] == 0:
                    assert got["dst"][64 + got["off"][j]:64 + got["off"][j + 1]] == body[full["off"][i]:full["off"][i + 1]], (name, j)
            failing = [j for j, i in enumerate(sel) if full["status"][1 + i] != 0]
            assert got["first_error"] == (failing[0] if failing else -1), name
            assert got["total"] == sum(full["off"][i + 1] - full["off"][i] for i in sel), name
            assert got["compressed"] == sum(1 for i in sel if fr.ref_unwrap(a.items[i])[1] == "comp"), name
    assert unwrap_call(a, [], 9, 0)["total"] == 0                           # no span at all


def bad_spans(a):
    i = 6
    b, e = int(a.off[i]), int(a.off[i + 1])
    return [(-1, e), (e, b), (b, a.src_len + 1), (-1, -1)]


def test_unwrap_bad_spans_and_clip(oracle):
    a = arena_a(oracle)
    good = a.spans_of([4, 7, 8, 9])
    for bad in bad_spans(a):
        spans = good[:2] + [bad] + good[2:]
        got = unwrap_call(a, spans, 1 << 16, 3)
        assert got["status"][1:-1] == [0, 0, E_ARGUMENT, 0, 0] and got["off"][2] == got["off"][3] and got["first_error"] == 2
    # a prefix in call order, for a permuted selection with a repeat
    sel = [9, 1, 38, 7, 9, 0, 6, 19, 28]
    spans = a.spans_of(sel)
    offs = unwrap_call(a, spans, 1 << 20, 0)["off"]
    for dst_cap in cap_values(offs):
        for grid in GRIDS:
            unwrap_call(a, spans, dst_cap, grid)
    # the corrupt message counts only once it is written
    spans = a.spans_of([8, CORRUPT_MSG, 9])
    offs = unwrap_call(a, spans, 1 << 20, 0)["off"]
    assert unwrap_call(a, spans, offs[2] - 1, 0)["first_error"] == -1 and unwrap_call(a, spans, offs[2], 0)["first_error"] == 1


def test_select_kernel(oracle):
    L = lib()
    a = arena_a(oracle)
    sel = i64([5, -1, a.n, 0, a.n - 1, 5, 1 << 40, -(1 << 40)] + list(range(a.n)) * 20)
    for grid in GRIDS:
        begin, end = np.full(sel.size + 2, -77, np.int64), np.full(sel.size + 2, -77, np.int64)
        assert L.emu_spans_select(addr(a.off), a.n, addr(sel), sel.size, addr(begin, 1), addr(end, 1), grid) == 0
        inside = (sel >= 0) & (sel < a.n)
        safe = np.where(inside, sel, 0)
        assert begin.tolist() == [-77] + np.where(inside, a.off[safe], -1).tolist() + [-77]
        assert end.tolist() == [-77] + np.where(inside, a.off[safe + 1], -1).tolist() + [-77]
    # what it writes for sel = -1 and sel = n is a bad span to the decoders
    got = unwrap_call(a, [(int(begin[1 + k]), int(end[1 + k])) for k in range(4)], 1 << 16, 0)
    assert got["status"][1:-1] == [0, E_ARGUMENT, E_ARGUMENT, 0]
    assert L.emu_spans_select(addr(a.off), a.n, addr(sel), 0, None, None, 0) == 0
    for args in ((None, a.n, addr(sel), 3, addr(begin), addr(end)), (addr(a.off), a.n, None, 3, addr(begin), addr(end)),
                 (addr(a.off), a.n, addr(sel), 3, None, addr(end)), (addr(a.off), a.n, addr(sel), 3, addr(begin), None),
                 (addr(a.off), -1, addr(sel), 3, addr(begin), addr(end)), (addr(a.off), a.n, addr(sel), -1, addr(begin), addr(end))):
        assert L.emu_spans_select(*args, 0) == E_ARGUMENT


# ---- arena B: LZ4Stream items -----------------------------------------------------------------------------------------------------
B = 256
CUT_ITEM, CORRUPT_ITEM, PASSES_ITEM, EMPTIES_ITEM = 9, 18, 17, 21


@functools.lru_cache(maxsize=None)
def arena_b(oracle):
    sizes = [0, 1, 255, 256, 257, 700, 1024, 2560, 90, 1500, 513, 2048]
    items, plain = [], []
    for i in range(24):
        size = sizes[i % 12]
        p = fr.noise(size, i) if i % 4 == 3 else fr.mixed(oracle, size, i)  # raw chunks, and compressed ones
        items.append(expected_stream(oracle, p, B, False))
        plain.append(p.tobytes())
    rows = fr.ref_walk(items[CUT_ITEM])["rows"]
    items[CUT_ITEM] = items[CUT_ITEM][:rows[-1][1] + 1]                      # cut inside its last header
    items[PASSES_ITEM], plain[PASSES_ITEM] = frame([(0, 4, b"abcd"), (5, 9, b"\x40abc")]), b"abcd"       # passes != 0, behind a raw chunk
    p = np.frombuffer(plain[EMPTIES_ITEM], np.uint8)
    items[EMPTIES_ITEM] = b"\x00\x00" + expected_stream(oracle, p[:B], B, False) + b"\x00\x00\x00\x00" + expected_stream(oracle, p[B:], B, False) + b"\x00\x00"
    a = Arena(items, plain, fr.TAIL)
    walks = [fr.ref_walk(s) for s in items]
    assert [walks[i]["status"] for i in (CUT_ITEM, PASSES_ITEM, EMPTIES_ITEM)] == [EOS, PASSES, OK] and walks[0]["chunks"] == 0
    assert max(w["chunks"] for w in walks) == 10 and walks[EMPTIES_ITEM]["decoded_bytes"] == p.size
    victim = [r for r in walks[CORRUPT_ITEM]["rows"] if r[0]]
    assert len(victim) >= 2
    a.corrupt = {int(a.off[CORRUPT_ITEM]) + victim[1][1]}
    assert sum(w["compressed_chunks"] for w in walks) >= 20 and sum(w["chunks"] - w["compressed_chunks"] for w in walks) >= 20
    return a


def streams_call(a, spans, max_chunks, dst_cap, grid, consecutive=False, want_written=True):
    """One call on the items `spans` of the arena -- through the consecutive entry point when the spans ARE the arena's offsets --
    checked against the model; -> every output, as bytes and lists."""
    L = lib()
    m = len(spans)
    none = dict(rows=[], status=E_ARGUMENT, error_offset=-1, chunks=0, compressed_chunks=0, decoded_bytes=0)
    walks = [fr.ref_walk(bytes(a.src[b:e])) if valid_span(b, e, a.src_len) else none for b, e in spans]
    want_off = [0] + np.cumsum([w["decoded_bytes"] for w in walks]).tolist() if m else [0]
    total = want_off[-1]
    truth = np.zeros(total + 8, np.uint8)
    chunks = sum(w["chunks"] for w in walks)
    comp = [(j, r) for j, w in enumerate(walks) for r in w["rows"] if r[0]]
    for j, r in comp:
        truth[want_off[j] + r[5]:want_off[j] + r[5] + r[4]] = a.plain[spans[j]][r[5]:r[5] + r[4]]
    is_full = chunks > max_chunks
    tabled = [] if is_full else comp                                        # (a full table is not filled at all)
    hurt = lambda j, r: spans[j][0] + r[1] in a.corrupt                     # noqa: E731
    results = [r[3] - (1 if hurt(j, r) else 0) for j, r in comp]
    w_items = 0 if is_full else sum(1 for j in range(m) if want_off[j + 1] <= dst_cap)
    end = want_off[w_items]
    status, err_off = [w["status"] for w in walks], [w["error_offset"] for w in walks]
    for j in sorted({j for j, r in comp if j < w_items and hurt(j, r)}):
        status[j] = CORRUPT_BLOCK
        err_off[j] = min(r[1] for jj, r in comp if jj == j and hurt(jj, r))
    failing = [j for j in range(m) if status[j] != OK]
    want_info = (m, chunks, len(comp), total, failing[0] if failing else -1, err_off[failing[0]] if failing else -1, status[failing[0]] if failing else OK)
    if is_full:
        want_info = want_info[:4] + (-1, -1, TABLE_FULL)
    want = np.full(dst_cap + 32, FILL, np.uint8)
    for j in range(w_items):
        for r in walks[j]["rows"]:
            o, at = want_off[j] + r[5], spans[j][0] + r[2]
            want[o:o + r[4]] = truth[o:o + r[4]] if r[0] else a.src[at:at + r[3]]
    what = f"{m} items, max_chunks {max_chunks}, dst_cap {dst_cap}, grid {grid}, consecutive {consecutive}"
    pad = [0] * (max_chunks - len(tabled))
    run, keep = run_record(results, truth, [spans[j][0] + r[2] for j, r in tabled], [want_off[j] + r[5] for j, r in tabled],
                           [r[3] if j < w_items else 0 for j, r in tabled] + pad, [r[4] if j < w_items else 0 for j, r in tabled] + pad,
                           max_chunks, len(tabled), grid)
    size = L.emu_into_scratch_bytes(1, m, max_chunks)
    scratch, dst = Buf(size, 0xC3), Buf(dst_cap + 32)
    info = StreamsInfo(items=-5, error=-5, reserved=-5)
    dst_off, st_arr, eo = np.full(m + 3, -77, np.int64), np.full(m + 2, -77, np.int32), np.full(m + 2, -77, np.int64)
    out_written = np.full(3, -77, np.int64)
    begin, stop = i64([s[0] for s in spans] + [-99]), i64([s[1] for s in spans] + [-99])
    tail = (max_chunks, scratch.ptr if size else None, size, dst.ptr if dst_cap else None, dst_cap, addr(dst_off, 1), addr(st_arr, 1), addr(eo, 1),
            ref(info), addr(out_written, 1) if want_written else None, ref(run))
    if consecutive:
        assert spans == a.spans_of(range(a.n))
        rc = L.emu_streams_decode_into(addr(a.src), a.src_len, addr(a.off), m, *tail)
    else:
        rc = L.emu_streams_decode_spans_into(addr(a.src), a.src_len, addr(begin), addr(stop), m, *tail)
    assert rc == 0 and run.shape_errors == 0 and run.calls == (1 if m and max_chunks else 0), (what, rc, run.shape_errors, run.calls, run.error)
    assert run.decoded_rows == sum(1 for j, r in tabled if j < w_items), what
    assert scratch.guards_intact() and dst.guards_intact(), what
    got = (info.items, info.chunks, info.compressed_chunks, info.decoded_bytes, info.first_error, info.error_offset, info.error)
    assert got == want_info and info.reserved == 0, (what, got, want_info)
    assert dst_off.tolist() == [-77] + want_off + [-77], what
    assert st_arr.tolist() == [-77] + status + [-77] and eo.tolist() == [-77] + err_off + [-77], what
    assert out_written.tolist() == [-77, w_items if want_written else -77, -77], (what, out_written.tolist(), w_items)
    assert np.array_equal(dst.a, want), f"{what}: first difference at byte {int(np.flatnonzero(dst.a != want)[0])}, end {end}"
    assert (dst.a[end:] == FILL).all(), what
    return dict(dst=dst.whole.tobytes(), dst_off=dst_off.tolist(), status=st_arr.tolist(), error_offset=eo.tolist(), info=info_bytes(info),
                written=out_written.tolist(), off=want_off, total=total, first_error=info.first_error, chunks=info.chunks,
                compressed_chunks=info.compressed_chunks, walks=walks)


def test_streams_identity(oracle):
    a = arena_b(oracle)
    spans = a.spans_of(range(a.n))
    full = streams_call(a, spans, 1 << 10, 1 << 20, 0)
    count = full["chunks"]
    assert [full["status"][1 + i] for i in (CUT_ITEM, CORRUPT_ITEM, PASSES_ITEM)] == [EOS, CORRUPT_BLOCK, PASSES]
    for i in range(a.n):                                                    # the good items decode to their source
        if full["status"][1 + i] == OK:
            assert full["dst"][64 + full["off"][i]:64 + full["off"][i + 1]] == a.plain[spans[i]].tobytes(), i
    for dst_cap in cap_values(full["off"]):
        for grid in GRIDS:
            assert streams_call(a, spans, count + 5, dst_cap, grid, consecutive=True) == streams_call(a, spans, count + 5, dst_cap, grid), (dst_cap, grid)
    for mc in (count - 1, count, count + 37, 0):
        assert streams_call(a, spans, mc, full["total"] + 24, 0, consecutive=True) == streams_call(a, spans, mc, full["total"] + 24, 0), mc
    assert (streams_call(a, spans, count, full["total"], 0, consecutive=True, want_written=False) ==
            streams_call(a, spans, count, full["total"], 0, want_written=False))


def test_streams_selection(oracle):
    a = arena_b(oracle)
    full = streams_call(a, a.spans_of(range(a.n)), 1 << 10, 1 << 20, 0)
    body = full["dst"][64:]
    for name, sel in selections(a.n, CORRUPT_ITEM).items():
        need = sum(full["walks"][i]["chunks"] for i in sel)
        for grid in GRIDS:
            got = streams_call(a, a.spans_of(sel), need + 37, full["total"] * 2, grid)     # a table with 37 rows to spare
            for j, i in enumerate(sel):
                assert (got["status"][1 + j], got["error_offset"][1 + j]) == (full["status"][1 + i], full["error_offset"][1 + i]), (name, j)
                if full["status"][1 + i] != CORRUPT_BLOCK:                  # (a corrupt block's own bytes are unspecified; its neighbours' are not)
                    assert got["dst"][64 + got["off"][j]:64 + got["off"][j + 1]] == body[full["off"][i]:full["off"][i + 1]], (name, j)
            failing = [j for j, i in enumerate(sel) if full["status"][1 + i] != OK]
            assert got["first_error"] == (failing[0] if failing else -1), name
            assert got["chunks"] == need and got["total"] == sum(full["off"][i + 1] - full["off"][i] for i in sel), name
            assert got["compressed_chunks"] == sum(full["walks"][i]["compressed_chunks"] for i in sel), name
        streams_call(a, a.spans_of(sel), need, full["total"] * 2, 0)        # the exact table
    assert streams_call(a, [], 5, 9, 0)["total"] == 0                       # no span at all


def test_streams_bad_spans_clip_and_table_full(oracle):
    a = arena_b(oracle)
    good = a.spans_of([4, 7, 8, 10])
    for bad in bad_spans(a):
        spans = good[:2] + [bad] + good[2:]
        got = streams_call(a, spans, 64, 1 << 16, 3)
        assert got["status"][1:-1] == [0, 0, E_ARGUMENT, 0, 0] and got["off"][2] == got["off"][3] and got["first_error"] == 2
    sel = [7, 1, 22, 9, 7, 0, 6, 20, 5]                                      # a permuted selection with a repeat and a header error
    spans = a.spans_of(sel)
    ref_run = streams_call(a, spans, 128, 1 << 20, 0)
    for dst_cap in cap_values(ref_run["off"]):
        for grid in GRIDS:
            streams_call(a, spans, ref_run["chunks"] + 2, dst_cap, grid)
    # repeats push the chunk count over max_chunks: nothing is written, written_items = 0, info.chunks is the need
    one = fr.ref_walk(a.items[7])["chunks"]
    assert one == 10
    for grid in GRIDS:
        got = streams_call(a, a.spans_of([7, 7, 7]), 2 * one + 3, 1 << 16, grid)
        assert got["chunks"] == 3 * one and got["written"][1] == 0 and got["first_error"] == -1
        streams_call(a, a.spans_of([7, 7, 7]), 3 * one, 1 << 16, grid)
    # the corrupt item counts only once it is written
    spans = a.spans_of([8, CORRUPT_ITEM, 10])
    offs = streams_call(a, spans, 64, 1 << 20, 0)["off"]
    assert streams_call(a, spans, 64, offs[2] - 1, 0)["first_error"] == -1 and streams_call(a, spans, 64, offs[2], 0)["first_error"] == 1


def test_argument_checks_without_a_device(oracle):
    L = lib()
    a = arena_b(oracle)
    m, mc = 3, 8
    begin, end = i64(a.off[:m]), i64(a.off[1:m + 1])
    dst, dst_off, status, eo = np.zeros(64, np.uint8), np.zeros(m + 1, np.int64), np.zeros(m, np.int32), np.zeros(m, np.int64)
    run, keep = run_record([], np.zeros(0, np.uint8), [], [], [0] * mc, [0] * mc, mc, 0, 0)
    need = L.emu_into_scratch_bytes(1, m, mc)
    scratch = np.zeros(need, np.uint8)
    info = StreamsInfo()
    good = dict(src=addr(a.src), src_len=a.src_len, begin=addr(begin), end=addr(end), m=m, max_chunks=mc, scratch=addr(scratch), scratch_bytes=need,
                dst=addr(dst), dst_cap=64, dst_off=addr(dst_off), status=addr(status), eo=addr(eo), info=ref(info), written=None)

    def streams(**change):
        g = dict(good, **change)
        run.calls = 0
        rc = L.emu_streams_decode_spans_into(g["src"], g["src_len"], g["begin"], g["end"], g["m"], g["max_chunks"], g["scratch"], g["scratch_bytes"],
                                             g["dst"], g["dst_cap"], g["dst_off"], g["status"], g["eo"], g["info"], g["written"], ref(run))
        assert rc == 0 or run.calls == 0                                    # a refusal launches nothing
        return rc

    for change in (dict(begin=None), dict(end=None), dict(status=None), dict(eo=None), dict(scratch=None), dict(src=None), dict(dst=None),
                   dict(dst_off=None), dict(info=None), dict(src_len=-1), dict(m=-1), dict(max_chunks=-1), dict(dst_cap=-1),
                   dict(scratch_bytes=need - 1), dict(m=1 << 31), dict(max_chunks=1 << 31)):
        assert streams(**change) == E_ARGUMENT, change
        assert run.error, change
    assert streams(m=0, begin=None, end=None, status=None, eo=None, scratch=None, scratch_bytes=0) == 0     # nothing chosen: nothing needed

    a = arena_a(oracle)
    begin, end = i64(a.off[:m]), i64(a.off[1:m + 1])
    need = L.emu_into_scratch_bytes(2, m, 0)
    scratch = np.zeros(need, np.uint8)
    uinfo = UnwrapInfo()
    urun, ukeep = run_record([], np.zeros(0, np.uint8), [], [], [0] * m, [0] * m, m, 0, 0)
    good = dict(src=addr(a.src), src_len=a.src_len, begin=addr(begin), end=addr(end), m=m, scratch=addr(scratch), scratch_bytes=need, dst=addr(dst),
                dst_cap=64, dst_off=addr(dst_off), status=addr(status), info=ref(uinfo), written=None)

    def unwrap(**change):
        g = dict(good, **change)
        urun.calls = 0
        rc = L.emu_unwrap_spans_into(g["src"], g["src_len"], g["begin"], g["end"], g["m"], g["scratch"], g["scratch_bytes"], g["dst"], g["dst_cap"],
                                     g["dst_off"], g["status"], g["info"], g["written"], ref(urun))
        assert rc == 0 or urun.calls == 0
        return rc

    for change in (dict(begin=None), dict(end=None), dict(status=None), dict(scratch=None), dict(src=None), dict(dst=None), dict(dst_off=None),
                   dict(info=None), dict(src_len=-1), dict(m=-1), dict(dst_cap=-1), dict(scratch_bytes=need - 1), dict(m=1 << 31)):
        assert unwrap(**change) == E_ARGUMENT, change
        assert urun.error, change

    hdr, out, sinfo = np.zeros(4, np.int64), np.zeros(4, np.int64), StreamInfo()
    src = np.frombuffer(a.items[0] + fr.TAIL, np.uint8).copy()
    for args in ((None, 8, 3, addr(hdr), addr(out), ref(sinfo)), (addr(src), -1, 3, addr(hdr), addr(out), ref(sinfo)),
                 (addr(src), 8, -1, addr(hdr), addr(out), ref(sinfo)), (addr(src), 8, 3, None, addr(out), ref(sinfo)),
                 (addr(src), 8, 3, addr(hdr), None, ref(sinfo)), (addr(src), 8, 3, addr(hdr), addr(out), None)):
        assert L.emu_stream_directory(*args) == E_ARGUMENT, args


# ---- the chunk directory of one stream ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def directory_stream(oracle):
    """about 40 chunks with block sizes 256 .. 4096, raw and compressed, with empty chunks between the parts -> (stream, plain)"""
    parts, plain = [], []
    for k, block in enumerate((256, 1000, 4096, 512)):
        data = np.concatenate([fr.mixed(oracle, 4 * block + 17, k), fr.noise(3 * block, 20 + k), fr.mixed(oracle, 3 * block, 30 + k)])
        parts += [expected_stream(oracle, data, block, False), b"\x00\x00"]
        plain.append(data.tobytes())
    stream, plain = b"".join(parts), b"".join(plain)
    rows = fr.ref_walk(stream)["rows"]
    assert 40 <= len(rows) <= 50 and sum(1 for r in rows if r[0]) >= 12 and sum(1 for r in rows if not r[0]) >= 8
    return stream, plain


def python_directory(stream):
    """stream.parse_chunks plus the header lengths -> (hdr_off, out_off) of the non-empty chunks, without the closing entry"""
    hdr_off, out_off, out = [], [], 0
    for compressed, original, payload, clen in st.parse_chunks(stream):
        hdr = payload - len(st.write_varint(1 if compressed else 0)) - len(st.write_varint(original)) - (len(st.write_varint(clen)) if compressed else 0)
        if original:
            hdr_off.append(hdr)
            out_off.append(out)
        out += original
    return hdr_off, out_off


def run_directory(stream, max_chunks):
    """-> (hdr_off, out_off with the guard entries around them, info bytes, the index's info bytes for the same table)"""
    L = lib()
    src = np.frombuffer(bytes(stream) + fr.TAIL, np.uint8).copy()
    hdr, out = np.full(max_chunks + 3, -77, np.int64), np.full(max_chunks + 3, -77, np.int64)
    info, index_info = StreamInfo(chunks=-5, error=-5, reserved=-5), StreamInfo()
    assert L.emu_stream_directory(addr(src), len(stream), max_chunks, addr(hdr, 1), addr(out, 1), ref(info)) == 0
    size = L.emu_into_scratch_bytes(10, max_chunks, 0)
    scratch = Buf(size)
    assert L.emu_spans_stream_index(addr(src), len(stream), max_chunks, scratch.ptr, size, ref(index_info)) == 0
    assert info_bytes(info) == info_bytes(index_info), (max_chunks, len(stream))
    return hdr.tolist(), out.tolist(), info


def test_directory(oracle):
    stream, plain = directory_stream(oracle)
    want_hdr, want_out = python_directory(stream)
    count = len(want_hdr)
    for mc in (count, count + 37):
        hdr, out, info = run_directory(stream, mc)
        pad = [-77] * (mc - count + 1)
        assert hdr == [-77] + want_hdr + [len(stream)] + pad and out == [-77] + want_out + [len(plain)] + pad
        assert (info.chunks, info.decoded_bytes, info.error, info.error_offset) == (count, len(plain), OK, -1)
    # max_chunks = chunks - 1: TABLE_FULL, the count needed, no closing entry and no entry past max_chunks
    hdr, out, info = run_directory(stream, count - 1)
    assert hdr == [-77] + want_hdr[:count - 1] + [-77, -77] and out == [-77] + want_out[:count - 1] + [-77, -77]
    assert (info.chunks, info.error, info.error_offset) == (count, TABLE_FULL, want_hdr[count - 1])
    hdr, out, info = run_directory(stream, 0)
    assert hdr == [-77] * 3 and info.error == TABLE_FULL
    # truncated inside a header and inside a payload: the entries up to the failing chunk, the closing entry at error_offset
    rows = fr.ref_walk(stream)["rows"]
    k = 30
    for cut in (rows[k][1] + 1, rows[k][2] + rows[k][3] - 1):
        hdr, out, info = run_directory(stream[:cut], count)
        assert (info.chunks, info.error, info.error_offset) == (k, EOS, rows[k][1])
        assert hdr[:k + 3] == [-77] + want_hdr[:k] + [rows[k][1], -77] and out[:k + 3] == [-77] + want_out[:k] + [want_out[k], -77]
    hdr, out, info = run_directory(b"", 2)
    assert hdr == [-77, 0, -77, -77, -77] and out == [-77, 0, -77, -77, -77] and info.chunks == 0
    hdr, out, info = run_directory(b"\x00\x00\x00\x00", 2)                  # only empty chunks: the closing entry alone
    assert hdr == [-77, 4, -77, -77, -77] and out == [-77, 0, -77, -77, -77]


def test_directory_spans_decode(oracle):
    stream, plain = directory_stream(oracle)
    hdr, out, info = run_directory(stream, 64)
    count = info.chunks
    hdr, out = hdr[1:count + 2], out[1:count + 2]
    chunk_plain = [plain[out[k]:out[k + 1]] for k in range(count)]
    a = Arena([stream], [b""], fr.TAIL)
    a.plain = {(hdr[k], hdr[k + 1]): np.frombuffer(chunk_plain[k], np.uint8) for k in range(count)}
    spans = [(hdr[k], hdr[k + 1]) for k in range(count)]
    for grid in GRIDS:
        got = streams_call(a, spans, count, len(plain) + 24, grid)          # all chunks as one-chunk spans: the whole plain text
        assert got["dst"][64:64 + len(plain)] == plain and got["status"][1:-1] == [OK] * count and got["off"][:-1] == out[:-1]
    for k0, k1 in ((0, 0), (3, 5), (11, 30), (count - 1, count - 1)):
        got = streams_call(a, spans[k0:k1 + 1], k1 - k0 + 1, out[k1 + 1] - out[k0], 3)
        assert got["dst"][64:64 + got["total"]] == plain[out[k0]:out[k1 + 1]], (k0, k1)
        assert got["written"][1] == k1 - k0 + 1 and got["first_error"] == -1
