"""CPU-only: the legacy frame path (lz4net_amd/csrc/lz4hip_frame.hpp and its host code in lz4hip_framing.hpp) under the SIMT emulator
(tests/simt/emu_frame.inc): the real kernels, the library's fronts, launch sequences and host-pointer calls, with the block codec
replaced by results and bytes computed here with the oracle.  Every case runs with the library's grids and with grids forced to 1 and 3
workgroups.  The reference reader is modelled by frame_cases.reader: parse_frame's walk plus LZ4_uncompress_unknownOutputSize(in, out, size,
chunk_size) per chunk."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import ref_records as rr
import sizes_helpers as sh
from emu_lib import E_ARGUMENT, GRIDS, GUARD, Guarded, u8
from frame_cases import (BAD_MAGIC, BAD_SIZE, CORRUPT_BLOCK, MAGIC, OK, TABLE_FULL, TRUNCATED, FrameTables, Index, bound, emu, info_tuple,
                         make_frame, reader, sample, walk)
from lz4net_amd import legacy_frame as lf
from lz4net_amd._lib import FrameInfo


# ---- the calls ----------------------------------------------------------------------------------------------------------------
def encode(oracle, data, chunk, hc=False, grid=0, results=None, chunk_arg=None):
    """frame_encode under the emulator with the oracle as the block encoder -> (rc, frame bytes, dst_len)"""
    data = u8(data)
    n = (data.size + chunk - 1) // chunk
    stride = bound(min(chunk, data.size))
    comp = np.zeros(n * stride + 1, np.uint8)
    res = np.zeros(n + 1, np.int32)
    for k in range(n):
        piece = data[k * chunk:(k + 1) * chunk]
        if results is None:
            c = oracle.compress(piece, hc=hc)
        else:
            c = np.full(results(piece.size), 0x40 + k % 64, np.uint8)
        res[k] = len(c)
        comp[k * stride:k * stride + len(c)] = c
    chunk_arg = chunk if chunk_arg is None else chunk_arg
    cap = emu().emu_frame_bound(data.size, chunk_arg)
    dst = Guarded(cap)
    scratch = Guarded(emu().emu_frame_encode_scratch_bytes(data.size, chunk_arg))
    dst_len = np.full(3, -77, np.int64)
    text = C.create_string_buffer(200)
    rc = emu().emu_frame_encode(data.ctypes.data, data.size, chunk_arg, int(hc), dst.ptr, cap, dst_len.ctypes.data + 8, scratch.ptr, scratch.n,
                                res.ctypes.data, comp.ctypes.data, grid, text, 200)
    assert rc == 0, text.value
    assert dst.intact() and scratch.intact() and dst_len[0] == -77 and dst_len[2] == -77
    total = int(dst_len[1])
    assert 4 <= total <= cap and (dst.a[total:] == GUARD).all(), "bytes after dst_len were written"
    expect = MAGIC + b"".join(int(res[k]).to_bytes(4, "little") + comp[k * stride:k * stride + res[k]].tobytes() for k in range(n))
    return bytes(dst.a[:total]), expect, cap


def check_index(oracle, frame, chunk, grid, max_chunks=None):
    """the index of `frame` against parse_frame / `walk` and the reference's sizes; returns the Index"""
    chunks, err, err_off = walk(frame, chunk)
    m = len(chunks) + 3 if max_chunks is None else max_chunks
    ix = Index(frame, chunk, m, grid)
    assert ix.rc == 0, ix.text
    assert ix.rows() == chunks
    if err == OK:
        assert chunks == lf.parse_frame(bytes(frame))
    a = u8(frame)
    sizes = sh.reference_sizes([a[at:at + size] for at, size in chunks])     # unbounded: what the walk finds
    caps = [int(r) if 0 <= r <= chunk else 0 for r in sizes]
    offs = np.concatenate(([0], np.cumsum(caps, dtype=np.int64))).astype(np.int64)
    bad = [k for k, r in enumerate(sizes) if not 0 <= r <= chunk]
    n = len(chunks)
    assert list(ix.dst_cap[:n]) == caps and list(ix.dst_off[:n + 1]) == list(offs)
    assert (ix.src_len[n:] == 0).all() and (ix.dst_cap[n:] == 0).all() and (ix.dst_off[n:] == offs[-1]).all(), "rows past the count are not empty"
    if bad:
        want = (n, int(offs[-1]), int(offs[bad[0]]), chunks[bad[0]][0] - 4, CORRUPT_BLOCK)
    else:
        want = (n, int(offs[-1]), int(offs[-1]), err_off, err)
    assert info_tuple(ix.info) == want
    return ix


def check_decode(oracle, frame, chunk, grid):
    """index + decode against the reference's reader -> (the Index, the final info, the output).  A chunk is decoded at the capacity its
    size walk found, so a block that breaks the format's end rules at that capacity is refused although the reader, with chunk_size
    bytes of room, would take it: never the other way round, and what is accepted has the reader's bytes."""
    chunks, rets, outs, offs, want = reader(oracle, frame, chunk)
    ix = check_index(oracle, frame, chunk, grid)
    rc, info, dst = ix.decode(oracle)
    assert rc == 0
    a, caps, good = ix.frame, ix.dst_cap, []
    for k, (at, size) in enumerate(chunks):
        tight = oracle.uncompress_unknown_raw(a[at:at + size], size, int(caps[k]))[0]
        good.append(0 <= ix.result[k] == caps[k] and tight == caps[k] and (size == 0 or caps[k] > 0 or rets[k] == 0))
        if rets[k] < 0:
            assert not good[k], "accepted a chunk the reference's reader fails on"
        if good[k]:
            assert rets[k] == caps[k] and bytes(dst.a[ix.dst_off[k]:ix.dst_off[k] + caps[k]]) == outs[k], k
    bad = [k for k, g in enumerate(good) if not g]
    total = int(ix.dst_off[len(chunks)])
    if bad:
        assert info_tuple(info) == (len(chunks), total, int(ix.dst_off[bad[0]]), chunks[bad[0]][0] - 4, CORRUPT_BLOCK)
    else:
        assert info_tuple(info) == want
    return ix, info, dst


ENCODE_CASES = [(chunk, n) for chunk in (1, 17, 4096, 65536) for n in sorted({0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk, 3 * chunk + 7})]


# ---- encode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_encode_writes_the_reference_frame(oracle, grid):
    for chunk, n in ENCODE_CASES:
        data = sample(oracle, n)
        got, expect, cap = encode(oracle, data, chunk, grid=grid)
        assert got == expect == make_frame(oracle, data, chunk), (chunk, n)
        assert cap == 4 + sum(4 + bound(min(chunk, n - i)) for i in range(0, n, chunk))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("hc", [False, True])
def test_encode_single_chunk_frames_are_the_cli_s(oracle, grid, hc):
    frames = rr.load()["frames"]
    for n, dist in ((1000, 2), (70000, 2), (300000, 3)):
        rec = frames[rr.frame_key(n, dist, hc)]
        got, expect, _ = encode(oracle, rr.frame_sample(oracle, n, dist), lf.CHUNK_SIZE, hc=hc, grid=grid, chunk_arg=0)    # 0: the CLI's 8 MiB
        assert got == expect and (len(got), rr.sha(got)) == (rec["len"], rec["sha"])


@pytest.mark.parametrize("grid", GRIDS)
def test_bound_is_exact_when_no_chunk_shrinks(oracle, grid):
    """an encoder that fills every compressBound buffer to the last byte: the frame is lz4hip_frame_bound bytes, and never more"""
    for chunk, n in ((17, 0), (17, 3 * 17 + 7), (4096, 4095), (4096, 3 * 4096), (4096, 3 * 4096 + 7), (65536, 65537)):
        got, expect, cap = encode(oracle, sample(oracle, n), chunk, grid=grid, results=bound)
        assert got == expect and len(got) == cap


def test_encode_argument_checks():
    L = emu()
    text = C.create_string_buffer(200)
    buf = Guarded(4096)
    one = np.zeros(1, np.int64)
    call = lambda src_len, chunk, mode, cap, scratch_bytes: L.emu_frame_encode(buf.ptr, src_len, chunk, mode, buf.ptr, cap, one.ctypes.data, buf.ptr,    # noqa: E731
                                                                               scratch_bytes, None, None, 0, text, 200)
    assert call(-1, 0, 0, 4096, 4096) == E_ARGUMENT
    assert call(10, -1, 0, 4096, 4096) == E_ARGUMENT and call(10, 0x7E000001, 0, 4096, 4096) == E_ARGUMENT and b"chunk_size" in text.value
    assert call(10, 0, 2, 4096, 4096) == E_ARGUMENT
    assert call(10, 0, 0, L.emu_frame_bound(10, 0) - 1, 4096) == E_ARGUMENT and b"lz4hip_frame_bound" in text.value
    assert call(10, 0, 0, 4096, L.emu_frame_encode_scratch_bytes(10, 0) - 1) == E_ARGUMENT and b"scratch" in text.value
    assert L.emu_frame_bound(10, -1) == E_ARGUMENT and L.emu_frame_bound(0, 0) == 4 and L.emu_frame_bound(10, 0x7E000000) == 4 + 4 + bound(10)
    assert buf.intact()


# ---- index ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def index_frames():
    from oracle.oracle import Oracle
    oracle = Oracle()
    out = []
    for chunk, n in ((17, 3 * 17 + 7), (4096, 4095), (4096, 3 * 4096 + 7), (65536, 65537)):
        out.append((make_frame(oracle, sample(oracle, n), chunk), chunk))
    for n, dist, hc in ((1000, 2, False), (70000, 2, True), (300000, 3, False)):
        out.append((make_frame(oracle, rr.frame_sample(oracle, n, dist), lf.CHUNK_SIZE, hc), lf.CHUNK_SIZE))
    frame, chunk = out[2]
    out += [(frame + frame, chunk), (MAGIC + frame, chunk), (frame + MAGIC, chunk), (frame[:4], chunk), (frame[:4] + MAGIC + MAGIC + frame[4:], chunk)]
    return out


@pytest.mark.parametrize("grid", GRIDS)
def test_index_equals_parse_frame(oracle, grid):
    for frame, chunk in index_frames():
        ix = check_index(oracle, frame, chunk, grid)
        assert ix.info.error == OK and ix.rows() == lf.parse_frame(frame)
        raw = b"".join(reader(oracle, frame, chunk)[2])
        assert ix.info.decoded_bytes == len(raw)


@pytest.mark.parametrize("grid", GRIDS)
def test_index_of_synthetic_frames(oracle, grid):
    """200 frames of random payloads, built as test_framing_host_logic_properties builds them: the table is parse_frame's, the sizes are
    what the reference's walk gives for such bytes (mostly failures: the lowest one is the frame's outcome)"""
    rnd = random.Random(4)
    for _ in range(200):
        frame, want = MAGIC, []
        for _ in range(rnd.randint(0, 6)):
            if rnd.random() < 0.2:
                frame += MAGIC
                continue
            n = rnd.randint(0, 50)
            frame += n.to_bytes(4, "little")
            want.append((len(frame), n))
            frame += bytes(rnd.randrange(256) for _ in range(n))
        assert lf.parse_frame(frame) == want
        ix = check_index(oracle, frame, lf.CHUNK_SIZE, grid, max_chunks=len(want))
        assert ix.rows() == want


@pytest.mark.parametrize("grid", GRIDS)
def test_index_header_errors(oracle, grid):
    frame, chunk = index_frames()[2]
    for bad in (b"", MAGIC[:1], MAGIC[:2], MAGIC[:3], b"\x00\x00\x00\x00" + frame[4:], b"\x03" + frame[1:]):
        assert info_tuple(check_index(oracle, bad, chunk, grid, max_chunks=4).info) == (0, 0, 0, 0, BAD_MAGIC)
    n, total = len(lf.parse_frame(frame)), len(b"".join(reader(oracle, frame, chunk)[2]))
    for extra in (1, 2, 3):
        assert info_tuple(check_index(oracle, frame + frame[4:4 + extra], chunk, grid).info) == (n, total, total, len(frame), TRUNCATED)
    last = lf.parse_frame(frame)[-1][0] - 4
    ix = check_index(oracle, frame[:-1], chunk, grid)
    assert (ix.info.chunks, ix.info.error, ix.info.error_offset) == (n - 1, TRUNCATED, last)
    # a size field one above compressBound(chunk_size) is refused as such, inside the buffer and past its end alike: tested first
    size = (bound(chunk) + 1).to_bytes(4, "little")
    for tail in (size + bytes(bound(chunk) + 1), size + bytes(10), size):
        assert info_tuple(check_index(oracle, frame + tail, chunk, grid).info) == (n, total, total, len(frame), BAD_SIZE)
    ok = frame + bound(chunk).to_bytes(4, "little") + bytes(10)
    assert check_index(oracle, ok, chunk, grid).info.error == TRUNCATED


@pytest.mark.parametrize("grid", GRIDS)
def test_index_table_full(oracle, grid):
    frame, chunk = index_frames()[2]
    frame = frame + frame
    chunks = lf.parse_frame(frame)
    n = len(chunks)
    for m in (n - 1, 1, 0):
        ix = Index(frame, chunk, m, grid)
        assert ix.rc == 0 and (ix.info.chunks, ix.info.error, ix.info.error_offset) == (n, TABLE_FULL, chunks[m][0] - 4)
        assert ix.rows() == chunks[:m]
        rc, _, _ = ix.decode(oracle)
        assert rc == E_ARGUMENT, "the decode took the info of a full table"
        again = check_index(oracle, frame, chunk, grid, max_chunks=ix.info.chunks)
        assert again.info.error == OK
    # a full table wins over the header error behind it
    ix = Index(frame + b"\x01", chunk, n - 1, grid)
    assert (ix.info.chunks, ix.info.error) == (n, TABLE_FULL)


def test_index_and_decode_argument_checks(oracle):
    frame, chunk = index_frames()[2]
    m = len(lf.parse_frame(frame))
    assert Index(frame, chunk, -1).rc == E_ARGUMENT
    assert Index(frame, chunk, m, chunk_arg=-5).rc == E_ARGUMENT
    L, src, info, text = emu(), u8(frame), FrameInfo(), C.create_string_buffer(200)
    scratch = Guarded(L.emu_frame_decode_scratch_bytes(m))
    assert L.emu_frame_index(src.ctypes.data, src.size, chunk, m, scratch.ptr, scratch.n - 1, C.addressof(info), 0, text, 200) == E_ARGUMENT
    assert b"lz4hip_frame_decode_scratch_bytes" in text.value and scratch.intact()
    ix = check_index(oracle, frame, chunk, 0, max_chunks=m)
    dst = Guarded(ix.info.decoded_bytes)
    call = lambda host, mc, cap: L.emu_frame_decode(ix.src.ctypes.data, C.addressof(host), mc, ix.scratch.ptr, ix.scratch.n, dst.ptr, cap,    # noqa: E731
                                                    C.addressof(info), None, None, 0, text, 200)
    host = FrameInfo.from_buffer_copy(bytes(ix.info))
    assert call(host, m, ix.info.decoded_bytes - 1) == E_ARGUMENT and b"dst_cap" in text.value
    assert call(host, m - 1, ix.info.decoded_bytes) == E_ARGUMENT
    host.error = TABLE_FULL
    assert call(host, m, ix.info.decoded_bytes) == E_ARGUMENT
    host.error, host.chunks = OK, -1
    assert call(host, m, ix.info.decoded_bytes) == E_ARGUMENT
    assert dst.intact() and (dst.a == GUARD).all()


# ---- decode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_round_trips(oracle, grid):
    for chunk, n in ENCODE_CASES:
        data = sample(oracle, n)
        ix, info, dst = check_decode(oracle, make_frame(oracle, data, chunk), chunk, grid)
        assert info_tuple(info) == ((n + chunk - 1) // chunk, n, n, -1, OK) and bytes(dst.a) == data
    for frame, chunk in index_frames():
        ix, info, dst = check_decode(oracle, frame, chunk, grid)
        assert info.error == OK and bytes(dst.a) == b"".join(reader(oracle, frame, chunk)[2])
    # an empty chunk decodes to nothing, as it does in the reference (LZ4_uncompress_unknownOutputSize with isize = 0 returns 0)
    assert oracle.uncompress_unknown_raw(np.zeros(0, np.uint8), 0, 4096)[0] == 0
    frame, chunk = index_frames()[1]
    ix, info, dst = check_decode(oracle, frame[:4] + bytes(4) + frame[4:] + bytes(4), chunk, grid)
    assert (info.chunks, info.error, info.decoded_bytes) == (3, OK, 4095)
    ix, info, dst = check_decode(oracle, MAGIC + bytes(8), chunk, grid)
    assert info_tuple(info) == (2, 0, 0, -1, OK)


CHUNK9 = 4096
END_RULE_BLOCK = bytes([0x10, 0x30, 1, 0, 0x50, 1, 2, 3, 4, 5])     # walks to 10 bytes; its match ends inside the last 5: the decoder refuses it


def nine_chunks(oracle, replace):
    """a frame of 9 chunks of CHUNK9 bytes with the payloads of `replace` = {chunk index: payload} swapped in -> (frame, the nine sources)"""
    data = u8(sample(oracle, 9 * CHUNK9))
    raws = [data[k * CHUNK9:(k + 1) * CHUNK9] for k in range(9)]
    comps = [bytes(oracle.compress(r)) for r in raws]
    for k, payload in replace.items():
        comps[k] = bytes(payload)
    return MAGIC + b"".join(len(c).to_bytes(4, "little") + c for c in comps), raws, comps


def bad_payloads(oracle):
    data = u8(sample(oracle, 9 * CHUNK9))
    good = bytes(oracle.compress(data[4 * CHUNK9:5 * CHUNK9]))
    walk_fails = b"\xFF\xFF\xFF" + good[3:]
    too_long = bytes(oracle.compress(data[4 * CHUNK9:5 * CHUNK9 + 1]))
    sizes = sh.reference_sizes([u8(walk_fails), u8(too_long), u8(END_RULE_BLOCK)])
    assert sizes[0] < 0 and sizes[1] == CHUNK9 + 1 and sizes[2] == 10
    assert oracle.uncompress_unknown_raw(u8(END_RULE_BLOCK), len(END_RULE_BLOCK), 10)[0] < 0
    return {"walk": walk_fails, "long": too_long, "end": END_RULE_BLOCK}


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("kind", ["walk", "long", "end"])
def test_one_bad_chunk_among_nine(oracle, grid, kind):
    frame, raws, comps = nine_chunks(oracle, {4: bad_payloads(oracle)[kind]})
    field = 4 + sum(4 + len(c) for c in comps[:4])
    ix, info, dst = check_decode(oracle, frame, CHUNK9, grid)
    slot = 10 if kind == "end" else 0                                   # (what the size walk gave the chunk; the decoder alone fails it)
    assert ix.info.error == (OK if kind == "end" else CORRUPT_BLOCK)
    assert info_tuple(info) == (9, 8 * CHUNK9 + slot, 4 * CHUNK9, field, CORRUPT_BLOCK)
    assert info.good_bytes == ix.dst_off[4]
    for k in range(9):
        if k != 4:
            assert ix.dst_off[k] == (k * CHUNK9 if k < 4 else (k - 1) * CHUNK9 + slot)
            assert bytes(dst.a[ix.dst_off[k]:ix.dst_off[k] + CHUNK9]) == bytes(raws[k]), k


@pytest.mark.parametrize("grid", GRIDS)
def test_the_lowest_bad_chunk_wins(oracle, grid):
    bad = bad_payloads(oracle)
    for first, second in (("walk", "end"), ("end", "long"), ("long", "walk")):
        frame, raws, comps = nine_chunks(oracle, {6: bad[second], 2: bad[first]})
        ix, info, dst = check_decode(oracle, frame, CHUNK9, grid)
        assert (info.error, info.error_offset, info.good_bytes) == (CORRUPT_BLOCK, 4 + sum(4 + len(c) for c in comps[:2]), 2 * CHUNK9)
        # a bad chunk followed by a truncated tail is still a corrupt block: it comes first
        for tail in (b"\x01\x02", (50).to_bytes(4, "little") + bytes(49)):
            ix, info, dst = check_decode(oracle, frame + tail, CHUNK9, grid)
            assert ix.info.error in (CORRUPT_BLOCK, TRUNCATED)
            assert (info.chunks, info.error, info.good_bytes) == (9, CORRUPT_BLOCK, 2 * CHUNK9)


def test_sequences_alone_over_a_table_of_the_test_s(oracle):
    """frame_index_run / frame_decode_run entered below their fronts, on a table laid out by emu_frame_tables"""
    frame, chunk = index_frames()[2]
    chunks, rets, outs, offs, want = reader(oracle, frame, chunk)
    L, src, m = emu(), u8(frame), len(chunks) + 2
    scratch = Guarded(L.emu_frame_decode_scratch_bytes(m))
    t, info, final = FrameTables(), FrameInfo(), FrameInfo()
    L.emu_frame_tables(scratch.ptr, m, C.addressof(t))
    assert L.emu_frame_index_run(src.ctypes.data, src.size, chunk, C.addressof(t), C.addressof(info), 3) == 0
    assert info_tuple(info) == want
    decoded = u8(b"".join(outs))
    dst = Guarded(len(decoded))
    res = np.array(rets + [0], np.int32)
    assert L.emu_frame_decode_run(src.ctypes.data, C.addressof(info), C.addressof(t), dst.ptr, C.addressof(final), res.ctypes.data,
                                  decoded.ctypes.data, 3) == 0
    assert info_tuple(final) == want and bytes(dst.a) == bytes(decoded) and dst.intact() and scratch.intact()


# ---- the host-pointer calls -----------------------------------------------------------------------------------------------------
def host_run(grid, results=None, data=None):
    run = sh.EmuHostRun()
    run.grid_items = grid
    run.results = None if results is None else results.ctypes.data
    run.bytes = None if data is None else data.ctypes.data
    return run


@pytest.mark.parametrize("grid", GRIDS)
def test_host_encode(oracle, grid):
    for chunk, n in ((4096, 0), (4096, 3 * 4096 + 7), (17, 17 * 3), (65536, 65537)):
        data = u8(sample(oracle, n))
        count = (n + chunk - 1) // chunk
        stride = bound(min(chunk, n))
        comp, res = np.zeros(count * stride + 1, np.uint8), np.zeros(count + 1, np.int32)
        for k in range(count):
            c = oracle.compress(data[k * chunk:(k + 1) * chunk])
            res[k] = len(c)
            comp[k * stride:k * stride + len(c)] = c
        # the stand-in hands out bytes at the encoder's own output offsets: those of the image's scratch piece are k * stride as well
        run = host_run(grid, res, comp)
        cap = emu().emu_frame_bound(n, chunk)
        dst = Guarded(cap)
        dst_len = C.c_int64(-1)
        rc = emu().emu_host_frame_encode(data.ctypes.data, n, chunk, 0, dst.ptr, cap, C.addressof(dst_len), C.addressof(run))
        assert rc == 0, run.error
        want = make_frame(oracle, data, chunk)
        assert dst_len.value == len(want) and bytes(dst.a[:len(want)]) == want and (dst.a[len(want):] == GUARD).all()
        assert run.intact and dst.intact() and run.reserves == 1
        assert emu().emu_host_frame_encode(data.ctypes.data, n, chunk, 0, dst.ptr, cap - 1, C.addressof(dst_len), C.addressof(run)) == E_ARGUMENT


def host_decode(oracle, frame, chunk, grid, dst_cap=None):
    """frame_decode_host with the oracle's bytes for the decoder -> (rc, info, dst, run); the stand-in's bytes are laid out at the
    offsets the reference's sizes give, which are the table's"""
    chunks, rets, outs, offs, want = reader(oracle, frame, chunk)
    a = u8(frame)
    sizes = sh.reference_sizes([a[at:at + size] for at, size in chunks])
    caps = [int(r) if 0 <= r <= chunk else 0 for r in sizes]
    at = np.concatenate(([0], np.cumsum(caps, dtype=np.int64))).astype(np.int64)
    decoded = np.full(int(at[-1]) + 1, 0x33, np.uint8)
    res = np.zeros(len(chunks) + 1, np.int32)
    for k, (p, size) in enumerate(chunks):
        r, out = oracle.uncompress_unknown_raw(a[p:p + size], size, caps[k])
        res[k] = r
        decoded[at[k]:at[k] + caps[k]] = out[:caps[k]]
    run = host_run(grid, res, decoded)
    cap = int(at[-1]) if dst_cap is None else dst_cap
    dst = Guarded(cap)
    info = FrameInfo(-7, -7, -7, -7, -7, -7)
    rc = emu().emu_host_frame_decode(a.ctypes.data if a.size else None, a.size, chunk, dst.ptr, cap, C.addressof(info), C.addressof(run))
    assert run.intact and dst.intact(), "the image or the caller's buffer was written outside its bytes"
    return rc, info, dst, run, want


@pytest.mark.parametrize("grid", GRIDS)
def test_host_decode(oracle, grid):
    for frame, chunk in index_frames()[:3] + index_frames()[7:]:
        rc, info, dst, run, want = host_decode(oracle, frame, chunk, grid)
        assert rc == OK and info_tuple(info) == want and bytes(dst.a) == b"".join(reader(oracle, frame, chunk)[2])
        assert run.passes == 1 and run.reserves == 1
        # the size query: no output, the info filled, nothing written
        rc, info, dst, run, want = host_decode(oracle, frame, chunk, grid, dst_cap=0)
        if want[1] > 0:
            assert rc == E_ARGUMENT and b"decoded_bytes" in run.error
        assert info_tuple(info) == want and run.passes == 1
    # errors come back as the return value, with the chunks before them decoded
    bad = bad_payloads(oracle)
    frame, raws, comps = nine_chunks(oracle, {4: bad["walk"]})
    rc, info, dst, run, want = host_decode(oracle, frame + b"\x01", CHUNK9, grid)
    assert rc == CORRUPT_BLOCK and info_tuple(info) == want and bytes(dst.a) == b"".join(bytes(r) for k, r in enumerate(raws) if k != 4)
    rc, info, dst, run, want = host_decode(oracle, frame[:4] + frame[4:8] * 2, CHUNK9, grid)
    assert rc == TRUNCATED and info_tuple(info) == (0, 0, 0, 4, TRUNCATED)
    rc, info, dst, run, want = host_decode(oracle, b"abcd", CHUNK9, grid)
    assert rc == BAD_MAGIC


@pytest.mark.parametrize("grid", GRIDS)
def test_host_decode_indexes_again_for_a_larger_table(oracle, grid):
    """40 chunks of 17 bytes read with a chunk_size of 4096: the first table (src_len / chunk_size + 16 rows) is too small, the image moves,
    the source is staged again and the second walk fills a table of the count the first one reported"""
    data = sample(oracle, 40 * 17)
    frame = make_frame(oracle, data, 17)
    assert len(frame) // 4096 + 16 < 40
    rc, info, dst, run, want = host_decode(oracle, frame, 4096, grid)
    assert rc == OK and info_tuple(info) == want == (40, len(data), len(data), -1, OK) and bytes(dst.a) == data
    assert run.passes == 2 and run.moves == 2 and run.uploads == 2
    # highly compressible: more than the 4 * src_len the image first holds, so one more pass at exactly the decoded size
    zeros = bytes(100000)
    frame = make_frame(oracle, zeros, 65536)
    rc, info, dst, run, want = host_decode(oracle, frame, 65536, grid)
    assert rc == OK and bytes(dst.a) == zeros and run.passes == 2


# ---- the library itself, device or none -------------------------------------------------------------------------------------------
def test_library_checks_arguments_before_it_looks_for_a_device():
    """the C entry points refuse bad arguments with LZ4HIP_E_ARGUMENT on any machine; a good call without a device is LZ4HIP_E_DEVICE"""
    from lz4net_amd import _lib
    L = _lib.lib()
    assert L.lz4hip_frame_bound(0, 0) == 4 and L.lz4hip_frame_bound(100, 0) == 4 + 4 + bound(100)
    assert L.lz4hip_frame_bound(3 * 4096 + 7, 4096) == 4 + 3 * (4 + bound(4096)) + 4 + bound(7)
    assert L.lz4hip_frame_bound(10, -1) == E_ARGUMENT and L.lz4hip_frame_bound(10, 0x7E000001) == E_ARGUMENT
    assert L.lz4hip_frame_encode_scratch_bytes(10, -1) == E_ARGUMENT
    assert L.lz4hip_frame_encode_scratch_bytes(0, 0) == emu().emu_frame_encode_scratch_bytes(0, 0) > 0
    assert L.lz4hip_frame_encode_scratch_bytes(3 * 4096 + 7, 4096) == emu().emu_frame_encode_scratch_bytes(3 * 4096 + 7, 4096)
    assert L.lz4hip_frame_decode_scratch_bytes(37) == emu().emu_frame_decode_scratch_bytes(37)
    buf = np.zeros(4096, np.uint8)
    p, info = buf.ctypes.data, FrameInfo()
    assert L.lz4hip_frame_encode_device(p, -1, 0, 0, p, 4096, p, p, 4096, None) == E_ARGUMENT
    assert L.lz4hip_frame_encode_device(p, 10, 0, 0, p, 3, p, p, 4096, None) == E_ARGUMENT and b"lz4hip_frame_bound" in L.lz4hip_last_error()
    assert L.lz4hip_frame_index_device(p, 10, 0, -1, p, 4096, p, None) == E_ARGUMENT
    assert L.lz4hip_frame_index_device(p, 10, 0x7E000001, 1, p, 4096, p, None) == E_ARGUMENT
    assert L.lz4hip_frame_decode_device(p, None, 1, p, 4096, p, 4096, p, None) == E_ARGUMENT
    info.error = TABLE_FULL
    assert L.lz4hip_frame_decode_device(p, C.byref(info), 1, p, 4096, p, 4096, p, None) == E_ARGUMENT
    if L.lz4hip_device_count() == 0:
        assert L.lz4hip_frame_encode_device(p, 10, 0, 0, p, 4096, p, p, 4096, None) == _lib.E_DEVICE
        one = C.c_int64(0)
        assert L.lz4hip_frame_encode_host(p, 10, 0, 0, p, 4096, C.byref(one)) == _lib.E_DEVICE
