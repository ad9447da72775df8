"""ctypes front-end for tests/simt/libsimt_kernels.so and the LZ4Stream / Wrap entry points of tests/simt/libsimt_framing.so (TEST
INFRASTRUCTURE): runs the real kernel sources under the CPU SIMT emulator.  Same call shapes as the GPU batch API so tests can share code."""
import ctypes as C

import numpy as np

import emu_lib
from emu_lib import I32 as _I32, I64 as _I64, P as _P, U32 as _U32

_use_starved = False


def lib():
    return emu_lib.kernels(_use_starved)


class starved_flush:
    """with emu.starved_flush(): ...  -- run the kernels of the 'starved' build (4 flush records per round)."""

    def __enter__(self):
        global _use_starved
        _use_starved = True

    def __exit__(self, *a):
        global _use_starved
        _use_starved = False
        return False


def _p(a):
    return C.c_void_p(a.ctypes.data)


def pack(rows, pad=16):
    n = len(rows)
    stride = max([len(r) for r in rows] + [1]) + pad
    buf = np.zeros((n, stride), np.uint8)
    for i, r in enumerate(rows):
        buf[i, :len(r)] = r
    return buf, np.array([len(r) for r in rows], np.int32)


def decode(comps, out_sizes, known=True, src_lens=None, waves_per_group=1, auto=False, lane=0, stage=64, gen=2):
    src, sl = pack(comps)
    if src_lens is not None:
        sl = np.array(src_lens, np.int32)
    caps = np.array(out_sizes, np.int32)
    ds = max(int(caps.max()), 1) + 64
    dst = np.full((len(comps), ds), 0xA5, np.uint8)
    res = np.full(len(comps), -12345678, np.int32)
    args = (int(known), _p(src), C.c_int64(src.shape[1]), _p(sl), _p(dst), C.c_int64(ds), _p(caps), _p(res), C.c_int64(len(comps)))
    if lane and gen == 6:                       # generation 4 in workgroups of four wavefronts (lane = 1: dual ring stores, 2: wrapped rows)
        lib().emu_decode_lane4_wg4(*args, 0, int(lane == 2))
    elif lane and gen == 5:                     # the persistent variant of generation 4: `lane` wavefronts in the grid
        lib().emu_decode_lane4_persistent(*args, 0, lane)
    elif lane and gen == 4:
        lib().emu_decode_lane4(*args, 0, lane)
    elif lane and gen == 3:
        lib().emu_decode_lane3(*args, 0, lane, stage)
    elif lane:
        lib().emu_decode_lane(*args, 0, lane, stage)
    elif auto:        # the library's default: the batch is partitioned between the two mappings
        lib().emu_decode_lane4(*args, 2, 59192)
        lib().emu_decode(*args, waves_per_group, 1)
    else:
        lib().emu_decode(*args, waves_per_group, 0)
    return res, dst


def encode(blocks, caps=None, hc=False, groups=2, lane=False, conv=False, nat=False, lcp=False, wg5=False, pad=16):
    """pad=0: a row of the greatest length ends directly in front of the next row's first byte"""
    src, sl = pack(blocks, pad=pad)
    if caps is None:
        caps = [len(b) + len(b) // 255 + 16 for b in blocks]
    caps = np.array(caps, np.int32)
    ds = max(int(caps.max()), 1) + 64
    dst = np.full((len(blocks), ds), 0xA5, np.uint8)
    res = np.zeros(len(blocks), np.int32)
    args = (_p(src), C.c_int64(src.shape[1]), _p(sl), _p(dst), C.c_int64(ds), _p(caps), _p(res), C.c_int64(len(blocks)))
    if hc and lcp:
        lib().emu_encode_hc_lcp(*args, groups)
    elif hc and nat:
        lib().emu_encode_hc_nat(*args, groups)
    elif hc and conv:
        lib().emu_encode_hc_conv(*args, 1, int(max(len(b) for b in blocks) > 65536))
    elif hc and lane:
        lib().emu_encode_hc_lane(*args, 1, int(max(len(b) for b in blocks) > 65536))
    elif hc:
        lib().emu_encode_hc(*args, groups, int(max(len(b) for b in blocks) > 65536))
    elif lane:
        lib().emu_encode_fast_lane(*args, 1)
    elif wg5:
        lib().emu_encode_fast_wg5(*args)
    else:
        lib().emu_encode_fast(*args)
    return res, dst


def hc_stats(reset=True):
    """lz4hip::HcStat: the branch counters of the LZ4HC lane kernels and their table builders since the last reset"""
    st = (C.c_ulonglong * 96)()
    n = lib().emu_hc_stats(st, int(reset))
    return [int(x) for x in st[:n]]


def enc_stats(reset=True, library=None):
    """lz4hip::EncStat: the branch counters of the wavefront fast encoder since the last reset (library: another build of emu_kernels.cpp)"""
    st = (C.c_ulonglong * 64)()
    n = (library or lib()).emu_enc_stats(st, int(reset))
    return [int(x) for x in st[:n]]


def lane_enc_stats(reset=True):
    """lz4hip::LaneEncStat: the branch counters of the fast lane encoder since the last reset"""
    st = (C.c_ulonglong * 96)()
    n = lib().emu_lane_enc_stats(st, int(reset))
    return [int(x) for x in st[:n]]


class descending_lanes:
    """with emu.descending_lanes(): the scheduler runs the live lanes of a wavefront from the highest down between two rendezvous, so of
    several stores to one address the LOWEST lane's lands last (tests/simt/simt.hpp)"""

    def __init__(self, library=None):
        self.lib = library

    def __enter__(self):
        (self.lib or lib()).emu_lane_order(1)

    def __exit__(self, *a):
        (self.lib or lib()).emu_lane_order(0)
        return False


def hc_lcp_tables(blocks):
    """(len(blocks), 65536) uint32: the tables hc_nat_chain_kernel<uint32_t> and hc_lcp_fill_kernel leave of poisoned memory"""
    src, sl = pack(blocks)
    tables = np.zeros((len(blocks), 65536), np.uint32)
    lib().emu_hc_lcp_tables(_p(src), C.c_int64(src.shape[1]), _p(sl), C.c_int64(len(blocks)), _p(tables))
    return tables


def encode_hc_lane_static(blocks):
    """LZ4HC lane kernel's per-block function with STATIC assignment: lane L encodes blocks L, L+64, L+128, ... in order on
    one slab (slab-reuse test)."""
    src, sl = pack(blocks)
    caps = np.array([len(b) + len(b) // 255 + 16 for b in blocks], np.int32)
    ds = max(int(caps.max()), 1) + 64
    dst = np.full((len(blocks), ds), 0xA5, np.uint8)
    res = np.zeros(len(blocks), np.int32)
    lib().emu_encode_hc_lane_static(_p(src), C.c_int64(src.shape[1]), _p(sl), _p(dst), C.c_int64(ds), _p(caps), _p(res), C.c_int64(len(blocks)))
    return res, dst


def encode_two_launches(blocks, caps=None):
    """launch_encode's default for large batches: wavefront-per-block launch with the hand-over rule, then the lane-per-block
    launch over the blocks handed over.  Returns (result, dst, deferred flags)."""
    src, sl = pack(blocks)
    if caps is None:
        caps = [len(b) + len(b) // 255 + 16 for b in blocks]
    caps = np.array(caps, np.int32)
    ds = max(int(caps.max()), 1) + 64
    dst = np.full((len(blocks), ds), 0xA5, np.uint8)
    res = np.zeros(len(blocks), np.int32)
    deferred = np.zeros(len(blocks), np.int32)
    lib().emu_encode_fast_two_launches(_p(src), C.c_int64(src.shape[1]), _p(sl), _p(dst), C.c_int64(ds), _p(caps), _p(res),
                                       C.c_int64(len(blocks)), _p(deferred))
    return res, dst, deferred


def synth(dist, seed, first_block, n, length, stride=None, block_step=1):
    stride = length if stride is None else stride
    out = np.zeros((n, max(stride, 1)), np.uint8)
    lib().emu_synth(dist, C.c_uint64(seed), C.c_uint64(first_block), C.c_uint64(block_step), C.c_int64(n), _p(out), C.c_int64(out.shape[1]), length)
    return out


def checksum(rows):
    buf, ln = pack(rows, pad=0)
    sums = np.zeros(len(rows), np.uint64)
    lib().emu_checksum(_p(buf), C.c_int64(buf.shape[1]), _p(ln), _p(sums), C.c_int64(len(rows)))
    return sums


def compare(a, b, lens):
    lens = np.array(lens, np.int32)
    return lib().emu_compare(_p(a), C.c_int64(a.shape[1]), _p(b), C.c_int64(b.shape[1]), _p(lens), C.c_int64(a.shape[0]))


# ---- framing kernels (tests/simt/emu_stream.inc): ctypes twins of the kernels' argument structs --------------------------------------
class StreamEncodeArgs(C.Structure):
    _fields_ = [("src", _P), ("comp", _P), ("src_len", _I64), ("n", _I64), ("block", _I32), ("hc_flag", _U32), ("result", _P), ("offs", _P)]


class StreamTables(C.Structure):
    _fields_ = [("max_chunks", _I64), ("c_src_off", _P), ("c_dst_off", _P), ("c_hdr_off", _P), ("c_src_len", _P), ("c_dst_cap", _P),
                ("c_result", _P), ("r_dst_off", _P), ("r_src_off", _P), ("r_len", _P), ("min_bad", _P)]


class StreamInfo(C.Structure):
    _fields_ = [("chunks", _I64), ("compressed_chunks", _I64), ("decoded_bytes", _I64), ("error_offset", _I64), ("error", _I32), ("reserved", _I32)]


class WrapArgs(C.Structure):
    _fields_ = [("src", _P), ("comp", _P), ("off", _P), ("src_len", _I64), ("n", _I64), ("enc", _P), ("dst_off", _P)]


class UnwrapTables(C.Structure):
    _fields_ = [("n", _I64), ("min_bad", _P), ("ncomp", _P), ("cidx", _P), ("partial", _P), ("c_src_off", _P), ("c_dst_off", _P), ("c_msg", _P),
                ("c_src_len", _P), ("c_dst_cap", _P), ("c_result", _P), ("raw_len", _P)]


class UnwrapArgs(C.Structure):
    _fields_ = [("src", _P), ("off", _P), ("src_len", _I64), ("n", _I64), ("dst_off", _P), ("status", _P)]


class UnwrapInfo(C.Structure):
    _fields_ = [("messages", _I64), ("compressed", _I64), ("decoded_bytes", _I64), ("first_error", _I64), ("error", _I32), ("reserved", _I32)]


class StreamsEncodeArgs(C.Structure):
    _fields_ = [("src", _P), ("comp", _P), ("off", _P), ("src_len", _I64), ("n", _I64), ("cap", _I64), ("block", _I32), ("hc_flag", _U32),
                ("first", _P), ("total", _P), ("c_at", _P), ("c_len", _P), ("result", _P), ("offs", _P)]


class StreamsTables(C.Structure):
    _fields_ = [("t", StreamTables), ("totals", _P), ("chunk_base", _P), ("comp_base", _P), ("item_bad", _P), ("partial", _P), ("c_item", _P)]


class StreamsDecodeArgs(C.Structure):
    _fields_ = [("src", _P), ("off", _P), ("src_len", _I64), ("n", _I64), ("dst_off", _P), ("status", _P), ("error_offset", _P)]


class StreamsInfo(C.Structure):
    _fields_ = [("items", _I64), ("chunks", _I64), ("compressed_chunks", _I64), ("decoded_bytes", _I64), ("first_error", _I64),
                ("error_offset", _I64), ("error", _I32), ("reserved", _I32)]


HostRun = emu_lib.EmuHostRun

_FRAMING_STRUCTS = [StreamEncodeArgs, StreamTables, StreamInfo, WrapArgs, UnwrapTables, UnwrapArgs, UnwrapInfo, StreamsEncodeArgs,
                    StreamsTables, StreamsDecodeArgs, StreamsInfo, HostRun]
_framing = None


def framing():
    """The library with the framing entry points typed; checks once that the ctypes twins above have the kernels' struct sizes."""
    global _framing
    if _framing is None:
        L = emu_lib.framing()
        for i, s in enumerate(_FRAMING_STRUCTS):
            assert L.emu_framing_sizeof(i) == C.sizeof(s), (s.__name__, L.emu_framing_sizeof(i), C.sizeof(s))
        for name, args in {
            "emu_scan": [_P, _I64, _P, _P],
            "emu_stream_index": [_P, _I64, _P, _P],
            "emu_copy_encode": [_P, _P, _P, _I32],
            "emu_copy_raw": [_P, _P, _I64, _P, _I64, _I32],
            "emu_copy_wrap": [_P, _P, _I64, _I32],
            "emu_copy_unwrap_raw": [_P, _P, _P, _I64, _I32],
            "emu_copy_streams": [_P, _P, _I64, _I32],
            "emu_streams_walk": [_I32, _P, _P, _I32],
            "emu_stream_check": [_P, _I64, _I32],
            "emu_stream_encode": [_P, _P, _P, _P, _P, _I64, _I32, _I32],
            "emu_stream_decode": [_P, _I64, _P, _P, _P, _P, _P, _P, _I32, _I32],
            "emu_wrap": [_P, _P, _P, _P, _P, _P, _I64, _I64, _I32, _I32],
            "emu_unwrap_index": [_P, _P, _P, _I32],
            "emu_unwrap_decode": [_P, _P, _P, _P, _P, _P, _P, _I32, _I32],
            "emu_streams_plan": [_P, _P, _I32],
            "emu_streams_pack": [_P, _P, _P, _P, _I64, _I64, _I32, _I32],
            "emu_streams_index": [_P, _P, _P, _I32],
            "emu_streams_decode": [_P, _P, _P, _P, _P, _P, _P, _I32, _I32],
            # the whole functions of lz4hip_framing.hpp: the library's arguments, then the codec's stand-in (results, bytes) and the grids
            "emu_lib_stream_encode": [_P, _I64, _I32, _I32, _P, _I64, _P, _P, _I64, _P, _P, _I32, _I32],
            "emu_lib_stream_index": [_P, _I64, _I64, _P, _I64, _P],
            "emu_lib_stream_decode": [_P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _I32, _I32],
            "emu_lib_wrap": [_P, _I64, _P, _I64, _I32, _P, _I64, _P, _P, _P, _I64, _P, _P, _I32, _I32],
            "emu_lib_unwrap_index": [_P, _I64, _P, _I64, _P, _P, _P, _I64, _P, _I32],
            "emu_lib_unwrap_decode": [_P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _I32, _I32],
            "emu_lib_streams_encode": [_P, _I64, _P, _I64, _I32, _I32, _P, _I64, _P, _P, _I64, _P, _P, _I32, _I32],
            "emu_lib_streams_index": [_P, _I64, _P, _I64, _I64, _P, _P, _P, _P, _I64, _P, _I32],
            "emu_lib_streams_decode": [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _I32, _I32],
            # the host-pointer calls: the library's arguments, then a HostRun
            "emu_host_stream_encode": [_P, _I64, _I32, _I32, _P, _I64, _P, _P],
            "emu_host_stream_decode": [_P, _I64, _P, _I64, _P, _P],
            "emu_host_wrap": [_P, _I64, _P, _I64, _I32, _P, _I64, _P, _P, _P],
            "emu_host_unwrap": [_P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P],
            "emu_host_streams_encode": [_P, _I64, _P, _I64, _I32, _I32, _P, _I64, _P, _P],
            "emu_host_streams_decode": [_P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _P],
        }.items():
            getattr(L, name).argtypes = args
            getattr(L, name).restype = C.c_int if name in ("emu_stream_decode", "emu_streams_decode") or name.startswith(("emu_lib_", "emu_host_")) else None
        L.emu_scratch_bytes.argtypes = [_I32, _I64, _I64, _I64]
        L.emu_scratch_bytes.restype = C.c_int64
        for name in ("emu_items_grid", "emu_copy_grid", "emu_walk_grid"):
            getattr(L, name).argtypes = [_I64]
            getattr(L, name).restype = C.c_int
        _framing = L
    return _framing


def scan_tile():
    return int(framing().emu_framing_sizeof(100))


def copy_span():
    return int(framing().emu_framing_sizeof(101))


def addr(a, offset=0):
    """Address of element `offset` of a numpy array (the arrays must outlive the call they are passed to)."""
    return a.ctypes.data + offset * a.itemsize


def ref(s):
    return C.addressof(s)


def stream_tables(max_chunks, guard=4, fill=-77):
    """StreamTables over fresh arrays of max_chunks + guard entries each, pre-filled; returns (struct, dict of the arrays)."""
    m = max_chunks + guard
    arrays = {k: np.full(m, fill, np.int64) for k in ("c_src_off", "c_dst_off", "c_hdr_off", "r_dst_off", "r_src_off")}
    arrays.update({k: np.full(m, fill, np.int32) for k in ("c_src_len", "c_dst_cap", "c_result", "r_len")})
    arrays["min_bad"] = np.full(1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    t = StreamTables(max_chunks=max_chunks, **{k: addr(v) for k, v in arrays.items()})
    return t, arrays


# ---- the host-pointer block batch calls (tests/simt/emu_hostbatch.hpp over lz4net_amd/csrc/lz4hip_hostbatch.hpp) -------------------------
class HostBatch(C.Structure):
    """EmuHostBatch: what an emu_host_batch call is to do (the block codec's stand-in, the knobs and limits, EmuStage's behaviour) and
    what the stage saw (its log of 8-word records, the rows as the kernels found them staged, counters, violations, guard bytes)"""
    _fields_ = [("results", _P), ("bytes", _P), ("bytes_stride", _I64), ("row0", _I64), ("decoder", _I32), ("fail_at", _I32), ("lag", _I32),
                ("slices_knob", _I32), ("dst_len_is_result", _I32), ("pad", _I32), ("slice_hint", _I64), ("slice_floor", _I64),
                ("slice_ceiling", _I64), ("hinted_ceiling", _I64), ("pool_floor", _I64), ("seen_src", _P), ("seen_stride", _I64),
                ("seen_len", _P), ("seen_cap", _P), ("log", _P), ("log_cap", _I64), ("log_n", _I64), ("rows_seen", _I64),
                ("kernel_calls", _I64), ("quiesces", _I64), ("reserves", _I64), ("violations", _I32), ("intact", _I32), ("error", C.c_char * 160)]


_hostbatch = None


def hostbatch():
    """The library with the emu_host_* entry points typed."""
    global _hostbatch
    if _hostbatch is None:
        L = lib()
        L.emu_hostbatch_sizeof.restype = C.c_int64
        assert L.emu_hostbatch_sizeof() == C.sizeof(HostBatch), (L.emu_hostbatch_sizeof(), C.sizeof(HostBatch))
        L.emu_host_rule.argtypes, L.emu_host_rule.restype = [_I32, _I64, _I64, _I64], C.c_int64
        L.emu_host_plan.argtypes, L.emu_host_plan.restype = [_P, _I32, _I64, _P, _P, _P], C.c_int
        L.emu_host_batch.argtypes, L.emu_host_batch.restype = [_P, _P], C.c_int
        L.emu_host_shards.argtypes, L.emu_host_shards.restype = [_P, _I32, _P, C.c_uint, _P, _P, _P], C.c_int
        _hostbatch = L
    return _hostbatch
