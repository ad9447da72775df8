// emu_framing.hpp -- TEST INFRASTRUCTURE ONLY, included by emu_kernels.cpp.
// C entry points that run the framing kernels (lz4hip_stream.hpp, lz4hip_wrap.hpp, lz4hip_streams.hpp) under the SIMT emulator
// for tests/test_simt_framing.py: single kernels, and the kernel sequences of lz4hip_api.hip with the block codec step replaced
// by arrays the test hands in.  The argument structs are passed by pointer; tests/emu_helpers.py mirrors them with ctypes and
// checks the sizes against emu_framing_sizeof().  A grid argument of 0 means "the product's formula".
#pragma once

namespace emu_framing {

using namespace lz4hip;

constexpr size_t kScanLds = kStreamThreads * 8;
constexpr unsigned kStreamMaxGroups = 8192;        // lz4hip_api.hip: "constexpr unsigned kStreamMaxGroups = 8192;"

// lz4hip_api.hip, stream_grid(): "const int64_t g = (items + kStreamThreads - 1) / kStreamThreads;
//                                 return g < 1 ? 1u : (g > kStreamMaxGroups ? kStreamMaxGroups : (unsigned)g);"
static unsigned items_grid(int64_t items, int grid)
{
    if (grid > 0) return (unsigned)grid;
    const int64_t g = (items + kStreamThreads - 1) / kStreamThreads;
    return g < 1 ? 1u : (g > kStreamMaxGroups ? kStreamMaxGroups : (unsigned)g);
}

// lz4hip_api.hip, copy_grid(): "const int64_t g = (bytes + kCopySpan - 1) / kCopySpan;
//                               return g < 1 ? 1u : (g > kStreamMaxGroups ? kStreamMaxGroups : (unsigned)g);"
// `bytes` is what the product passes there: the bound for the packs, decoded_bytes for the raw copies.
static unsigned copy_grid(int64_t bytes, int grid)
{
    if (grid > 0) return (unsigned)grid;
    const int64_t g = (bytes + kCopySpan - 1) / kCopySpan;
    return g < 1 ? 1u : (g > kStreamMaxGroups ? kStreamMaxGroups : (unsigned)g);
}

// lz4hip_api.hip, streams_index(): "const unsigned walkers = n < (int64_t)kStreamsMaxWalkGroups ? (unsigned)n : kStreamsMaxWalkGroups;"
// with "constexpr unsigned kStreamsMaxWalkGroups = 1u << 22;"
static unsigned walk_grid(int64_t n, int grid)
{
    if (grid > 0) return (unsigned)grid;
    return n < (int64_t)(1u << 22) ? (unsigned)n : (1u << 22);
}

// lz4hip_api.hip, launch_scan(): the three kernels, "dim3((unsigned)tiles)" / "dim3(1)" / "dim3((unsigned)tiles)".  Reduce and apply
// index their tile by blockIdx.x (no grid-stride loop), so the scan has no grid parameter.
static void scan(int64_t* x, int64_t n, int64_t* partial, int64_t* total)
{
    const int64_t tiles = (n + kScanTile - 1) / kScanTile;
    simt::launch(dim3((unsigned)tiles), dim3(kStreamThreads), kScanLds, [=] { stream_scan_reduce_kernel(x, n, partial); });
    simt::launch(dim3(1), dim3(kStreamThreads), kScanLds, [=] { stream_scan_partials_kernel(partial, tiles, total); });
    simt::launch(dim3((unsigned)tiles), dim3(kStreamThreads), kScanLds, [=] { stream_scan_apply_kernel(x, n, partial); });
}

// the block decoder's stand-in: row j of the compressed table gets the caller's result and the caller's bytes
static void fake_decode(const StreamTables& t, int64_t ncomp, const int32_t* results, const uint8_t* decoded, uint8_t* dst)
{
    for (int64_t j = 0; j < ncomp; j++) {
        t.c_result[j] = results[j];
        if (t.c_dst_cap[j] > 0) memcpy(dst + t.c_dst_off[j], decoded + t.c_dst_off[j], (size_t)t.c_dst_cap[j]);
    }
}

}  // namespace emu_framing

extern "C" {

int64_t emu_framing_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(StreamEncodeArgs);
    case 1: return sizeof(StreamTables);
    case 2: return sizeof(StreamInfo);
    case 3: return sizeof(WrapArgs);
    case 4: return sizeof(UnwrapTables);
    case 5: return sizeof(UnwrapArgs);
    case 6: return sizeof(UnwrapInfo);
    case 7: return sizeof(StreamsEncodeArgs);
    case 8: return sizeof(StreamsTables);
    case 9: return sizeof(StreamsDecodeArgs);
    case 10: return sizeof(StreamsInfo);
    case 100: return kScanTile;
    case 101: return kCopySpan;
    default: return -1;
    }
}

// the product's grid formulas, for the entries below that take an explicit grid
int emu_items_grid(int64_t items) { return (int)emu_framing::items_grid(items, 0); }
int emu_copy_grid(int64_t bytes) { return (int)emu_framing::copy_grid(bytes, 0); }
int emu_walk_grid(int64_t n) { return (int)emu_framing::walk_grid(n, 0); }

// ---- single kernels ----------------------------------------------------------------------------------------------------------
void emu_scan(int64_t* x, int64_t n, int64_t* partial, int64_t* total) { emu_framing::scan(x, n, partial, total); }

void emu_stream_index(const uint8_t* src, int64_t src_len, const StreamTables* t, StreamInfo* info)
{
    const StreamTables tt = *t;
    simt::launch(dim3(1), dim3(64), 0, [=] { stream_index_kernel(src, src_len, tt, info); });
}

void emu_copy_encode(const StreamEncodeArgs* a, uint8_t* dst, const int64_t* total, int grid)
{
    EncodeLayout L = { *a };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { stream_pack_kernel(L, dst, total); });
}

void emu_copy_raw(const uint8_t* src, const StreamTables* t, int64_t n, uint8_t* dst, int64_t end, int grid)
{
    RawLayout L = { src, *t, n };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { stream_raw_copy_kernel(L, dst, end); });
}

void emu_copy_wrap(const WrapArgs* a, uint8_t* dst, int64_t cap, int grid)
{
    WrapLayout L = { *a };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { wrap_pack_kernel(L, dst, cap); });
}

void emu_copy_unwrap_raw(const UnwrapArgs* a, const UnwrapTables* t, uint8_t* dst, int64_t end, int grid)
{
    UnwrapRawLayout L = { *a, *t };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { wrap_raw_copy_kernel(L, dst, end); });
}

void emu_copy_streams(const StreamsEncodeArgs* a, uint8_t* dst, int64_t cap, int grid)
{
    StreamsEncodeLayout L = { *a };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { streams_pack_kernel(L, dst, cap); });
}

void emu_streams_walk(int fill, const StreamsDecodeArgs* a, const StreamsTables* t, int grid)
{
    const StreamsDecodeArgs aa = *a;
    const StreamsTables tt = *t;
    const unsigned g = emu_framing::walk_grid(aa.n, grid);
    if (fill) simt::launch(dim3(g), dim3(64), 0, [=] { streams_walk_kernel<true>(aa, tt); });
    else      simt::launch(dim3(g), dim3(64), 0, [=] { streams_walk_kernel<false>(aa, tt); });
}

void emu_stream_check(const StreamTables* t, int64_t n, int grid)
{
    const StreamTables tt = *t;
    simt::launch(dim3(emu_framing::items_grid(n, grid)), dim3(kStreamThreads), 0, [=] { stream_check_kernel(tt, n); });
}

// ---- stream_encode of lz4hip_api.hip without launch_encode: a->result and a->comp are the test's ---------------------------------
void emu_stream_encode(const StreamEncodeArgs* a, int32_t* lens, int64_t* partial, uint8_t* dst, int64_t* dst_len, int64_t bound,
                       int grid_items, int grid_copy)
{
    const StreamEncodeArgs aa = *a;
    const unsigned gi = emu_framing::items_grid(aa.n, grid_items);
    simt::launch(dim3(gi), dim3(kStreamThreads), 0, [=] { stream_lens_kernel(lens, aa.n, aa.src_len, aa.block); });
    simt::launch(dim3(gi), dim3(kStreamThreads), 0, [=] { stream_sizes_kernel(aa); });
    emu_framing::scan(aa.offs, aa.n, partial, dst_len);
    EncodeLayout L = { aa };
    simt::launch(dim3(emu_framing::copy_grid(bound, grid_copy)), dim3(kStreamThreads), 0, [=] { stream_pack_kernel(L, dst, dst_len); });
}

// ---- stream_index + stream_decode without launch_decode: results[j] / decoded stand for the decoder on row j ----------------------
// Returns 0, or 1 when the index reported a full table (stream_decode refuses that info).
int emu_stream_decode(const uint8_t* src, int64_t src_len, const StreamTables* t, const int32_t* results, const uint8_t* decoded,
                      uint8_t* dst, StreamInfo* index_info, StreamInfo* info, int grid_items, int grid_copy)
{
    const StreamTables tt = *t;
    simt::launch(dim3(1), dim3(64), 0, [=] { stream_index_kernel(src, src_len, tt, index_info); });
    const StreamInfo h = *index_info;
    if (h.error == kStreamTableFull) return 1;
    simt::launch(dim3(1), dim3(64), 0, [=] { stream_info_init_kernel(h, info, tt.min_bad); });
    if (h.compressed_chunks > 0) {
        emu_framing::fake_decode(tt, h.compressed_chunks, results, decoded, dst);
        const int64_t nc = h.compressed_chunks;
        simt::launch(dim3(emu_framing::items_grid(nc, grid_items)), dim3(kStreamThreads), 0, [=] { stream_check_kernel(tt, nc); });
    }
    if (h.chunks > h.compressed_chunks) {
        RawLayout L = { src, tt, h.chunks - h.compressed_chunks };
        const int64_t end = h.decoded_bytes;
        simt::launch(dim3(emu_framing::copy_grid(end, grid_copy)), dim3(kStreamThreads), 0, [=] { stream_raw_copy_kernel(L, dst, end); });
    }
    simt::launch(dim3(1), dim3(64), 0, [=] { stream_info_finish_kernel(info, tt.min_bad); });
    return 0;
}

// ---- wrap_encode without launch_encode: a->enc and a->comp are the test's -----------------------------------------------------------
void emu_wrap(const WrapArgs* a, int64_t* at, int32_t* lens, int32_t* result, int64_t* partial, uint8_t* dst, int64_t cap, int64_t bound,
              int grid_items, int grid_copy)
{
    const WrapArgs aa = *a;
    const unsigned gi = emu_framing::items_grid(aa.n, grid_items);
    simt::launch(dim3(gi), dim3(kStreamThreads), 0, [=] { wrap_lens_kernel(aa.off, aa.n, aa.src_len, at, lens); });
    simt::launch(dim3(gi), dim3(kStreamThreads), 0, [=] { wrap_sizes_kernel(aa, result); });
    emu_framing::scan(aa.dst_off, aa.n, partial, aa.dst_off + aa.n);
    WrapLayout L = { aa };
    simt::launch(dim3(emu_framing::copy_grid(bound, grid_copy)), dim3(kStreamThreads), 0, [=] { wrap_pack_kernel(L, dst, cap); });
}

// ---- unwrap_index (n > 0) -------------------------------------------------------------------------------------------------------------
void emu_unwrap_index(const UnwrapArgs* a, const UnwrapTables* t, UnwrapInfo* info, int grid_items)
{
    const UnwrapArgs aa = *a;
    const UnwrapTables tt = *t;
    *tt.min_bad = ~0ull;
    *tt.ncomp = 0;
    const unsigned gi = emu_framing::items_grid(aa.n, grid_items);
    simt::launch(dim3(gi), dim3(kStreamThreads), 0, [=] { unwrap_index_kernel(aa, tt); });
    emu_framing::scan(aa.dst_off, aa.n, tt.partial, aa.dst_off + aa.n);
    emu_framing::scan(tt.cidx, aa.n, tt.partial, tt.ncomp);
    simt::launch(dim3(gi), dim3(kStreamThreads), 0, [=] { unwrap_compact_kernel(aa, tt); });
    simt::launch(dim3(1), dim3(64), 0, [=] { unwrap_info_kernel(aa, tt, info); });
}

// ---- unwrap_decode without launch_decode, on the tables emu_unwrap_index left -------------------------------------------------------
void emu_unwrap_decode(const UnwrapArgs* a, const UnwrapTables* t, const UnwrapInfo* index_info, const int32_t* results, const uint8_t* decoded,
                       uint8_t* dst, UnwrapInfo* info, int grid_items, int grid_copy)
{
    const UnwrapArgs aa = *a;
    const UnwrapTables tt = *t;
    const UnwrapInfo h = *index_info;
    if (h.compressed > 0)
        for (int64_t j = 0; j < h.compressed; j++) {
            tt.c_result[j] = results[j];
            if (tt.c_dst_cap[j] > 0) memcpy(dst + tt.c_dst_off[j], decoded + tt.c_dst_off[j], (size_t)tt.c_dst_cap[j]);
        }
    if (aa.n > h.compressed && h.decoded_bytes > 0) {
        UnwrapRawLayout L = { aa, tt };
        const int64_t end = h.decoded_bytes;
        simt::launch(dim3(emu_framing::copy_grid(end, grid_copy)), dim3(kStreamThreads), 0, [=] { wrap_raw_copy_kernel(L, dst, end); });
    }
    if (h.compressed > 0) {
        const int64_t nc = h.compressed;
        int32_t* const status = aa.status;
        simt::launch(dim3(emu_framing::items_grid(nc, grid_items)), dim3(kStreamThreads), 0, [=] { unwrap_check_kernel(tt, nc, status); });
    }
    simt::launch(dim3(1), dim3(64), 0, [=] { unwrap_info_kernel(aa, tt, info); });
}

// ---- streams_encode in two halves around launch_encode: the chunk table, then (a->result and a->comp filled by the test) the pack -----
void emu_streams_plan(const StreamsEncodeArgs* a, int64_t* partial, int grid_items)
{
    const StreamsEncodeArgs aa = *a;
    simt::launch(dim3(emu_framing::items_grid(aa.n, grid_items)), dim3(kStreamThreads), 0, [=] { streams_counts_kernel(aa); });
    emu_framing::scan(aa.first, aa.n, partial, (int64_t*)aa.total);
    simt::launch(dim3(emu_framing::items_grid(aa.cap, grid_items)), dim3(kStreamThreads), 0, [=] { streams_chunks_kernel(aa); });
}

void emu_streams_pack(const StreamsEncodeArgs* a, int64_t* partial, int64_t* dst_off, uint8_t* dst, int64_t cap, int64_t bound,
                      int grid_items, int grid_copy)
{
    const StreamsEncodeArgs aa = *a;
    simt::launch(dim3(emu_framing::items_grid(aa.cap, grid_items)), dim3(kStreamThreads), 0, [=] { streams_sizes_kernel(aa); });
    emu_framing::scan(aa.offs, aa.cap, partial, aa.offs + aa.cap);
    simt::launch(dim3(emu_framing::items_grid(aa.n + 1, grid_items)), dim3(kStreamThreads), 0, [=] { streams_offsets_kernel(aa, dst_off); });
    StreamsEncodeLayout L = { aa };
    simt::launch(dim3(emu_framing::copy_grid(bound, grid_copy)), dim3(kStreamThreads), 0, [=] { streams_pack_kernel(L, dst, cap); });
}

// ---- streams_index (n > 0); `head` is the first 256 bytes of the scratch: [min_bad, totals[0], totals[1], ...] --------------------------
void emu_streams_index(const StreamsDecodeArgs* a, const StreamsTables* t, StreamsInfo* info, int grid_walk)
{
    const StreamsDecodeArgs aa = *a;
    const StreamsTables tt = *t;
    *tt.t.min_bad = ~0ull;
    tt.totals[0] = tt.totals[1] = 0;
    const unsigned g = emu_framing::walk_grid(aa.n, grid_walk);
    simt::launch(dim3(g), dim3(64), 0, [=] { streams_walk_kernel<false>(aa, tt); });
    emu_framing::scan(aa.dst_off, aa.n, tt.partial, aa.dst_off + aa.n);
    emu_framing::scan(tt.chunk_base, aa.n, tt.partial, tt.totals);
    emu_framing::scan(tt.comp_base, aa.n, tt.partial, tt.totals + 1);
    simt::launch(dim3(g), dim3(64), 0, [=] { streams_walk_kernel<true>(aa, tt); });
    simt::launch(dim3(1), dim3(64), 0, [=] { streams_info_kernel(aa, tt, info); });
}

// ---- streams_decode without launch_decode, on the tables emu_streams_index left; returns 1 for a full table ---------------------------
int emu_streams_decode(const StreamsDecodeArgs* a, const StreamsTables* t, const StreamsInfo* index_info, const int32_t* results,
                       const uint8_t* decoded, uint8_t* dst, StreamsInfo* info, int grid_items, int grid_copy)
{
    const StreamsDecodeArgs aa = *a;
    const StreamsTables tt = *t;
    const StreamsInfo h = *index_info;
    if (h.error == kStreamTableFull) return 1;
    *tt.t.min_bad = ~0ull;
    for (int64_t i = 0; i < aa.n; i++) tt.item_bad[i] = ~0ull;
    if (h.compressed_chunks > 0) {
        emu_framing::fake_decode(tt.t, h.compressed_chunks, results, decoded, dst);
        const int64_t nc = h.compressed_chunks;
        simt::launch(dim3(emu_framing::items_grid(nc, grid_items)), dim3(kStreamThreads), 0, [=] { streams_check_kernel(tt, nc); });
    }
    if (h.chunks > h.compressed_chunks) {
        RawLayout L = { aa.src, tt.t, h.chunks - h.compressed_chunks };
        const int64_t end = h.decoded_bytes;
        simt::launch(dim3(emu_framing::copy_grid(end, grid_copy)), dim3(kStreamThreads), 0, [=] { stream_raw_copy_kernel(L, dst, end); });
    }
    simt::launch(dim3(emu_framing::items_grid(aa.n, grid_items)), dim3(kStreamThreads), 0, [=] { streams_finish_kernel(aa, tt); });
    simt::launch(dim3(1), dim3(64), 0, [=] { streams_info_kernel(aa, tt, info); });
    return 0;
}

}  // extern "C"
