// emu_framing.hpp -- TEST INFRASTRUCTURE ONLY, included by emu_kernels.cpp.
// C entry points that run the framing kernels (lz4hip_stream.hpp, lz4hip_wrap.hpp, lz4hip_streams.hpp) under the SIMT emulator
// for tests/test_simt_framing.py: single kernels, and the library's own host code for the framing paths (lz4hip_framing.hpp: layouts,
// grids, kernel sequences and the staging of the host-pointer calls) over EmuBackend, with the block codec step replaced by arrays the
// test hands in and the device image served from host memory.  The argument structs are passed by pointer; tests/emu_helpers.py mirrors them with ctypes and checks the sizes against emu_framing_sizeof().  A grid
// argument of 0 means "the library's formula".
#pragma once
#include "lz4hip_framing.hpp"

#include <string>
#include <tuple>
#include <vector>

namespace emu_framing {

using namespace lz4hip;
using namespace lz4hip::framing;

// a kernel and its arguments, as the closure simt::launch runs in every lane
template <class... P>
struct KernelCall {
    void (*kernel)(P...);
    std::tuple<P...> args;
    void operator()() const { std::apply(kernel, args); }
};

template <class K, class L> bool same_kernel(K k, L l) { return (void (*)())k == (void (*)())l; }

// The device of lz4hip_framing.hpp's sequences, faked: the emulator's launcher, plain stores, and a block codec that hands out what
// the test computed.
struct EmuBackend {
    int grid_items = 0, grid_copy = 0, grid_walk = 0;       // the test's grid for each formula; 0 = the formula's own
    const int32_t* results = nullptr;                        // the block codec's stand-in: row j of a batch gets results[j] ...
    const uint8_t* bytes = nullptr;                          // ... and its output bytes from here, at the row's own output offset
    std::string error;

    // the emulator serves LZ4HIP_STATIC_LDS from its one LDS array: the scan kernels need their kStreamThreads * 8 bytes, the others do not mind
    template <class... P, class... A>
    void launch(void (*kernel)(P...), Grid grid, unsigned threads, A&&... a)
    {
        passes += same_kernel(kernel, stream_index_kernel) || same_kernel(kernel, unwrap_index_kernel) || same_kernel(kernel, streams_walk_kernel<false>);
        const int mine = grid.kind == kGridItems ? grid_items : (grid.kind == kGridCopy ? grid_copy : (grid.kind == kGridWalk ? grid_walk : 0));
        simt::launch(dim3(mine > 0 ? (unsigned)mine : grid.groups), dim3(threads), kStreamThreads * 8, KernelCall<P...>{ kernel, std::tuple<P...>{ P(a)... } });
    }
    int fill(void* p, int byte, size_t bytes) { memset(p, byte, bytes); return 0; }
    // results == NULL: the test wrote the encoder's results and bytes in place before the call
    int encode(const lz4hip_batch_t* b, int)
    {
        for (int64_t j = 0; results && j < b->n_blocks; j++) {
            const int64_t at = b->dst_off ? b->dst_off[j] : j * b->dst_stride;
            const int32_t r = results[j] < b->dst_cap[j] ? results[j] : b->dst_cap[j];
            b->result[j] = results[j];
            if (r > 0) memcpy((uint8_t*)b->dst + at, bytes + at, (size_t)r);
        }
        return 0;
    }
    int decode(const lz4hip_batch_t* b, int)
    {
        for (int64_t j = 0; j < b->n_blocks; j++) {
            b->result[j] = results[j];
            if (b->dst_cap[j] > 0) memcpy((uint8_t*)b->dst + b->dst_off[j], bytes + b->dst_off[j], (size_t)b->dst_cap[j]);
        }
        return 0;
    }
    int last_error() { return 0; }
    int fail(int code, const char* what) { error = what; return code; }

    // The staging image of the host-pointer calls: exactly the bytes asked for between guard bytes, at a multiple of 256 as a device
    // allocation is.  A reserve that grows MOVES: the new block is a new allocation and the old one is filled with kStale and kept
    // until the backend dies, so code that goes on using an old base reads kStale, and what it writes there shows in intact().
    static constexpr size_t kGuard = 256;
    static constexpr uint8_t kGuardByte = 0xC3, kFresh = 0xEE, kStale = 0xDD;
    struct Block { std::vector<uint8_t> store; uint8_t* base; size_t bytes; };
    std::vector<Block> blocks;
    int64_t reserves = 0, moves = 0, uploads = 0, downloads = 0, syncs = 0, passes = 0;

    int reserve(size_t bytes, uint8_t*& base)
    {
        reserves++;
        if (blocks.empty() || bytes > blocks.back().bytes) {
            if (!blocks.empty()) memset(blocks.back().base, kStale, blocks.back().bytes);
            moves++;
            blocks.emplace_back();
            Block& b = blocks.back();
            b.store.assign(bytes + 2 * kGuard + 256, kGuardByte);
            b.base = (uint8_t*)(((uintptr_t)b.store.data() + kGuard + 255) / 256 * 256);
            b.bytes = bytes;
            memset(b.base, kFresh, bytes);
        }
        base = blocks.back().base;
        return 0;
    }
    int upload(void* dev, const void* host, size_t bytes) { uploads++; memcpy(dev, host, bytes); return 0; }
    int download(void* host, const void* dev, size_t bytes) { downloads++; memcpy(host, dev, bytes); return 0; }
    int sync() { syncs++; return 0; }
    // no byte outside any block's image was written, and none of a block that was given up
    bool intact() const
    {
        for (size_t k = 0; k < blocks.size(); k++) {
            const Block& b = blocks[k];
            for (const uint8_t* p = b.store.data(); p < b.store.data() + b.store.size(); p++) {
                const bool inside = p >= b.base && p < b.base + b.bytes;
                if (inside ? (k + 1 < blocks.size() && *p != kStale) : *p != kGuardByte) return false;
            }
        }
        return true;
    }
};

inline EmuBackend backend(int grid_items, int grid_copy, int grid_walk = 0, const int32_t* results = nullptr, const uint8_t* bytes = nullptr)
{
    EmuBackend be;
    be.grid_items = grid_items; be.grid_copy = grid_copy; be.grid_walk = grid_walk; be.results = results; be.bytes = bytes;
    return be;
}

}  // namespace emu_framing

// the host-pointer calls of lz4hip_framing.hpp (emu_host_*): what the emulated device is to do, and what it did
struct EmuHostRun {
    const int32_t* results; const uint8_t* bytes;            // the block codec's stand-in
    int32_t grid_items, grid_copy, grid_walk, intact;        // intact: EmuBackend::intact() after the call
    int64_t reserves, moves, uploads, downloads, syncs, passes, image_bytes;    // image_bytes: the last reserve's
    char error[160];                                         // what fail() recorded
};

template <class Call>
int emu_host_run(EmuHostRun* r, Call call)
{
    emu_framing::EmuBackend be = emu_framing::backend(r->grid_items, r->grid_copy, r->grid_walk, r->results, r->bytes);
    const int rc = call(be);
    r->intact = be.intact();
    r->reserves = be.reserves; r->moves = be.moves; r->uploads = be.uploads; r->downloads = be.downloads; r->syncs = be.syncs; r->passes = be.passes;
    r->image_bytes = be.blocks.empty() ? 0 : (int64_t)be.blocks.back().bytes;
    snprintf(r->error, sizeof r->error, "%s", be.error.c_str());
    return rc;
}

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
    case 11: return sizeof(EmuHostRun);
    case 100: return kScanTile;
    case 101: return kCopySpan;
    default: return -1;
    }
}

// the library's grid formulas, for the entries below that take an explicit grid
int emu_items_grid(int64_t items) { return (int)framing::stream_grid(items).groups; }
int emu_copy_grid(int64_t bytes) { return (int)framing::copy_grid(bytes).groups; }
int emu_walk_grid(int64_t n) { return (int)framing::walk_grid(n).groups; }

// ---- single kernels ----------------------------------------------------------------------------------------------------------
void emu_scan(int64_t* x, int64_t n, int64_t* partial, int64_t* total)
{
    emu_framing::EmuBackend be;
    framing::launch_scan(be, x, n, partial, total);
}

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
    const unsigned g = grid > 0 ? (unsigned)grid : framing::walk_grid(aa.n).groups;
    if (fill) simt::launch(dim3(g), dim3(64), 0, [=] { streams_walk_kernel<true>(aa, tt); });
    else      simt::launch(dim3(g), dim3(64), 0, [=] { streams_walk_kernel<false>(aa, tt); });
}

void emu_stream_check(const StreamTables* t, int64_t n, int grid)
{
    const StreamTables tt = *t;
    simt::launch(dim3(grid > 0 ? (unsigned)grid : framing::stream_grid(n).groups), dim3(kStreamThreads), 0, [=] { stream_check_kernel(tt, n); });
}

// ---- the sequences of lz4hip_framing.hpp over the test's own arrays ------------------------------------------------------------------
// stream_encode without the block encoder: a->result and a->comp are the test's
void emu_stream_encode(const StreamEncodeArgs* a, int32_t* lens, int64_t* partial, uint8_t* dst, int64_t* dst_len, int64_t bound,
                       int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy);
    framing::stream_encode_run(be, *a, LZ4HIP_MODE_FAST, lens, partial, dst, dst_len);
}

// stream_index + stream_decode: results[j] / decoded stand for the block decoder on row j.  Returns 0, or 1 when the index reported a
// full table (stream_decode refuses that info).
int emu_stream_decode(const uint8_t* src, int64_t src_len, const StreamTables* t, const int32_t* results, const uint8_t* decoded,
                      uint8_t* dst, StreamInfo* index_info, StreamInfo* info, int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, decoded);
    framing::stream_index_run(be, src, src_len, *t, index_info);
    if (index_info->error == kStreamTableFull) return 1;
    framing::stream_decode_run(be, src, *index_info, *t, dst, info);
    return 0;
}

// wrap_encode without the block encoder: a->enc and a->comp are the test's
void emu_wrap(const WrapArgs* a, int64_t* at, int32_t* lens, int32_t* result, int64_t* partial, uint8_t* dst, int64_t cap, int64_t bound,
              int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy);
    framing::wrap_encode_run(be, *a, LZ4HIP_MODE_FAST, at, lens, result, partial, dst, cap);
}

void emu_unwrap_index(const UnwrapArgs* a, const UnwrapTables* t, UnwrapInfo* info, int grid_items)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, 0);
    framing::unwrap_index_run(be, *a, *t, info);
}

// unwrap_decode on the tables emu_unwrap_index left
void emu_unwrap_decode(const UnwrapArgs* a, const UnwrapTables* t, const UnwrapInfo* index_info, const int32_t* results, const uint8_t* decoded,
                       uint8_t* dst, UnwrapInfo* info, int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, decoded);
    framing::unwrap_decode_run(be, *a, *t, *index_info, dst, info);
}

// streams_encode in its two parts: the chunk table, then (a->result and a->comp filled by the test) the pack
void emu_streams_plan(const StreamsEncodeArgs* a, int64_t* partial, int grid_items)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, 0);
    framing::streams_encode_plan(be, *a, partial);
}

void emu_streams_pack(const StreamsEncodeArgs* a, int64_t* partial, int64_t* dst_off, uint8_t* dst, int64_t cap, int64_t bound,
                      int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy);
    framing::streams_encode_pack(be, *a, partial, dst_off, dst, cap);
}

void emu_streams_index(const StreamsDecodeArgs* a, const StreamsTables* t, StreamsInfo* info, int grid_walk)
{
    emu_framing::EmuBackend be = emu_framing::backend(0, 0, grid_walk);
    framing::streams_index_run(be, *a, *t, info);
}

// streams_decode on the tables emu_streams_index left; returns 1 for a full table
int emu_streams_decode(const StreamsDecodeArgs* a, const StreamsTables* t, const StreamsInfo* index_info, const int32_t* results,
                       const uint8_t* decoded, uint8_t* dst, StreamsInfo* info, int grid_items, int grid_copy)
{
    if (index_info->error == kStreamTableFull) return 1;
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, decoded);
    framing::streams_decode_run(be, *a, *t, *index_info, dst, info);
    return 0;
}

// ---- the whole functions of lz4hip_framing.hpp (front and sequence) on a scratch buffer the test brings -----------------------------
// The library's argument lists, then the block codec's stand-in (results, bytes) and the grids.
int64_t emu_scratch_bytes(int which, int64_t a, int64_t b, int64_t c)
{
    switch (which) {
    case 0: return framing::stream_encode_scratch(nullptr, a, framing::stream_block((int32_t)b)).bytes;      // (src_len, block_size)
    case 1: return framing::stream_decode_scratch_bytes(a);                                                   // (max_chunks)
    case 2: return framing::wrap_scratch(nullptr, a, b).bytes;                                                // (n, src_len)
    case 3: return framing::unwrap_scratch_bytes(a);                                                          // (n)
    case 4: return framing::streams_encode_scratch(nullptr, a, b, framing::stream_block((int32_t)c)).bytes;  // (n, src_len, block_size)
    case 5: return framing::streams_decode_scratch_bytes(a, b);                                               // (n, max_chunks)
    default: return -1;
    }
}

int emu_lib_stream_encode(const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len,
                          void* scratch, int64_t scratch_bytes, const int32_t* results, const uint8_t* bytes, int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, bytes);
    return framing::stream_encode(be, src, src_len, block_size, mode, dst, dst_cap, dst_len, scratch, scratch_bytes);
}

int emu_lib_stream_index(const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes, lz4hip_stream_info_t* info)
{
    emu_framing::EmuBackend be;
    return framing::stream_index(be, src, src_len, max_chunks, scratch, scratch_bytes, info);
}

int emu_lib_stream_decode(const void* src, const lz4hip_stream_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                          void* dst, int64_t dst_cap, lz4hip_stream_info_t* info, const int32_t* results, const uint8_t* bytes,
                          int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, bytes);
    return framing::stream_decode(be, src, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, info);
}

int emu_lib_wrap(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode, void* dst, int64_t dst_cap, int64_t* dst_off,
                 int32_t* result, void* scratch, int64_t scratch_bytes, const int32_t* results, const uint8_t* bytes, int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, bytes);
    return framing::wrap_encode(be, src, src_len, src_off, n, mode, dst, dst_cap, dst_off, result, scratch, scratch_bytes);
}

int emu_lib_unwrap_index(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t* dst_off, int32_t* status,
                         void* scratch, int64_t scratch_bytes, lz4hip_unwrap_info_t* info, int grid_items)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, 0);
    return framing::unwrap_index(be, src, src_len, src_off, n, dst_off, status, scratch, scratch_bytes, info);
}

int emu_lib_unwrap_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const lz4hip_unwrap_info_t* info_host,
                          void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, const int64_t* dst_off, int32_t* status,
                          lz4hip_unwrap_info_t* info, const int32_t* results, const uint8_t* bytes, int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, bytes);
    return framing::unwrap_decode(be, src, src_len, src_off, n, info_host, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info);
}

int emu_lib_streams_encode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode, void* dst,
                           int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, const int32_t* results, const uint8_t* bytes,
                           int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, bytes);
    return framing::streams_encode(be, src, src_len, src_off, n, block_size, mode, dst, dst_cap, dst_off, scratch, scratch_bytes);
}

int emu_lib_streams_index(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks, int64_t* dst_off,
                          int32_t* status, int64_t* error_offset, void* scratch, int64_t scratch_bytes, lz4hip_streams_info_t* info, int grid_walk)
{
    emu_framing::EmuBackend be = emu_framing::backend(0, 0, grid_walk);
    return framing::streams_index(be, src, src_len, src_off, n, max_chunks, dst_off, status, error_offset, scratch, scratch_bytes, info);
}

int emu_lib_streams_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const lz4hip_streams_info_t* info_host,
                           int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, const int64_t* dst_off,
                           int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info, const int32_t* results, const uint8_t* bytes,
                           int grid_items, int grid_copy)
{
    emu_framing::EmuBackend be = emu_framing::backend(grid_items, grid_copy, 0, results, bytes);
    return framing::streams_decode(be, src, src_len, src_off, n, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, dst_off, status,
                                   error_offset, info);
}

// ---- the host-pointer calls of lz4hip_framing.hpp: the library's argument lists, then an EmuHostRun ------------------------------------
int emu_host_stream_encode(const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len, EmuHostRun* r)
{
    return emu_host_run(r, [&](emu_framing::EmuBackend& be) { return framing::stream_encode_host(be, src, src_len, block_size, mode, dst, dst_cap, dst_len); });
}

int emu_host_stream_decode(const void* src, int64_t src_len, void* dst, int64_t dst_cap, lz4hip_stream_info_t* info, EmuHostRun* r)
{
    return emu_host_run(r, [&](emu_framing::EmuBackend& be) { return framing::stream_decode_host(be, src, src_len, dst, dst_cap, info); });
}

int emu_host_wrap(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode, void* dst, int64_t dst_cap, int64_t* dst_off,
                  int32_t* result, EmuHostRun* r)
{
    return emu_host_run(r, [&](emu_framing::EmuBackend& be) { return framing::wrap_host(be, src, src_len, src_off, n, mode, dst, dst_cap, dst_off, result); });
}

int emu_host_unwrap(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status,
                    lz4hip_unwrap_info_t* info, EmuHostRun* r)
{
    return emu_host_run(r, [&](emu_framing::EmuBackend& be) { return framing::unwrap_host(be, src, src_len, src_off, n, dst, dst_cap, dst_off, status, info); });
}

int emu_host_streams_encode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode, void* dst,
                            int64_t dst_cap, int64_t* dst_off, EmuHostRun* r)
{
    return emu_host_run(r, [&](emu_framing::EmuBackend& be) {
        return framing::streams_encode_host(be, src, src_len, src_off, n, block_size, mode, dst, dst_cap, dst_off);
    });
}

int emu_host_streams_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* dst, int64_t dst_cap, int64_t* dst_off,
                            int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info, EmuHostRun* r)
{
    return emu_host_run(r, [&](emu_framing::EmuBackend& be) {
        return framing::streams_decode_host(be, src, src_len, src_off, n, dst, dst_cap, dst_off, status, error_offset, info);
    });
}

}  // extern "C"
