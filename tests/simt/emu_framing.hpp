// emu_framing.hpp -- TEST INFRASTRUCTURE ONLY, included by emu_framing.cpp.
// The device of lz4hip_framing.hpp's sequences, faked once for every part of libsimt_framing.so: EmuBackend (the emulator's launcher,
// plain stores, the moving staging image of the host-pointer calls between guard bytes, and the base block codec stand-in), the
// counters record every run record embeds (EmuCounters, filled by finish) and the run record of the plain host-pointer calls
// (EmuHostRun).  tests/emu_lib.py mirrors the two records with ctypes.  The parts (emu_*.inc) add only their own stand-in codec, which
// verifies the promises of its own sequence, and their C entry points.
#pragma once
#include "lz4hip_framing.hpp"

#include <string>
#include <tuple>
#include <vector>

// what a backend counted during a call, the state of its guard bytes after it and the failure text it recorded
struct EmuCounters {
    int64_t intact;                                          // EmuBackend::intact() after the call
    int64_t reserves, moves, uploads, downloads, syncs;
    int64_t passes;                                          // walk / index kernels launched
    int64_t last_download, image_bytes;                      // the bytes of the last download; of the last reserve
    char error[160];                                         // what fail() recorded
};

// the host-pointer calls without a stand-in of their own (emu_host_*): what the emulated device is to do, and what it did
struct EmuHostRun {
    const int32_t* results; const uint8_t* bytes;            // the block codec's stand-in
    int32_t grid_items, grid_copy, grid_walk, pad;           // > 0 replaces the formula's answer
    EmuCounters counters;
};

namespace emu_framing {

using namespace lz4hip;
using namespace lz4hip::framing;

constexpr uint8_t kJunk = 0xBD;                              // what a stand-in codec may leave inside a row's capacity

// what a workgroup of the wavefront decoder has on the device: the LDS of the calls that run the real decoder (linked blocks, dictionaries)
constexpr size_t kWaveDecodeLdsBytes = (size_t)kWaveDecodeWavesPerGroup * kWaveLdsBytes;
static_assert(kWaveDecodeLdsBytes >= kSizesLdsBytes && kWaveDecodeLdsBytes >= kStreamThreads * 8, "one LDS size serves every kernel of the sequences");

// the kernels' view of a batch of the C interface (to_device_batch of lz4hip_api.hip)
inline Batch device_batch(const lz4hip_batch_t* b)
{
    Batch d;
    memset(&d, 0, sizeof d);
    d.src = (const uint8_t*)b->src; d.src_off = b->src_off; d.src_stride = b->src_stride; d.src_len = b->src_len; d.src_len_all = b->src_len_all;
    d.dst = (uint8_t*)b->dst; d.dst_off = b->dst_off; d.dst_stride = b->dst_stride; d.dst_cap = b->dst_cap; d.dst_cap_all = b->dst_cap_all;
    d.result = b->result; d.n_blocks = b->n_blocks;
    return d;
}

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
    // the emulator serves LZ4HIP_STATIC_LDS from its one LDS array: the scan kernels need their kStreamThreads * 8 bytes, the others
    // do not mind; the frame and size paths set what their walk's workgroup has on the device (kSizesLdsBytes)
    size_t lds_bytes = kStreamThreads * 8;
    const int32_t* results = nullptr;                        // the block codec's stand-in: row j of a batch gets results[j] ...
    const uint8_t* bytes = nullptr;                          // ... and its output bytes from here, at the row's own output offset
    std::string error;

    template <class... P, class... A>
    void launch(void (*kernel)(P...), Grid grid, unsigned threads, A&&... a)
    {
        passes += same_kernel(kernel, stream_index_kernel) || same_kernel(kernel, unwrap_index_kernel) || same_kernel(kernel, streams_walk_kernel<false>) ||
                  same_kernel(kernel, frame_walk_kernel) || same_kernel(kernel, lz4f_walk_kernel);
        const int mine = grid.kind == kGridItems ? grid_items : (grid.kind == kGridCopy ? grid_copy : (grid.kind == kGridWalk ? grid_walk : 0));
        simt::launch(dim3(mine > 0 ? (unsigned)mine : grid.groups), dim3(threads), lds_bytes, KernelCall<P...>{ kernel, std::tuple<P...>{ P(a)... } });
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
    int64_t reserves = 0, moves = 0, uploads = 0, downloads = 0, syncs = 0, passes = 0, last_download = 0;

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
    int download(void* host, const void* dev, size_t bytes) { downloads++; last_download = (int64_t)bytes; memcpy(host, dev, bytes); return 0; }
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

// `Backend` with the test's grids and the base stand-in's arrays
template <class Backend = EmuBackend>
Backend backend(int grid_items, int grid_copy, int grid_walk = 0, const int32_t* results = nullptr, const uint8_t* bytes = nullptr)
{
    Backend be;
    be.grid_items = grid_items; be.grid_copy = grid_copy; be.grid_walk = grid_walk; be.results = results; be.bytes = bytes;
    return be;
}

// the end of every entry point: the failure text for a caller that keeps only that ...
inline int finish(const EmuBackend& be, int rc, char* error, size_t error_bytes)
{
    if (error) snprintf(error, error_bytes, "%s", be.error.c_str());
    return rc;
}

// ... and the whole record
inline int finish(const EmuBackend& be, int rc, EmuCounters* c)
{
    c->intact = be.intact();
    c->reserves = be.reserves; c->moves = be.moves; c->uploads = be.uploads; c->downloads = be.downloads; c->syncs = be.syncs; c->passes = be.passes;
    c->last_download = be.last_download;
    c->image_bytes = be.blocks.empty() ? 0 : (int64_t)be.blocks.back().bytes;
    return finish(be, rc, c->error, sizeof c->error);
}

}  // namespace emu_framing
