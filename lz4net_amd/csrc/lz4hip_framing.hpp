// lz4hip_framing.hpp -- host side of the framing paths (LZ4Stream buffers, wrapped messages, batches of LZ4Stream buffers, legacy
// frames, LZ4 frames and batches of them), of the block batch's size query (lz4hip_sizes.hpp), of its packed encode (lz4hip_packed.hpp) and of its compact decode
// (lz4hip_compact.hpp): the scratch
// layouts, the grids and the kernel sequences around the block codec, written ONCE for the library (lz4hip_api.hip, HipBackend) and for
// the CPU emulator (tests/simt/emu_framing.hpp, EmuBackend).  Host code only: no kernel is defined here and nothing here calls the HIP
// runtime or the emulator; everything that touches the device goes through the backend B, which has exactly
//
//     void launch(kernel, Grid, threads, args...)    the kernel on the call's stream, no dynamic LDS
//     int  fill(p, byte, bytes)                      device bytes set to a value, in stream order
//     int  encode(const lz4hip_batch_t*, mode)       the block encoder / decoder over a batch (launch_encode / launch_decode)
//     int  decode(const lz4hip_batch_t*, known)
//     int  encode_dict_prime(dict_end, reach, primed), encode_dict(batch, dict_end, reach, primed), decode_dict(batch, dict_end, reach, known)
//                                                    the dictionary forms, only where a sequence is instantiated with a dictionary
//     int  last_error()                              0, or the failure of a launch since the last look
//     int  fail(code, text)                          records the text, returns the code
//
// and, for the host-pointer calls at the end (*_host) alone, the staging of caller memory in a device image:
//
//     int  reserve(bytes, base&)                     an image of at least `bytes` bytes; base may change whenever the image grows
//     int  upload(dev, host, bytes)                  copies in stream order
//     int  download(host, dev, bytes)
//     int  sync()                                    waits for the stream
//
// Each operation is a front (argument checks, the caller's scratch laid out into the kernels' argument structs) over a sequence
// (*_run: structs in, launches out); the emulator's tests enter at either.
#pragma once
#include "lz4hip_stream.hpp"
#include "lz4hip_wrap.hpp"
#include "lz4hip_streams.hpp"
#include "lz4hip_sizes.hpp"
#include "lz4hip_frame.hpp"
#include "lz4hip_packed.hpp"
#include "lz4hip_compact.hpp"
#include "lz4hip_lz4f.hpp"
#include "lz4hip_lz4f_batch.hpp"
#include "lz4hip_lz4f_linked.hpp"

#include "../../include/lz4hip.h"

#include <cstddef>
#include <cstring>
#include <string>

namespace lz4hip {
namespace framing {

static_assert(sizeof(StreamInfo) == sizeof(lz4hip_stream_info_t) && offsetof(StreamInfo, error) == offsetof(lz4hip_stream_info_t, error),
              "StreamInfo must mirror lz4hip_stream_info_t");
static_assert(sizeof(UnwrapInfo) == sizeof(lz4hip_unwrap_info_t) && offsetof(UnwrapInfo, error) == offsetof(lz4hip_unwrap_info_t, error),
              "UnwrapInfo must mirror lz4hip_unwrap_info_t");
static_assert(kWrapBadOffsets == LZ4HIP_E_ARGUMENT && kWrapSizeInvalid == LZ4HIP_WRAP_SIZE_INVALID &&
              kWrapCorruptHeader == LZ4HIP_WRAP_CORRUPT_HEADER && kWrapCorruptBlock == LZ4HIP_WRAP_CORRUPT_BLOCK, "wrap statuses");
static_assert(sizeof(StreamsInfo) == sizeof(lz4hip_streams_info_t) && offsetof(StreamsInfo, error) == offsetof(lz4hip_streams_info_t, error) &&
              offsetof(StreamsInfo, first_error) == offsetof(lz4hip_streams_info_t, first_error), "StreamsInfo must mirror lz4hip_streams_info_t");
static_assert(kStreamsBadOffsets == LZ4HIP_E_ARGUMENT, "streams statuses");
static_assert(sizeof(SizesInfo) == sizeof(lz4hip_sizes_info_t) && offsetof(SizesInfo, first_error) == offsetof(lz4hip_sizes_info_t, first_error) &&
              offsetof(SizesInfo, error) == offsetof(lz4hip_sizes_info_t, error), "SizesInfo must mirror lz4hip_sizes_info_t");
static_assert(kSizesTooLarge == LZ4HIP_E_ARGUMENT, "sizes results");
static_assert(sizeof(FrameInfo) == sizeof(lz4hip_frame_info_t) && offsetof(FrameInfo, good_bytes) == offsetof(lz4hip_frame_info_t, good_bytes) &&
              offsetof(FrameInfo, error) == offsetof(lz4hip_frame_info_t, error), "FrameInfo must mirror lz4hip_frame_info_t");
static_assert(kFrameOk == LZ4HIP_FRAME_OK && kFrameBadMagic == LZ4HIP_FRAME_BAD_MAGIC && kFrameTruncated == LZ4HIP_FRAME_TRUNCATED &&
              kFrameBadSize == LZ4HIP_FRAME_BAD_SIZE && kFrameCorruptBlock == LZ4HIP_FRAME_CORRUPT_BLOCK &&
              kFrameTableFull == LZ4HIP_FRAME_TABLE_FULL, "frame statuses");
static_assert(kPackedBadLength == LZ4HIP_E_ARGUMENT, "packed results");
static_assert(sizeof(PackedInfo) == sizeof(lz4hip_packed_info_t) && offsetof(PackedInfo, first_failed) == offsetof(lz4hip_packed_info_t, first_failed) &&
              offsetof(PackedInfo, error) == offsetof(lz4hip_packed_info_t, error), "PackedInfo must mirror lz4hip_packed_info_t");
// (the compact decode's record is written by the packed encode's info kernels)
static_assert(sizeof(PackedInfo) == sizeof(lz4hip_compact_info_t) && offsetof(PackedInfo, blocks) == offsetof(lz4hip_compact_info_t, blocks) &&
              offsetof(PackedInfo, packed_bytes) == offsetof(lz4hip_compact_info_t, decoded_bytes) &&
              offsetof(PackedInfo, written_blocks) == offsetof(lz4hip_compact_info_t, written_blocks) &&
              offsetof(PackedInfo, first_failed) == offsetof(lz4hip_compact_info_t, first_failed) &&
              offsetof(PackedInfo, error) == offsetof(lz4hip_compact_info_t, error), "PackedInfo must mirror lz4hip_compact_info_t");

#define LZ4HIP_FRAMING_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

// ---- grids ---------------------------------------------------------------------------------------------------------------------
// A launch's workgroups and the formula they came from: the emulator's tests replace each formula's answer by grids of 1 and 3.
enum GridKind { kGridFixed, kGridItems, kGridCopy, kGridWalk };
struct Grid { unsigned groups; GridKind kind; };

constexpr unsigned kStreamMaxGroups = 8192;                   // grid-stride kernels: at most 32 workgroups of 256 per CU
constexpr unsigned kStreamsMaxWalkGroups = 1u << 22;          // one wavefront per item; more items than this share wavefronts

inline Grid fixed_grid(int64_t groups) { return { (unsigned)groups, kGridFixed }; }
inline Grid stream_grid(int64_t items)
{
    const int64_t g = (items + kStreamThreads - 1) / kStreamThreads;
    return { g < 1 ? 1u : (g > kStreamMaxGroups ? kStreamMaxGroups : (unsigned)g), kGridItems };
}
// the copy kernels: one workgroup per kCopySpan output bytes, at most kStreamMaxGroups (then each takes several spans)
inline Grid copy_grid(int64_t bytes)
{
    const int64_t g = (bytes + kCopySpan - 1) / kCopySpan;
    return { g < 1 ? 1u : (g > kStreamMaxGroups ? kStreamMaxGroups : (unsigned)g), kGridCopy };
}
inline Grid walk_grid(int64_t n) { return { n < (int64_t)kStreamsMaxWalkGroups ? (unsigned)n : kStreamsMaxWalkGroups, kGridWalk }; }
// the size query: one lane per block in single-wavefront workgroups, at most kStreamsMaxWalkGroups of them (then a lane takes several
// blocks); `groups` > 0 (the knob sizes_groups, the emulator's tests) replaces the formula's answer
inline Grid sizes_grid(int64_t n, int groups)
{
    const int64_t g = (n + kSizesThreads - 1) / kSizesThreads;
    if (groups > 0) return { (unsigned)groups, kGridFixed };
    return { g < 1 ? 1u : (g > (int64_t)kStreamsMaxWalkGroups ? kStreamsMaxWalkGroups : (unsigned)g), kGridFixed };
}

// ---- sizes ---------------------------------------------------------------------------------------------------------------------
inline int64_t stream_block(int32_t block_size) { return block_size < 16 ? 16 : block_size; }
inline int64_t stream_chunks(int64_t len, int64_t block) { return len <= 0 ? 0 : (len - 1) / block + 1; }
inline int64_t a256(int64_t v) { return (v + 255) / 256 * 256; }
inline int64_t scan_tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }

inline int64_t stream_bound(int64_t len, int32_t block_size)
{
    if (len <= 0) return 0;
    const int64_t block = stream_block(block_size);
    return len + stream_chunks(len, block) * (1 + 2 * varint_len((uint64_t)block));
}

inline int64_t wrap_bound(int64_t n, int64_t src_len) { return (src_len < 0 ? 0 : src_len) + kWrapHeader * (n < 0 ? 0 : n); }

// the chunk table's size: the host does not know the offsets, only that sum ceil(len_i / block) <= src_len / block + n
inline int64_t streams_chunk_cap(int64_t n, int64_t src_len, int64_t block) { return src_len / block + n; }

inline int64_t streams_bound(int64_t n, int64_t src_len, int32_t block_size)
{
    if (n < 0) n = 0;
    if (src_len < 0) src_len = 0;
    const int64_t block = stream_block(block_size);
    return src_len + streams_chunk_cap(n, src_len, block) * (1 + 2 * varint_len((uint64_t)block));
}

// ---- scratch layouts -------------------------------------------------------------------------------------------------------------
// Cuts a buffer into pieces that start at multiples of 256 bytes, in the order they are taken.  Every layout below is ONE walk of a
// Carver: over the caller's scratch it yields the pointers, over no buffer at all (`*_bytes`) the size the caller must bring -- so a
// piece cannot be added to one and forgotten in the other.  The *_host entry points cut their device images the same way.
struct Carver {
    uint8_t* base;
    int64_t at;
    explicit Carver(void* buffer = nullptr) : base((uint8_t*)buffer), at(0) {}
    int64_t take(int64_t bytes) { const int64_t piece = at; at += a256(bytes); return piece; }    // the piece's offset
    template <class T> T* take_as(int64_t bytes) { return (T*)((uintptr_t)base + (uintptr_t)take(bytes)); }
};

// stream encode: the encoder's output (chunk k at k * block), chunk lengths, results, sizes / offsets, tile sums of the scan
struct StreamEncodeScratch { uint8_t* comp; int32_t* lens; int32_t* result; int64_t* offs; int64_t* partial; int64_t bytes; };
inline StreamEncodeScratch stream_encode_scratch(void* scratch, int64_t len, int64_t block)
{
    const int64_t n = stream_chunks(len, block);
    Carver c(scratch);
    StreamEncodeScratch l;
    l.comp = c.take_as<uint8_t>(len);
    l.lens = c.take_as<int32_t>(4 * n);
    l.result = c.take_as<int32_t>(4 * n);
    l.offs = c.take_as<int64_t>(8 * n);
    l.partial = c.take_as<int64_t>(8 * scan_tiles(n));
    l.bytes = c.at;
    return l;
}

// stream decode: the corrupt-block minimum, then the two tables of max_chunks entries
inline StreamTables stream_tables(Carver& c, int64_t max_chunks)
{
    StreamTables t;
    t.max_chunks = max_chunks;
    t.min_bad = c.take_as<unsigned long long>(256);
    t.c_src_off = c.take_as<int64_t>(8 * max_chunks);
    t.c_dst_off = c.take_as<int64_t>(8 * max_chunks);
    t.c_hdr_off = c.take_as<int64_t>(8 * max_chunks);
    t.r_dst_off = c.take_as<int64_t>(8 * max_chunks);
    t.r_src_off = c.take_as<int64_t>(8 * max_chunks);
    t.c_src_len = c.take_as<int32_t>(4 * max_chunks);
    t.c_dst_cap = c.take_as<int32_t>(4 * max_chunks);
    t.c_result = c.take_as<int32_t>(4 * max_chunks);
    t.r_len = c.take_as<int32_t>(4 * max_chunks);
    return t;
}
inline int64_t stream_decode_scratch_bytes(int64_t max_chunks) { Carver c; stream_tables(c, max_chunks); return c.at; }

// wrap: the encoder's output (message i at src_off[i]), its view of the offsets and lengths, its results, the scan's tile sums
struct WrapScratch { uint8_t* comp; int64_t* at; int32_t* lens; int32_t* enc; int64_t* partial; int64_t bytes; };
inline WrapScratch wrap_scratch(void* scratch, int64_t n, int64_t src_len)
{
    Carver c(scratch);
    WrapScratch l;
    l.comp = c.take_as<uint8_t>(src_len);
    l.at = c.take_as<int64_t>(8 * n);
    l.lens = c.take_as<int32_t>(4 * n);
    l.enc = c.take_as<int32_t>(4 * n);
    l.partial = c.take_as<int64_t>(8 * scan_tiles(n));
    l.bytes = c.at;
    return l;
}

// unwrap: [min_bad, ncomp], the flags / table rows, the tile sums, then the table of up to n compressed messages
inline UnwrapTables unwrap_tables(Carver& c, int64_t n)
{
    UnwrapTables t;
    t.n = n;
    t.min_bad = c.take_as<unsigned long long>(256);
    t.ncomp = (int64_t*)t.min_bad + 1;
    t.cidx = c.take_as<int64_t>(8 * n);
    t.partial = c.take_as<int64_t>(8 * scan_tiles(n));
    t.c_src_off = c.take_as<int64_t>(8 * n);
    t.c_dst_off = c.take_as<int64_t>(8 * n);
    t.c_msg = c.take_as<int64_t>(8 * n);
    t.c_src_len = c.take_as<int32_t>(4 * n);
    t.c_dst_cap = c.take_as<int32_t>(4 * n);
    t.c_result = c.take_as<int32_t>(4 * n);
    t.raw_len = c.take_as<int32_t>(4 * n);
    return t;
}
inline int64_t unwrap_scratch_bytes(int64_t n) { Carver c; unwrap_tables(c, n); return c.at; }

// streams encode: the encoder's output (every chunk at its own source position), the items' first chunks, the chunk total, the chunk
// table (position, length, result, size / offset + the total), the scans' tile sums
struct StreamsEncodeScratch {
    uint8_t* comp; int64_t* first; int64_t* total; int64_t* c_at; int32_t* c_len; int32_t* result; int64_t* offs; int64_t* partial; int64_t bytes;
};
inline StreamsEncodeScratch streams_encode_scratch(void* scratch, int64_t n, int64_t src_len, int64_t block)
{
    const int64_t cap = streams_chunk_cap(n, src_len, block);
    Carver c(scratch);
    StreamsEncodeScratch l;
    l.comp = c.take_as<uint8_t>(src_len);
    l.first = c.take_as<int64_t>(8 * n);
    l.total = c.take_as<int64_t>(256);
    l.c_at = c.take_as<int64_t>(8 * cap);
    l.c_len = c.take_as<int32_t>(4 * cap);
    l.result = c.take_as<int32_t>(4 * cap);
    l.offs = c.take_as<int64_t>(8 * (cap + 1));
    l.partial = c.take_as<int64_t>(8 * scan_tiles(cap));               // (cap >= n: both scans fit)
    l.bytes = c.at;
    return l;
}

// streams decode: [lowest failing item, chunk total, compressed total], three per-item arrays, the scans' tile sums, then the two
// tables of max_chunks entries (those of the one-stream path plus each compressed chunk's item)
inline StreamsTables streams_tables(Carver& c, int64_t n, int64_t max_chunks)
{
    StreamsTables t;
    t.t.max_chunks = max_chunks;
    t.t.min_bad = c.take_as<unsigned long long>(256);
    t.totals = (int64_t*)t.t.min_bad + 1;
    t.chunk_base = c.take_as<int64_t>(8 * n);
    t.comp_base = c.take_as<int64_t>(8 * n);
    t.item_bad = c.take_as<unsigned long long>(8 * n);
    t.partial = c.take_as<int64_t>(8 * scan_tiles(n));
    t.t.c_src_off = c.take_as<int64_t>(8 * max_chunks);
    t.t.c_dst_off = c.take_as<int64_t>(8 * max_chunks);
    t.t.c_hdr_off = c.take_as<int64_t>(8 * max_chunks);
    t.t.r_dst_off = c.take_as<int64_t>(8 * max_chunks);
    t.t.r_src_off = c.take_as<int64_t>(8 * max_chunks);
    t.t.c_src_len = c.take_as<int32_t>(4 * max_chunks);
    t.t.c_dst_cap = c.take_as<int32_t>(4 * max_chunks);
    t.t.c_result = c.take_as<int32_t>(4 * max_chunks);
    t.t.r_len = c.take_as<int32_t>(4 * max_chunks);
    t.c_item = c.take_as<int32_t>(4 * max_chunks);
    return t;
}
inline int64_t streams_decode_scratch_bytes(int64_t n, int64_t max_chunks)
{
    if (n <= 0) return 0;                                              // (no item: the calls touch no scratch)
    Carver c;
    streams_tables(c, n, max_chunks);
    return c.at;
}

// ---- the scan --------------------------------------------------------------------------------------------------------------------
// exclusive scan of x[0, n) in place, n > 0; the sum goes to *total (device); partial holds ceil(n / kScanTile) tile sums.  Reduce and
// apply index their tile by blockIdx.x (no grid-stride loop): their grid is the tile count, whoever launches.
template <class B>
void launch_scan(B& be, int64_t* x, int64_t n, int64_t* partial, int64_t* total)
{
    const int64_t tiles = scan_tiles(n);
    be.launch(stream_scan_reduce_kernel, fixed_grid(tiles), kStreamThreads, x, n, partial);
    be.launch(stream_scan_partials_kernel, fixed_grid(1), kStreamThreads, partial, tiles, total);
    be.launch(stream_scan_apply_kernel, fixed_grid(tiles), kStreamThreads, x, n, partial);
}

// ---- LZ4Stream buffers (lz4hip_stream.hpp) ------------------------------------------------------------------------------------------
// a.comp and a.result are the block encoder's to write: chunk k at k * a.block
template <class B>
int stream_encode_run(B& be, const StreamEncodeArgs& a, int mode, int32_t* lens, int64_t* partial, uint8_t* dst, int64_t* dst_len)
{
    be.launch(stream_lens_kernel, stream_grid(a.n), kStreamThreads, lens, a.n, a.src_len, a.block);
    LZ4HIP_FRAMING_TRY(be.last_error());
    // FlushCurrentChunk: outputLength = inputLength per chunk; src_len_all = the block size, the upper bound LZ4HC picks its kernels from
    lz4hip_batch_t b = {};
    b.src = a.src; b.src_stride = a.block; b.src_len = lens;
    b.dst = (void*)a.comp; b.dst_stride = a.block; b.dst_cap = lens;
    b.src_len_all = a.block; b.result = (int32_t*)a.result; b.n_blocks = a.n;
    LZ4HIP_FRAMING_TRY(be.encode(&b, mode));
    be.launch(stream_sizes_kernel, stream_grid(a.n), kStreamThreads, a);
    launch_scan(be, a.offs, a.n, partial, dst_len);
    EncodeLayout layout = { a };
    be.launch(stream_pack_kernel, copy_grid(stream_bound(a.src_len, a.block)), kStreamThreads, layout, dst, dst_len);
    return be.last_error();
}

template <class B>
int stream_encode(B& be, const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len,
                  void* scratch, int64_t scratch_bytes)
{
    if (src_len < 0 || !dst_len) return be.fail(LZ4HIP_E_ARGUMENT, "stream encode: src_len < 0 or dst_len is NULL");
    if (mode != LZ4HIP_MODE_FAST && mode != LZ4HIP_MODE_HC) return be.fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    const int64_t block = stream_block(block_size), n = stream_chunks(src_len, block);
    if (n > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "stream encode: more than 2^31 - 1 chunks");
    if (dst_cap < stream_bound(src_len, block_size)) return be.fail(LZ4HIP_E_ARGUMENT, "stream encode: dst_cap < lz4hip_stream_bound");
    const StreamEncodeScratch l = stream_encode_scratch(scratch, src_len, block);
    if (scratch_bytes < l.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "stream encode: scratch_bytes < lz4hip_stream_encode_scratch_bytes");
    if (n == 0) return be.fill(dst_len, 0, sizeof(int64_t));
    if (!src || !dst || !scratch) return be.fail(LZ4HIP_E_ARGUMENT, "stream encode: src, dst and scratch must be non-NULL");
    StreamEncodeArgs a;
    a.src = (const uint8_t*)src; a.comp = l.comp; a.src_len = src_len; a.n = n; a.block = (int32_t)block;
    a.hc_flag = mode == LZ4HIP_MODE_HC ? kChunkHighCompression : 0u; a.result = l.result; a.offs = l.offs;
    return stream_encode_run(be, a, mode, l.lens, l.partial, (uint8_t*)dst, dst_len);
}

template <class B>
int stream_index_run(B& be, const uint8_t* src, int64_t src_len, const StreamTables& t, StreamInfo* info)
{
    be.launch(stream_index_kernel, fixed_grid(1), 64, src, src_len, t, info);
    return be.last_error();
}

template <class B>
int stream_index(B& be, const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes, lz4hip_stream_info_t* info)
{
    if (src_len < 0 || max_chunks < 0 || !info || !scratch || (src_len > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "stream index: negative size or NULL pointer");
    Carver c(scratch);
    const StreamTables t = stream_tables(c, max_chunks);
    if (scratch_bytes < c.at) return be.fail(LZ4HIP_E_ARGUMENT, "stream index: scratch_bytes < lz4hip_stream_decode_scratch_bytes");
    return stream_index_run(be, (const uint8_t*)src, src_len, t, (StreamInfo*)info);
}

// The walk of the index, kept in the caller's own arrays of max_chunks + 1 entries each (no scratch): see stream_directory_kernel
template <class B>
int stream_directory_check(B& be, const void* src, int64_t src_len, int64_t max_chunks, const int64_t* hdr_off, const int64_t* out_off,
                           const lz4hip_stream_info_t* info)
{
    if (src_len < 0 || max_chunks < 0 || !hdr_off || !out_off || !info || (src_len > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "stream directory: negative size or NULL pointer");
    return 0;
}

template <class B>
int stream_directory_run(B& be, const void* src, int64_t src_len, int64_t max_chunks, int64_t* hdr_off, int64_t* out_off, lz4hip_stream_info_t* info)
{
    be.launch(stream_directory_kernel, fixed_grid(1), 64, (const uint8_t*)src, src_len, max_chunks, hdr_off, out_off, (StreamInfo*)info);
    return be.last_error();
}

template <class B>
int stream_directory(B& be, const void* src, int64_t src_len, int64_t max_chunks, int64_t* hdr_off, int64_t* out_off, lz4hip_stream_info_t* info)
{
    LZ4HIP_FRAMING_TRY(stream_directory_check(be, src, src_len, max_chunks, hdr_off, out_off, info));
    return stream_directory_run(be, src, src_len, max_chunks, hdr_off, out_off, info);
}

// h: what the index reported, read back by the host
template <class B>
int stream_decode_run(B& be, const uint8_t* src, const StreamInfo& h, const StreamTables& t, uint8_t* dst, StreamInfo* info)
{
    be.launch(stream_info_init_kernel, fixed_grid(1), 64, h, info, t.min_bad);
    LZ4HIP_FRAMING_TRY(be.last_error());
    if (h.compressed_chunks > 0) {
        // AcquireNextChunk: Decode(..., knownOutputLength: true) -- the compressed table IS the batch
        lz4hip_batch_t b = {};
        b.src = src; b.src_off = t.c_src_off; b.src_len = t.c_src_len;
        b.dst = dst; b.dst_off = t.c_dst_off; b.dst_cap = t.c_dst_cap;
        b.result = t.c_result; b.n_blocks = h.compressed_chunks;
        LZ4HIP_FRAMING_TRY(be.decode(&b, 1));
        be.launch(stream_check_kernel, stream_grid(h.compressed_chunks), kStreamThreads, t, h.compressed_chunks);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    if (h.chunks > h.compressed_chunks) {
        RawLayout layout = { src, t, h.chunks - h.compressed_chunks };
        be.launch(stream_raw_copy_kernel, copy_grid(h.decoded_bytes), kStreamThreads, layout, dst, h.decoded_bytes);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    be.launch(stream_info_finish_kernel, fixed_grid(1), 64, info, t.min_bad);
    return be.last_error();
}

template <class B>
int stream_decode(B& be, const void* src, const lz4hip_stream_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                  void* dst, int64_t dst_cap, lz4hip_stream_info_t* info)
{
    if (!info_host || !info || !scratch || max_chunks < 0) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: NULL pointer or max_chunks < 0");
    const lz4hip_stream_info_t h = *info_host;
    if (h.error != LZ4HIP_STREAM_OK && h.error != LZ4HIP_STREAM_END_OF_STREAM && h.error != LZ4HIP_STREAM_PASSES)
        return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: the index reported a table too small (or the info is not an index's)");
    if (h.chunks < 0 || h.chunks > max_chunks || h.compressed_chunks < 0 || h.compressed_chunks > h.chunks || h.decoded_bytes < 0)
        return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: the info does not fit a table of max_chunks entries");
    if (h.decoded_bytes > dst_cap) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: decoded_bytes > dst_cap");
    if (h.chunks > 0 && (!src || !dst)) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: src and dst must be non-NULL");
    Carver c(scratch);
    const StreamTables t = stream_tables(c, max_chunks);
    if (scratch_bytes < c.at) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: scratch_bytes < lz4hip_stream_decode_scratch_bytes");
    if (h.compressed_chunks > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: more than 2^31 - 1 compressed chunks");
    StreamInfo from_index;
    memcpy(&from_index, &h, sizeof from_index);
    return stream_decode_run(be, (const uint8_t*)src, from_index, t, (uint8_t*)dst, (StreamInfo*)info);
}

// The one-call decode: the index's tables, then the decoder's own copy of the length and capacity columns.  The stand-in for a
// written_bytes the caller left out is the second qword of the tables' first piece.
struct StreamIntoScratch { StreamTables t; int32_t* s_src_len; int32_t* s_dst_cap; int64_t bytes; };
inline StreamIntoScratch stream_into_scratch(void* scratch, int64_t max_chunks)
{
    Carver c(scratch);
    StreamIntoScratch l;
    l.t = stream_tables(c, max_chunks);
    l.s_src_len = c.take_as<int32_t>(4 * max_chunks);
    l.s_dst_cap = c.take_as<int32_t>(4 * max_chunks);
    l.bytes = c.at;
    return l;
}
inline int64_t stream_decode_into_scratch_bytes(int64_t max_chunks) { return stream_into_scratch(nullptr, max_chunks).bytes; }

// `any`: an address for the rows of a decoder call that has no source or no output (all of them empty then)
struct StreamIntoPlan { const uint8_t* src; int64_t src_len; StreamClip clip; uint8_t* dst; StreamInfo* info; uint8_t* any; };

// The index as it is, then everything the two-call decode does, over ALL max_chunks rows and with the counts and the output's end taken
// from the device.  The offset columns the decoder reads are zeroed first: a row past the count is an empty block at offset 0.
template <class B>
int stream_decode_into_run(B& be, const StreamIntoPlan& p)
{
    const StreamTables& t = p.clip.t;
    LZ4HIP_FRAMING_TRY(be.fill(p.clip.written, 0, 8));
    LZ4HIP_FRAMING_TRY(be.fill(t.min_bad, 0xFF, 8));                   // min_bad = none
    if (t.max_chunks > 0) {
        LZ4HIP_FRAMING_TRY(be.fill(t.c_src_off, 0, (size_t)(8 * t.max_chunks)));
        LZ4HIP_FRAMING_TRY(be.fill(t.c_dst_off, 0, (size_t)(8 * t.max_chunks)));
    }
    LZ4HIP_FRAMING_TRY(stream_index_run(be, p.src, p.src_len, t, p.info));
    if (t.max_chunks > 0) {
        be.launch(stream_clip_kernel, stream_grid(t.max_chunks), kStreamThreads, p.clip, (const StreamInfo*)p.info);
        LZ4HIP_FRAMING_TRY(be.last_error());
        // AcquireNextChunk: Decode(..., knownOutputLength: true) -- the whole compressed table IS the batch
        lz4hip_batch_t b = {};
        b.src = p.src ? p.src : p.any; b.src_off = t.c_src_off; b.src_len = p.clip.s_src_len;
        b.dst = p.dst ? p.dst : p.any; b.dst_off = t.c_dst_off; b.dst_cap = p.clip.s_dst_cap;
        b.result = t.c_result; b.n_blocks = t.max_chunks;
        LZ4HIP_FRAMING_TRY(be.decode(&b, 1));
        const int64_t* counts = &p.info->chunks;
        be.launch(stream_check_into_kernel, stream_grid(t.max_chunks), kStreamThreads, t, (const int32_t*)p.clip.s_dst_cap, counts);
        RawLayout layout = { p.src, t, 0 };
        const int64_t most = p.src_len < p.clip.dst_cap / 255 ? p.src_len * 255 : p.clip.dst_cap;   // (an LZ4 block grows 255 times at most)
        be.launch(stream_raw_copy_into_kernel, copy_grid(most), kStreamThreads, layout, p.dst, counts, (const int64_t*)p.clip.written);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    be.launch(stream_info_finish_kernel, fixed_grid(1), 64, p.info, (const unsigned long long*)t.min_bad);
    return be.last_error();
}

template <class B>
int stream_decode_into_plan(B& be, const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst,
                            int64_t dst_cap, lz4hip_stream_info_t* info, int64_t* written_bytes, StreamIntoPlan& p)
{
    if (src_len < 0 || max_chunks < 0 || dst_cap < 0 || !info || !scratch || (src_len > 0 && !src) || (dst_cap > 0 && !dst))
        return be.fail(LZ4HIP_E_ARGUMENT, "stream decode into: negative size or NULL pointer");
    if (max_chunks > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode into: more than 2^31 - 1 table rows");
    const StreamIntoScratch l = stream_into_scratch(scratch, max_chunks);
    if (scratch_bytes < l.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode into: scratch_bytes < lz4hip_stream_decode_into_scratch_bytes");
    p.src = (const uint8_t*)src; p.src_len = src_len; p.dst = (uint8_t*)dst; p.info = (StreamInfo*)info; p.any = (uint8_t*)scratch;
    p.clip.t = l.t; p.clip.s_src_len = l.s_src_len; p.clip.s_dst_cap = l.s_dst_cap; p.clip.dst_cap = dst_cap;
    p.clip.written = written_bytes ? (unsigned long long*)written_bytes : l.t.min_bad + 1;
    return 0;
}

template <class B>
int stream_decode_into(B& be, const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst,
                       int64_t dst_cap, lz4hip_stream_info_t* info, int64_t* written_bytes)
{
    StreamIntoPlan p;
    LZ4HIP_FRAMING_TRY(stream_decode_into_plan(be, src, src_len, max_chunks, scratch, scratch_bytes, dst, dst_cap, info, written_bytes, p));
    return stream_decode_into_run(be, p);
}

// ---- wrapped messages (lz4hip_wrap.hpp) ---------------------------------------------------------------------------------------------
// a.comp and a.enc are the block encoder's to write: message i at a.off[i]
template <class B>
int wrap_encode_run(B& be, const WrapArgs& a, int mode, int64_t* at, int32_t* lens, int32_t* result, int64_t* partial, uint8_t* dst, int64_t dst_cap)
{
    be.launch(wrap_lens_kernel, stream_grid(a.n), kStreamThreads, a.off, a.n, a.src_len, at, lens);
    LZ4HIP_FRAMING_TRY(be.last_error());
    // Wrap: outputLength = inputLength per message, written at the message's own offset; src_len_all = 0 (no bound is known on the host)
    lz4hip_batch_t b = {};
    b.src = a.src; b.src_off = at; b.src_len = lens;
    b.dst = (void*)a.comp; b.dst_off = at; b.dst_cap = lens;
    b.src_len_all = 0; b.result = (int32_t*)a.enc; b.n_blocks = a.n;
    LZ4HIP_FRAMING_TRY(be.encode(&b, mode));
    be.launch(wrap_sizes_kernel, stream_grid(a.n), kStreamThreads, a, result);
    launch_scan(be, a.dst_off, a.n, partial, a.dst_off + a.n);
    WrapLayout layout = { a };
    be.launch(wrap_pack_kernel, copy_grid(wrap_bound(a.n, a.src_len)), kStreamThreads, layout, dst, dst_cap);
    return be.last_error();
}

template <class B>
int wrap_encode(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode, void* dst, int64_t dst_cap, int64_t* dst_off,
                int32_t* result, void* scratch, int64_t scratch_bytes)
{
    if (src_len < 0 || n < 0 || !dst_off) return be.fail(LZ4HIP_E_ARGUMENT, "wrap: src_len < 0, n < 0 or dst_off is NULL");
    if (mode != LZ4HIP_MODE_FAST && mode != LZ4HIP_MODE_HC) return be.fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    if (n > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "wrap: more than 2^31 - 1 messages");
    if (dst_cap < wrap_bound(n, src_len)) return be.fail(LZ4HIP_E_ARGUMENT, "wrap: dst_cap < lz4hip_wrap_bound");
    if (n == 0) return be.fill(dst_off, 0, sizeof(int64_t));
    const WrapScratch l = wrap_scratch(scratch, n, src_len);
    if (scratch_bytes < l.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "wrap: scratch_bytes < lz4hip_wrap_scratch_bytes");
    if ((src_len > 0 && !src) || !src_off || !dst || !scratch) return be.fail(LZ4HIP_E_ARGUMENT, "wrap: src, src_off, dst and scratch must be non-NULL");
    WrapArgs a;
    a.src = (const uint8_t*)src; a.comp = l.comp; a.off = src_off; a.src_len = src_len; a.n = n; a.enc = l.enc; a.dst_off = dst_off;
    return wrap_encode_run(be, a, mode, l.at, l.lens, result, l.partial, (uint8_t*)dst, dst_cap);
}

// `end`: NULL for consecutive messages (a.off has n + 1 entries), else the n ends of the spans that begin at a.off[i]
template <class B>
int unwrap_index_run(B& be, const UnwrapArgs& a, const UnwrapTables& t, UnwrapInfo* info, const int64_t* end = nullptr)
{
    LZ4HIP_FRAMING_TRY(be.fill(t.min_bad, 0xFF, 8));                   // min_bad = none
    LZ4HIP_FRAMING_TRY(be.fill(t.ncomp, 0, 8));
    if (a.n == 0) {
        LZ4HIP_FRAMING_TRY(be.fill(a.dst_off, 0, sizeof(int64_t)));
    } else {
        if (end) be.launch(unwrap_index_spans_kernel, stream_grid(a.n), kStreamThreads, a, t, end);
        else be.launch(unwrap_index_kernel, stream_grid(a.n), kStreamThreads, a, t);
        launch_scan(be, a.dst_off, a.n, t.partial, a.dst_off + a.n);
        launch_scan(be, t.cidx, a.n, t.partial, t.ncomp);
        be.launch(unwrap_compact_kernel, stream_grid(a.n), kStreamThreads, a, t);
    }
    be.launch(unwrap_info_kernel, fixed_grid(1), 64, a, t, info);
    return be.last_error();
}

template <class B>
int unwrap_index(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t* dst_off, int32_t* status,
                 void* scratch, int64_t scratch_bytes, lz4hip_unwrap_info_t* info)
{
    if (src_len < 0 || n < 0 || !dst_off || !info || !scratch) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap index: negative size or NULL pointer");
    if (n > 0 && (!src_off || !status || (src_len > 0 && !src))) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap index: NULL pointer");
    Carver c(scratch);
    const UnwrapTables t = unwrap_tables(c, n);
    if (scratch_bytes < c.at) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap index: scratch_bytes < lz4hip_unwrap_scratch_bytes");
    const UnwrapArgs a = { (const uint8_t*)src, src_off, src_len, n, dst_off, status };
    return unwrap_index_run(be, a, t, (UnwrapInfo*)info);
}

// h: what the index reported, read back by the host; the tables are as the index left them
template <class B>
int unwrap_decode_run(B& be, const UnwrapArgs& a, const UnwrapTables& t, const UnwrapInfo& h, uint8_t* dst, UnwrapInfo* info)
{
    if (h.compressed > 0) {
        // Unwrap: Decode(..., outputLength, knownOutputLength: true) -- the compacted table IS the batch
        lz4hip_batch_t b = {};
        b.src = a.src; b.src_off = t.c_src_off; b.src_len = t.c_src_len;
        b.dst = dst; b.dst_off = t.c_dst_off; b.dst_cap = t.c_dst_cap;
        b.result = t.c_result; b.n_blocks = h.compressed;
        LZ4HIP_FRAMING_TRY(be.decode(&b, 1));
    }
    if (a.n > h.compressed && h.decoded_bytes > 0) {
        UnwrapRawLayout layout = { a, t };
        be.launch(wrap_raw_copy_kernel, copy_grid(h.decoded_bytes), kStreamThreads, layout, dst, h.decoded_bytes);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    if (h.compressed > 0) be.launch(unwrap_check_kernel, stream_grid(h.compressed), kStreamThreads, t, h.compressed, a.status);
    be.launch(unwrap_info_kernel, fixed_grid(1), 64, a, t, info);
    return be.last_error();
}

template <class B>
int unwrap_decode(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const lz4hip_unwrap_info_t* info_host, void* scratch,
                  int64_t scratch_bytes, void* dst, int64_t dst_cap, const int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info)
{
    if (!info_host || !info || !scratch || !dst_off || src_len < 0 || n < 0) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap decode: negative size or NULL pointer");
    const lz4hip_unwrap_info_t h = *info_host;
    if (h.messages != n || h.compressed < 0 || h.compressed > n || h.decoded_bytes < 0)
        return be.fail(LZ4HIP_E_ARGUMENT, "unwrap decode: the info is not the index's of these n messages");
    if (h.decoded_bytes > dst_cap) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap decode: decoded_bytes > dst_cap");
    if (n > 0 && (!src_off || !status || (src_len > 0 && !src))) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap decode: NULL pointer");
    if (h.decoded_bytes > 0 && !dst) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap decode: dst is NULL");
    Carver c(scratch);
    const UnwrapTables t = unwrap_tables(c, n);
    if (scratch_bytes < c.at) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap decode: scratch_bytes < lz4hip_unwrap_scratch_bytes");
    if (h.compressed > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap decode: more than 2^31 - 1 compressed messages");
    const UnwrapArgs a = { (const uint8_t*)src, src_off, src_len, n, (int64_t*)dst_off, status };
    UnwrapInfo from_index;
    memcpy(&from_index, &h, sizeof from_index);
    return unwrap_decode_run(be, a, t, from_index, (uint8_t*)dst, (UnwrapInfo*)info);
}

// The one-call unwrap: the index's tables, then the decoder's own copy of the length and capacity columns.  The prefix's end, and the
// stand-in for a written_messages the caller left out, are the third and fourth qword of the tables' first piece.
struct UnwrapIntoScratch { UnwrapTables t; int32_t* s_src_len; int32_t* s_dst_cap; int64_t bytes; };
inline UnwrapIntoScratch unwrap_into_scratch(void* scratch, int64_t n)
{
    Carver c(scratch);
    UnwrapIntoScratch l;
    l.t = unwrap_tables(c, n);
    l.s_src_len = c.take_as<int32_t>(4 * n);
    l.s_dst_cap = c.take_as<int32_t>(4 * n);
    l.bytes = c.at;
    return l;
}
inline int64_t unwrap_into_scratch_bytes(int64_t n) { return unwrap_into_scratch(nullptr, n).bytes; }

// `end`: NULL for consecutive messages, else the span form's ends (a.off holds the begins)
struct UnwrapIntoPlan { UnwrapArgs a; UnwrapClip clip; uint8_t* dst; UnwrapInfo* info; uint8_t* any; const int64_t* end = nullptr; };

// The index as it is, then the two-call decode's steps over ALL n rows of the table, the count and the output's end taken from the device.
// Consecutive messages and spans are this one sequence: only the index kernel and the raw copy's grid know the difference.
template <class B>
int unwrap_into_run(B& be, const UnwrapIntoPlan& p)
{
    const UnwrapArgs& a = p.a;
    const UnwrapTables& t = p.clip.t;
    LZ4HIP_FRAMING_TRY(be.fill(p.clip.written_messages, 0, 8));
    LZ4HIP_FRAMING_TRY(be.fill(p.clip.written_end, 0, 8));
    if (a.n > 0) {
        LZ4HIP_FRAMING_TRY(be.fill(t.c_src_off, 0, (size_t)(8 * a.n)));
        LZ4HIP_FRAMING_TRY(be.fill(t.c_dst_off, 0, (size_t)(8 * a.n)));
    }
    LZ4HIP_FRAMING_TRY(unwrap_index_run(be, a, t, p.info, p.end));
    if (a.n == 0) return 0;
    be.launch(unwrap_clip_kernel, stream_grid(a.n), kStreamThreads, a, p.clip);
    LZ4HIP_FRAMING_TRY(be.last_error());
    // Unwrap: Decode(..., outputLength, knownOutputLength: true) -- the whole table IS the batch
    lz4hip_batch_t b = {};
    b.src = a.src ? a.src : p.any; b.src_off = t.c_src_off; b.src_len = p.clip.s_src_len;
    b.dst = p.dst ? p.dst : p.any; b.dst_off = t.c_dst_off; b.dst_cap = p.clip.s_dst_cap;
    b.result = t.c_result; b.n_blocks = a.n;
    LZ4HIP_FRAMING_TRY(be.decode(&b, 1));
    UnwrapRawLayout layout = { a, t };
    // (an LZ4 block grows 255 times at most; spans may repeat, so their output has no bound in src_len)
    const int64_t most = !p.end && a.src_len < p.clip.dst_cap / 255 ? a.src_len * 255 : p.clip.dst_cap;
    be.launch(wrap_raw_copy_into_kernel, copy_grid(most), kStreamThreads, layout, p.dst, (const int64_t*)p.clip.written_end);
    be.launch(unwrap_check_into_kernel, stream_grid(a.n), kStreamThreads, t, (const int32_t*)p.clip.s_dst_cap, a.status);
    be.launch(unwrap_info_kernel, fixed_grid(1), 64, a, t, p.info);
    return be.last_error();
}

template <class B>
int unwrap_into_plan(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* scratch, int64_t scratch_bytes, void* dst,
                     int64_t dst_cap, int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info, int64_t* written_messages, UnwrapIntoPlan& p)
{
    if (src_len < 0 || n < 0 || dst_cap < 0 || !dst_off || !info || !scratch || (dst_cap > 0 && !dst))
        return be.fail(LZ4HIP_E_ARGUMENT, "unwrap into: negative size or NULL pointer");
    if (n > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap into: more than 2^31 - 1 messages");
    if (n > 0 && (!src_off || !status || (src_len > 0 && !src))) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap into: NULL pointer");
    const UnwrapIntoScratch l = unwrap_into_scratch(scratch, n);
    if (scratch_bytes < l.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap into: scratch_bytes < lz4hip_unwrap_into_scratch_bytes");
    p.a = { (const uint8_t*)src, src_off, src_len, n, dst_off, status };
    p.dst = (uint8_t*)dst; p.info = (UnwrapInfo*)info; p.any = (uint8_t*)scratch;
    p.clip.t = l.t; p.clip.s_src_len = l.s_src_len; p.clip.s_dst_cap = l.s_dst_cap; p.clip.dst_cap = dst_cap;
    p.clip.written_end = (int64_t*)l.t.min_bad + 2;
    p.clip.written_messages = written_messages ? written_messages : (int64_t*)l.t.min_bad + 3;
    return 0;
}

template <class B>
int unwrap_into(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* scratch, int64_t scratch_bytes, void* dst,
                int64_t dst_cap, int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info, int64_t* written_messages)
{
    UnwrapIntoPlan p;
    LZ4HIP_FRAMING_TRY(unwrap_into_plan(be, src, src_len, src_off, n, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info, written_messages, p));
    return unwrap_into_run(be, p);
}

// The span form: message j is src[src_begin[j], src_end[j]); everything else is unwrap_into's, with m in the place of n
template <class B>
int unwrap_spans_into_plan(B& be, const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m, void* scratch,
                           int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info,
                           int64_t* written_messages, UnwrapIntoPlan& p)
{
    if (m > 0 && !src_end) return be.fail(LZ4HIP_E_ARGUMENT, "unwrap spans into: NULL pointer");
    LZ4HIP_FRAMING_TRY(unwrap_into_plan(be, src, src_len, src_begin, m, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info, written_messages, p));
    p.end = m > 0 ? src_end : nullptr;
    return 0;
}

template <class B>
int unwrap_spans_into(B& be, const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m, void* scratch,
                      int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info,
                      int64_t* written_messages)
{
    UnwrapIntoPlan p;
    LZ4HIP_FRAMING_TRY(unwrap_spans_into_plan(be, src, src_len, src_begin, src_end, m, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info,
                                              written_messages, p));
    return unwrap_into_run(be, p);
}

// begin[j] = src_off[sel[j]], end[j] = src_off[sel[j] + 1], or (-1, -1) for a sel[j] outside [0, n): one launch, no scratch
template <class B>
int spans_select_check(B& be, const int64_t* src_off, int64_t n, const int64_t* sel, int64_t m, const int64_t* src_begin, const int64_t* src_end)
{
    if (n < 0 || m < 0) return be.fail(LZ4HIP_E_ARGUMENT, "spans select: n < 0 or m < 0");
    if (m > 0 && (!sel || !src_begin || !src_end || (n > 0 && !src_off))) return be.fail(LZ4HIP_E_ARGUMENT, "spans select: NULL pointer");
    return 0;
}

template <class B>
int spans_select_run(B& be, const int64_t* src_off, int64_t n, const int64_t* sel, int64_t m, int64_t* src_begin, int64_t* src_end)
{
    if (m == 0) return 0;
    be.launch(spans_select_kernel, stream_grid(m), kStreamThreads, src_off, n, sel, m, src_begin, src_end);
    return be.last_error();
}

template <class B>
int spans_select(B& be, const int64_t* src_off, int64_t n, const int64_t* sel, int64_t m, int64_t* src_begin, int64_t* src_end)
{
    LZ4HIP_FRAMING_TRY(spans_select_check(be, src_off, n, sel, m, src_begin, src_end));
    return spans_select_run(be, src_off, n, sel, m, src_begin, src_end);
}

// ---- batches of LZ4Stream buffers (lz4hip_streams.hpp) --------------------------------------------------------------------------------
// Many independent streams per call: the framing kernels of the one-stream path and its scan and copy routine, around ONE block
// encoder / decoder call over the chunks of all items.  The encode sequence comes in two parts around the encoder: the chunk table
// (a.first, *a.total, a.c_at, a.c_len), then -- a.comp and a.result written, every chunk at its own source position -- the pack.
template <class B>
int streams_encode_plan(B& be, const StreamsEncodeArgs& a, int64_t* partial)
{
    be.launch(streams_counts_kernel, stream_grid(a.n), kStreamThreads, a);
    launch_scan(be, a.first, a.n, partial, (int64_t*)a.total);
    be.launch(streams_chunks_kernel, stream_grid(a.cap), kStreamThreads, a);
    return be.last_error();
}

template <class B>
int streams_encode_pack(B& be, const StreamsEncodeArgs& a, int64_t* partial, int64_t* dst_off, uint8_t* dst, int64_t dst_cap)
{
    be.launch(streams_sizes_kernel, stream_grid(a.cap), kStreamThreads, a);
    launch_scan(be, a.offs, a.cap, partial, a.offs + a.cap);
    be.launch(streams_offsets_kernel, stream_grid(a.n + 1), kStreamThreads, a, dst_off);
    StreamsEncodeLayout layout = { a };
    be.launch(streams_pack_kernel, copy_grid(streams_bound(a.n, a.src_len, a.block)), kStreamThreads, layout, dst, dst_cap);
    return be.last_error();
}

template <class B>
int streams_encode(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode, void* dst,
                   int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes)
{
    if (src_len < 0 || n < 0 || !dst_off) return be.fail(LZ4HIP_E_ARGUMENT, "streams encode: src_len < 0, n < 0 or dst_off is NULL");
    if (mode != LZ4HIP_MODE_FAST && mode != LZ4HIP_MODE_HC) return be.fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    const int64_t block = stream_block(block_size), cap = streams_chunk_cap(n, src_len, block);
    if (n > 0x7FFFFFFF || cap > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "streams encode: more than 2^31 - 1 items or chunks");
    if (n > 0 && dst_cap < streams_bound(n, src_len, block_size)) return be.fail(LZ4HIP_E_ARGUMENT, "streams encode: dst_cap < lz4hip_streams_bound");
    if (n == 0 || src_len == 0) return be.fill(dst_off, 0, sizeof(int64_t) * (size_t)(n + 1));
    const StreamsEncodeScratch l = streams_encode_scratch(scratch, n, src_len, block);
    if (scratch_bytes < l.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "streams encode: scratch_bytes < lz4hip_streams_encode_scratch_bytes");
    if (!src || !src_off || !dst || !scratch) return be.fail(LZ4HIP_E_ARGUMENT, "streams encode: src, src_off, dst and scratch must be non-NULL");
    StreamsEncodeArgs a;
    a.src = (const uint8_t*)src; a.comp = l.comp; a.off = src_off; a.src_len = src_len; a.n = n; a.cap = cap; a.block = (int32_t)block;
    a.hc_flag = mode == LZ4HIP_MODE_HC ? kChunkHighCompression : 0u;
    a.first = l.first; a.total = l.total; a.c_at = l.c_at; a.c_len = l.c_len; a.result = l.result; a.offs = l.offs;
    LZ4HIP_FRAMING_TRY(streams_encode_plan(be, a, l.partial));
    // FlushCurrentChunk: outputLength = inputLength per chunk, written at the chunk's own source position; src_len_all = the block size,
    // the upper bound LZ4HC picks its kernels from
    lz4hip_batch_t b = {};
    b.src = src; b.src_off = a.c_at; b.src_len = a.c_len;
    b.dst = l.comp; b.dst_off = a.c_at; b.dst_cap = a.c_len;
    b.src_len_all = (int32_t)block; b.result = l.result; b.n_blocks = cap;
    LZ4HIP_FRAMING_TRY(be.encode(&b, mode));
    return streams_encode_pack(be, a, l.partial, dst_off, (uint8_t*)dst, dst_cap);
}

// no item: no table, nothing to walk
template <class B>
int streams_empty_info(B& be, StreamsInfo* info)
{
    be.launch(streams_empty_info_kernel, fixed_grid(1), 64, info);
    return be.last_error();
}

// `end`: NULL for consecutive items (a.off has n + 1 entries), else the n ends of the spans that begin at a.off[i]
template <class B>
int streams_index_run(B& be, const StreamsDecodeArgs& a, const StreamsTables& t, StreamsInfo* info, const int64_t* end = nullptr)
{
    LZ4HIP_FRAMING_TRY(be.fill(t.totals, 0, 16));
    LZ4HIP_FRAMING_TRY(be.fill(t.t.min_bad, 0xFF, 8));                 // min_bad = none
    if (end) be.launch(streams_walk_spans_kernel<false>, walk_grid(a.n), 64, a, t, end);
    else be.launch(streams_walk_kernel<false>, walk_grid(a.n), 64, a, t);
    launch_scan(be, a.dst_off, a.n, t.partial, a.dst_off + a.n);
    launch_scan(be, t.chunk_base, a.n, t.partial, t.totals);
    launch_scan(be, t.comp_base, a.n, t.partial, t.totals + 1);
    if (end) be.launch(streams_walk_spans_kernel<true>, walk_grid(a.n), 64, a, t, end);
    else be.launch(streams_walk_kernel<true>, walk_grid(a.n), 64, a, t);
    be.launch(streams_info_kernel, fixed_grid(1), 64, a, t, info);
    return be.last_error();
}

template <class B>
int streams_index(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks, int64_t* dst_off, int32_t* status,
                  int64_t* error_offset, void* scratch, int64_t scratch_bytes, lz4hip_streams_info_t* info)
{
    if (src_len < 0 || n < 0 || max_chunks < 0 || !dst_off || !info) return be.fail(LZ4HIP_E_ARGUMENT, "streams index: negative size or NULL pointer");
    if (n > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "streams index: more than 2^31 - 1 items");
    if (n > 0 && (!src_off || !status || !error_offset || !scratch || (src_len > 0 && !src))) return be.fail(LZ4HIP_E_ARGUMENT, "streams index: NULL pointer");
    if (scratch_bytes < streams_decode_scratch_bytes(n, max_chunks))
        return be.fail(LZ4HIP_E_ARGUMENT, "streams index: scratch_bytes < lz4hip_streams_decode_scratch_bytes");
    if (n == 0) {
        LZ4HIP_FRAMING_TRY(be.fill(dst_off, 0, sizeof(int64_t)));
        return streams_empty_info(be, (StreamsInfo*)info);
    }
    Carver c(scratch);
    const StreamsTables t = streams_tables(c, n, max_chunks);
    const StreamsDecodeArgs a = { (const uint8_t*)src, src_off, src_len, n, dst_off, status, error_offset };
    return streams_index_run(be, a, t, (StreamsInfo*)info);
}

// h: what the index reported, read back by the host; the tables are as the index left them
template <class B>
int streams_decode_run(B& be, const StreamsDecodeArgs& a, const StreamsTables& t, const StreamsInfo& h, uint8_t* dst, StreamsInfo* info)
{
    LZ4HIP_FRAMING_TRY(be.fill(t.t.min_bad, 0xFF, 8));
    LZ4HIP_FRAMING_TRY(be.fill(t.item_bad, 0xFF, (size_t)(8 * a.n)));
    if (h.compressed_chunks > 0) {
        // AcquireNextChunk: Decode(..., knownOutputLength: true) -- the compressed table of all items IS the batch
        lz4hip_batch_t b = {};
        b.src = a.src; b.src_off = t.t.c_src_off; b.src_len = t.t.c_src_len;
        b.dst = dst; b.dst_off = t.t.c_dst_off; b.dst_cap = t.t.c_dst_cap;
        b.result = t.t.c_result; b.n_blocks = h.compressed_chunks;
        LZ4HIP_FRAMING_TRY(be.decode(&b, 1));
        be.launch(streams_check_kernel, stream_grid(h.compressed_chunks), kStreamThreads, t, h.compressed_chunks);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    if (h.chunks > h.compressed_chunks) {
        RawLayout layout = { a.src, t.t, h.chunks - h.compressed_chunks };
        be.launch(stream_raw_copy_kernel, copy_grid(h.decoded_bytes), kStreamThreads, layout, dst, h.decoded_bytes);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    be.launch(streams_finish_kernel, stream_grid(a.n), kStreamThreads, a, t);
    be.launch(streams_info_kernel, fixed_grid(1), 64, a, t, info);
    return be.last_error();
}

template <class B>
int streams_decode(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const lz4hip_streams_info_t* info_host,
                   int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, const int64_t* dst_off, int32_t* status,
                   int64_t* error_offset, lz4hip_streams_info_t* info)
{
    if (!info_host || !info || !dst_off || src_len < 0 || n < 0 || max_chunks < 0) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: negative size or NULL pointer");
    const lz4hip_streams_info_t h = *info_host;
    if (h.error == LZ4HIP_STREAM_TABLE_FULL) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: the index reported tables too small");
    if (h.items != n || h.chunks < 0 || h.chunks > max_chunks || h.compressed_chunks < 0 || h.compressed_chunks > h.chunks || h.decoded_bytes < 0)
        return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: the info is not the index's of these n items and max_chunks entries");
    if (h.decoded_bytes > dst_cap) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: decoded_bytes > dst_cap");
    if (n > 0 && (!src_off || !status || !error_offset || !scratch || (src_len > 0 && !src))) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: NULL pointer");
    if (h.decoded_bytes > 0 && !dst) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: dst is NULL");
    if (scratch_bytes < streams_decode_scratch_bytes(n, max_chunks))
        return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: scratch_bytes < lz4hip_streams_decode_scratch_bytes");
    if (h.compressed_chunks > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: more than 2^31 - 1 compressed chunks");
    if (n == 0) return streams_empty_info(be, (StreamsInfo*)info);
    Carver c(scratch);
    const StreamsTables t = streams_tables(c, n, max_chunks);
    const StreamsDecodeArgs a = { (const uint8_t*)src, src_off, src_len, n, (int64_t*)dst_off, status, error_offset };
    StreamsInfo from_index;
    memcpy(&from_index, &h, sizeof from_index);
    return streams_decode_run(be, a, t, from_index, (uint8_t*)dst, (StreamsInfo*)info);
}

// The one-call decode: the index's tables, then the decoder's own copy of the length and capacity columns.  The prefix's end, and the
// stand-in for a written_items the caller left out, are the fourth and fifth qword of the tables' first piece.
struct StreamsIntoScratch { StreamsTables t; int32_t* s_src_len; int32_t* s_dst_cap; int64_t bytes; };
inline StreamsIntoScratch streams_into_scratch(void* scratch, int64_t n, int64_t max_chunks)
{
    Carver c(scratch);
    StreamsIntoScratch l;
    l.t = streams_tables(c, n, max_chunks);
    l.s_src_len = c.take_as<int32_t>(4 * max_chunks);
    l.s_dst_cap = c.take_as<int32_t>(4 * max_chunks);
    l.bytes = c.at;
    return l;
}
inline int64_t streams_decode_into_scratch_bytes(int64_t n, int64_t max_chunks)
{
    return n <= 0 ? 0 : streams_into_scratch(nullptr, n, max_chunks).bytes;       // (no item: the call touches no scratch)
}

// a.n == 0: only a.dst_off, info and written are looked at.  `end`: NULL for consecutive items, else the span form's ends (a.off holds
// the begins)
struct StreamsIntoPlan {
    StreamsDecodeArgs a; StreamsClip clip; uint8_t* dst; StreamsInfo* info; int64_t* written; uint8_t* any; const int64_t* end = nullptr;
};

// The index as it is, then the two-call decode's steps over ALL max_chunks rows, the counts and the output's end taken from the device.
// Consecutive items and spans are this one sequence: only the walk kernels and the raw copy's grid know the difference.
template <class B>
int streams_decode_into_run(B& be, const StreamsIntoPlan& p)
{
    const StreamsDecodeArgs& a = p.a;
    if (a.n == 0) {
        LZ4HIP_FRAMING_TRY(be.fill(a.dst_off, 0, sizeof(int64_t)));
        if (p.written) LZ4HIP_FRAMING_TRY(be.fill(p.written, 0, 8));
        return streams_empty_info(be, p.info);
    }
    const StreamsTables& t = p.clip.t;
    const int64_t rows = t.t.max_chunks;
    LZ4HIP_FRAMING_TRY(be.fill(p.clip.written_items, 0, 8));
    LZ4HIP_FRAMING_TRY(be.fill(p.clip.written_end, 0, 8));
    if (rows > 0) {
        LZ4HIP_FRAMING_TRY(be.fill(t.t.c_src_off, 0, (size_t)(8 * rows)));
        LZ4HIP_FRAMING_TRY(be.fill(t.t.c_dst_off, 0, (size_t)(8 * rows)));
    }
    LZ4HIP_FRAMING_TRY(streams_index_run(be, a, t, p.info, p.end));
    LZ4HIP_FRAMING_TRY(be.fill(t.t.min_bad, 0xFF, 8));
    LZ4HIP_FRAMING_TRY(be.fill(t.item_bad, 0xFF, (size_t)(8 * a.n)));
    be.launch(streams_clip_kernel, stream_grid(rows > a.n ? rows : a.n), kStreamThreads, a, p.clip);
    LZ4HIP_FRAMING_TRY(be.last_error());
    if (rows > 0) {
        // AcquireNextChunk: Decode(..., knownOutputLength: true) -- the whole compressed table of all items IS the batch
        lz4hip_batch_t b = {};
        b.src = a.src ? a.src : p.any; b.src_off = t.t.c_src_off; b.src_len = p.clip.s_src_len;
        b.dst = p.dst ? p.dst : p.any; b.dst_off = t.t.c_dst_off; b.dst_cap = p.clip.s_dst_cap;
        b.result = t.t.c_result; b.n_blocks = rows;
        LZ4HIP_FRAMING_TRY(be.decode(&b, 1));
        be.launch(streams_check_into_kernel, stream_grid(rows), kStreamThreads, t, (const int32_t*)p.clip.s_dst_cap);
        RawLayout layout = { a.src, t.t, 0 };
        // (an LZ4 block grows 255 times at most; spans may repeat, so their output has no bound in src_len)
        const int64_t most = !p.end && a.src_len < p.clip.dst_cap / 255 ? a.src_len * 255 : p.clip.dst_cap;
        be.launch(stream_raw_copy_into_kernel, copy_grid(most), kStreamThreads, layout, p.dst, (const int64_t*)t.totals, (const int64_t*)p.clip.written_end);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    be.launch(streams_finish_kernel, stream_grid(a.n), kStreamThreads, a, t);
    be.launch(streams_info_kernel, fixed_grid(1), 64, a, t, p.info);
    return be.last_error();
}

template <class B>
int streams_decode_into_plan(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks, void* scratch,
                             int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status, int64_t* error_offset,
                             lz4hip_streams_info_t* info, int64_t* written_items, StreamsIntoPlan& p)
{
    if (src_len < 0 || n < 0 || max_chunks < 0 || dst_cap < 0 || !dst_off || !info || (dst_cap > 0 && !dst))
        return be.fail(LZ4HIP_E_ARGUMENT, "streams decode into: negative size or NULL pointer");
    if (n > 0x7FFFFFFF || max_chunks > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode into: more than 2^31 - 1 items or table rows");
    if (n > 0 && (!src_off || !status || !error_offset || !scratch || (src_len > 0 && !src))) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode into: NULL pointer");
    if (scratch_bytes < streams_decode_into_scratch_bytes(n, max_chunks))
        return be.fail(LZ4HIP_E_ARGUMENT, "streams decode into: scratch_bytes < lz4hip_streams_decode_into_scratch_bytes");
    p.a = { (const uint8_t*)src, src_off, src_len, n, dst_off, status, error_offset };
    p.dst = (uint8_t*)dst; p.info = (StreamsInfo*)info; p.written = written_items; p.any = (uint8_t*)scratch;
    if (n == 0) return 0;
    const StreamsIntoScratch l = streams_into_scratch(scratch, n, max_chunks);
    p.clip.t = l.t; p.clip.s_src_len = l.s_src_len; p.clip.s_dst_cap = l.s_dst_cap; p.clip.dst_cap = dst_cap;
    p.clip.written_end = (int64_t*)l.t.t.min_bad + 3;
    p.clip.written_items = written_items ? written_items : (int64_t*)l.t.t.min_bad + 4;
    return 0;
}

template <class B>
int streams_decode_into(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks, void* scratch,
                        int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status, int64_t* error_offset,
                        lz4hip_streams_info_t* info, int64_t* written_items)
{
    StreamsIntoPlan p;
    LZ4HIP_FRAMING_TRY(streams_decode_into_plan(be, src, src_len, src_off, n, max_chunks, scratch, scratch_bytes, dst, dst_cap, dst_off, status,
                                                error_offset, info, written_items, p));
    return streams_decode_into_run(be, p);
}

// The span form: item j is src[src_begin[j], src_end[j]); everything else is streams_decode_into's, with m in the place of n
template <class B>
int streams_decode_spans_into_plan(B& be, const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m,
                                   int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off,
                                   int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info, int64_t* written_items, StreamsIntoPlan& p)
{
    if (m > 0 && !src_end) return be.fail(LZ4HIP_E_ARGUMENT, "streams decode spans into: NULL pointer");
    LZ4HIP_FRAMING_TRY(streams_decode_into_plan(be, src, src_len, src_begin, m, max_chunks, scratch, scratch_bytes, dst, dst_cap, dst_off, status,
                                                error_offset, info, written_items, p));
    p.end = m > 0 ? src_end : nullptr;
    return 0;
}

template <class B>
int streams_decode_spans_into(B& be, const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m,
                              int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off,
                              int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info, int64_t* written_items)
{
    StreamsIntoPlan p;
    LZ4HIP_FRAMING_TRY(streams_decode_spans_into_plan(be, src, src_len, src_begin, src_end, m, max_chunks, scratch, scratch_bytes, dst, dst_cap,
                                                      dst_off, status, error_offset, info, written_items, p));
    return streams_decode_into_run(be, p);
}

// ---- legacy frames (lz4hip_frame.hpp) ----------------------------------------------------------------------------------------------------
inline bool frame_chunk_valid(int32_t chunk_size) { return chunk_size >= 0 && chunk_size <= kFrameMaxChunk; }
inline int32_t frame_chunk(int32_t chunk_size) { return chunk_size == 0 ? kFrameDefaultChunk : chunk_size; }   // (of a valid chunk_size)

// 4 + sum over the chunks of (4 + compressBound(len_k)): all chunks but the last are full
inline int64_t frame_bound(int64_t src_len, int32_t chunk_size)
{
    if (!frame_chunk_valid(chunk_size)) return LZ4HIP_E_ARGUMENT;
    if (src_len < 0) src_len = 0;
    const int64_t chunk = frame_chunk(chunk_size), full = src_len / chunk, rest = src_len % chunk;
    return kFrameField + full * (kFrameField + frame_block_bound((int32_t)chunk)) + (rest ? kFrameField + frame_block_bound((int32_t)rest) : 0);
}

// the encoder's slot per chunk: compressBound of the longest chunk there is
inline int64_t frame_stride(int64_t src_len, int64_t chunk) { return frame_block_bound((int32_t)(src_len < chunk ? src_len : chunk)); }

// frame encode: the encoder's output (chunk k at k * stride), chunk lengths, capacities, results, the n + 1 sizes / offsets, tile sums
struct FrameEncodeScratch { uint8_t* comp; int32_t* lens; int32_t* caps; int32_t* result; int64_t* offs; int64_t* partial; int64_t bytes; };
inline FrameEncodeScratch frame_encode_scratch(void* scratch, int64_t src_len, int64_t chunk)
{
    const int64_t n = stream_chunks(src_len, chunk);
    Carver c(scratch);
    FrameEncodeScratch l;
    l.comp = c.take_as<uint8_t>(n * frame_stride(src_len, chunk));
    l.lens = c.take_as<int32_t>(4 * n);
    l.caps = c.take_as<int32_t>(4 * n);
    l.result = c.take_as<int32_t>(4 * n);
    l.offs = c.take_as<int64_t>(8 * (n + 1));
    l.partial = c.take_as<int64_t>(8 * scan_tiles(n + 1));
    l.bytes = c.at;
    return l;
}

// frame decode: [the lowest bad chunk, what the walk found], then the table of max_chunks rows and the scan's tile sums
inline FrameTables frame_tables(Carver& c, int64_t max_chunks)
{
    FrameTables t;
    t.max_chunks = max_chunks;
    t.min_bad = c.take_as<unsigned long long>(256);
    t.walk = (int64_t*)t.min_bad + 1;
    t.src_off = c.take_as<int64_t>(8 * max_chunks);
    t.hdr_off = c.take_as<int64_t>(8 * max_chunks);
    t.dst_off = c.take_as<int64_t>(8 * (max_chunks + 1));
    t.src_len = c.take_as<int32_t>(4 * max_chunks);
    t.dst_cap = c.take_as<int32_t>(4 * max_chunks);
    t.result = c.take_as<int32_t>(4 * max_chunks);
    t.partial = c.take_as<int64_t>(8 * scan_tiles(max_chunks));
    return t;
}
inline int64_t frame_decode_scratch_bytes(int64_t max_chunks) { Carver c; frame_tables(c, max_chunks); return c.at; }

// what a front hands its sequence
struct FrameEncodePlan { FrameEncodeArgs a; int mode; int32_t* lens; int32_t* caps; int64_t* partial; uint8_t* dst; int64_t dst_cap; int64_t* dst_len; int64_t bound; };
struct FrameIndexPlan { const uint8_t* src; int64_t src_len; int32_t chunk; FrameTables t; FrameInfo* info; int groups; };
struct FrameDecodePlan { const uint8_t* src; FrameInfo h; FrameTables t; uint8_t* dst; FrameInfo* info; };

// p.a.comp and p.a.result are the block encoder's to write: chunk k at k * p.a.stride.  An empty source is the scan of the magic's size alone.
template <class B>
int frame_encode_run(B& be, const FrameEncodePlan& p)
{
    const FrameEncodeArgs& a = p.a;
    if (a.n > 0) {
        be.launch(frame_lens_kernel, stream_grid(a.n), kStreamThreads, p.lens, p.caps, a.n, a.src_len, a.chunk);
        LZ4HIP_FRAMING_TRY(be.last_error());
        // compress_file: every chunk into a compressBound buffer; src_len_all = the chunk size, the upper bound LZ4HC picks its kernels from
        lz4hip_batch_t b = {};
        b.src = a.src; b.src_stride = a.chunk; b.src_len = p.lens;
        b.dst = (void*)a.comp; b.dst_stride = a.stride; b.dst_cap = p.caps;
        b.src_len_all = a.chunk; b.result = (int32_t*)a.result; b.n_blocks = a.n;
        LZ4HIP_FRAMING_TRY(be.encode(&b, p.mode));
    }
    be.launch(frame_sizes_kernel, stream_grid(a.n + 1), kStreamThreads, a);
    launch_scan(be, a.offs, a.n + 1, p.partial, p.dst_len);
    FrameLayout layout = { a };
    be.launch(frame_pack_kernel, copy_grid(p.bound), kStreamThreads, layout, p.dst, p.dst_len, p.dst_cap);
    return be.last_error();
}

template <class B>
int frame_encode_plan(B& be, const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len,
                      void* scratch, int64_t scratch_bytes, FrameEncodePlan& p)
{
    if (src_len < 0 || !dst_len) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: src_len < 0 or dst_len is NULL");
    if (!frame_chunk_valid(chunk_size)) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: chunk_size must be 0 (8 MiB) or 1 .. 0x7E000000");
    if (mode != LZ4HIP_MODE_FAST && mode != LZ4HIP_MODE_HC) return be.fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    const int64_t chunk = frame_chunk(chunk_size), n = stream_chunks(src_len, chunk);
    if (n >= 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: more than 2^31 - 2 chunks");
    p.bound = frame_bound(src_len, chunk_size);
    if (dst_cap < p.bound) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: dst_cap < lz4hip_frame_bound");
    const FrameEncodeScratch l = frame_encode_scratch(scratch, src_len, chunk);
    if (scratch_bytes < l.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: scratch_bytes < lz4hip_frame_encode_scratch_bytes");
    if ((n > 0 && !src) || !dst || !scratch) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: src, dst and scratch must be non-NULL");
    FrameEncodeArgs& a = p.a;
    a.src = (const uint8_t*)src; a.comp = l.comp; a.src_len = src_len; a.n = n; a.stride = frame_stride(src_len, chunk); a.chunk = (int32_t)chunk;
    a.result = l.result; a.offs = l.offs;
    p.mode = mode; p.lens = l.lens; p.caps = l.caps; p.partial = l.partial; p.dst = (uint8_t*)dst; p.dst_cap = dst_cap; p.dst_len = dst_len;
    return 0;
}

template <class B>
int frame_encode(B& be, const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len,
                 void* scratch, int64_t scratch_bytes)
{
    FrameEncodePlan p;
    LZ4HIP_FRAMING_TRY(frame_encode_plan(be, src, src_len, chunk_size, mode, dst, dst_cap, dst_len, scratch, scratch_bytes, p));
    return frame_encode_run(be, p);
}

// The rows past the walk's count must read as empty blocks: the two columns the size walk looks at are zeroed first.  It then runs over
// ALL max_chunks rows (an empty row costs nothing and gives 0), so nothing is read on the host between the steps.
template <class B>
int frame_index_run(B& be, const FrameIndexPlan& p)
{
    const FrameTables& t = p.t;
    LZ4HIP_FRAMING_TRY(be.fill(t.min_bad, 0xFF, 8));                   // min_bad = none
    if (t.max_chunks > 0) {
        LZ4HIP_FRAMING_TRY(be.fill(t.src_off, 0, (size_t)(8 * t.max_chunks)));
        LZ4HIP_FRAMING_TRY(be.fill(t.src_len, 0, (size_t)(4 * t.max_chunks)));
    }
    be.launch(frame_walk_kernel, fixed_grid(1), 64, p.src, p.src_len, (int64_t)frame_block_bound(p.chunk), t);
    LZ4HIP_FRAMING_TRY(be.last_error());
    if (t.max_chunks > 0) {
        SizesArgs a;
        a.src = p.src; a.src_off = t.src_off; a.src_stride = 0; a.src_len = t.src_len; a.src_len_all = 0; a.n = t.max_chunks;
        a.result = t.result; a.dst_cap = t.dst_cap; a.offs = t.dst_off; a.min_bad = t.min_bad;
        be.launch(sizes_walk_kernel, sizes_grid(a.n, p.groups), kSizesThreads, a);
        be.launch(frame_caps_kernel, stream_grid(t.max_chunks), kStreamThreads, t, p.chunk);
        launch_scan(be, t.dst_off, t.max_chunks, t.partial, t.dst_off + t.max_chunks);
    } else {
        LZ4HIP_FRAMING_TRY(be.fill(t.dst_off, 0, sizeof(int64_t)));
    }
    be.launch(frame_info_kernel, fixed_grid(1), 64, t, p.info);
    return be.last_error();
}

template <class B>
int frame_index_plan(B& be, const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                     lz4hip_frame_info_t* info, int groups, FrameIndexPlan& p)
{
    if (src_len < 0 || max_chunks < 0 || !info || !scratch || (src_len > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "frame index: negative size or NULL pointer");
    if (!frame_chunk_valid(chunk_size)) return be.fail(LZ4HIP_E_ARGUMENT, "frame index: chunk_size must be 0 (8 MiB) or 1 .. 0x7E000000");
    if (max_chunks > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "frame index: more than 2^31 - 1 table rows");
    Carver c(scratch);
    p.t = frame_tables(c, max_chunks);
    if (scratch_bytes < c.at) return be.fail(LZ4HIP_E_ARGUMENT, "frame index: scratch_bytes < lz4hip_frame_decode_scratch_bytes");
    p.src = (const uint8_t*)src; p.src_len = src_len; p.chunk = frame_chunk(chunk_size); p.info = (FrameInfo*)info; p.groups = groups;
    return 0;
}

template <class B>
int frame_index(B& be, const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                lz4hip_frame_info_t* info, int groups = 0)
{
    FrameIndexPlan p;
    LZ4HIP_FRAMING_TRY(frame_index_plan(be, src, src_len, chunk_size, max_chunks, scratch, scratch_bytes, info, groups, p));
    return frame_index_run(be, p);
}

// p.h: what the index reported, read back by the host; the table is as the index left it.  A frame that decodes to nothing has only
// capacities of 0 -- no chunk can write -- and keeps the walk's results for the check.
template <class B>
int frame_decode_run(B& be, const FrameDecodePlan& p)
{
    const FrameTables& t = p.t;
    if (p.h.chunks > 0) {
        if (p.h.decoded_bytes > 0) {
            // decode_file: LZ4_uncompress_unknownOutputSize per chunk -- the table IS the batch, its capacities the sizes the walk found
            lz4hip_batch_t b = {};
            b.src = p.src; b.src_off = t.src_off; b.src_len = t.src_len;
            b.dst = p.dst; b.dst_off = t.dst_off; b.dst_cap = t.dst_cap;
            b.result = t.result; b.n_blocks = p.h.chunks;
            LZ4HIP_FRAMING_TRY(be.decode(&b, 0));
        }
        be.launch(frame_check_kernel, stream_grid(p.h.chunks), kStreamThreads, t, p.h.chunks);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    be.launch(frame_info_kernel, fixed_grid(1), 64, t, p.info);
    return be.last_error();
}

template <class B>
int frame_decode_plan(B& be, const void* src, const lz4hip_frame_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                      void* dst, int64_t dst_cap, lz4hip_frame_info_t* info, FrameDecodePlan& p)
{
    if (!info_host || !info || !scratch || max_chunks < 0) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: NULL pointer or max_chunks < 0");
    const lz4hip_frame_info_t h = *info_host;
    if (h.error < LZ4HIP_FRAME_OK || h.error >= LZ4HIP_FRAME_TABLE_FULL)
        return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: the index reported a table too small (or the info is not an index's)");
    if (h.chunks < 0 || h.chunks > max_chunks || h.chunks > 0x7FFFFFFF || h.decoded_bytes < 0)
        return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: the info does not fit a table of max_chunks entries");
    if (h.decoded_bytes > dst_cap) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: decoded_bytes > dst_cap");
    if ((h.chunks > 0 && !src) || (h.decoded_bytes > 0 && !dst)) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: src and dst must be non-NULL");
    Carver c(scratch);
    p.t = frame_tables(c, max_chunks);
    if (scratch_bytes < c.at) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: scratch_bytes < lz4hip_frame_decode_scratch_bytes");
    p.src = (const uint8_t*)src; p.dst = (uint8_t*)dst; p.info = (FrameInfo*)info;
    memcpy(&p.h, &h, sizeof p.h);
    return 0;
}

template <class B>
int frame_decode(B& be, const void* src, const lz4hip_frame_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                 void* dst, int64_t dst_cap, lz4hip_frame_info_t* info)
{
    FrameDecodePlan p;
    LZ4HIP_FRAMING_TRY(frame_decode_plan(be, src, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, info, p));
    return frame_decode_run(be, p);
}

// ---- the decoded sizes of a block batch (lz4hip_sizes.hpp) ----------------------------------------------------------------------------
// scratch: the lowest failing index, then stand-ins for the outputs the caller left out (results, sizes / offsets), the scan's tile sums
struct SizesScratch { unsigned long long* min_bad; int32_t* result; int64_t* offs; int64_t* partial; int64_t bytes; };
inline SizesScratch sizes_scratch(void* scratch, int64_t n)
{
    Carver c(scratch);
    SizesScratch l;
    l.min_bad = c.take_as<unsigned long long>(256);
    l.result = c.take_as<int32_t>(4 * n);
    l.offs = c.take_as<int64_t>(8 * (n + 1));
    l.partial = c.take_as<int64_t>(8 * scan_tiles(n));
    l.bytes = c.at;
    return l;
}
inline int64_t sizes_scratch_bytes(int64_t n) { return n <= 0 ? 0 : sizes_scratch(nullptr, n).bytes; }

// a.n > 0; a.offs has n + 1 entries and receives the offsets, a.offs[n] the total
template <class B>
int decoded_sizes_run(B& be, const SizesArgs& a, int64_t* partial, SizesInfo* info, int groups, int32_t history = -1)
{
    LZ4HIP_FRAMING_TRY(be.fill(a.min_bad, 0xFF, 8));                   // min_bad = none
    if (history < 0) be.launch(sizes_walk_kernel, sizes_grid(a.n, groups), kSizesThreads, a);
    else             be.launch(sizes_walk_dict_kernel, sizes_grid(a.n, groups), kSizesThreads, a, history);
    launch_scan(be, a.offs, a.n, partial, a.offs + a.n);
    if (info) be.launch(sizes_info_kernel, fixed_grid(1), 64, a, info);
    return be.last_error();
}

// reads b's src, src_off / src_stride, src_len / src_len_all, result and n_blocks; any of result, dst_off, dst_cap and info may be NULL.
// dict_len >= 0: the blocks are decoded against a dictionary of that many bytes (lz4hip_decoded_sizes_dict_*), whose last 65 535 a match
// may reach; -1: blocks that stand alone.
template <class B>
int decoded_sizes(B& be, const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap, void* scratch, int64_t scratch_bytes,
                  lz4hip_sizes_info_t* info, int groups = 0, int64_t dict_len = -1)
{
    if (!b) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: batch descriptor is NULL");
    const int64_t n = b->n_blocks;
    if (n < 0) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: n_blocks < 0");
    if (n > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: more than 2^31 - 1 blocks");
    if (scratch_bytes < sizes_scratch_bytes(n)) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: scratch_bytes < lz4hip_decoded_sizes_scratch_bytes");
    if (n == 0) {
        if (dst_off) LZ4HIP_FRAMING_TRY(be.fill(dst_off, 0, sizeof(int64_t)));
        if (info) be.launch(sizes_empty_info_kernel, fixed_grid(1), 64, (SizesInfo*)info);
        return be.last_error();
    }
    if (!b->src || !scratch) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: src and scratch must be non-NULL");
    if (!b->src_len && b->src_len_all < 0) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: src_len_all < 0");
    const SizesScratch l = sizes_scratch(scratch, n);
    SizesArgs a;
    a.src = (const uint8_t*)b->src; a.src_off = b->src_off; a.src_stride = b->src_stride; a.src_len = b->src_len; a.src_len_all = b->src_len_all;
    a.n = n; a.result = b->result ? b->result : l.result; a.dst_cap = dst_cap; a.offs = dst_off ? dst_off : l.offs; a.min_bad = l.min_bad;
    return decoded_sizes_run(be, a, l.partial, (SizesInfo*)info, groups, dict_len < 0 ? -1 : (int32_t)(dict_len < 65535 ? dict_len : 65535));
}

// ---- a block batch encoded into one packed buffer (lz4hip_packed.hpp) -------------------------------------------------------------------
// The batch runs in rounds of at most `round` blocks through ONE ring of `round` slots: the scratch is the ring, the round's limits and
// results, the scan's tile sums and the state block, and does not grow with the batch once it has more blocks than a round.
inline int64_t packed_slot(int32_t slot_bytes) { return ((int64_t)slot_bytes + 15) / 16 * 16; }
// blocks per round: all of them for round_blocks = 0 (or more than there are)
inline int64_t packed_round(int64_t n, int64_t round_blocks) { return round_blocks <= 0 || round_blocks > n ? n : round_blocks; }

struct PackedScratch { uint8_t* ring; int32_t* caps; int32_t* lens; int32_t* result; int64_t* partial; int64_t* state; int64_t bytes; };
inline PackedScratch packed_scratch(void* scratch, int64_t n, int32_t slot_bytes, int64_t round_blocks)
{
    const int64_t round = packed_round(n, round_blocks);
    Carver c(scratch);
    PackedScratch l;
    l.ring = c.take_as<uint8_t>(round * packed_slot(slot_bytes));
    l.caps = c.take_as<int32_t>(4 * round);
    l.lens = c.take_as<int32_t>(4 * round);
    l.result = c.take_as<int32_t>(4 * round);
    l.partial = c.take_as<int64_t>(8 * scan_tiles(round));
    l.state = c.take_as<int64_t>(kPackedStateBytes);
    l.bytes = c.at;
    return l;
}
// 0 for an empty batch; LZ4HIP_E_ARGUMENT for a slot width or a round the call refuses
inline int64_t encode_packed_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t round_blocks)
{
    if (n <= 0) return 0;
    if (slot_bytes <= 0 || round_blocks < 0) return LZ4HIP_E_ARGUMENT;
    return packed_scratch(nullptr, n, slot_bytes, round_blocks).bytes;
}

// what the front hands the sequence: b is the caller's descriptor (its source side and result are read)
struct PackedPlan {
    lz4hip_batch_t b; int mode; int64_t n, round, slot; int32_t limit; PackedScratch l;
    uint8_t* dst; int64_t dst_cap; int64_t* dst_off; int32_t* packed_len; PackedInfo* info;
};

// The state block before the first round; what may mark a lowest failed index ahead of the rounds (the linked plan of lz4hip_lz4f_linked.hpp)
// comes after it.
template <class B>
int packed_state_init(B& be, const PackedScratch& l)
{
    LZ4HIP_FRAMING_TRY(be.fill(l.state, 0, (size_t)kPackedStateBytes));
    return be.fill(l.state + kPackedBad, 0xFF, 8);                      // the lowest failed index = none
}

// The rounds, written ONCE for the packed encode, the compact decode (lz4hip_compact.hpp) and the decodes of LZ4 frames (lz4hip_lz4f.hpp,
// lz4hip_lz4f_batch.hpp): `codec` runs the block encoder or decoder over a round's descriptor, `sizes` launches the step that turns its
// results into sizes under the caller's failure rule, `pack` the copy of the round's rows out of the ring.  p.b says where the rows lie:
// the caller's descriptor, or a table's columns dressed as one.
// Each round is a normal batch encode (decode) of its rows: the descriptor's array pointers are advanced here, on the host, its output is the
// ring, its capacities the round's array in scratch and its lengths the round's sanitised copy there (the encoders do not check a
// length's sign: a negative one would send their literal copy before the slot).  Rounds follow each other in stream order: a round's pack has read the ring
// before the next round's encoder writes it.
template <class B, class Codec, class Sizes, class Pack>
int packed_rounds(B& be, const PackedPlan& p, Codec codec, Sizes sizes, Pack pack)
{
    const lz4hip_batch_t& b = p.b;
    const Grid pack_grid = copy_grid(p.round * p.slot);
    int32_t parity = 0;
    for (int64_t first = 0; first < p.n; first += p.round, parity ^= 1) {
        PackedRound a;
        a.first = first; a.cnt = p.n - first < p.round ? p.n - first : p.round; a.slot = p.slot; a.limit = p.limit; a.parity = parity;
        a.cap_in = b.dst_cap ? b.dst_cap + first : nullptr; a.caps = p.l.caps; a.result = b.result ? b.result + first : p.l.result;
        a.len_in = b.src_len ? b.src_len + first : nullptr; a.lens_enc = p.l.lens;
        a.ring = p.l.ring; a.offs = p.dst_off + first; a.lens = p.packed_len ? p.packed_len + first : nullptr; a.state = p.l.state;
        be.launch(packed_caps_kernel, stream_grid(a.cnt), kStreamThreads, a);
        LZ4HIP_FRAMING_TRY(be.last_error());
        lz4hip_batch_t rb = {};
        rb.src = b.src_off ? b.src : (const void*)((const uint8_t*)b.src + first * b.src_stride);
        rb.src_off = b.src_off ? b.src_off + first : nullptr; rb.src_stride = b.src_stride;
        rb.src_len = b.src_len ? p.l.lens : nullptr; rb.src_len_all = b.src_len_all;      // (no negative length reaches the encoder)
        rb.dst = p.l.ring; rb.dst_stride = p.slot; rb.dst_cap = p.l.caps;
        rb.result = a.result; rb.n_blocks = a.cnt;
        LZ4HIP_FRAMING_TRY(codec(&rb));
        sizes(a, stream_grid(a.cnt));
        launch_scan(be, a.offs, a.cnt, p.l.partial, p.l.state + kPackedTotal);
        be.launch(packed_rebase_kernel, stream_grid(a.cnt), kStreamThreads, a);
        pack(a, pack_grid);
        LZ4HIP_FRAMING_TRY(be.last_error());
    }
    return 0;
}

// a block batch through the rounds: the empty batch, the state block, the rounds with the sizes kernel of the codec's failure rule and
// PackedLayout, the record
template <class B, class Codec>
int packed_rounds_run(B& be, const PackedPlan& p, Codec codec, void (*sizes)(PackedRound))
{
    if (p.n == 0) {
        LZ4HIP_FRAMING_TRY(be.fill(p.dst_off, 0, sizeof(int64_t)));
        if (p.info) be.launch(packed_empty_info_kernel, fixed_grid(1), 64, p.info);
        return be.last_error();
    }
    LZ4HIP_FRAMING_TRY(packed_state_init(be, p.l));
    LZ4HIP_FRAMING_TRY(packed_rounds(be, p, codec, [&](const PackedRound& a, Grid grid) { be.launch(sizes, grid, kStreamThreads, a); },
                                     [&](const PackedRound& a, Grid grid) { be.launch(packed_pack_kernel, grid, kStreamThreads, PackedLayout{ a }, p.dst, p.dst_cap); }));
    if (p.info) be.launch(packed_info_kernel, fixed_grid(1), 64, (const int64_t*)p.dst_off, p.n, p.dst_cap, (const int64_t*)p.l.state, p.info);
    return be.last_error();
}

template <class B>
int encode_packed_run(B& be, const PackedPlan& p)
{
    return packed_rounds_run(be, p, [&](const lz4hip_batch_t* rb) { return be.encode(rb, p.mode); }, packed_sizes_kernel);
}

// reads b's src, src_off / src_stride, src_len / src_len_all, dst_cap / dst_cap_all (the slot width), result and n_blocks; b's dst,
// dst_off and dst_stride are ignored.  packed_len and info may be NULL.
// What the device call and the host call check alike, for the packed encode (`what` = "encode packed") and the compact decode ("decode
// compact", whose mode is LZ4HIP_MODE_FAST: it has none): everything but the scratch, which only the device call is handed
template <class B>
int packed_check(B& be, const char* what, const lz4hip_batch_t* b, int mode, int64_t round_blocks, const void* dst, int64_t dst_cap, const int64_t* dst_off)
{
    const auto fail = [&](const char* text) { return be.fail(LZ4HIP_E_ARGUMENT, (std::string(what) + ": " + text).c_str()); };
    if (!b) return fail("batch descriptor is NULL");
    const int64_t n = b->n_blocks;
    if (n < 0) return fail("n_blocks < 0");
    if (dst_cap < 0 || round_blocks < 0) return fail("dst_cap < 0 or round_blocks < 0");
    if (b->dst_cap_all <= 0) return fail("dst_cap_all (the slot width) must be > 0");
    if (mode != LZ4HIP_MODE_FAST && mode != LZ4HIP_MODE_HC) return be.fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    if (!dst_off) return fail("dst_off is NULL");
    if (packed_round(n, round_blocks) > 0x7FFFFFFF) return fail("more than 2^31 - 1 blocks in a round");
    if (n > 0) {
        if (!b->src || (dst_cap > 0 && !dst)) return fail("src and dst must be non-NULL");
        if (!b->src_len && b->src_len_all < 0) return fail("src_len_all < 0");
    }
    return 0;
}

template <class B>
int encode_packed_check(B& be, const lz4hip_batch_t* b, int mode, int64_t round_blocks, const void* dst, int64_t dst_cap, const int64_t* dst_off)
{
    return packed_check(be, "encode packed", b, mode, round_blocks, dst, dst_cap, dst_off);
}

// `lens`: the caller's packed_len or decoded_len.  The scratch query's name in the failure text is the public one: lz4hip_<what, with
// underscores>_scratch_bytes.
template <class B>
int packed_plan(B& be, const char* what, const lz4hip_batch_t* b, int mode, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                int32_t* lens, void* scratch, int64_t scratch_bytes, PackedInfo* info, PackedPlan& p)
{
    LZ4HIP_FRAMING_TRY(packed_check(be, what, b, mode, round_blocks, dst, dst_cap, dst_off));
    const int64_t n = b->n_blocks;
    if (scratch_bytes < encode_packed_scratch_bytes(n, b->dst_cap_all, round_blocks)) {
        std::string query = what;
        for (char& ch : query) ch = ch == ' ' ? '_' : ch;
        return be.fail(LZ4HIP_E_ARGUMENT, (std::string(what) + ": scratch_bytes < lz4hip_" + query + "_scratch_bytes").c_str());
    }
    if (n > 0 && !scratch) return be.fail(LZ4HIP_E_ARGUMENT, (std::string(what) + ": scratch must be non-NULL").c_str());
    p.n = n; p.round = packed_round(n, round_blocks);
    p.b = *b; p.mode = mode; p.limit = b->dst_cap_all; p.slot = packed_slot(b->dst_cap_all);
    p.l = packed_scratch(scratch, n, b->dst_cap_all, round_blocks);
    p.dst = (uint8_t*)dst; p.dst_cap = dst_cap; p.dst_off = dst_off; p.packed_len = lens; p.info = info;
    return 0;
}

template <class B>
int encode_packed_plan(B& be, const lz4hip_batch_t* b, int mode, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                       int32_t* packed_len, void* scratch, int64_t scratch_bytes, lz4hip_packed_info_t* info, PackedPlan& p)
{
    return packed_plan(be, "encode packed", b, mode, round_blocks, dst, dst_cap, dst_off, packed_len, scratch, scratch_bytes, (PackedInfo*)info, p);
}

template <class B>
int encode_packed(B& be, const lz4hip_batch_t* b, int mode, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                  int32_t* packed_len, void* scratch, int64_t scratch_bytes, lz4hip_packed_info_t* info)
{
    PackedPlan p;
    LZ4HIP_FRAMING_TRY(encode_packed_plan(be, b, mode, round_blocks, dst, dst_cap, dst_off, packed_len, scratch, scratch_bytes, info, p));
    return encode_packed_run(be, p);
}

// ---- a block batch decoded into one packed buffer (lz4hip_compact.hpp) -------------------------------------------------------------------
// The packed encode the other way: the same rounds through the same ring, tables and state block (packed_scratch), the block decoder
// (unknown size) in the encoder's place and compact_sizes_kernel, whose failure rule is result < 0, in packed_sizes_kernel's.  The plan
// is a PackedPlan whose mode is not looked at and whose packed_len is the caller's decoded_len.
// 0 for an empty batch; LZ4HIP_E_ARGUMENT for a slot width or a round the call refuses
inline int64_t decode_compact_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t round_blocks)
{
    return encode_packed_scratch_bytes(n, slot_bytes, round_blocks);
}

// Each round is a normal unknown-size batch decode of its rows into the ring, dst_stride the slot: the decoders' dispatch rules see
// the round's size.  They are handed the round's sanitised lengths, never the caller's.
template <class B>
int decode_compact_run(B& be, const PackedPlan& p)
{
    return packed_rounds_run(be, p, [&](const lz4hip_batch_t* rb) { return be.decode(rb, 0); }, compact_sizes_kernel);
}

// The packed encode's check and plan (packed_check, packed_plan) under this call's name; decoded_len and info may be NULL.
template <class B>
int decode_compact_check(B& be, const lz4hip_batch_t* b, int64_t round_blocks, const void* dst, int64_t dst_cap, const int64_t* dst_off)
{
    return packed_check(be, "decode compact", b, LZ4HIP_MODE_FAST, round_blocks, dst, dst_cap, dst_off);
}

template <class B>
int decode_compact_plan(B& be, const lz4hip_batch_t* b, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                        int32_t* decoded_len, void* scratch, int64_t scratch_bytes, lz4hip_compact_info_t* info, PackedPlan& p)
{
    return packed_plan(be, "decode compact", b, LZ4HIP_MODE_FAST, round_blocks, dst, dst_cap, dst_off, decoded_len, scratch, scratch_bytes, (PackedInfo*)info, p);
}

template <class B>
int decode_compact(B& be, const lz4hip_batch_t* b, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                   int32_t* decoded_len, void* scratch, int64_t scratch_bytes, lz4hip_compact_info_t* info)
{
    PackedPlan p;
    LZ4HIP_FRAMING_TRY(decode_compact_plan(be, b, round_blocks, dst, dst_cap, dst_off, decoded_len, scratch, scratch_bytes, info, p));
    return decode_compact_run(be, p);
}

// ---- a legacy frame decoded in one call (lz4hip_compact.hpp) -------------------------------------------------------------------------------
// The size field walk, then the compact decode over ALL max_chunks rows of the table -- slot and limit chunk_size, as the reference's
// reader gives every chunk (original/lz4demo.c:276-300); the rows past the walk's count are empty blocks, which decode to nothing --
// straight into dst, then the record.  Nothing is read on the host between the steps.
// scratch: the index's table (its dst_off column receives the offsets, its result column the decoder's results), then the compact
// decode's scratch for max_chunks rows
struct FrameCompactScratch { FrameTables t; void* compact; int64_t compact_bytes; int64_t bytes; };
inline FrameCompactScratch frame_compact_scratch(void* scratch, int32_t chunk, int64_t max_chunks, int64_t round_chunks)
{
    Carver c(scratch);
    FrameCompactScratch l;
    l.t = frame_tables(c, max_chunks);
    l.compact = c.take_as<uint8_t>(0);
    l.compact_bytes = packed_scratch(nullptr, max_chunks, chunk, round_chunks).bytes;
    l.bytes = c.at + l.compact_bytes;
    return l;
}
inline int64_t frame_decode_compact_scratch_bytes(int32_t chunk_size, int64_t max_chunks, int64_t round_chunks)
{
    if (!frame_chunk_valid(chunk_size) || max_chunks < 0 || round_chunks < 0) return LZ4HIP_E_ARGUMENT;
    return frame_compact_scratch(nullptr, frame_chunk(chunk_size), max_chunks, round_chunks).bytes;
}

struct FrameCompactPlan { const uint8_t* src; int64_t src_len; int32_t chunk; FrameTables t; PackedPlan decode; FrameInfo* info; };

template <class B>
int frame_decode_compact_run(B& be, const FrameCompactPlan& p)
{
    const FrameTables& t = p.t;
    if (t.max_chunks > 0) {
        LZ4HIP_FRAMING_TRY(be.fill(t.src_off, 0, (size_t)(8 * t.max_chunks)));
        LZ4HIP_FRAMING_TRY(be.fill(t.src_len, 0, (size_t)(4 * t.max_chunks)));
    }
    be.launch(frame_walk_kernel, fixed_grid(1), 64, p.src, p.src_len, (int64_t)frame_block_bound(p.chunk), t);
    LZ4HIP_FRAMING_TRY(be.last_error());
    LZ4HIP_FRAMING_TRY(decode_compact_run(be, p.decode));
    if (t.max_chunks == 0) LZ4HIP_FRAMING_TRY(be.fill(p.decode.l.state + kPackedBad, 0xFF, 8));   // (no row: the decode left its state block alone)
    be.launch(frame_compact_info_kernel, fixed_grid(1), 64, t, (const int64_t*)(p.decode.l.state + kPackedBad), p.info);
    return be.last_error();
}

template <class B>
int frame_decode_compact_plan(B& be, const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, int64_t round_chunks, void* scratch,
                              int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_frame_info_t* info, FrameCompactPlan& p)
{
    if (src_len < 0 || max_chunks < 0 || round_chunks < 0 || dst_cap < 0 || !info || !scratch || (src_len > 0 && !src) || (dst_cap > 0 && !dst))
        return be.fail(LZ4HIP_E_ARGUMENT, "frame decode compact: negative size or NULL pointer");
    if (!frame_chunk_valid(chunk_size)) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode compact: chunk_size must be 0 (8 MiB) or 1 .. 0x7E000000");
    if (packed_round(max_chunks, round_chunks) > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode compact: more than 2^31 - 1 table rows in a round");
    p.chunk = frame_chunk(chunk_size);
    const FrameCompactScratch l = frame_compact_scratch(scratch, p.chunk, max_chunks, round_chunks);
    if (scratch_bytes < l.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode compact: scratch_bytes < lz4hip_frame_decode_compact_scratch_bytes");
    p.src = (const uint8_t*)src; p.src_len = src_len; p.t = l.t; p.info = (FrameInfo*)info;
    // the table IS the batch: every row at its offset in the frame (an empty frame's rows are all empty: any address will do for them)
    lz4hip_batch_t b = {};
    b.src = src ? src : scratch; b.src_off = l.t.src_off; b.src_len = l.t.src_len;
    b.dst_cap_all = p.chunk; b.result = l.t.result; b.n_blocks = max_chunks;
    return decode_compact_plan(be, &b, round_chunks, dst, dst_cap, l.t.dst_off, nullptr, l.compact, l.compact_bytes, nullptr, p.decode);
}

template <class B>
int frame_decode_compact(B& be, const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, int64_t round_chunks, void* scratch,
                         int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_frame_info_t* info)
{
    FrameCompactPlan p;
    LZ4HIP_FRAMING_TRY(frame_decode_compact_plan(be, src, src_len, chunk_size, max_chunks, round_chunks, scratch, scratch_bytes, dst, dst_cap, info, p));
    return frame_decode_compact_run(be, p);
}

// ---- xxHash32 of rows, and LZ4 frames (lz4hip_lz4f.hpp) ----------------------------------------------------------------------------------
static_assert(kLz4fBlockChecksum == LZ4HIP_LZ4F_BLOCK_CHECKSUM && kLz4fContentChecksum == LZ4HIP_LZ4F_CONTENT_CHECKSUM &&
              kLz4fContentSize == LZ4HIP_LZ4F_CONTENT_SIZE && kLz4fVerifyBlocks == LZ4HIP_LZ4F_VERIFY_BLOCKS &&
              kLz4fVerifyContent == LZ4HIP_LZ4F_VERIFY_CONTENT && kLz4fAcceptLinked == LZ4HIP_LZ4F_ACCEPT_LINKED &&
              kLz4fKindSkippable == LZ4HIP_LZ4F_KIND_SKIPPABLE, "lz4f flags");
static_assert(kLz4fOk == LZ4HIP_LZ4F_OK && kLz4fBadMagic == LZ4HIP_LZ4F_BAD_MAGIC && kLz4fBadHeader == LZ4HIP_LZ4F_BAD_HEADER &&
              kLz4fHeaderChecksum == LZ4HIP_LZ4F_HEADER_CHECKSUM && kLz4fUnsupportedLinked == LZ4HIP_LZ4F_UNSUPPORTED_LINKED &&
              kLz4fUnsupportedDict == LZ4HIP_LZ4F_UNSUPPORTED_DICT && kLz4fSlotTooSmall == LZ4HIP_LZ4F_SLOT_TOO_SMALL &&
              kLz4fTruncated == LZ4HIP_LZ4F_TRUNCATED && kLz4fBadBlockSize == LZ4HIP_LZ4F_BAD_BLOCK_SIZE &&
              kLz4fCorruptBlock == LZ4HIP_LZ4F_CORRUPT_BLOCK && kLz4fBlockChecksumError == LZ4HIP_LZ4F_BLOCK_CHECKSUM_ERROR &&
              kLz4fContentSizeError == LZ4HIP_LZ4F_CONTENT_SIZE_ERROR && kLz4fContentChecksumError == LZ4HIP_LZ4F_CONTENT_CHECKSUM_ERROR &&
              kLz4fTableFull == LZ4HIP_LZ4F_TABLE_FULL && kLz4fDictIdMismatch == LZ4HIP_LZ4F_DICT_ID_MISMATCH, "lz4f statuses");
static_assert(sizeof(Lz4fInfo) == sizeof(lz4hip_lz4f_info_t) && offsetof(Lz4fInfo, frame_bytes) == offsetof(lz4hip_lz4f_info_t, frame_bytes) &&
              offsetof(Lz4fInfo, error) == offsetof(lz4hip_lz4f_info_t, error) && offsetof(Lz4fInfo, checks) == offsetof(lz4hip_lz4f_info_t, checks),
              "Lz4fInfo must mirror lz4hip_lz4f_info_t");

// sixteen rows per wavefront, four wavefronts per workgroup; more rows than the grid holds share wavefronts
inline Grid xxh_grid(int64_t n)
{
    const int64_t rows = kXxhRowsPerWave * (kXxhThreads / 64), g = (n + rows - 1) / rows;
    return { g < 1 ? 1u : (g > kStreamMaxGroups ? kStreamMaxGroups : (unsigned)g), kGridItems };
}

template <class B>
int xxh32_rows_run(B& be, const XxhRows& rows)
{
    if (rows.n <= 0) return 0;
    be.launch(xxh32_rows_kernel, xxh_grid(rows.n), kXxhThreads, rows);
    return be.last_error();
}

template <class B>
int xxh32_rows_check(B& be, const void* data, const int64_t* off, int64_t stride, const int32_t* len, int64_t len_all, const uint32_t* sums, int64_t n)
{
    if (n < 0) return be.fail(LZ4HIP_E_ARGUMENT, "xxh32 rows: n_rows < 0");
    if (n > 0 && !sums) return be.fail(LZ4HIP_E_ARGUMENT, "xxh32 rows: sums is NULL");
    if (n > 0 && !data && (len || len_all > 0)) return be.fail(LZ4HIP_E_ARGUMENT, "xxh32 rows: data is NULL");
    return 0;
}

// ---- the dictionary of the dictionary calls (lz4hip_lz4f_*_dict_*), for the encode and decode sequences below -----------------------------
// What a sequence is handed in its place: Lz4fNoDict by the plain calls, whose sequences are what they were, or the bytes of the call's
// dictionary that a match can reach -- its last min(dict_len, 65 535), in device memory, which END at `end` -- and the ID a frame's must
// equal (0: any).  The overloads below are all that differs: the walk's flag and ID, the rounds' block decoder (a backend needs
// decode_dict only where a sequence is instantiated with a dictionary) and the linked decode's kernel.  To the encode sequences `id` is
// the ID to write (0: none) and `primed` the 16 KiB of the call's scratch that hold the encoder's primed table; what differs there are
// the block encoder (be.encode_dict_prime once, then be.encode_dict in be.encode's place), the head kernel and the head's length.
struct Lz4fNoDict {};
struct Lz4fDict { const uint8_t* end; int32_t len; uint32_t id; uint8_t* primed; };
inline Lz4fDict lz4f_dict_of(const void* dict, int64_t dict_len, uint32_t dict_id)
{
    return { (const uint8_t*)dict + dict_len, (int32_t)(dict_len < kLz4fLinkedHistory ? dict_len : kLz4fLinkedHistory), dict_id, nullptr };
}
inline unsigned lz4f_walk_flags(unsigned flags, Lz4fNoDict) { return flags; }
inline unsigned lz4f_walk_flags(unsigned flags, const Lz4fDict&) { return flags | kLz4fWithDict; }
inline uint32_t lz4f_walk_dict_id(Lz4fNoDict) { return 0; }
inline uint32_t lz4f_walk_dict_id(const Lz4fDict& d) { return d.id; }
template <class B> int lz4f_round_decode(B& be, const lz4hip_batch_t* rb, Lz4fNoDict) { return be.decode(rb, 0); }
template <class B> int lz4f_round_decode(B& be, const lz4hip_batch_t* rb, const Lz4fDict& d) { return be.decode_dict(rb, d.end, d.len, 0); }
// the encode sequences' block call: the primed table first, once per call
template <class B> int lz4f_blocks_encode(B& be, const lz4hip_batch_t* b, int mode, Lz4fNoDict) { return be.encode(b, mode); }
template <class B> int lz4f_blocks_encode(B& be, const lz4hip_batch_t* b, int, const Lz4fDict& d)
{
    if (int rc = be.encode_dict_prime(d.end, d.len, d.primed)) return rc;
    return be.encode_dict(b, d.end, d.len, d.primed);
}
inline Lz4fPlainHead lz4f_head_of(Lz4fNoDict) { return {}; }
inline Lz4fDictHead lz4f_head_of(const Lz4fDict& d) { return { d.id }; }
inline int64_t lz4f_dict_reach(Lz4fNoDict) { return 0; }
inline int64_t lz4f_dict_reach(const Lz4fDict& d) { return d.len; }
// dict_len < 0, or no dictionary where there should be one
template <class B>
int lz4f_dict_check(B& be, const void* dict, int64_t dict_len)
{
    if (dict_len < 0) return be.fail(LZ4HIP_E_ARGUMENT, "dictionary: dict_len < 0");
    if (dict_len > 0 && !dict) return be.fail(LZ4HIP_E_ARGUMENT, "dictionary: dict is NULL and dict_len > 0");
    return 0;
}

inline bool lz4f_id_valid(int block_size_id) { return block_size_id == 0 || (block_size_id >= 4 && block_size_id <= 7); }
inline int lz4f_id(int block_size_id) { return block_size_id == 0 ? 4 : block_size_id; }                        // (of a valid id)
constexpr unsigned kLz4fEncodeFlags = kLz4fBlockChecksum | kLz4fContentChecksum | kLz4fContentSize;
// an empty source carries no content size: 0 means "unknown" to the format library, which writes none
inline unsigned lz4f_flags(int64_t src_len, unsigned flags) { return src_len > 0 ? flags : flags & ~kLz4fContentSize; }
// the descriptor's length: the plain calls', or with `dict_id` != 0 (the dictionary encode) the four bytes of the ID more
inline int32_t lz4f_head_len(unsigned flags, uint32_t dict_id = 0) { return Lz4fDictHead{ dict_id }.len(flags); }

// the descriptor, every block stored raw behind its size field (and before its checksum), the EndMark and the content checksum
inline int64_t lz4f_bound(int64_t src_len, int block_size_id, unsigned flags, uint32_t dict_id = 0)
{
    if (!lz4f_id_valid(block_size_id) || (flags & ~kLz4fEncodeFlags)) return LZ4HIP_E_ARGUMENT;
    if (src_len < 0) src_len = 0;
    flags = lz4f_flags(src_len, flags);
    const int64_t n = stream_chunks(src_len, lz4f_block_bytes(lz4f_id(block_size_id)));
    return lz4f_head_len(flags, dict_id) + src_len + n * (4 + ((flags & kLz4fBlockChecksum) ? 4 : 0)) + 4 + ((flags & kLz4fContentChecksum) ? 4 : 0);
}
// lz4hip_lz4f_dict_bound: without a dictionary the plain bound, whatever the ID
inline int64_t lz4f_dict_bound(int64_t src_len, int block_size_id, unsigned flags, int64_t dict_len, uint32_t dict_id)
{
    if (dict_len < 0) return LZ4HIP_E_ARGUMENT;
    return lz4f_bound(src_len, block_size_id, flags, dict_len > 0 ? dict_id : 0);
}

// the encoder's slot per block: a block is given one byte less than its length
inline int64_t lz4f_stride(int64_t src_len, int64_t block) { return src_len < block ? src_len : block; }

// lz4f encode: the encoder's output (block k at k * stride), block lengths, capacities, results, the checksum rows, the n + 1 checksums,
// the descriptor, the n + 2 sizes / offsets, tile sums
// With a dictionary (dict_len > 0) the plain layout, then the descriptor's kLz4fDictHeadMax bytes and the 16 KiB primed table.
struct Lz4fEncodeScratch {
    uint8_t* comp; int32_t* lens; int32_t* caps; int32_t* result; int64_t* row_off; int32_t* row_len; uint32_t* sums; uint8_t* head; int64_t* offs;
    int64_t* partial; uint8_t* primed; int64_t bytes;
};
inline Lz4fEncodeScratch lz4f_encode_scratch(void* scratch, int64_t src_len, int64_t block, int64_t dict_len = 0)
{
    const int64_t n = stream_chunks(src_len, block);
    Carver c(scratch);
    Lz4fEncodeScratch l;
    l.comp = c.take_as<uint8_t>(n * lz4f_stride(src_len, block));
    l.lens = c.take_as<int32_t>(4 * n);
    l.caps = c.take_as<int32_t>(4 * n);
    l.result = c.take_as<int32_t>(4 * n);
    l.row_off = c.take_as<int64_t>(8 * n);
    l.row_len = c.take_as<int32_t>(4 * n);
    l.sums = c.take_as<uint32_t>(4 * (n + 1));
    l.head = c.take_as<uint8_t>(kLz4fHeadMax);
    l.offs = c.take_as<int64_t>(8 * (n + 2));
    l.partial = c.take_as<int64_t>(8 * scan_tiles(n + 2));
    l.primed = nullptr;
    if (dict_len > 0) {
        l.head = c.take_as<uint8_t>(kLz4fDictHeadMax);
        l.primed = c.take_as<uint8_t>(kFastTableBytes);
    }
    l.bytes = c.at;
    return l;
}

struct Lz4fEncodePlan {
    Lz4fEncodeArgs a; int mode; int32_t* lens; int32_t* caps; int64_t* row_off; int32_t* row_len; int64_t* partial; uint8_t* dst; int64_t dst_cap;
    int64_t* dst_len; int64_t bound;
};

template <class B> void lz4f_head_launch(B& be, const Lz4fEncodeArgs& a, Lz4fNoDict) { be.launch(lz4f_head_kernel, fixed_grid(1), 64, a); }
template <class B> void lz4f_head_launch(B& be, const Lz4fEncodeArgs& a, const Lz4fDict& d) { be.launch(lz4f_dict_head_kernel, fixed_grid(1), 64, a, lz4f_head_of(d)); }

// p.a.comp and p.a.result are the block encoder's to write: block k at k * p.a.stride.  An empty source is a descriptor and an EndMark.
// `dict`: Lz4fNoDict, or the call's dictionary in device memory (the fast mode's dictionary encoder, whatever p.mode).
template <class B, class D = Lz4fNoDict>
int lz4f_encode_run(B& be, const Lz4fEncodePlan& p, const D& dict = D())
{
    const Lz4fEncodeArgs& a = p.a;
    if (a.n > 0) {
        be.launch(lz4f_lens_kernel, stream_grid(a.n), kStreamThreads, p.lens, p.caps, a.n, a.src_len, a.block);
        LZ4HIP_FRAMING_TRY(be.last_error());
        lz4hip_batch_t b = {};
        b.src = a.src; b.src_stride = a.block; b.src_len = p.lens;
        b.dst = (void*)a.comp; b.dst_stride = a.stride; b.dst_cap = p.caps;
        b.src_len_all = a.block; b.result = (int32_t*)a.result; b.n_blocks = a.n;
        LZ4HIP_FRAMING_TRY(lz4f_blocks_encode(be, &b, p.mode, dict));
        if (a.flags & kLz4fBlockChecksum) {
            be.launch(lz4f_rows_kernel, stream_grid(a.n), kStreamThreads, a, p.row_off, p.row_len);
            const XxhRows rows = { a.src, p.row_off, 0, p.row_len, nullptr, 0, 0u, a.sums, a.n };
            LZ4HIP_FRAMING_TRY(xxh32_rows_run(be, rows));
        }
    }
    if (a.flags & kLz4fContentChecksum) {
        const XxhRows content = { a.src, nullptr, 0, nullptr, nullptr, a.src_len, 0u, a.sums + a.n, 1 };
        LZ4HIP_FRAMING_TRY(xxh32_rows_run(be, content));
    }
    lz4f_head_launch(be, a, dict);
    be.launch(lz4f_sizes_kernel, stream_grid(a.n + 2), kStreamThreads, a);
    launch_scan(be, a.offs, a.n + 2, p.partial, p.dst_len);
    Lz4fLayout layout = { a };
    be.launch(lz4f_pack_kernel, copy_grid(p.bound), kStreamThreads, layout, p.dst, p.dst_len, p.dst_cap);
    return be.last_error();
}

template <class B>
int lz4f_encode_plan(B& be, const void* src, int64_t src_len, int block_size_id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len,
                     void* scratch, int64_t scratch_bytes, Lz4fEncodePlan& p, int64_t dict_len = 0, uint32_t dict_id = 0, uint8_t** primed = nullptr)
{
    if (src_len < 0 || !dst_len) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: src_len < 0 or dst_len is NULL");
    if (!lz4f_id_valid(block_size_id)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: block_size_id must be 0 (64 KiB) or 4 .. 7");
    if (flags & ~kLz4fEncodeFlags) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: unknown flag");
    if (mode != LZ4HIP_MODE_FAST && mode != LZ4HIP_MODE_HC) return be.fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    const int id = lz4f_id(block_size_id);
    const int64_t block = lz4f_block_bytes(id), n = stream_chunks(src_len, block);
    if (n >= 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: more than 2^31 - 2 blocks");
    p.bound = lz4f_bound(src_len, block_size_id, flags, dict_id);
    if (dst_cap < p.bound) return be.fail(LZ4HIP_E_ARGUMENT, dict_len > 0 ? "lz4f encode: dst_cap < lz4hip_lz4f_dict_bound" : "lz4f encode: dst_cap < lz4hip_lz4f_bound");
    const Lz4fEncodeScratch l = lz4f_encode_scratch(scratch, src_len, block, dict_len);
    if (scratch_bytes < l.bytes)
        return be.fail(LZ4HIP_E_ARGUMENT, dict_len > 0 ? "lz4f encode: scratch_bytes < lz4hip_lz4f_encode_dict_scratch_bytes"
                                                       : "lz4f encode: scratch_bytes < lz4hip_lz4f_encode_scratch_bytes");
    if ((n > 0 && !src) || !dst || !scratch) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: src, dst and scratch must be non-NULL");
    Lz4fEncodeArgs& a = p.a;
    a.src = (const uint8_t*)src; a.comp = l.comp; a.src_len = src_len; a.n = n; a.stride = lz4f_stride(src_len, block); a.block = (int32_t)block;
    a.block_id = id; a.flags = lz4f_flags(src_len, flags); a.head_len = lz4f_head_len(a.flags, dict_id);
    a.result = l.result; a.sums = l.sums; a.head = l.head; a.offs = l.offs;
    p.mode = mode; p.lens = l.lens; p.caps = l.caps; p.row_off = l.row_off; p.row_len = l.row_len; p.partial = l.partial;
    p.dst = (uint8_t*)dst; p.dst_cap = dst_cap; p.dst_len = dst_len;
    if (primed) *primed = l.primed;
    return 0;
}

template <class B>
int lz4f_encode(B& be, const void* src, int64_t src_len, int block_size_id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len,
                void* scratch, int64_t scratch_bytes)
{
    Lz4fEncodePlan p;
    LZ4HIP_FRAMING_TRY(lz4f_encode_plan(be, src, src_len, block_size_id, mode, flags, dst, dst_cap, dst_len, scratch, scratch_bytes, p));
    return lz4f_encode_run(be, p);
}

// lz4hip_lz4f_encode_dict_device: the dictionary's check, then the plain call's plan in fast mode with the dictionary's bound, scratch
// and head length; `d` is what the sequence is handed (d.len == 0: no dictionary, the plain sequence).  `dict` is device memory.
template <class B>
int lz4f_encode_dict_plan(B& be, const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int block_size_id, unsigned flags,
                          void* dst, int64_t dst_cap, int64_t* dst_len, void* scratch, int64_t scratch_bytes, Lz4fEncodePlan& p, Lz4fDict& d)
{
    LZ4HIP_FRAMING_TRY(lz4f_dict_check(be, dict, dict_len));
    d = lz4f_dict_of(dict, dict_len, dict_len > 0 ? dict_id : 0);
    return lz4f_encode_plan(be, src, src_len, block_size_id, LZ4HIP_MODE_FAST, flags, dst, dst_cap, dst_len, scratch, scratch_bytes, p, dict_len, d.id, &d.primed);
}
template <class B>
int lz4f_encode_dict_run(B& be, const Lz4fEncodePlan& p, const Lz4fDict& d) { return d.len > 0 ? lz4f_encode_run(be, p, d) : lz4f_encode_run(be, p); }

template <class B>
int lz4f_encode_dict(B& be, const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int block_size_id, unsigned flags, void* dst,
                     int64_t dst_cap, int64_t* dst_len, void* scratch, int64_t scratch_bytes)
{
    Lz4fEncodePlan p;
    Lz4fDict d;
    LZ4HIP_FRAMING_TRY(lz4f_encode_dict_plan(be, src, src_len, dict, dict_len, dict_id, block_size_id, flags, dst, dst_cap, dst_len, scratch, scratch_bytes, p, d));
    return lz4f_encode_dict_run(be, p, d);
}

// lz4f decode: the table of max_blocks rows (the n + 1 checksums and what the walk found with it), then the compact decode's scratch for
// max_blocks rows of slot_bytes
inline bool lz4f_slot_valid(int32_t slot_bytes) { return slot_bytes == 0 || slot_bytes == 65536 || slot_bytes == 262144 || slot_bytes == 1048576 || slot_bytes == 4194304; }
inline int32_t lz4f_slot(int32_t slot_bytes) { return slot_bytes == 0 ? 4194304 : slot_bytes; }                    // (of a valid slot_bytes)
constexpr unsigned kLz4fDecodeFlags = kLz4fVerifyBlocks | kLz4fVerifyContent | kLz4fAcceptLinked;
static_assert(!(kLz4fDecodeFlags & kLz4fWithDict), "the walk's internal bit is no public flag");

// ---- frames with linked blocks (lz4hip_lz4f_linked.hpp), for both decode sequences below ------------------------------------------------
// one lane per table row in single-wavefront workgroups; one wavefront per item in workgroups of kWaveDecodeWavesPerGroup: more rows
// or items than the grid holds share lanes and wavefronts
inline Grid lz4f_linked_rows_grid(int64_t rows)
{
    const int64_t g = (rows + kSizesThreads - 1) / kSizesThreads;
    return { g < 1 ? 1u : (g > (int64_t)kStreamsMaxWalkGroups ? kStreamsMaxWalkGroups : (unsigned)g), kGridItems };
}
inline Grid lz4f_linked_items_grid(int64_t n)
{
    const int64_t g = (n + kWaveDecodeWavesPerGroup - 1) / kWaveDecodeWavesPerGroup;
    return { g < 1 ? 1u : (g > (int64_t)kStreamsMaxWalkGroups ? kStreamsMaxWalkGroups : (unsigned)g), kGridWalk };
}
// before the rounds (and after the block checksums and the fill of the lowest bad rows): every linked row's size, every linked item's plan
template <class B>
int lz4f_linked_plan_run(B& be, const Lz4fLinked& a)
{
    be.launch(lz4f_linked_sizes_kernel, lz4f_linked_rows_grid(a.max_blocks), kSizesThreads, a);
    be.launch(lz4f_linked_plan_kernel, stream_grid(a.n), kStreamThreads, a);
    return be.last_error();
}
// after the last round, before the records: the linked items, one wavefront each
template <class B>
int lz4f_linked_decode_run(B& be, const Lz4fLinked& a, Lz4fNoDict)
{
    be.launch(lz4f_linked_decode_kernel, lz4f_linked_items_grid(a.n), 64 * kWaveDecodeWavesPerGroup, a);
    return be.last_error();
}
template <class B>
int lz4f_linked_decode_run(B& be, const Lz4fLinked& a, const Lz4fDict& d)
{
    be.launch(lz4f_linked_decode_dict_kernel, lz4f_linked_items_grid(a.n), 64 * kWaveDecodeWavesPerGroup, a, d.end, d.len);
    return be.last_error();
}

// The table's rows, for one frame (items < 0: one walk record, the content's checksum behind the rows', no item column) and for a batch
// of `items` frames (a walk record per item, each row's item).
inline Lz4fTables lz4f_tables(Carver& c, int64_t max_blocks, int64_t items = -1)
{
    Lz4fTables t;
    t.max_blocks = max_blocks;
    t.walk = c.take_as<int64_t>(8 * kLz4fWalkSlots * (items < 0 ? 1 : items));
    t.src_off = c.take_as<int64_t>(8 * max_blocks);
    t.hdr_off = c.take_as<int64_t>(8 * max_blocks);
    t.dst_off = c.take_as<int64_t>(8 * (max_blocks + 1));
    t.stored = c.take_as<int32_t>(4 * max_blocks);
    t.dec_len = c.take_as<int32_t>(4 * max_blocks);
    t.sum_len = c.take_as<int32_t>(4 * max_blocks);
    t.result = c.take_as<int32_t>(4 * max_blocks);
    t.sums = c.take_as<uint32_t>(4 * (max_blocks + (items < 0 ? 1 : 0)));
    t.row = c.take_as<uint8_t>(max_blocks);
    t.plan = c.take_as<int32_t>(4 * max_blocks);
    t.item = items < 0 ? nullptr : c.take_as<int32_t>(4 * max_blocks);
    return t;
}

// Both decodes of LZ4 frames over such a table.  Before the walk: the columns a row past the walks' count is read from are those of an
// empty block that belongs to item 0.
template <class B>
int lz4f_tables_init(B& be, const Lz4fTables& t)
{
    const int64_t n = t.max_blocks;
    LZ4HIP_FRAMING_TRY(be.fill(t.src_off, 0, (size_t)(8 * n)));
    LZ4HIP_FRAMING_TRY(be.fill(t.stored, 0, (size_t)(4 * n)));
    LZ4HIP_FRAMING_TRY(be.fill(t.dec_len, 0, (size_t)(4 * n)));
    LZ4HIP_FRAMING_TRY(be.fill(t.sum_len, 0, (size_t)(4 * n)));
    if (t.item) LZ4HIP_FRAMING_TRY(be.fill(t.item, 0, (size_t)(4 * n)));
    return be.fill(t.row, 0, (size_t)n);
}

// After the walk: the block checksums if asked for, the state block, the linked rows' plan if accepted, the compact decode's rounds
// over ALL max_blocks rows with the frames' own sizes step and pack layout (p.b is the table: its src_off, dec_len and result columns
// and its dst_off as p.dst_off), the linked items' decode.  `total` and `base` are the batch's (nullptr: one frame), `item_bad` every
// item's lowest bad row: for one frame the state block's kPackedBad slot.  `dict`: Lz4fNoDict, or the call's dictionary, which every
// compressed row of the rounds and every linked row then has in front of it.
template <class B, class D>
int lz4f_rows_run(B& be, const PackedPlan& p, const Lz4fTables& t, unsigned flags, int64_t items, const int64_t* base, const int64_t* total,
                  unsigned long long* item_bad, const D& dict)
{
    const uint8_t* src = (const uint8_t*)p.b.src;
    if (flags & kLz4fVerifyBlocks) {
        const XxhRows rows = { src, t.src_off, 0, t.sum_len, nullptr, 0, 0u, t.sums, t.max_blocks };
        LZ4HIP_FRAMING_TRY(xxh32_rows_run(be, rows));
        be.launch(lz4f_verify_kernel, stream_grid(t.max_blocks), kStreamThreads, src, t, total);
    }
    LZ4HIP_FRAMING_TRY(packed_state_init(be, p.l));
    const Lz4fLinked linked = { src, p.dst, p.dst_cap, items, t.max_blocks, t.walk, base, total, t.src_off, t.stored, t.dst_off, t.row, t.plan, item_bad };
    if (flags & kLz4fAcceptLinked) LZ4HIP_FRAMING_TRY(lz4f_linked_plan_run(be, linked));
    const auto round = [&](const PackedRound& a) {
        const int64_t f = a.first;
        return Lz4fRound{ a, src, t.src_off + f, t.stored + f, t.row + f, t.plan + f, t.item ? t.item + f : nullptr, t.walk, item_bad };
    };
    LZ4HIP_FRAMING_TRY(packed_rounds(be, p, [&](const lz4hip_batch_t* rb) { return lz4f_round_decode(be, rb, dict); },
                                     [&](const PackedRound& a, Grid grid) { be.launch(lz4f_round_sizes_kernel, grid, kStreamThreads, round(a)); },
                                     [&](const PackedRound& a, Grid grid) { be.launch(lz4f_round_pack_kernel, grid, kStreamThreads, Lz4fRoundLayout{ round(a) }, p.dst, p.dst_cap); }));
    if (flags & kLz4fAcceptLinked) LZ4HIP_FRAMING_TRY(lz4f_linked_decode_run(be, linked, dict));
    return 0;
}

// the rounds' plan over a table: the table IS the batch, every row at its offset in the source, decoded at its dec_len
inline PackedPlan lz4f_rounds_plan(const uint8_t* src, const Lz4fTables& t, const PackedScratch& l, int32_t slot_bytes, int64_t round_blocks, uint8_t* dst, int64_t dst_cap)
{
    PackedPlan p = {};
    p.b.src = src; p.b.src_off = t.src_off; p.b.src_len = t.dec_len; p.b.result = t.result; p.b.n_blocks = t.max_blocks;
    p.n = t.max_blocks; p.round = packed_round(t.max_blocks, round_blocks); p.slot = packed_slot(slot_bytes); p.limit = slot_bytes; p.l = l;
    p.dst = dst; p.dst_cap = dst_cap; p.dst_off = t.dst_off;
    return p;
}

struct Lz4fDecodeScratch { Lz4fTables t; PackedScratch l; int64_t bytes; };
inline Lz4fDecodeScratch lz4f_decode_scratch(void* scratch, int32_t slot, int64_t max_blocks, int64_t round_blocks)
{
    Carver c(scratch);
    Lz4fDecodeScratch d;
    d.t = lz4f_tables(c, max_blocks);
    d.l = packed_scratch(c.take_as<uint8_t>(0), max_blocks, slot, round_blocks);
    d.bytes = c.at + d.l.bytes;
    return d;
}
inline int64_t lz4f_decode_scratch_bytes(int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    if (!lz4f_slot_valid(slot_bytes) || max_blocks < 1 || round_blocks < 0) return LZ4HIP_E_ARGUMENT;
    return lz4f_decode_scratch(nullptr, lz4f_slot(slot_bytes), max_blocks, round_blocks).bytes;
}

struct Lz4fDecodePlan {
    const uint8_t* src; int64_t src_len; int32_t slot_bytes; unsigned flags; Lz4fTables t; PackedPlan rounds; Lz4fInfo* info;
};

// The walk, then what both decodes of LZ4 frames share (lz4f_rows_run: the block checksums and the rounds over ALL max_blocks rows of the
// table; the rows past the walk's count are empty blocks, which decode to nothing), the record, the content checksum.  Nothing is
// read on the host between the steps.  The decoders are handed the table's dec_len column through the round's sanitised copy: a raw
// row and a row with a bad checksum arrive as empty blocks, and so does every row of a frame with linked blocks, which a caller who
// accepts them (kLz4fAcceptLinked) gets sized before the rounds and decoded after them.  The frame is the batch of one item, whose
// lowest bad row is the state block's lowest failed index.  `dict`: as lz4f_rows_run's.
template <class B, class D = Lz4fNoDict>
int lz4f_decode_run(B& be, const Lz4fDecodePlan& p, const D& dict = D())
{
    const Lz4fTables& t = p.t;
    unsigned long long* const bad = (unsigned long long*)(p.rounds.l.state + kPackedBad);
    LZ4HIP_FRAMING_TRY(lz4f_tables_init(be, t));
    be.launch(lz4f_walk_kernel, fixed_grid(1), 64, p.src, p.src_len, p.slot_bytes, lz4f_walk_flags(p.flags, dict), t, lz4f_walk_dict_id(dict));
    LZ4HIP_FRAMING_TRY(be.last_error());
    LZ4HIP_FRAMING_TRY(lz4f_rows_run(be, p.rounds, t, p.flags, 1, nullptr, nullptr, bad, dict));
    be.launch(lz4f_info_kernel, fixed_grid(1), 64, t, (const unsigned long long*)bad, p.flags, p.rounds.dst_cap, p.info);
    if (p.flags & kLz4fVerifyContent) {
        const XxhRows content = { p.rounds.dst, nullptr, 0, nullptr, t.walk + kLz4fWalkContentLen, 0, 0u, t.sums + t.max_blocks, 1 };
        LZ4HIP_FRAMING_TRY(xxh32_rows_run(be, content));
        be.launch(lz4f_final_kernel, fixed_grid(1), 64, p.src, t, p.info);
    }
    return be.last_error();
}

template <class B>
int lz4f_decode_plan(B& be, const void* src, int64_t src_len, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags,
                     void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, Lz4fDecodePlan& p)
{
    if (src_len < 0 || max_blocks < 1 || round_blocks < 0 || dst_cap < 0 || !info || !scratch || (src_len > 0 && !src) || (dst_cap > 0 && !dst))
        return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: negative size, max_blocks < 1 or NULL pointer");
    if (!lz4f_slot_valid(slot_bytes)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: slot_bytes must be 0 (4 MiB), 65536, 262144, 1048576 or 4194304");
    if (flags & ~kLz4fDecodeFlags) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: unknown flag");
    if (packed_round(max_blocks, round_blocks) > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: more than 2^31 - 1 table rows in a round");
    p.slot_bytes = lz4f_slot(slot_bytes);
    const Lz4fDecodeScratch d = lz4f_decode_scratch(scratch, p.slot_bytes, max_blocks, round_blocks);
    if (scratch_bytes < d.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: scratch_bytes < lz4hip_lz4f_decode_scratch_bytes");
    // (an empty source's rows are all empty: any address will do for them)
    p.src = src ? (const uint8_t*)src : (const uint8_t*)scratch; p.src_len = src_len; p.flags = flags; p.t = d.t;
    p.rounds = lz4f_rounds_plan(p.src, d.t, d.l, p.slot_bytes, round_blocks, (uint8_t*)dst, dst_cap);
    p.info = (Lz4fInfo*)info;
    return 0;
}

template <class B, class D = Lz4fNoDict>
int lz4f_decode(B& be, const void* src, int64_t src_len, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch,
                int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, const D& dict = D())
{
    Lz4fDecodePlan p;
    LZ4HIP_FRAMING_TRY(lz4f_decode_plan(be, src, src_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info, p));
    return lz4f_decode_run(be, p, dict);
}

// lz4hip_lz4f_decode_dict_device: the plain call's checks and plan behind the dictionary's own check; without a dictionary (dict_len
// == 0) the plain sequence, which refuses a frame with a dictionary ID as ever
template <class B>
int lz4f_decode_dict_plan(B& be, const void* src, int64_t src_len, const void* dict, int64_t dict_len, int32_t slot_bytes, int64_t max_blocks,
                          int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info,
                          Lz4fDecodePlan& p)
{
    LZ4HIP_FRAMING_TRY(lz4f_dict_check(be, dict, dict_len));
    return lz4f_decode_plan(be, src, src_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info, p);
}
template <class B>
int lz4f_decode_dict_run(B& be, const Lz4fDecodePlan& p, const void* dict, int64_t dict_len, uint32_t dict_id)
{
    return dict_len > 0 ? lz4f_decode_run(be, p, lz4f_dict_of(dict, dict_len, dict_id)) : lz4f_decode_run(be, p);
}

// ---- batches of LZ4 frames (lz4hip_lz4f_batch.hpp) --------------------------------------------------------------------------------------
// Many independent frames per call: the one-frame path's kernels, scan, copy routine and row checksums around ONE block encoder call
// over the blocks of all items, and around the compact decode's rounds over the rows of all items.
static_assert(sizeof(Lz4fBatchInfo) == sizeof(lz4hip_lz4f_batch_info_t) && offsetof(Lz4fBatchInfo, first_error) == offsetof(lz4hip_lz4f_batch_info_t, first_error) &&
              offsetof(Lz4fBatchInfo, error) == offsetof(lz4hip_lz4f_batch_info_t, error), "Lz4fBatchInfo must mirror lz4hip_lz4f_batch_info_t");
static_assert(kLz4fBatchBadOffsets == LZ4HIP_E_ARGUMENT, "lz4f batch statuses");

// the block table's rows: the host does not know the offsets, only that sum ceil(len_i / block) <= src_len / block + n
inline int64_t lz4f_batch_cap(int64_t n, int64_t src_len, int64_t block) { return src_len / block + n; }

// n descriptors, EndMarks and content checksums, and every row of the block table stored raw behind its size field
inline int64_t lz4f_batch_bound(int64_t n, int64_t src_len, int block_size_id, unsigned flags, uint32_t dict_id = 0)
{
    if (!lz4f_id_valid(block_size_id) || (flags & ~kLz4fEncodeFlags)) return LZ4HIP_E_ARGUMENT;
    if (n < 0) n = 0;
    if (src_len < 0) src_len = 0;
    const int64_t cap = lz4f_batch_cap(n, src_len, lz4f_block_bytes(lz4f_id(block_size_id)));
    return n * (lz4f_head_len(flags, dict_id) + 4 + ((flags & kLz4fContentChecksum) ? 4 : 0)) + src_len + cap * (4 + ((flags & kLz4fBlockChecksum) ? 4 : 0));
}
inline int64_t lz4f_batch_dict_bound(int64_t n, int64_t src_len, int block_size_id, unsigned flags, int64_t dict_len, uint32_t dict_id)
{
    if (dict_len < 0) return LZ4HIP_E_ARGUMENT;
    return lz4f_batch_bound(n, src_len, block_size_id, flags, dict_len > 0 ? dict_id : 0);
}

// lz4f batch encode: the encoder's output (every block at its own source position), the items' spans and first blocks, the block total,
// the block table (position, length, capacity, result, checksum row), the cap + n checksums, the n descriptors, the segments' items and
// sizes / offsets + the total, the scans' tile sums
struct Lz4fBatchEncodeScratch {
    uint8_t* comp; int64_t* item_at; int64_t* item_len; int64_t* first; int64_t* total; int64_t* c_at; int32_t* c_len; int32_t* c_cap; int32_t* result;
    int64_t* row_off; int32_t* row_len; uint32_t* sums; uint8_t* head; int32_t* seg_item; int64_t* offs; int64_t* partial; uint8_t* primed; int64_t bytes;
};
// With a dictionary (dict_len > 0) the plain layout, then the n descriptors' kLz4fDictHeadMax bytes each and the 16 KiB primed table.
inline Lz4fBatchEncodeScratch lz4f_batch_encode_scratch(void* scratch, int64_t n, int64_t src_len, int64_t block, int64_t dict_len = 0)
{
    const int64_t cap = lz4f_batch_cap(n, src_len, block), segs = cap + 2 * n;
    Carver c(scratch);
    Lz4fBatchEncodeScratch l;
    l.comp = c.take_as<uint8_t>(src_len);
    l.item_at = c.take_as<int64_t>(8 * n);
    l.item_len = c.take_as<int64_t>(8 * n);
    l.first = c.take_as<int64_t>(8 * n);
    l.total = c.take_as<int64_t>(256);
    l.c_at = c.take_as<int64_t>(8 * cap);
    l.c_len = c.take_as<int32_t>(4 * cap);
    l.c_cap = c.take_as<int32_t>(4 * cap);
    l.result = c.take_as<int32_t>(4 * cap);
    l.row_off = c.take_as<int64_t>(8 * cap);
    l.row_len = c.take_as<int32_t>(4 * cap);
    l.sums = c.take_as<uint32_t>(4 * (cap + n));
    l.head = c.take_as<uint8_t>(kLz4fHeadMax * n);
    l.seg_item = c.take_as<int32_t>(4 * segs);
    l.offs = c.take_as<int64_t>(8 * (segs + 1));
    l.partial = c.take_as<int64_t>(8 * scan_tiles(segs));              // (segs >= n: both scans fit)
    l.primed = nullptr;
    if (dict_len > 0) {
        l.head = c.take_as<uint8_t>(kLz4fDictHeadMax * n);
        l.primed = c.take_as<uint8_t>(kFastTableBytes);
    }
    l.bytes = c.at;
    return l;
}

struct Lz4fBatchEncodePlan {
    Lz4fBatchEncodeArgs a; int mode; int32_t* result; int64_t* row_off; int32_t* row_len; int64_t* partial; uint8_t* dst; int64_t dst_cap; int64_t* dst_off;
    int64_t bound;
};

// a.comp and a.result are the block encoder's to write, every block at its own source position.  Rows past the blocks' count are
// empty blocks, which read and write nothing.  `dict`: as lz4f_encode_run's.
template <class B> void lz4f_batch_head_launch(B& be, const Lz4fBatchEncodeArgs& a, int64_t segs, Lz4fNoDict)
{
    be.launch(lz4f_batch_head_kernel, stream_grid(a.n), kStreamThreads, a);
    be.launch(lz4f_batch_sizes_kernel, stream_grid(segs), kStreamThreads, a);
}
template <class B> void lz4f_batch_head_launch(B& be, const Lz4fBatchEncodeArgs& a, int64_t segs, const Lz4fDict& d)
{
    be.launch(lz4f_batch_dict_head_kernel, stream_grid(a.n), kStreamThreads, a, lz4f_head_of(d));
    be.launch(lz4f_batch_dict_sizes_kernel, stream_grid(segs), kStreamThreads, a, lz4f_head_of(d));
}
template <class B> void lz4f_batch_pack_launch(B& be, const Lz4fBatchEncodePlan& p, Lz4fNoDict)
{
    Lz4fBatchLayout layout = { p.a };
    be.launch(lz4f_batch_pack_kernel, copy_grid(p.bound), kStreamThreads, layout, p.dst, p.dst_cap);
}
template <class B> void lz4f_batch_pack_launch(B& be, const Lz4fBatchEncodePlan& p, const Lz4fDict& d)
{
    Lz4fBatchDictLayout layout = { p.a, lz4f_head_of(d) };
    be.launch(lz4f_batch_dict_pack_kernel, copy_grid(p.bound), kStreamThreads, layout, p.dst, p.dst_cap);
}

template <class B, class D = Lz4fNoDict>
int lz4f_batch_encode_run(B& be, const Lz4fBatchEncodePlan& p, const D& dict = D())
{
    const Lz4fBatchEncodeArgs& a = p.a;
    if (a.n == 0) return be.fill(p.dst_off, 0, sizeof(int64_t));
    const int64_t segs = a.cap + 2 * a.n;
    be.launch(lz4f_batch_counts_kernel, stream_grid(a.n), kStreamThreads, a);
    launch_scan(be, a.first, a.n, p.partial, (int64_t*)a.total);
    be.launch(lz4f_batch_blocks_kernel, stream_grid(a.cap), kStreamThreads, a);
    LZ4HIP_FRAMING_TRY(be.last_error());
    lz4hip_batch_t b = {};
    b.src = a.src; b.src_off = a.c_at; b.src_len = a.c_len;
    b.dst = (void*)a.comp; b.dst_off = a.c_at; b.dst_cap = a.c_cap;
    b.src_len_all = a.block; b.result = p.result; b.n_blocks = a.cap;
    LZ4HIP_FRAMING_TRY(lz4f_blocks_encode(be, &b, p.mode, dict));
    if (a.flags & kLz4fBlockChecksum) {
        be.launch(lz4f_batch_rows_kernel, stream_grid(a.cap), kStreamThreads, a, p.row_off, p.row_len);
        const XxhRows rows = { a.src, p.row_off, 0, p.row_len, nullptr, 0, 0u, a.sums, a.cap };
        LZ4HIP_FRAMING_TRY(xxh32_rows_run(be, rows));
    }
    if (a.flags & kLz4fContentChecksum) {
        const XxhRows content = { a.src, a.item_at, 0, nullptr, a.item_len, 0, 0u, a.sums + a.cap, a.n };
        LZ4HIP_FRAMING_TRY(xxh32_rows_run(be, content));
    }
    lz4f_batch_head_launch(be, a, segs, dict);
    launch_scan(be, a.offs, segs, p.partial, a.offs + segs);
    be.launch(lz4f_batch_offsets_kernel, stream_grid(a.n + 1), kStreamThreads, a, p.dst_off);
    lz4f_batch_pack_launch(be, p, dict);
    return be.last_error();
}

template <class B>
int lz4f_batch_encode_plan(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int mode, unsigned flags,
                           void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, Lz4fBatchEncodePlan& p, int64_t dict_len = 0,
                           uint32_t dict_id = 0, uint8_t** primed = nullptr)
{
    if (src_len < 0 || n < 0 || !dst_off) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: src_len < 0, n < 0 or dst_off is NULL");
    if (!lz4f_id_valid(block_size_id)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: block_size_id must be 0 (64 KiB) or 4 .. 7");
    if (flags & ~kLz4fEncodeFlags) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: unknown flag");
    if (mode != LZ4HIP_MODE_FAST && mode != LZ4HIP_MODE_HC) return be.fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    const int id = lz4f_id(block_size_id);
    const int64_t block = lz4f_block_bytes(id), cap = lz4f_batch_cap(n, src_len, block);
    if (n > 0x3FFFFFFF || cap > 0x3FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: more than 2^30 - 1 items or blocks");
    p.bound = lz4f_batch_bound(n, src_len, block_size_id, flags, dict_id);
    if (n > 0 && dst_cap < p.bound)
        return be.fail(LZ4HIP_E_ARGUMENT, dict_len > 0 ? "lz4f batch encode: dst_cap < lz4hip_lz4f_batch_dict_bound" : "lz4f batch encode: dst_cap < lz4hip_lz4f_batch_bound");
    const Lz4fBatchEncodeScratch l = lz4f_batch_encode_scratch(scratch, n, src_len, block, dict_len);
    if (n > 0 && scratch_bytes < l.bytes)
        return be.fail(LZ4HIP_E_ARGUMENT, dict_len > 0 ? "lz4f batch encode: scratch_bytes < lz4hip_lz4f_batch_encode_dict_scratch_bytes"
                                                       : "lz4f batch encode: scratch_bytes < lz4hip_lz4f_batch_encode_scratch_bytes");
    if (n > 0 && ((src_len > 0 && !src) || !src_off || !dst || !scratch))
        return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: src, src_off, dst and scratch must be non-NULL");
    Lz4fBatchEncodeArgs& a = p.a;
    // (an empty source's items are all empty: any address will do for them)
    a.src = src ? (const uint8_t*)src : (const uint8_t*)scratch; a.comp = l.comp; a.off = src_off; a.src_len = src_len; a.n = n; a.cap = cap;
    a.block = (int32_t)block; a.block_id = id; a.flags = flags;
    a.item_at = l.item_at; a.item_len = l.item_len; a.first = l.first; a.total = l.total; a.c_at = l.c_at; a.c_len = l.c_len; a.c_cap = l.c_cap;
    a.result = l.result; a.sums = l.sums; a.head = l.head; a.seg_item = l.seg_item; a.offs = l.offs;
    p.mode = mode; p.result = l.result; p.row_off = l.row_off; p.row_len = l.row_len; p.partial = l.partial;
    p.dst = (uint8_t*)dst; p.dst_cap = dst_cap; p.dst_off = dst_off;
    if (primed) *primed = l.primed;
    return 0;
}

template <class B>
int lz4f_batch_encode(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int mode, unsigned flags, void* dst,
                      int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes)
{
    Lz4fBatchEncodePlan p;
    LZ4HIP_FRAMING_TRY(lz4f_batch_encode_plan(be, src, src_len, src_off, n, block_size_id, mode, flags, dst, dst_cap, dst_off, scratch, scratch_bytes, p));
    return lz4f_batch_encode_run(be, p);
}

// lz4hip_lz4f_batch_encode_dict_device, as lz4f_encode_dict_plan / _run: one dictionary and one ID for every item
template <class B>
int lz4f_batch_encode_dict_plan(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                int block_size_id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes,
                                Lz4fBatchEncodePlan& p, Lz4fDict& d)
{
    LZ4HIP_FRAMING_TRY(lz4f_dict_check(be, dict, dict_len));
    d = lz4f_dict_of(dict, dict_len, dict_len > 0 ? dict_id : 0);
    return lz4f_batch_encode_plan(be, src, src_len, src_off, n, block_size_id, LZ4HIP_MODE_FAST, flags, dst, dst_cap, dst_off, scratch, scratch_bytes, p, dict_len,
                                  d.id, &d.primed);
}
template <class B>
int lz4f_batch_encode_dict_run(B& be, const Lz4fBatchEncodePlan& p, const Lz4fDict& d)
{
    return d.len > 0 ? lz4f_batch_encode_run(be, p, d) : lz4f_batch_encode_run(be, p);
}

template <class B>
int lz4f_batch_encode_dict(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                           int block_size_id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes)
{
    Lz4fBatchEncodePlan p;
    Lz4fDict d;
    LZ4HIP_FRAMING_TRY(lz4f_batch_encode_dict_plan(be, src, src_len, src_off, n, dict, dict_len, dict_id, block_size_id, flags, dst, dst_cap, dst_off, scratch,
                                                   scratch_bytes, p, d));
    return lz4f_batch_encode_dict_run(be, p, d);
}

// lz4f batch decode: what is kept per item (the walk's records, spans, first rows, lowest bad rows, content rows), the totals, the
// scan's tile sums, the table of max_blocks rows, then the compact decode's scratch for max_blocks rows of slot_bytes
inline Lz4fBatchTables lz4f_batch_tables(Carver& c, int64_t n, int64_t max_blocks)
{
    Lz4fBatchTables t;
    t.n = n;
    t.total = c.take_as<int64_t>(256);
    t.min_bad = (unsigned long long*)t.total + 1;
    t.item_at = c.take_as<int64_t>(8 * n);
    t.base = c.take_as<int64_t>(8 * n);
    t.item_bad = c.take_as<unsigned long long>(8 * n);
    t.content_off = c.take_as<int64_t>(8 * n);
    t.content_len = c.take_as<int64_t>(8 * n);
    t.content_sums = c.take_as<uint32_t>(4 * n);
    t.rows = lz4f_tables(c, max_blocks, n);
    return t;
}
struct Lz4fBatchDecodeScratch { Lz4fBatchTables t; int64_t* partial; PackedScratch l; int64_t bytes; };
inline Lz4fBatchDecodeScratch lz4f_batch_decode_scratch(void* scratch, int64_t n, int32_t slot, int64_t max_blocks, int64_t round_blocks)
{
    Carver c(scratch);
    Lz4fBatchDecodeScratch d;
    d.t = lz4f_batch_tables(c, n, max_blocks);
    d.partial = c.take_as<int64_t>(8 * scan_tiles(n));
    d.l = packed_scratch(c.take_as<uint8_t>(0), max_blocks, slot, round_blocks);
    d.bytes = c.at + d.l.bytes;
    return d;
}
inline int64_t lz4f_batch_decode_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    if (n < 0 || !lz4f_slot_valid(slot_bytes) || max_blocks < 1 || round_blocks < 0) return LZ4HIP_E_ARGUMENT;
    return lz4f_batch_decode_scratch(nullptr, n, lz4f_slot(slot_bytes), max_blocks, round_blocks).bytes;
}

struct Lz4fBatchDecodePlan {
    Lz4fBatchDecodeArgs a; Lz4fBatchTables t; int64_t* partial; PackedPlan rounds; Lz4fBatchInfo* info;
};

// The two walks around their scan, then what both decodes of LZ4 frames share (lz4f_rows_run: the block checksums and the rounds over ALL
// max_blocks rows of the table, a linked item's rows sized before them and decoded after them), the items' records, their content
// checksums as n rows of one launch, the batch's record.  Nothing is read on the host between the steps.  `dict`: as lz4f_rows_run's.
template <class B, class D = Lz4fNoDict>
int lz4f_batch_decode_run(B& be, const Lz4fBatchDecodePlan& p, const D& dict = D())
{
    Lz4fBatchDecodeArgs a = p.a;
    a.flags = lz4f_walk_flags(p.a.flags, dict); a.dict_id = lz4f_walk_dict_id(dict);
    const Lz4fBatchTables& t = p.t;
    LZ4HIP_FRAMING_TRY(be.fill(a.written_items, 0, sizeof(int64_t)));
    if (a.n == 0) {
        LZ4HIP_FRAMING_TRY(be.fill(a.dst_off, 0, sizeof(int64_t)));
        be.launch(lz4f_batch_empty_record_kernel, fixed_grid(1), 64, p.info);
        return be.last_error();
    }
    LZ4HIP_FRAMING_TRY(lz4f_tables_init(be, t.rows));
    LZ4HIP_FRAMING_TRY(be.fill(t.total, 0, 8));
    LZ4HIP_FRAMING_TRY(be.fill(t.min_bad, 0xFF, 8));                   // the lowest failing item = none
    LZ4HIP_FRAMING_TRY(be.fill(t.item_bad, 0xFF, (size_t)(8 * a.n)));  // every item's lowest bad row = none
    be.launch(lz4f_batch_walk_kernel<false>, walk_grid(a.n), 64, a, t);
    launch_scan(be, t.base, a.n, p.partial, t.total);
    be.launch(lz4f_batch_walk_kernel<true>, walk_grid(a.n), 64, a, t);
    LZ4HIP_FRAMING_TRY(be.last_error());
    LZ4HIP_FRAMING_TRY(lz4f_rows_run(be, p.rounds, t.rows, a.flags, a.n, t.base, t.total, t.item_bad, dict));
    be.launch(lz4f_batch_offsets_out_kernel, stream_grid(a.n + 1), kStreamThreads, a, t);
    be.launch(lz4f_batch_info_kernel, stream_grid(a.n), kStreamThreads, a, t);
    if (a.flags & kLz4fVerifyContent) {
        const XxhRows content = { p.rounds.dst, t.content_off, 0, nullptr, t.content_len, 0, 0u, t.content_sums, a.n };
        LZ4HIP_FRAMING_TRY(xxh32_rows_run(be, content));
        be.launch(lz4f_batch_final_kernel, stream_grid(a.n), kStreamThreads, a, t);
    }
    be.launch(lz4f_batch_record_kernel, fixed_grid(1), 64, a, t, p.info);
    return be.last_error();
}

template <class B>
int lz4f_batch_decode_plan(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t slot_bytes, int64_t max_blocks,
                           int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off,
                           lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, int64_t* written_items, Lz4fBatchDecodePlan& p)
{
    if (src_len < 0 || n < 0 || max_blocks < 1 || round_blocks < 0 || dst_cap < 0 || !dst_off || !info || !written_items || (dst_cap > 0 && !dst))
        return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: negative size, max_blocks < 1 or NULL pointer");
    if (n > 0 && (!src_off || !item_info || !scratch || (src_len > 0 && !src))) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: NULL pointer");
    if (n > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: more than 2^31 - 1 items");
    if (!lz4f_slot_valid(slot_bytes)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: slot_bytes must be 0 (4 MiB), 65536, 262144, 1048576 or 4194304");
    if (flags & ~kLz4fDecodeFlags) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: unknown flag");
    if (packed_round(max_blocks, round_blocks) > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: more than 2^31 - 1 table rows in a round");
    const int32_t slot = lz4f_slot(slot_bytes);
    const Lz4fBatchDecodeScratch d = lz4f_batch_decode_scratch(scratch, n, slot, max_blocks, round_blocks);
    if (n > 0 && scratch_bytes < d.bytes) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: scratch_bytes < lz4hip_lz4f_batch_decode_scratch_bytes");
    Lz4fBatchDecodeArgs& a = p.a;
    // (an empty source's rows are all empty: any address will do for them)
    a.src = src ? (const uint8_t*)src : (const uint8_t*)scratch; a.off = src_off; a.src_len = src_len; a.n = n; a.slot_bytes = slot; a.flags = flags;
    a.dst_cap = dst_cap; a.dst_off = dst_off; a.item_info = (Lz4fInfo*)item_info; a.written_items = written_items; a.dict_id = 0;
    p.t = d.t; p.partial = d.partial; p.rounds = lz4f_rounds_plan(a.src, d.t.rows, d.l, slot, round_blocks, (uint8_t*)dst, dst_cap);
    p.info = (Lz4fBatchInfo*)info;
    return 0;
}

template <class B, class D = Lz4fNoDict>
int lz4f_batch_decode(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks,
                      unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info,
                      lz4hip_lz4f_batch_info_t* info, int64_t* written_items, const D& dict = D())
{
    Lz4fBatchDecodePlan p;
    LZ4HIP_FRAMING_TRY(lz4f_batch_decode_plan(be, src, src_len, src_off, n, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap,
                                              dst_off, item_info, info, written_items, p));
    return lz4f_batch_decode_run(be, p, dict);
}

// lz4hip_lz4f_batch_decode_dict_device, as lz4f_decode_dict_plan / lz4f_decode_dict_run are the one-frame call's
template <class B>
int lz4f_batch_decode_dict_plan(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, int32_t slot_bytes,
                                int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, int64_t* written_items, Lz4fBatchDecodePlan& p)
{
    LZ4HIP_FRAMING_TRY(lz4f_dict_check(be, dict, dict_len));
    return lz4f_batch_decode_plan(be, src, src_len, src_off, n, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, dst_off,
                                  item_info, info, written_items, p);
}
template <class B>
int lz4f_batch_decode_dict_run(B& be, const Lz4fBatchDecodePlan& p, const void* dict, int64_t dict_len, uint32_t dict_id)
{
    return dict_len > 0 ? lz4f_batch_decode_run(be, p, lz4f_dict_of(dict, dict_len, dict_id)) : lz4f_batch_decode_run(be, p);
}


// ---- the host-pointer calls ------------------------------------------------------------------------------------------------------------
// Each stages its arguments in ONE device image, runs the device path above on it and copies the results out.  An image is a Carver's
// walk over no buffer -- its pieces are offsets, good for any base -- plus the base of the backend's reserve.  That base may move
// whenever the image grows: a decoder that reserves again stages its source again, and keeps no pointer into the image across it.

// a call's per-item arrays on the host and their pieces of the image
struct Items { int64_t n; int64_t* dst_off; int64_t doff_at; int32_t* status; int64_t st_at; int64_t* error_offset; int64_t eo_at; };

template <class B>
struct Image {
    B& be;
    uint8_t* d = nullptr;
    int64_t* i64(int64_t piece) const { return (int64_t*)(d + piece); }
    int32_t* i32(int64_t piece) const { return (int32_t*)(d + piece); }
    int reserve(int64_t bytes) { return be.reserve((size_t)bytes, d); }
    int upload(int64_t piece, const void* host, int64_t bytes) { return be.upload(d + piece, host, (size_t)bytes); }
    int download(void* host, int64_t piece, int64_t bytes) { return be.download(host, d + piece, (size_t)bytes); }
    // the source, which is the image's first piece, and the n + 1 offsets of a call that has any
    int upload_source(const void* src, int64_t src_len, const int64_t* src_off = nullptr, int64_t n = 0, int64_t off_at = -1)
    {
        if (src_len > 0) LZ4HIP_FRAMING_TRY(upload(0, src, src_len));
        return off_at < 0 ? 0 : upload(off_at, src_off, 8 * (n + 1));
    }
    // the per-item arrays: n + 1 output offsets, then n statuses (wrap: results) and n error offsets where the caller has such an array
    int download_items(const Items& it)
    {
        LZ4HIP_FRAMING_TRY(download(it.dst_off, it.doff_at, 8 * (it.n + 1)));
        if (it.status && it.n > 0) LZ4HIP_FRAMING_TRY(download(it.status, it.st_at, 4 * it.n));
        if (it.error_offset) LZ4HIP_FRAMING_TRY(download(it.error_offset, it.eo_at, 8 * it.n));
        return 0;
    }
    // an encoder's output: the total has arrived on the host, the bytes follow
    int download_encoded(void* dst, int64_t out_at, int64_t total)
    {
        if (total > 0) LZ4HIP_FRAMING_TRY(download(dst, out_at, total));
        return be.sync();
    }
    // a decoder's results: the final info, the per-item arrays where there are any, the bytes
    template <class Info>
    int download_decoded(Info* info, int64_t info_at, void* dst, int64_t out_at, int64_t decoded_bytes, const Items* it = nullptr)
    {
        LZ4HIP_FRAMING_TRY(download(info, info_at, sizeof *info));
        if (it) LZ4HIP_FRAMING_TRY(download_items(*it));
        if (decoded_bytes > 0) LZ4HIP_FRAMING_TRY(download(dst, out_at, decoded_bytes));
        return be.sync();
    }
};

// The LZ4Stream decoders and the legacy frame's (whose code for a full table is its own: `table_full`) index until their guesses hold.  `index` lays the image out for the current max_chunks and out_bytes,
// stages the source, runs the index and queues the download of its info into h.  A full table is indexed again with the count it
// reported, an output that has to grow with the size it reported: three passes at most, whatever they went on.  A size above dst_cap
// ends the loop at once; the caller refuses it, as it does a table still full after the third pass.
template <class B, class Info, class Index>
int settle(B& be, int64_t dst_cap, int64_t& max_chunks, int64_t& out_bytes, const Info& h, Index index, int table_full = LZ4HIP_STREAM_TABLE_FULL)
{
    for (int attempt = 0;; attempt++) {
        LZ4HIP_FRAMING_TRY(index());
        LZ4HIP_FRAMING_TRY(be.sync());
        if (attempt >= 2) return 0;
        if (h.error == table_full) max_chunks = h.chunks;
        else if (h.decoded_bytes > dst_cap || h.decoded_bytes <= out_bytes) return 0;
        else out_bytes = h.decoded_bytes;
    }
}

inline int64_t guessed_output(int64_t src_len, int64_t dst_cap) { return dst_cap < 4 * src_len ? dst_cap : 4 * src_len; }

template <class B>
int stream_encode_host(B& be, const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len)
{
    if (src_len < 0 || !dst_len || (src_len > 0 && (!src || !dst))) return be.fail(LZ4HIP_E_ARGUMENT, "stream encode: negative size or NULL pointer");
    const int64_t bound = stream_bound(src_len, block_size);
    if (dst_cap < bound) return be.fail(LZ4HIP_E_ARGUMENT, "stream encode: dst_cap < lz4hip_stream_bound");
    if (src_len == 0) { *dst_len = 0; return 0; }
    // device image: [source | stream | scratch | length]
    const int64_t scratch_bytes = stream_encode_scratch(nullptr, src_len, stream_block(block_size)).bytes;
    Carver c;
    c.take(src_len);
    const int64_t out_at = c.take(bound), scratch_at = c.take(scratch_bytes), len_at = c.take(256);
    Image<B> im = { be };
    LZ4HIP_FRAMING_TRY(im.reserve(c.at));
    LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len));
    LZ4HIP_FRAMING_TRY(stream_encode(be, im.d, src_len, block_size, mode, im.d + out_at, bound, im.i64(len_at), im.d + scratch_at, scratch_bytes));
    int64_t total = 0;
    LZ4HIP_FRAMING_TRY(im.download(&total, len_at, sizeof total));
    LZ4HIP_FRAMING_TRY(be.sync());
    LZ4HIP_FRAMING_TRY(im.download_encoded(dst, out_at, total));
    *dst_len = total;
    return 0;
}

// On dst_cap < decoded_bytes only *info is filled: there are no per-item arrays.
template <class B>
int stream_decode_host(B& be, const void* src, int64_t src_len, void* dst, int64_t dst_cap, lz4hip_stream_info_t* info)
{
    if (src_len < 0 || dst_cap < 0 || !info || (src_len > 0 && !src)) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: negative size or NULL pointer");
    // device image: [source | info | output | table]
    Image<B> im = { be };
    int64_t max_chunks = (src_len + 4095) / 4096 + 16, out_bytes = guessed_output(src_len, dst_cap), info_at = 0, out_at = 0, table_at = 0, table_bytes = 0;
    lz4hip_stream_info_t h = {};
    LZ4HIP_FRAMING_TRY(settle(be, dst_cap, max_chunks, out_bytes, h, [&] {
        table_bytes = stream_decode_scratch_bytes(max_chunks);
        Carver c;
        c.take(src_len);
        info_at = c.take(256); out_at = c.take(out_bytes); table_at = c.take(table_bytes);
        LZ4HIP_FRAMING_TRY(im.reserve(c.at));
        LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len));
        LZ4HIP_FRAMING_TRY(stream_index(be, im.d, src_len, max_chunks, im.d + table_at, table_bytes, (lz4hip_stream_info_t*)(im.d + info_at)));
        return im.download(&h, info_at, sizeof h);
    }));
    *info = h;
    if (h.error == LZ4HIP_STREAM_TABLE_FULL) return be.fail(LZ4HIP_E_DEVICE, "stream decode: the header walk did not settle");
    if (h.decoded_bytes > dst_cap) return be.fail(LZ4HIP_E_ARGUMENT, "stream decode: dst_cap < decoded_bytes (reported in info->decoded_bytes)");
    LZ4HIP_FRAMING_TRY(stream_decode(be, im.d, &h, max_chunks, im.d + table_at, table_bytes, im.d + out_at, out_bytes,
                                     (lz4hip_stream_info_t*)(im.d + info_at)));
    LZ4HIP_FRAMING_TRY(im.download_decoded(info, info_at, dst, out_at, h.decoded_bytes));
    return info->error;
}

template <class B>
int wrap_host(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode, void* dst, int64_t dst_cap, int64_t* dst_off,
              int32_t* result)
{
    if (src_len < 0 || n < 0 || !dst_off || (n > 0 && (!src_off || !dst)) || (src_len > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "wrap: negative size or NULL pointer");
    const int64_t bound = wrap_bound(n, src_len);
    if (dst_cap < bound) return be.fail(LZ4HIP_E_ARGUMENT, "wrap: dst_cap < lz4hip_wrap_bound");
    if (n == 0) { dst_off[0] = 0; return 0; }
    // device image: [source | offsets | output | output offsets | results | scratch]
    const int64_t scratch_bytes = wrap_scratch(nullptr, n, src_len).bytes;
    Carver c;
    c.take(src_len);
    const int64_t off_at = c.take(8 * (n + 1)), out_at = c.take(bound), doff_at = c.take(8 * (n + 1)), res_at = c.take(4 * n),
                  scratch_at = c.take(scratch_bytes);
    Image<B> im = { be };
    LZ4HIP_FRAMING_TRY(im.reserve(c.at));
    LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len, src_off, n, off_at));
    LZ4HIP_FRAMING_TRY(wrap_encode(be, im.d, src_len, im.i64(off_at), n, mode, im.d + out_at, bound, im.i64(doff_at),
                                   im.i32(res_at), im.d + scratch_at, scratch_bytes));
    LZ4HIP_FRAMING_TRY(im.download_items({ n, dst_off, doff_at, result, res_at, nullptr, 0 }));
    LZ4HIP_FRAMING_TRY(be.sync());
    return im.download_encoded(dst, out_at, dst_off[n] < dst_cap ? dst_off[n] : dst_cap);
}

// No table to outgrow, so two passes: the guessed output, then the size the first one reported.  On dst_cap < decoded_bytes the index's
// offsets and statuses are the caller's with the info: the Python wrappers' size query (dst_cap = 0) reads them.
template <class B>
int unwrap_host(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status,
                lz4hip_unwrap_info_t* info)
{
    if (src_len < 0 || n < 0 || dst_cap < 0 || !dst_off || !info || (n > 0 && (!src_off || !status)) || (src_len > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "unwrap: negative size or NULL pointer");
    // device image: [source | offsets | output offsets | statuses | info | scratch | output], the output not rounded up
    const int64_t scratch_bytes = unwrap_scratch_bytes(n);
    Carver c;
    c.take(src_len);
    const int64_t off_at = c.take(8 * (n + 1)), doff_at = c.take(8 * (n + 1)), st_at = c.take(4 * n), info_at = c.take(256),
                  scratch_at = c.take(scratch_bytes), out_at = c.at;
    const Items items = { n, dst_off, doff_at, status, st_at, nullptr, 0 };
    Image<B> im = { be };
    int64_t out_bytes = guessed_output(src_len, dst_cap);
    lz4hip_unwrap_info_t h = {};
    for (int attempt = 0; attempt < 2; attempt++) {
        LZ4HIP_FRAMING_TRY(im.reserve(out_at + out_bytes));
        LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len, src_off, n, off_at));
        LZ4HIP_FRAMING_TRY(unwrap_index(be, im.d, src_len, im.i64(off_at), n, im.i64(doff_at),
                                        im.i32(st_at), im.d + scratch_at, scratch_bytes, (lz4hip_unwrap_info_t*)(im.d + info_at)));
        LZ4HIP_FRAMING_TRY(im.download(&h, info_at, sizeof h));
        LZ4HIP_FRAMING_TRY(be.sync());
        if (h.decoded_bytes <= out_bytes || h.decoded_bytes > dst_cap) break;
        out_bytes = h.decoded_bytes;
    }
    *info = h;
    if (h.decoded_bytes > dst_cap || h.decoded_bytes > out_bytes) {
        LZ4HIP_FRAMING_TRY(im.download_items(items));
        LZ4HIP_FRAMING_TRY(be.sync());
        return be.fail(LZ4HIP_E_ARGUMENT, "unwrap: dst_cap < decoded_bytes (reported in info->decoded_bytes)");
    }
    LZ4HIP_FRAMING_TRY(unwrap_decode(be, im.d, src_len, im.i64(off_at), n, &h, im.d + scratch_at, scratch_bytes, im.d + out_at, out_bytes,
                                     im.i64(doff_at), im.i32(st_at), (lz4hip_unwrap_info_t*)(im.d + info_at)));
    LZ4HIP_FRAMING_TRY(im.download_decoded(info, info_at, dst, out_at, h.decoded_bytes, &items));
    return info->error;
}

template <class B>
int streams_encode_host(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode, void* dst,
                        int64_t dst_cap, int64_t* dst_off)
{
    if (src_len < 0 || n < 0 || !dst_off || (n > 0 && !src_off) || (src_len > 0 && n > 0 && (!src || !dst)))
        return be.fail(LZ4HIP_E_ARGUMENT, "streams encode: negative size or NULL pointer");
    // (the offsets are host memory here: bad ones are refused instead of encoded as empty items)
    for (int64_t i = 0; i < n; i++)
        if (src_off[i] < 0 || src_off[i + 1] < src_off[i] || src_off[i + 1] > src_len)
            return be.fail(LZ4HIP_E_ARGUMENT, "streams encode: offsets decrease or fall outside [0, src_len]");
    const int64_t bound = streams_bound(n, src_len, block_size);
    if (n > 0 && dst_cap < bound) return be.fail(LZ4HIP_E_ARGUMENT, "streams encode: dst_cap < lz4hip_streams_bound");
    if (n == 0 || src_len == 0) { for (int64_t i = 0; i <= n; i++) dst_off[i] = 0; return 0; }
    // device image: [source | offsets | output | output offsets | scratch]
    const int64_t scratch_bytes = streams_encode_scratch(nullptr, n, src_len, stream_block(block_size)).bytes;
    Carver c;
    c.take(src_len);
    const int64_t off_at = c.take(8 * (n + 1)), out_at = c.take(bound), doff_at = c.take(8 * (n + 1)), scratch_at = c.take(scratch_bytes);
    Image<B> im = { be };
    LZ4HIP_FRAMING_TRY(im.reserve(c.at));
    LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len, src_off, n, off_at));
    LZ4HIP_FRAMING_TRY(streams_encode(be, im.d, src_len, im.i64(off_at), n, block_size, mode, im.d + out_at, bound,
                                      im.i64(doff_at), im.d + scratch_at, scratch_bytes));
    LZ4HIP_FRAMING_TRY(im.download_items({ n, dst_off, doff_at, nullptr, 0, nullptr, 0 }));
    LZ4HIP_FRAMING_TRY(be.sync());
    return im.download_encoded(dst, out_at, dst_off[n] < dst_cap ? dst_off[n] : dst_cap);
}

// On dst_cap < decoded_bytes the index's offsets, statuses and error offsets are the caller's with the info, as in unwrap_host.
template <class B>
int streams_decode_host(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* dst, int64_t dst_cap, int64_t* dst_off,
                        int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info)
{
    if (src_len < 0 || n < 0 || dst_cap < 0 || !dst_off || !info || (n > 0 && (!src_off || !status || !error_offset)) || (src_len > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: negative size or NULL pointer");
    if (n == 0) { lz4hip_streams_info_t r = {}; r.first_error = r.error_offset = -1; *info = r; dst_off[0] = 0; return 0; }
    // device image: [source | offsets | output offsets | statuses | error offsets | info | output | tables]
    Carver head;
    head.take(src_len);
    const int64_t off_at = head.take(8 * (n + 1)), doff_at = head.take(8 * (n + 1)), st_at = head.take(4 * n), eo_at = head.take(8 * n),
                  info_at = head.take(256), out_at = head.at;
    const Items items = { n, dst_off, doff_at, status, st_at, error_offset, eo_at };
    Image<B> im = { be };
    int64_t max_chunks = src_len / 4096 + n + 16, out_bytes = guessed_output(src_len, dst_cap), table_at = 0, table_bytes = 0;
    lz4hip_streams_info_t h = {};
    LZ4HIP_FRAMING_TRY(settle(be, dst_cap, max_chunks, out_bytes, h, [&] {
        table_bytes = streams_decode_scratch_bytes(n, max_chunks);
        Carver c = head;
        c.take(out_bytes);
        table_at = c.take(table_bytes);
        LZ4HIP_FRAMING_TRY(im.reserve(c.at));
        LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len, src_off, n, off_at));
        LZ4HIP_FRAMING_TRY(streams_index(be, im.d, src_len, im.i64(off_at), n, max_chunks, im.i64(doff_at),
                                         im.i32(st_at), im.i64(eo_at), im.d + table_at, table_bytes,
                                         (lz4hip_streams_info_t*)(im.d + info_at)));
        return im.download(&h, info_at, sizeof h);
    }));
    *info = h;
    if (h.error == LZ4HIP_STREAM_TABLE_FULL) return be.fail(LZ4HIP_E_DEVICE, "streams decode: the header walk did not settle");
    if (h.decoded_bytes > dst_cap || h.decoded_bytes > out_bytes) {
        LZ4HIP_FRAMING_TRY(im.download_items(items));
        LZ4HIP_FRAMING_TRY(be.sync());
        return be.fail(LZ4HIP_E_ARGUMENT, "streams decode: dst_cap < decoded_bytes (reported in info->decoded_bytes)");
    }
    LZ4HIP_FRAMING_TRY(streams_decode(be, im.d, src_len, im.i64(off_at), n, &h, max_chunks, im.d + table_at, table_bytes, im.d + out_at,
                                      out_bytes, im.i64(doff_at), im.i32(st_at), im.i64(eo_at),
                                      (lz4hip_streams_info_t*)(im.d + info_at)));
    LZ4HIP_FRAMING_TRY(im.download_decoded(info, info_at, dst, out_at, h.decoded_bytes, &items));
    return info->error;
}

template <class B>
int frame_encode_host(B& be, const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len)
{
    if (src_len < 0 || !dst_len || !dst || (src_len > 0 && !src)) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: negative size or NULL pointer");
    if (!frame_chunk_valid(chunk_size)) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: chunk_size must be 0 (8 MiB) or 1 .. 0x7E000000");
    const int64_t bound = frame_bound(src_len, chunk_size);
    if (dst_cap < bound) return be.fail(LZ4HIP_E_ARGUMENT, "frame encode: dst_cap < lz4hip_frame_bound");
    // device image: [source | frame | scratch | length]
    const int64_t scratch_bytes = frame_encode_scratch(nullptr, src_len, frame_chunk(chunk_size)).bytes;
    Carver c;
    c.take(src_len);
    const int64_t out_at = c.take(bound), scratch_at = c.take(scratch_bytes), len_at = c.take(256);
    Image<B> im = { be };
    LZ4HIP_FRAMING_TRY(im.reserve(c.at));
    LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len));
    LZ4HIP_FRAMING_TRY(frame_encode(be, im.d, src_len, chunk_size, mode, im.d + out_at, bound, im.i64(len_at), im.d + scratch_at, scratch_bytes));
    int64_t total = 0;
    LZ4HIP_FRAMING_TRY(im.download(&total, len_at, sizeof total));
    LZ4HIP_FRAMING_TRY(be.sync());
    LZ4HIP_FRAMING_TRY(im.download_encoded(dst, out_at, total));
    *dst_len = total;
    return 0;
}

// The index knows the decoded size, so the output's piece of the image is never too small for long: min(dst_cap, 4 * src_len) at first
// -- all of it when the caller sized dst from a size query -- and exactly decoded_bytes on the pass after one that reported more.
// That later pass follows stream_decode_host: the image may have moved, so the source is staged and the WHOLE index runs again (the
// size field walk, the size walk, the scan) although the size is already known -- for a frame that shrank to less than a quarter, twice the
// latency-bound walk.  Keeping the table across the move would save it.
// On dst_cap < decoded_bytes only *info is filled.
template <class B>
int frame_decode_host(B& be, const void* src, int64_t src_len, int32_t chunk_size, void* dst, int64_t dst_cap, lz4hip_frame_info_t* info)
{
    if (src_len < 0 || dst_cap < 0 || !info || (src_len > 0 && !src)) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: negative size or NULL pointer");
    if (!frame_chunk_valid(chunk_size)) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: chunk_size must be 0 (8 MiB) or 1 .. 0x7E000000");
    // device image: [source | info | output | table]
    Image<B> im = { be };
    int64_t max_chunks = src_len / frame_chunk(chunk_size) + 16, out_bytes = guessed_output(src_len, dst_cap), info_at = 0, out_at = 0, table_at = 0,
            table_bytes = 0;
    lz4hip_frame_info_t h = {};
    LZ4HIP_FRAMING_TRY(settle(be, dst_cap, max_chunks, out_bytes, h, [&] {
        table_bytes = frame_decode_scratch_bytes(max_chunks);
        Carver c;
        c.take(src_len);
        info_at = c.take(256); out_at = c.take(out_bytes); table_at = c.take(table_bytes);
        LZ4HIP_FRAMING_TRY(im.reserve(c.at));
        LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len));
        LZ4HIP_FRAMING_TRY(frame_index(be, im.d, src_len, chunk_size, max_chunks, im.d + table_at, table_bytes, (lz4hip_frame_info_t*)(im.d + info_at)));
        return im.download(&h, info_at, sizeof h);
    }, LZ4HIP_FRAME_TABLE_FULL));
    *info = h;
    if (h.error == LZ4HIP_FRAME_TABLE_FULL) return be.fail(LZ4HIP_E_DEVICE, "frame decode: the size field walk did not settle");
    if (h.decoded_bytes > dst_cap || h.decoded_bytes > out_bytes)
        return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: dst_cap < decoded_bytes (reported in info->decoded_bytes)");
    if (h.decoded_bytes > 0 && !dst) return be.fail(LZ4HIP_E_ARGUMENT, "frame decode: dst is NULL");
    LZ4HIP_FRAMING_TRY(frame_decode(be, im.d, &h, max_chunks, im.d + table_at, table_bytes, im.d + out_at, out_bytes,
                                    (lz4hip_frame_info_t*)(im.d + info_at)));
    LZ4HIP_FRAMING_TRY(im.download_decoded(info, info_at, dst, out_at, h.decoded_bytes));
    return info->error;
}

// the device call of the host-pointer encoders over their image: the plain call, or the dictionary call in its place
template <class B>
int lz4f_encode_image(B& be, const void* src, int64_t src_len, int block_size_id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len,
                      void* scratch, int64_t scratch_bytes, Lz4fNoDict)
{
    return lz4f_encode(be, src, src_len, block_size_id, mode, flags, dst, dst_cap, dst_len, scratch, scratch_bytes);
}
template <class B>
int lz4f_encode_image(B& be, const void* src, int64_t src_len, int block_size_id, int, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len,
                      void* scratch, int64_t scratch_bytes, const Lz4fDict& d)
{
    return lz4f_encode_dict(be, src, src_len, d.end - d.len, d.len, d.id, block_size_id, flags, dst, dst_cap, dst_len, scratch, scratch_bytes);
}

// The LZ4 frame's encoder staged the way frame_encode_host stages the legacy frame's.  `dict`: Lz4fNoDict, or the call's dictionary ALREADY
// in device memory, in staging that is not the image's (lz4f_dict_stage); its primed table lies in the image's scratch.
template <class B, class D = Lz4fNoDict>
int lz4f_encode_host(B& be, const void* src, int64_t src_len, int block_size_id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len,
                     const D& dict = D())
{
    const int64_t reach = lz4f_dict_reach(dict);
    if (src_len < 0 || !dst_len || !dst || (src_len > 0 && !src)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: negative size or NULL pointer");
    if (!lz4f_id_valid(block_size_id) || (flags & ~kLz4fEncodeFlags)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: block_size_id must be 0 or 4 .. 7, flags known");
    const int64_t bound = lz4f_bound(src_len, block_size_id, flags, lz4f_walk_dict_id(dict));
    if (dst_cap < bound) return be.fail(LZ4HIP_E_ARGUMENT, reach ? "lz4f encode: dst_cap < lz4hip_lz4f_dict_bound" : "lz4f encode: dst_cap < lz4hip_lz4f_bound");
    // device image: [source | frame | scratch | length]
    const int64_t scratch_bytes = lz4f_encode_scratch(nullptr, src_len, lz4f_block_bytes(lz4f_id(block_size_id)), reach).bytes;
    Carver c;
    c.take(src_len);
    const int64_t out_at = c.take(bound), scratch_at = c.take(scratch_bytes), len_at = c.take(256);
    Image<B> im = { be };
    LZ4HIP_FRAMING_TRY(im.reserve(c.at));
    LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len));
    LZ4HIP_FRAMING_TRY(lz4f_encode_image(be, im.d, src_len, block_size_id, mode, flags, im.d + out_at, bound, im.i64(len_at), im.d + scratch_at, scratch_bytes, dict));
    int64_t total = 0;
    LZ4HIP_FRAMING_TRY(im.download(&total, len_at, sizeof total));
    LZ4HIP_FRAMING_TRY(be.sync());
    LZ4HIP_FRAMING_TRY(im.download_encoded(dst, out_at, total));
    *dst_len = total;
    return 0;
}

// The descriptor lies in host memory here: the block maximum sizes the slot, the content size (or four times the frame) the output's
// piece of the image and the table.  A table that was too small or an output that has to grow is decoded again with what the record
// reported, three passes at most.  On dst_cap < decoded_bytes only *info is filled (a size query: dst_cap = 0).  `dict`: Lz4fNoDict,
// or the call's dictionary ALREADY in device memory, in staging that is not the image's (lz4f_dict_stage).
template <class B, class D = Lz4fNoDict>
int lz4f_decode_host(B& be, const void* src, int64_t src_len, unsigned flags, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, const D& dict = D())
{
    if (src_len < 0 || dst_cap < 0 || !info || (src_len > 0 && !src)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: negative size or NULL pointer");
    if (flags & ~kLz4fDecodeFlags) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: unknown flag");
    const uint8_t* s = (const uint8_t*)src;
    const int id = src_len >= 6 ? (s[5] >> 4) & 7 : 4;
    const int32_t slot = lz4f_block_bytes(id < 4 ? 4 : id);
    int64_t known = -1;
    if (src_len >= 14 && (s[4] & 0x08)) memcpy(&known, s + 6, 8);
    int64_t out_bytes = known >= 0 && known <= 255 * src_len ? known : guessed_output(src_len, dst_cap);
    if (out_bytes > dst_cap) out_bytes = dst_cap;
    int64_t max_blocks = (known >= 0 && known <= 255 * src_len ? known : src_len) / slot + 16;
    // device image: [source | info | output | scratch]
    Image<B> im = { be };
    lz4hip_lz4f_info_t h = {};
    int64_t info_at = 0, out_at = 0;
    for (int attempt = 0;; attempt++) {
        const int64_t scratch_bytes = lz4f_decode_scratch_bytes(slot, max_blocks, 0);
        Carver c;
        c.take(src_len);
        info_at = c.take(256); out_at = c.take(out_bytes);
        const int64_t scratch_at = c.take(scratch_bytes);
        LZ4HIP_FRAMING_TRY(im.reserve(c.at));
        LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len));
        LZ4HIP_FRAMING_TRY(lz4f_decode(be, im.d, src_len, slot, max_blocks, 0, flags, im.d + scratch_at, scratch_bytes, im.d + out_at, out_bytes,
                                       (lz4hip_lz4f_info_t*)(im.d + info_at), dict));
        LZ4HIP_FRAMING_TRY(im.download(&h, info_at, sizeof h));
        LZ4HIP_FRAMING_TRY(be.sync());
        if (attempt >= 2) break;
        if (h.error == LZ4HIP_LZ4F_TABLE_FULL) max_blocks = h.blocks;
        else if (h.decoded_bytes > dst_cap || h.decoded_bytes <= out_bytes) break;
        else out_bytes = h.decoded_bytes;
    }
    *info = h;
    if (h.error == LZ4HIP_LZ4F_TABLE_FULL) return be.fail(LZ4HIP_E_DEVICE, "lz4f decode: the size field walk did not settle");
    if (h.decoded_bytes > dst_cap || h.decoded_bytes > out_bytes)
        return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: dst_cap < decoded_bytes (reported in info->decoded_bytes)");
    if (h.decoded_bytes > 0 && !dst) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: dst is NULL");
    if (h.decoded_bytes > 0) LZ4HIP_FRAMING_TRY(im.download(dst, out_at, h.decoded_bytes));
    LZ4HIP_FRAMING_TRY(be.sync());
    return info->error;
}

// The dictionary of a host-pointer dictionary call: the bytes a match can reach -- its last min(dict_len, 65 535) -- go up ONCE per call,
// before the first pass, into staging of the backend's that is the dictionary's alone (be.dict_upload, which has landed when it returns:
// hostbatch::upload_dictionary's contract).  The image of a later pass may grow and move; the dictionary stays where it is.
template <class B>
int lz4f_dict_stage(B& be, const void* dict, int64_t dict_len, uint32_t dict_id, Lz4fDict& d)
{
    const int64_t reach = dict_len < kLz4fLinkedHistory ? dict_len : kLz4fLinkedHistory;
    uint8_t* dev = nullptr;
    LZ4HIP_FRAMING_TRY(be.dict_upload((const uint8_t*)dict + (dict_len - reach), reach, dev));
    d = lz4f_dict_of(dev, reach, dict_id);
    return 0;
}

// lz4hip_lz4f_decode_dict_host; the dictionary's check comes first (the API repeats it before it looks for a device)
template <class B>
int lz4f_decode_dict_host(B& be, const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, unsigned flags, void* dst,
                          int64_t dst_cap, lz4hip_lz4f_info_t* info)
{
    LZ4HIP_FRAMING_TRY(lz4f_dict_check(be, dict, dict_len));
    if (dict_len == 0) return lz4f_decode_host(be, src, src_len, flags, dst, dst_cap, info);
    if (src_len < 0 || dst_cap < 0 || !info || (src_len > 0 && !src)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: negative size or NULL pointer");
    if (flags & ~kLz4fDecodeFlags) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f decode: unknown flag");
    Lz4fDict d;
    LZ4HIP_FRAMING_TRY(lz4f_dict_stage(be, dict, dict_len, dict_id, d));
    return lz4f_decode_host(be, src, src_len, flags, dst, dst_cap, info, d);
}

// lz4hip_lz4f_encode_dict_host: three phases -- the dictionary's reachable tail goes up once (lz4f_dict_stage), its table is primed once
// and the device sequence runs over one image (both inside lz4f_encode_dict).  The front checks that come before the staging are
// repeated here, so that a call that is refused uploads nothing.
template <class B>
int lz4f_encode_dict_host(B& be, const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int block_size_id, unsigned flags,
                          void* dst, int64_t dst_cap, int64_t* dst_len)
{
    LZ4HIP_FRAMING_TRY(lz4f_dict_check(be, dict, dict_len));
    if (dict_len == 0) return lz4f_encode_host(be, src, src_len, block_size_id, LZ4HIP_MODE_FAST, flags, dst, dst_cap, dst_len);
    if (src_len < 0 || !dst_len || !dst || (src_len > 0 && !src)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: negative size or NULL pointer");
    if (!lz4f_id_valid(block_size_id) || (flags & ~kLz4fEncodeFlags)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: block_size_id must be 0 or 4 .. 7, flags known");
    if (dst_cap < lz4f_bound(src_len, block_size_id, flags, dict_id)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f encode: dst_cap < lz4hip_lz4f_dict_bound");
    Lz4fDict d;
    LZ4HIP_FRAMING_TRY(lz4f_dict_stage(be, dict, dict_len, dict_id, d));
    return lz4f_encode_host(be, src, src_len, block_size_id, LZ4HIP_MODE_FAST, flags, dst, dst_cap, dst_len, d);
}

// A batch of frames staged the way streams_encode_host stages a batch of streams; the offsets are host memory here, so bad ones are
// refused instead of encoded as items of no bytes.  `dict`: as lz4f_encode_host's.
template <class B>
int lz4f_batch_encode_image(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int mode, unsigned flags, void* dst,
                            int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, Lz4fNoDict)
{
    return lz4f_batch_encode(be, src, src_len, src_off, n, block_size_id, mode, flags, dst, dst_cap, dst_off, scratch, scratch_bytes);
}
template <class B>
int lz4f_batch_encode_image(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int, unsigned flags, void* dst,
                            int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, const Lz4fDict& d)
{
    return lz4f_batch_encode_dict(be, src, src_len, src_off, n, d.end - d.len, d.len, d.id, block_size_id, flags, dst, dst_cap, dst_off, scratch, scratch_bytes);
}

template <class B, class D = Lz4fNoDict>
int lz4f_batch_encode_host(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int mode, unsigned flags,
                           void* dst, int64_t dst_cap, int64_t* dst_off, const D& dict = D())
{
    const int64_t reach = lz4f_dict_reach(dict);
    if (src_len < 0 || n < 0 || !dst_off || (n > 0 && (!src_off || !dst)) || (src_len > 0 && n > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: negative size or NULL pointer");
    if (!lz4f_id_valid(block_size_id) || (flags & ~kLz4fEncodeFlags)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: block_size_id must be 0 or 4 .. 7, flags known");
    if (mode != LZ4HIP_MODE_FAST && mode != LZ4HIP_MODE_HC) return be.fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    for (int64_t i = 0; i < n; i++)
        if (src_off[i] < 0 || src_off[i + 1] < src_off[i] || src_off[i + 1] > src_len)
            return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: offsets decrease or fall outside [0, src_len]");
    const int64_t bound = lz4f_batch_bound(n, src_len, block_size_id, flags, lz4f_walk_dict_id(dict));
    if (n > 0 && dst_cap < bound)
        return be.fail(LZ4HIP_E_ARGUMENT, reach ? "lz4f batch encode: dst_cap < lz4hip_lz4f_batch_dict_bound" : "lz4f batch encode: dst_cap < lz4hip_lz4f_batch_bound");
    if (n == 0) { dst_off[0] = 0; return 0; }
    // device image: [source | offsets | output | output offsets | scratch]
    const int64_t scratch_bytes = lz4f_batch_encode_scratch(nullptr, n, src_len, lz4f_block_bytes(lz4f_id(block_size_id)), reach).bytes;
    Carver c;
    c.take(src_len);
    const int64_t off_at = c.take(8 * (n + 1)), out_at = c.take(bound), doff_at = c.take(8 * (n + 1)), scratch_at = c.take(scratch_bytes);
    Image<B> im = { be };
    LZ4HIP_FRAMING_TRY(im.reserve(c.at));
    LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len, src_off, n, off_at));
    LZ4HIP_FRAMING_TRY(lz4f_batch_encode_image(be, im.d, src_len, im.i64(off_at), n, block_size_id, mode, flags, im.d + out_at, bound, im.i64(doff_at),
                                               im.d + scratch_at, scratch_bytes, dict));
    LZ4HIP_FRAMING_TRY(im.download_items({ n, dst_off, doff_at, nullptr, 0, nullptr, 0 }));
    LZ4HIP_FRAMING_TRY(be.sync());
    return im.download_encoded(dst, out_at, dst_off[n] < dst_cap ? dst_off[n] : dst_cap);
}

// lz4hip_lz4f_batch_encode_dict_host, as lz4f_encode_dict_host: a call that is refused, or has no items, uploads nothing
template <class B>
int lz4f_batch_encode_dict_host(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                int block_size_id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off)
{
    LZ4HIP_FRAMING_TRY(lz4f_dict_check(be, dict, dict_len));
    if (dict_len == 0 || n <= 0) return lz4f_batch_encode_host(be, src, src_len, src_off, n, block_size_id, LZ4HIP_MODE_FAST, flags, dst, dst_cap, dst_off);
    if (src_len < 0 || !dst_off || !src_off || !dst || (src_len > 0 && !src)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: negative size or NULL pointer");
    if (!lz4f_id_valid(block_size_id) || (flags & ~kLz4fEncodeFlags)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: block_size_id must be 0 or 4 .. 7, flags known");
    for (int64_t i = 0; i < n; i++)
        if (src_off[i] < 0 || src_off[i + 1] < src_off[i] || src_off[i + 1] > src_len)
            return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: offsets decrease or fall outside [0, src_len]");
    if (dst_cap < lz4f_batch_bound(n, src_len, block_size_id, flags, dict_id)) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: dst_cap < lz4hip_lz4f_batch_dict_bound");
    Lz4fDict d;
    LZ4HIP_FRAMING_TRY(lz4f_dict_stage(be, dict, dict_len, dict_id, d));
    return lz4f_batch_encode_host(be, src, src_len, src_off, n, block_size_id, LZ4HIP_MODE_FAST, flags, dst, dst_cap, dst_off, d);
}

// The descriptors lie in host memory here: the largest block maximum among them sizes the slots.  The table and the output's piece of
// the image start as guesses; a table that was too small or an output that has to grow is decoded again with what the record reported,
// three passes at most.  The rounds are bounded (a ring of 256 MiB, at least 64 slots), so the image does not grow with the table.
// On dst_cap < decoded_bytes the offsets and the items' records are the caller's with the info (a size query: dst_cap = 0).  `dict`: as
// lz4f_decode_host's.
template <class B, class D = Lz4fNoDict>
int lz4f_batch_decode_host(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, unsigned flags, void* dst, int64_t dst_cap,
                           int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, const D& dict = D())
{
    if (src_len < 0 || n < 0 || dst_cap < 0 || !dst_off || !info || (n > 0 && (!src_off || !item_info)) || (src_len > 0 && n > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: negative size or NULL pointer");
    if (flags & ~kLz4fDecodeFlags) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: unknown flag");
    if (n == 0) { lz4hip_lz4f_batch_info_t r = {}; r.first_error = r.error_offset = -1; *info = r; dst_off[0] = 0; return 0; }
    const uint8_t* s = (const uint8_t*)src;
    int id = 4;
    for (int64_t i = 0; i < n; i++) {
        if (src_off[i] < 0 || src_off[i + 1] < src_off[i] || src_off[i + 1] > src_len)
            return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: offsets decrease or fall outside [0, src_len]");
        const uint8_t* f = s + src_off[i];
        if (src_off[i + 1] - src_off[i] >= 6 && f[0] == 0x04 && f[1] == 0x22 && f[2] == 0x4D && f[3] == 0x18 && ((f[5] >> 4) & 7) > id) id = (f[5] >> 4) & 7;
    }
    const int32_t slot = lz4f_block_bytes(id);
    const int64_t round_blocks = ((int64_t)1 << 28) / slot;
    // device image: [source | offsets | output offsets | records | info | written | output | scratch]
    Carver head;
    head.take(src_len);
    const int64_t off_at = head.take(8 * (n + 1)), doff_at = head.take(8 * (n + 1)), rec_at = head.take((int64_t)sizeof(lz4hip_lz4f_info_t) * n),
                  info_at = head.take(256), written_at = head.take(256), out_at = head.at;
    Image<B> im = { be };
    int64_t max_blocks = src_len / 4096 + n + 16, out_bytes = guessed_output(src_len, dst_cap);
    lz4hip_lz4f_batch_info_t h = {};
    for (int attempt = 0;; attempt++) {
        const int64_t scratch_bytes = lz4f_batch_decode_scratch_bytes(n, slot, max_blocks, round_blocks);
        Carver c = head;
        c.take(out_bytes);
        const int64_t scratch_at = c.take(scratch_bytes);
        LZ4HIP_FRAMING_TRY(im.reserve(c.at));
        LZ4HIP_FRAMING_TRY(im.upload_source(src, src_len, src_off, n, off_at));
        LZ4HIP_FRAMING_TRY(lz4f_batch_decode(be, im.d, src_len, im.i64(off_at), n, slot, max_blocks, round_blocks, flags, im.d + scratch_at, scratch_bytes,
                                             im.d + out_at, out_bytes, im.i64(doff_at), (lz4hip_lz4f_info_t*)(im.d + rec_at),
                                             (lz4hip_lz4f_batch_info_t*)(im.d + info_at), im.i64(written_at), dict));
        LZ4HIP_FRAMING_TRY(im.download(&h, info_at, sizeof h));
        LZ4HIP_FRAMING_TRY(be.sync());
        if (attempt >= 2) break;
        if (h.error == LZ4HIP_LZ4F_TABLE_FULL) max_blocks = h.blocks;
        else if (h.decoded_bytes > dst_cap || h.decoded_bytes <= out_bytes) break;
        else out_bytes = h.decoded_bytes;
    }
    *info = h;
    if (h.error == LZ4HIP_LZ4F_TABLE_FULL) return be.fail(LZ4HIP_E_DEVICE, "lz4f batch decode: the size field walks did not settle");
    LZ4HIP_FRAMING_TRY(im.download(dst_off, doff_at, 8 * (n + 1)));
    LZ4HIP_FRAMING_TRY(im.download(item_info, rec_at, (int64_t)sizeof(lz4hip_lz4f_info_t) * n));
    if (h.decoded_bytes > dst_cap || h.decoded_bytes > out_bytes) {
        LZ4HIP_FRAMING_TRY(be.sync());
        return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: dst_cap < decoded_bytes (reported in info->decoded_bytes)");
    }
    if (h.decoded_bytes > 0 && !dst) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: dst is NULL");
    if (h.decoded_bytes > 0) LZ4HIP_FRAMING_TRY(im.download(dst, out_at, h.decoded_bytes));
    LZ4HIP_FRAMING_TRY(be.sync());
    return info->error;
}

// lz4hip_lz4f_batch_decode_dict_host: the front checks that come before the staging are repeated here, so that a call that is refused
// uploads nothing
template <class B>
int lz4f_batch_decode_dict_host(B& be, const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info)
{
    LZ4HIP_FRAMING_TRY(lz4f_dict_check(be, dict, dict_len));
    if (dict_len == 0 || n <= 0) return lz4f_batch_decode_host(be, src, src_len, src_off, n, flags, dst, dst_cap, dst_off, item_info, info);
    if (src_len < 0 || dst_cap < 0 || !dst_off || !info || !src_off || !item_info || (src_len > 0 && !src))
        return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: negative size or NULL pointer");
    if (flags & ~kLz4fDecodeFlags) return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: unknown flag");
    for (int64_t i = 0; i < n; i++)
        if (src_off[i] < 0 || src_off[i + 1] < src_off[i] || src_off[i + 1] > src_len)
            return be.fail(LZ4HIP_E_ARGUMENT, "lz4f batch decode: offsets decrease or fall outside [0, src_len]");
    Lz4fDict d;
    LZ4HIP_FRAMING_TRY(lz4f_dict_stage(be, dict, dict_len, dict_id, d));
    return lz4f_batch_decode_host(be, src, src_len, src_off, n, flags, dst, dst_cap, dst_off, item_info, info, d);
}

#undef LZ4HIP_FRAMING_TRY

}  // namespace framing
}  // namespace lz4hip
