// lz4hip_frame.hpp -- device-side framing of the legacy LZ4 command-line frame (original/lz4demo.c:84-87, 167-317) around the block
// kernels:
//
//     LE32 magic 0x184C2102   { LE32 compressedSize  payload }*
//
// (lz4net_amd/legacy_frame.py has the host twin and the citations).  The writer cuts the source into chunks of chunk_size bytes and
// compresses each into a compressBound buffer; the reader checks the magic, skips a size field that equals the magic (an appended
// frame's header) and decodes every payload with LZ4_uncompress_unknownOutputSize(in, out, size, chunk_size).  The block codecs and the
// size walk are the batch kernels of the library; this header holds only what goes around them, and reuses the int64 scan and the
// position-driven copy routine of lz4hip_stream.hpp:
//
//   encode: frame_lens_kernel (chunk lengths and compressBound capacities) -> [launch_encode into scratch, chunk k at k * stride] ->
//           frame_sizes_kernel (4 for the magic, 4 + result per chunk) -> stream_scan_* (the total, 4 + sum, to the caller's device
//           int64) -> frame_pack_kernel (copy_spans over FrameLayout: the magic, then size field + payload per chunk)
//   index:  frame_walk_kernel (ONE wavefront chases the size fields, one dependent global round trip per chunk) -> sizes_walk_kernel
//           (lz4hip_sizes.hpp, unchanged, over all max_chunks rows: the rows past the count are empty blocks) -> frame_caps_kernel
//           (a chunk that does not decode into <= chunk_size bytes gets capacity 0 and goes to the first-bad slot) -> stream_scan_*
//           (dst_off) -> frame_info_kernel
//   decode: [launch_decode, unknown size, on the table] -> frame_check_kernel (result != capacity: the first-bad slot again) ->
//           frame_info_kernel
//
// Every kernel here is launch-only work on the caller's stream over caller scratch.
#pragma once
#include "lz4hip_stream.hpp"
#include "lz4hip_sizes.hpp"

namespace lz4hip {

constexpr int kFrameOk = 0, kFrameBadMagic = 1, kFrameTruncated = 2, kFrameBadSize = 3, kFrameCorruptBlock = 4, kFrameTableFull = 5;
constexpr uint32_t kFrameMagic = 0x184C2102u;                          // ARCHIVE_MAGICNUMBER (original/lz4demo.c:86)
constexpr int32_t kFrameDefaultChunk = 8 << 20;                        // CHUNKSIZE (original/lz4demo.c:84)
constexpr int32_t kFrameMaxChunk = 0x7E000000;                         // LZ4_MAX_INPUT_SIZE
constexpr int64_t kFrameField = 4;                                     // the magic and every size field

// Device twin of lz4hip_frame_info_t (include/lz4hip.h; the API checks that the layouts agree).
struct FrameInfo {
    int64_t chunks, decoded_bytes, good_bytes, error_offset;
    int32_t error, reserved;
};

// LZ4_compressBound (original/lz4.h:85-86)
__host__ __device__ inline int32_t frame_block_bound(int32_t len) { return len + len / 255 + 16; }

// ---- encode ------------------------------------------------------------------------------------------------------------
struct FrameEncodeArgs {
    const uint8_t* src;          // the source run [0, src_len)
    const uint8_t* comp;         // launch_encode's output: chunk k at k * stride, at most compressBound(its length)
    int64_t src_len;
    int64_t n;                   // chunks = ceil(src_len / chunk)
    int64_t stride;              // compressBound(chunk)
    int32_t chunk;
    const int32_t* result;       // launch_encode's per-chunk results
    int64_t* offs;               // n + 1 entries: 4 for the magic, then 4 + result per chunk; scanned in place: [0] = 0, [k + 1] = chunk k's size field
};

LZ4HIP_DEVICE int32_t frame_chunk_len(int64_t src_len, int32_t chunk, int64_t k)
{
    const int64_t left = src_len - k * chunk;
    return left < chunk ? (int32_t)left : chunk;
}

// what the encoder wrote for chunk k.  With a compressBound capacity it is 0 < r <= capacity; anything else (an encoder that refused
// its arguments) is held inside the chunk's scratch slot, so that the pack stays inside the scratch and the frame inside its bound
LZ4HIP_DEVICE int32_t frame_payload_len(const FrameEncodeArgs& a, int64_t k)
{
    const int32_t r = a.result[k], cap = frame_block_bound(frame_chunk_len(a.src_len, a.chunk, k));
    return r < 0 ? 0 : (r > cap ? cap : r);
}

__global__ void __launch_bounds__(kStreamThreads) frame_lens_kernel(int32_t* lens, int32_t* caps, int64_t n, int64_t src_len, int32_t chunk)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < n; k += (int64_t)gridDim.x * kStreamThreads) {
        const int32_t len = frame_chunk_len(src_len, chunk, k);
        lens[k] = len;
        caps[k] = frame_block_bound(len);
    }
}

// n + 1 framed sizes: the magic, then every chunk's size field and payload
__global__ void __launch_bounds__(kStreamThreads) frame_sizes_kernel(FrameEncodeArgs a)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k <= a.n; k += (int64_t)gridDim.x * kStreamThreads)
        a.offs[k] = kFrameField + (k == 0 ? 0 : frame_payload_len(a, k - 1));
}

// Segment 0 is the magic (four header bytes, no payload); segment k + 1 is chunk k: four header bytes (its size) and its payload in the
// encoder's scratch.  start(k) is one load of the scanned offsets, so the cursor's search (CopyCursor::seek) reads nothing else, and a
// thread computes a segment only when its pieces have moved into it.
struct FrameLayout {
    FrameEncodeArgs a;
    LZ4HIP_DEVICE int64_t count() const { return a.n + 1; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.offs[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        s.start = a.offs[k];
        s.pbegin = s.start + kFrameField;
        s.flags = 0;
        if (k == 0) {
            s.pend = s.pbegin;
            s.payload = a.comp;
            s.original = s.clen = kFrameMagic;
            return s;
        }
        s.original = s.clen = (uint32_t)frame_payload_len(a, k - 1);
        s.pend = s.pbegin + s.clen;
        s.payload = a.comp + (k - 1) * a.stride;
        return s;
    }
    // the field's little-endian bytes
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg& s, int64_t x) const { return (uint8_t)(s.clen >> (8 * (int)(x - s.start))); }
};

// output bytes [0, min(total, cap)): the total stays within the bound by construction (frame_payload_len), and nothing past cap is written
__global__ void __launch_bounds__(kStreamThreads) frame_pack_kernel(FrameLayout L, uint8_t* dst, const int64_t* total, int64_t cap)
{
    const int64_t end = *total;
    copy_spans(L, dst, end < cap ? end : cap);
}

// ---- decode ------------------------------------------------------------------------------------------------------------
// The index: one table in caller scratch, max_chunks rows laid out as the arrays of a lz4hip_batch_t (src_off / src_len / dst_off /
// dst_cap / result) plus each chunk's size field offset (error reports), and what the walk found.
struct FrameTables {
    int64_t max_chunks;
    int64_t* src_off; int64_t* hdr_off;
    int64_t* dst_off;                                                  // max_chunks + 1 entries: the capacities, scanned in place
    int32_t* src_len; int32_t* dst_cap; int32_t* result;
    unsigned long long* min_bad;                                       // the lowest chunk that does not decode (~0: none)
    int64_t* walk;                                                     // [0] chunks, [1] the header error, [2] its offset, [3] the size field of the first chunk that did not fit
    int64_t* partial;                                                  // tile sums of the scan
};

// One wavefront walks the size fields in frame order, one dependent global round trip per chunk: a size, then a jump past its payload.
// Every lane runs the same walk on the same (wave-uniform) position; lane 0 writes.  The checks are decode_file's, in its order
// (original/lz4demo.c:276-300): the magic; per field, the appended frame's magic, then the size against the reader's input buffer
// (`bound` = compressBound(chunk_size): more than the writer can produce), then the payload against the end of the frame.
__global__ void __launch_bounds__(64) frame_walk_kernel(const uint8_t* src, int64_t src_len, int64_t bound, FrameTables t)
{
    const int lane = wv::lane();
    int64_t pos = kFrameField, chunks = 0, err_off = -1, full_off = -1;
    int err = kFrameOk;
    if (src_len < kFrameField || wv::uniform(load_u32(src)) != kFrameMagic) { err = kFrameBadMagic; err_off = 0; pos = src_len; }
    while (pos < src_len) {
        if (pos + kFrameField > src_len) { err = kFrameTruncated; err_off = pos; break; }
        const int64_t size = (int64_t)wv::uniform(load_u32(src + pos));
        if (size == (int64_t)kFrameMagic) { pos += kFrameField; continue; }
        if (size > bound) { err = kFrameBadSize; err_off = pos; break; }
        if (pos + kFrameField + size > src_len) { err = kFrameTruncated; err_off = pos; break; }
        if (chunks < t.max_chunks) {
            if (lane == 0) { t.src_off[chunks] = pos + kFrameField; t.hdr_off[chunks] = pos; t.src_len[chunks] = (int32_t)size; }
        } else if (chunks == t.max_chunks) {
            full_off = pos;
        }
        chunks++;
        pos += kFrameField + size;
    }
    if (lane == 0) { t.walk[0] = chunks; t.walk[1] = err; t.walk[2] = err_off; t.walk[3] = full_off; }
}

// after sizes_walk_kernel: the reader decodes chunk k with maxOutputSize = chunk_size, so a walk that failed (result < 0) or went past
// chunk_size is a chunk it fails on; such a chunk takes no bytes of the output.  Rows past the count are empty blocks: result 0.
__global__ void __launch_bounds__(kStreamThreads) frame_caps_kernel(FrameTables t, int32_t chunk)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < t.max_chunks; k += (int64_t)gridDim.x * kStreamThreads) {
        const int32_t r = t.result[k];
        const bool ok = r >= 0 && r <= chunk;
        t.dst_cap[k] = ok ? r : 0;
        t.dst_off[k] = ok ? r : 0;
        if (!ok) atomicMin(t.min_bad, (unsigned long long)k);
    }
}

// a chunk that walked to a size but breaks the format's end rules fails in the decoder, as it does in the reference's
__global__ void __launch_bounds__(kStreamThreads) frame_check_kernel(FrameTables t, int64_t n)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < n; k += (int64_t)gridDim.x * kStreamThreads)
        if (t.result[k] != t.dst_cap[k]) atomicMin(t.min_bad, (unsigned long long)k);
}

// The record, from the table as it stands: after the index, and again after the decode's check.  Every chunk in the table lies before
// the walk's header error (if any), so a bad chunk comes first; a frame with more chunks than rows is LZ4HIP_FRAME_TABLE_FULL whatever
// its chunks hold (the caller grows the table to `chunks` and indexes again).
// (`bad`: the lowest bad chunk, ~0 for none -- the two-call path keeps it in the table, the one-call path of lz4hip_compact.hpp elsewhere)
LZ4HIP_DEVICE FrameInfo frame_info_of(const FrameTables& t, unsigned long long bad)
{
    FrameInfo r;
    r.chunks = t.walk[0];
    r.decoded_bytes = r.good_bytes = t.dst_off[t.max_chunks];
    r.error = (int32_t)t.walk[1];
    r.error_offset = t.walk[2];
    r.reserved = 0;
    if (r.chunks > t.max_chunks) {
        r.error = kFrameTableFull;
        r.error_offset = t.walk[3];
    } else if (bad != ~0ull) {
        r.error = kFrameCorruptBlock;
        r.error_offset = t.hdr_off[bad];
        r.good_bytes = t.dst_off[bad];
    }
    return r;
}

__global__ void __launch_bounds__(64) frame_info_kernel(FrameTables t, FrameInfo* info)
{
    if (threadIdx.x != 0) return;
    *info = frame_info_of(t, *t.min_bad);
}

}  // namespace lz4hip
