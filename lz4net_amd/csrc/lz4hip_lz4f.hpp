// lz4hip_lz4f.hpp -- device-side framing of the LZ4 frame format (LZ4 Frame format v1.6.x, what every `lz4` tool since r120, K4os'
// streams and python-lz4 write) around the block kernels:
//
//     LE32 0x184D2204   FLG  BD  [LE64 contentSize if FLG.3]  [LE32 dictID if FLG.0]  HC
//     { LE32 blockSize (bit 31: stored raw)  data  [LE32 xxh32(data) if FLG.4] }*
//     LE32 0 (EndMark)   [LE32 xxh32(content) if FLG.2]
//
// (lz4net_amd/lz4_frame.py has the host twin of the descriptor).  The blocks inside are the block format the library already encodes;
// this header holds what goes around them, and reuses the int64 scan and the position-driven copy routine of lz4hip_stream.hpp:
//
//   xxHash32: xxh32_rows_kernel, one hash per row of bytes; FOUR lanes per row, sixteen rows per wavefront (below)
//   encode:   lz4f_lens_kernel (block lengths, capacities len - 1: a block that does not shrink is stored raw) -> [launch_encode into
//             scratch, block k at k * stride] -> lz4f_rows_kernel + xxh32_rows_kernel (the stored bytes of every block: its scratch slot
//             or, raw, the source) -> xxh32_rows_kernel (one row: the content) -> lz4f_head_kernel (the descriptor and its HC byte) ->
//             lz4f_sizes_kernel (n + 2 segment sizes) -> stream_scan_* (the frame's length to the caller's device int64) ->
//             lz4f_pack_kernel (copy_spans over Lz4fLayout)
//
//   decode:   lz4f_walk_kernel (ONE wavefront parses and validates the descriptor, then chases the size fields: one dependent global
//             round trip per block) -> [xxh32_rows_kernel over the stored bytes of every row + lz4f_verify_kernel: a mismatching row is
//             handed to the decoder as an empty row] -> the compact decode's rounds (lz4hip_packed.hpp, lz4hip_compact.hpp) with a sizes
//             step and a pack layout of their own (lz4f_round_sizes_kernel, Lz4fRoundLayout): a raw row's size is its stored size and
//             its payload the SOURCE, not the ring; the decoder sees it as an empty row -> lz4f_info_kernel -> [xxh32_rows_kernel, one
//             row over the output] -> lz4f_final_kernel
//
// The decode is the batch of frames' (lz4hip_lz4f_batch.hpp) with one item: from the block checksums' verdict to the item's record,
// everything but the walk is written here once for both, over one Lz4fTables whose rows name their item (or none: one item).
//
// The encoder's blocks are always independent (FLG.5); the dictionary calls (lz4hip_lz4f_*encode_dict_*) hand the block round to the
// dictionary encoder (lz4hip_encode_dict.hpp) and write the descriptor with lz4f_dict_head_kernel, which knows the dictionary ID: the
// rest of the sequence is the plain one.  The decoder refuses linked blocks unless the caller accepts
// them (kLz4fAcceptLinked): each decodes only against the 64 KiB before it, in order, so a linked frame is one serial chain --
// lz4hip_lz4f_linked.hpp runs it on one wavefront, after the rounds, which see its rows as holes.  A frame with a dictionary ID is
// refused by the plain calls; the dictionary calls (lz4hip_lz4f_*_dict_*) hand the walk kLz4fWithDict and the ID they expect, the rounds
// the dictionary decode (decode_dict_kernel) and the linked decode its dictionary form.  Every kernel here is launch-only work on the
// caller's stream over caller scratch.
#pragma once
#include "lz4hip_packed.hpp"

namespace lz4hip {

constexpr uint32_t kLz4fMagic = 0x184D2204u;
constexpr uint32_t kLz4fSkippableMagic = 0x184D2A50u;                   // ... 0x184D2A5F
constexpr uint32_t kLz4fRawBit = 0x80000000u;
constexpr unsigned kLz4fBlockChecksum = 1, kLz4fContentChecksum = 2, kLz4fContentSize = 4;   // LZ4HIP_LZ4F_* (include/lz4hip.h)
constexpr int kLz4fHeadMax = 16;                                        // magic + FLG + BD + content size + HC = 15

// block maximum size ids 4 .. 7: 64 KiB, 256 KiB, 1 MiB, 4 MiB
__host__ __device__ inline int32_t lz4f_block_bytes(int id) { return (int32_t)1 << (8 + 2 * id); }

// ---- xxHash32 -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kXxhP1 = 2654435761u, kXxhP2 = 2246822519u, kXxhP3 = 3266489917u, kXxhP4 = 668265263u, kXxhP5 = 374761393u;

LZ4HIP_DEVICE uint32_t xxh_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
LZ4HIP_DEVICE uint32_t xxh_round(uint32_t v, uint32_t w) { return xxh_rotl(v + w * kXxhP2, 13) * kXxhP1; }

// what follows the stripes, by ONE lane: the length, the remaining words and bytes at p (rest < 16 of them), the avalanche
LZ4HIP_DEVICE uint32_t xxh_finish(uint32_t h, uint64_t len, const uint8_t* p, int rest)
{
    h += (uint32_t)len;
    for (; rest >= 4; rest -= 4, p += 4) h = xxh_rotl(h + load_u32(p) * kXxhP3, 17) * kXxhP4;
    for (; rest > 0; rest--, p++) h = xxh_rotl(h + *p * kXxhP5, 11) * kXxhP1;
    h ^= h >> 15; h *= kXxhP2;
    h ^= h >> 13; h *= kXxhP3;
    h ^= h >> 16;
    return h;
}

// the whole hash by one thread: the descriptor's HC byte (at most 10 bytes), and the host twin of the kernel in tests
__host__ __device__ inline uint32_t xxh32_serial(const uint8_t* p, int64_t len, uint32_t seed)
{
    const uint8_t* end = p + len;
    uint32_t h = seed + kXxhP5;
    auto rd = [](const uint8_t* q) { return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; };
    auto rotl = [](uint32_t x, int r) { return (x << r) | (x >> (32 - r)); };
    if (len >= 16) {
        uint32_t v[4] = { seed + kXxhP1 + kXxhP2, seed + kXxhP2, seed, seed - kXxhP1 };
        for (; end - p >= 16; p += 16)
            for (int j = 0; j < 4; j++) v[j] = rotl(v[j] + rd(p + 4 * j) * kXxhP2, 13) * kXxhP1;
        h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
    }
    h += (uint32_t)len;
    for (; end - p >= 4; p += 4) h = rotl(h + rd(p) * kXxhP3, 17) * kXxhP4;
    for (; p < end; p++) h = rotl(h + *p * kXxhP5, 11) * kXxhP1;
    h ^= h >> 15; h *= kXxhP2;
    h ^= h >> 13; h *= kXxhP3;
    h ^= h >> 16;
    return h;
}

// n rows of bytes: row i is [p, p + len) with p = base + (off ? off[i] : i * stride) and len = len32 ? len32[i] : (len64 ? len64[i] :
// len_all); a negative length counts as 0.  off[i] may be any int64 (the encoder's rows lie in two allocations).
struct XxhRows {
    const uint8_t* base;
    const int64_t* off;
    int64_t stride;
    const int32_t* len32;
    const int64_t* len64;
    int64_t len_all;
    uint32_t seed;
    uint32_t* out;               // one hash per row
    int64_t n;
};

constexpr int kXxhThreads = 256;                                        // four wavefronts: 64 rows per workgroup and pass
constexpr int kXxhRowsPerWave = 16;
constexpr int kXxhDepth = 8;                                            // 64-byte groups of a row in flight while the eight before them are worked on

// lane i receives v from lane i ^ 1 / i ^ 2 of its quad: DPP quad_perm moves where the wave API has them (lz4hip_wave.hpp, and the
// emulator library of this header's own tests), else its general gather: every other emulator library reaches this header through
// lz4hip_framing.hpp over a wave API without the two moves, and has to compile it
#ifdef LZ4HIP_WAVE_QUAD
LZ4HIP_DEVICE uint32_t xxh_quad_xor1(uint32_t v) { return wv::quad_xor1(v); }
LZ4HIP_DEVICE uint32_t xxh_quad_xor2(uint32_t v) { return wv::quad_xor2(v); }
#else
LZ4HIP_DEVICE uint32_t xxh_quad_xor1(uint32_t v) { return wv::shuffle(v, wv::lane() ^ 1); }
LZ4HIP_DEVICE uint32_t xxh_quad_xor2(uint32_t v) { return wv::shuffle(v, wv::lane() ^ 2); }
#endif

// The 4 x 4 dwords a quad holds -- lane i the four words r0 .. r3 of ITS stripe -- transposed: lane j gets word j of the stripes 0 .. 3
// in r0 .. r3.  Two butterfly steps: lanes i and i ^ 1 swap the off-diagonal of every 2 x 2 block, then lanes i and i ^ 2 that of the
// 2 x 2 blocks of blocks: four DPP moves and eight selects.
LZ4HIP_DEVICE void xxh_quad_transpose(int j, uint32_t& r0, uint32_t& r1, uint32_t& r2, uint32_t& r3)
{
    const bool odd = (j & 1) != 0, high = (j & 2) != 0;
    uint32_t s = xxh_quad_xor1(odd ? r0 : r1);
    if (odd) r0 = s; else r1 = s;
    s = xxh_quad_xor1(odd ? r2 : r3);
    if (odd) r2 = s; else r3 = s;
    s = xxh_quad_xor2(high ? r0 : r2);
    if (high) r0 = s; else r2 = s;
    s = xxh_quad_xor2(high ? r1 : r3);
    if (high) r1 = s; else r3 = s;
}

// what a quad whose row has no such group loads instead: the loads of a batch are UNCONDITIONAL (a load under a branch cannot be counted,
// and the wait in front of the rounds would be for everything in flight, the next batch included), so an idle quad reads these 16 bytes
static __device__ const uint32_t kXxhIdleStripe[4] = { 0, 0, 0, 0 };

// One batch of the main loop: kXxhDepth groups of 64 bytes of every row of the wavefront, group k in s[k]: one global_load_dwordx4 per
// group and lane, at any alignment (not a flat load, which would also count on lgkmcnt).
LZ4HIP_DEVICE void xxh_fetch(Vec16 (&s)[kXxhDepth], const uint8_t* p, int j, int64_t first, int64_t groups)
{
#pragma unroll
    for (int k = 0; k < kXxhDepth; k++) {
        const uint8_t* q = first + k < groups ? p + (first + k) * 64 + 16 * j : (const uint8_t*)kXxhIdleStripe;
        wv::load_global16((uint64_t)(uintptr_t)q, s[k].w[0], s[k].w[1], s[k].w[2], s[k].w[3]);
    }
}

// ... and its rounds: each group transposed inside the quad (every lane takes part), then four rounds of this lane's accumulator
LZ4HIP_DEVICE uint32_t xxh_consume(const Vec16 (&s)[kXxhDepth], int j, int64_t first, int64_t groups, uint32_t v)
{
#pragma unroll
    for (int k = 0; k < kXxhDepth; k++) {
        uint32_t w0 = s[k].w[0], w1 = s[k].w[1], w2 = s[k].w[2], w3 = s[k].w[3];
        xxh_quad_transpose(j, w0, w1, w2, w3);
        if (first + k < groups) v = xxh_round(xxh_round(xxh_round(xxh_round(v, w0), w1), w2), w3);
    }
    return v;
}

// A row's four accumulators are four independent serial chains and that is all the parallelism a row has: lane j of a quad owns
// accumulator j, a wavefront works on sixteen rows.  The quad reads 64 bytes at a time, each lane ONE 16-byte stripe with one dwordx4
// load (any alignment), and the 4 x 4 block is transposed inside the quad so that lane j holds word j of four consecutive stripes.
// Two register sets of kXxhDepth groups take turns: one is loaded while the other is worked on.  The loads are plain loads and
// unconditional (xxh_fetch), so the COMPILER counts them: in front of each group's rounds it waits for that group alone (s_waitcnt vmcnt(14)
// down to vmcnt(7) in the gfx950 listing), the batch just asked for still in flight.  The loop is wave-uniform (it runs until the longest of the
// sixteen rows is through: the exchanges need whole quads, and the emulator whole wavefronts); a quad that is done leaves its
// accumulators alone.  The stripes past the last full group (at most three) go by one dword load per lane, inside the row; lane 0 of
// the quad merges and finishes.  No byte of the data outside [p, p + len) is read.
__global__ void __launch_bounds__(kXxhThreads) xxh32_rows_kernel(XxhRows a)
{
    const int lane = wv::lane(), j = lane & 3;
    const int64_t waves = (int64_t)gridDim.x * (kXxhThreads / 64);
    for (int64_t first = ((int64_t)blockIdx.x * (kXxhThreads / 64) + (int64_t)(threadIdx.x >> 6)) * kXxhRowsPerWave; first < a.n;
         first += waves * kXxhRowsPerWave) {
        const int64_t row = first + (lane >> 2);
        const bool live = row < a.n;
        int64_t len = !live ? 0 : (a.len32 ? (int64_t)a.len32[row] : (a.len64 ? a.len64[row] : a.len_all));
        if (len < 0) len = 0;
        const uint8_t* p = (const uint8_t*)((uintptr_t)a.base + (uintptr_t)(live ? (a.off ? a.off[row] : row * a.stride) : 0));
        const int64_t groups = len >> 6;
        uint32_t v = j == 0 ? a.seed + kXxhP1 + kXxhP2 : (j == 1 ? a.seed + kXxhP2 : (j == 2 ? a.seed : a.seed - kXxhP1));

        Vec16 s0[kXxhDepth], s1[kXxhDepth];
        xxh_fetch(s0, p, j, 0, groups);
        for (int64_t g = 0; wv::any(g < groups); g += 2 * kXxhDepth) {
            xxh_fetch(s1, p, j, g + kXxhDepth, groups);
            v = xxh_consume(s0, j, g, groups, v);
            xxh_fetch(s0, p, j, g + 2 * kXxhDepth, groups);
            v = xxh_consume(s1, j, g + kXxhDepth, groups, v);
        }
        const uint8_t* tail = p + groups * 64;
        const int stripes = (int)(len & 63) >> 4;
        for (int s = 0; s < stripes; s++) v = xxh_round(v, load_u32(tail + 16 * s + 4 * j));
        // lane 0 of the quad collects the other three accumulators
        const uint32_t v1 = xxh_quad_xor1(v), v2 = xxh_quad_xor2(v), v3 = xxh_quad_xor2(v1);
        if (live && j == 0) {
            const uint32_t h = len >= 16 ? xxh_rotl(v, 1) + xxh_rotl(v1, 7) + xxh_rotl(v2, 12) + xxh_rotl(v3, 18) : a.seed + kXxhP5;
            a.out[row] = xxh_finish(h, (uint64_t)len, tail + 16 * stripes, (int)(len & 15));
        }
    }
}

// ---- encode ---------------------------------------------------------------------------------------------------------------------
struct Lz4fEncodeArgs {
    const uint8_t* src;          // the source run [0, src_len)
    const uint8_t* comp;         // launch_encode's output: block k at k * stride, at most its length - 1
    int64_t src_len;
    int64_t n;                   // blocks = ceil(src_len / block)
    int64_t stride;
    int32_t block;               // the block maximum size
    int32_t block_id;            // 4 .. 7
    uint32_t flags;              // kLz4fBlockChecksum | kLz4fContentChecksum | kLz4fContentSize (the last one cleared for an empty source)
    int32_t head_len;            // 7, or 15 with the content size
    const int32_t* result;       // launch_encode's per-block results
    uint32_t* sums;              // n block checksums, then the content checksum
    uint8_t* head;               // kLz4fHeadMax bytes: the magic and the descriptor (lz4f_head_kernel)
    int64_t* offs;               // n + 2 segment sizes, scanned in place to their offsets
};

LZ4HIP_DEVICE int32_t lz4f_block_len(const Lz4fEncodeArgs& a, int64_t k)
{
    const int64_t left = a.src_len - k * a.block;
    return left < a.block ? (int32_t)left : a.block;
}

// the format library's rule: compressed iff the encoder, given length - 1 bytes of room, wrote something
LZ4HIP_DEVICE bool lz4f_block_compressed(const Lz4fEncodeArgs& a, int64_t k) { const int32_t r = a.result[k]; return r > 0 && r < lz4f_block_len(a, k); }
LZ4HIP_DEVICE int32_t lz4f_stored_len(const Lz4fEncodeArgs& a, int64_t k) { return lz4f_block_compressed(a, k) ? a.result[k] : lz4f_block_len(a, k); }
LZ4HIP_DEVICE const uint8_t* lz4f_stored(const Lz4fEncodeArgs& a, int64_t k) { return lz4f_block_compressed(a, k) ? a.comp + k * a.stride : a.src + k * a.block; }

__global__ void __launch_bounds__(kStreamThreads) lz4f_lens_kernel(int32_t* lens, int32_t* caps, int64_t n, int64_t src_len, int32_t block)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < n; k += (int64_t)gridDim.x * kStreamThreads) {
        const int64_t left = src_len - k * block;
        const int32_t len = left < block ? (int32_t)left : block;
        lens[k] = len;
        caps[k] = len - 1;
    }
}

// the checksum kernel's rows: where every block's stored bytes lie, relative to the source
__global__ void __launch_bounds__(kStreamThreads) lz4f_rows_kernel(Lz4fEncodeArgs a, int64_t* row_off, int32_t* row_len)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.n; k += (int64_t)gridDim.x * kStreamThreads) {
        row_off[k] = (int64_t)((uintptr_t)lz4f_stored(a, k) - (uintptr_t)a.src);
        row_len[k] = lz4f_stored_len(a, k);
    }
}

// One wavefront, lane 0: the magic, FLG, BD, the content size if asked for, and HC = the second byte of xxh32 over FLG .. before HC.
__global__ void __launch_bounds__(64) lz4f_head_kernel(Lz4fEncodeArgs a)
{
    if (threadIdx.x != 0) return;
    uint8_t h[kLz4fHeadMax];
    int at = 0;
    for (int b = 0; b < 4; b++) h[at++] = (uint8_t)(kLz4fMagic >> (8 * b));
    h[at++] = (uint8_t)(0x60 | ((a.flags & kLz4fBlockChecksum) ? 0x10 : 0) | ((a.flags & kLz4fContentSize) ? 0x08 : 0) |
                        ((a.flags & kLz4fContentChecksum) ? 0x04 : 0));
    h[at++] = (uint8_t)(a.block_id << 4);
    if (a.flags & kLz4fContentSize)
        for (int b = 0; b < 8; b++) h[at++] = (uint8_t)((uint64_t)a.src_len >> (8 * b));
    h[at] = (uint8_t)(xxh32_serial(h + 4, at - 4, 0) >> 8);
    at++;
    for (int b = 0; b < at; b++) a.head[b] = h[b];
}

// ---- the descriptor of the dictionary encode (lz4hip_lz4f_*encode_dict_*) ----------------------------------------------------------------
// What the kernels that lay out a descriptor are handed: nothing by the plain calls (Lz4fPlainHead: kLz4fHeadMax bytes of storage, two
// words), or the call's dictionary ID (Lz4fDictHead: FLG.0 and the ID behind the content size when it is not 0, 4 bytes more, so 24 bytes
// of storage, three words).
constexpr int kLz4fDictHeadMax = 24;                                    // magic + FLG + BD + content size + dictID + HC = 19
struct Lz4fPlainHead {
    static constexpr int kBytes = kLz4fHeadMax;
    __host__ __device__ int32_t len(uint32_t flags) const { return 7 + ((flags & kLz4fContentSize) ? 8 : 0); }
};
struct Lz4fDictHead {
    uint32_t dict_id;                                                   // 0: no ID is written
    static constexpr int kBytes = kLz4fDictHeadMax;
    __host__ __device__ int32_t len(uint32_t flags) const { return 7 + ((flags & kLz4fContentSize) ? 8 : 0) + (dict_id ? 4 : 0); }
};

// The descriptor's HC byte, the second byte of xxh32 (seed 0) over FLG, BD and the content size if there is one: 2 or 10 bytes, in
// registers (xxh32_serial reads memory, and a descriptor built in a local array would live in scratch).
LZ4HIP_DEVICE uint32_t lz4f_batch_hc(uint32_t flg, uint32_t bd, bool sized, uint64_t size)
{
    uint32_t h = kXxhP5 + (sized ? 10u : 2u);
    if (sized) {
        h = xxh_rotl(h + (flg | bd << 8 | (uint32_t)(size & 0xFFFFu) << 16) * kXxhP3, 17) * kXxhP4;
        h = xxh_rotl(h + (uint32_t)(size >> 16) * kXxhP3, 17) * kXxhP4;
        h = xxh_rotl(h + (uint32_t)((size >> 48) & 0xFFu) * kXxhP5, 11) * kXxhP1;
        h = xxh_rotl(h + (uint32_t)(size >> 56) * kXxhP5, 11) * kXxhP1;
    } else {
        h = xxh_rotl(h + flg * kXxhP5, 11) * kXxhP1;
        h = xxh_rotl(h + bd * kXxhP5, 11) * kXxhP1;
    }
    h ^= h >> 15; h *= kXxhP2;
    h ^= h >> 13; h *= kXxhP3;
    h ^= h >> 16;
    return (h >> 8) & 0xFFu;
}

// The HC byte of a descriptor with a dictionary ID: xxh32 (seed 0) over FLG, BD, the content size if there is one and the ID -- 6 bytes (one
// 4-byte lane, two tail bytes) or 14 (three lanes, two tail bytes) -- in registers, as lz4f_batch_hc (lz4hip_lz4f_batch.hpp) has the 2 and 10.
LZ4HIP_DEVICE uint32_t lz4f_dict_hc(uint32_t flg, uint32_t bd, bool sized, uint64_t size, uint32_t id)
{
    uint32_t h = kXxhP5 + (sized ? 14u : 6u);
    if (sized) {
        h = xxh_rotl(h + (flg | bd << 8 | (uint32_t)(size & 0xFFFFu) << 16) * kXxhP3, 17) * kXxhP4;
        h = xxh_rotl(h + (uint32_t)(size >> 16) * kXxhP3, 17) * kXxhP4;
        h = xxh_rotl(h + ((uint32_t)(size >> 48) | (id & 0xFFFFu) << 16) * kXxhP3, 17) * kXxhP4;
    } else {
        h = xxh_rotl(h + (flg | bd << 8 | (id & 0xFFFFu) << 16) * kXxhP3, 17) * kXxhP4;
    }
    h = xxh_rotl(h + ((id >> 16) & 0xFFu) * kXxhP5, 11) * kXxhP1;
    h = xxh_rotl(h + (id >> 24) * kXxhP5, 11) * kXxhP1;
    h ^= h >> 15; h *= kXxhP2;
    h ^= h >> 13; h *= kXxhP3;
    h ^= h >> 16;
    return (h >> 8) & 0xFFu;
}

// The descriptor of the dictionary encode as the three little-endian words of its kLz4fDictHeadMax bytes: with the ID `id` != 0, 11 bytes
// or 19 with the content size; without one the plain descriptor, 7 or 15.  `size` counts only with kLz4fContentSize in flags.
LZ4HIP_DEVICE void lz4f_dict_head_words(uint64_t* head, uint32_t flags, int32_t block_id, uint64_t size, uint32_t id)
{
    const bool sized = (flags & kLz4fContentSize) != 0;
    const uint32_t flg = 0x60u | (id ? 0x01u : 0u) | ((flags & kLz4fBlockChecksum) ? 0x10u : 0u) | (sized ? 0x08u : 0u) | ((flags & kLz4fContentChecksum) ? 0x04u : 0u);
    const uint32_t bd = (uint32_t)block_id << 4;
    const uint64_t front = (uint64_t)kLz4fMagic | (uint64_t)flg << 32 | (uint64_t)bd << 40;
    if (!sized) size = 0;
    if (id) {
        const uint64_t hc = lz4f_dict_hc(flg, bd, sized, size, id);
        head[0] = front | (sized ? size << 48 : (uint64_t)(id & 0xFFFFu) << 48);
        head[1] = sized ? (size >> 16 | (uint64_t)(id & 0xFFFFu) << 48) : ((uint64_t)(id >> 16) | hc << 16);
        head[2] = sized ? ((uint64_t)(id >> 16) | hc << 16) : 0;
    } else {
        const uint64_t hc = lz4f_batch_hc(flg, bd, sized, size);
        head[0] = front | (sized ? size << 48 : hc << 48);
        head[1] = sized ? (size >> 16 | hc << 48) : 0;
        head[2] = 0;
    }
}

// lz4f_head_kernel of the dictionary encode: a.head has kLz4fDictHeadMax bytes (at a multiple of 256), written as words (a descriptor
// built in a local array, as lz4f_head_kernel has it, would live in scratch memory)
__global__ void __launch_bounds__(64) lz4f_dict_head_kernel(Lz4fEncodeArgs a, Lz4fDictHead d)
{
    if (threadIdx.x == 0) lz4f_dict_head_words((uint64_t*)a.head, a.flags, a.block_id, (uint64_t)a.src_len, d.dict_id);
}

// The frame as n + 2 segments of the copy routine.  A block's checksum FOLLOWS its data, and a segment's header bytes come before its
// payload, so the checksum of block k - 1 opens the segment of block k:
//   segment 0       the magic and the descriptor (header bytes only)
//   segment k + 1   [checksum of block k - 1]  size field of block k  |  its stored bytes
//   segment n + 1   [checksum of block n - 1]  EndMark  [content checksum]
LZ4HIP_DEVICE bool lz4f_lead_sum(const Lz4fEncodeArgs& a, int64_t seg) { return seg >= 2 && (a.flags & kLz4fBlockChecksum) != 0; }

__global__ void __launch_bounds__(kStreamThreads) lz4f_sizes_kernel(Lz4fEncodeArgs a)
{
    for (int64_t s = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; s < a.n + 2; s += (int64_t)gridDim.x * kStreamThreads) {
        int64_t bytes = a.head_len;
        if (s > 0) {
            bytes = (lz4f_lead_sum(a, s) ? 4 : 0) + 4;
            if (s <= a.n) bytes += lz4f_stored_len(a, s - 1);
            else if (a.flags & kLz4fContentChecksum) bytes += 4;
        }
        a.offs[s] = bytes;
    }
}

struct Lz4fLayout {
    Lz4fEncodeArgs a;
    LZ4HIP_DEVICE int64_t count() const { return a.n + 2; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.offs[k]; }
    // original: the checksum that opens the segment; clen: the size field (0: the EndMark); flags: 1 = that checksum is there
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        s.start = a.offs[k];
        s.flags = 0; s.original = s.clen = 0;
        s.payload = a.src;
        if (k == 0) {
            s.pbegin = s.pend = s.start + a.head_len;
            return s;
        }
        if (lz4f_lead_sum(a, k)) { s.flags = 1; s.original = a.sums[k - 2]; }
        s.pbegin = s.start + (s.flags ? 8 : 4);
        if (k > a.n) {
            s.pbegin += (a.flags & kLz4fContentChecksum) ? 4 : 0;
            s.pend = s.pbegin;
            return s;
        }
        const int32_t stored = lz4f_stored_len(a, k - 1);
        s.clen = (uint32_t)stored | (lz4f_block_compressed(a, k - 1) ? 0u : kLz4fRawBit);
        s.pend = s.pbegin + stored;
        s.payload = lz4f_stored(a, k - 1);
        return s;
    }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg& s, int64_t x) const
    {
        int i = (int)(x - s.start);
        if (s.start == 0) return a.head[i];                             // (segment 0 alone starts there: the descriptor is never empty)
        if (s.flags) {
            if (i < 4) return (uint8_t)(s.original >> (8 * i));
            i -= 4;
        }
        if (i < 4) return (uint8_t)(s.clen >> (8 * i));
        return (uint8_t)(a.sums[a.n] >> (8 * (i - 4)));                 // (only the last segment has header bytes here)
    }
};

// output bytes [0, min(total, cap)): the total stays within the bound by construction (a stored block is at most its length)
__global__ void __launch_bounds__(kStreamThreads) lz4f_pack_kernel(Lz4fLayout L, uint8_t* dst, const int64_t* total, int64_t cap)
{
    const int64_t end = *total;
    copy_spans(L, dst, end < cap ? end : cap);
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------
constexpr int kLz4fOk = 0, kLz4fBadMagic = 1, kLz4fBadHeader = 2, kLz4fHeaderChecksum = 3, kLz4fUnsupportedLinked = 4, kLz4fUnsupportedDict = 5,
              kLz4fSlotTooSmall = 6, kLz4fTruncated = 7, kLz4fBadBlockSize = 8, kLz4fCorruptBlock = 9, kLz4fBlockChecksumError = 10,
              kLz4fContentSizeError = 11, kLz4fContentChecksumError = 12, kLz4fTableFull = 13, kLz4fDictIdMismatch = 14;
constexpr unsigned kLz4fVerifyBlocks = 1, kLz4fVerifyContent = 2;       // LZ4HIP_LZ4F_VERIFY_* (include/lz4hip.h)
constexpr unsigned kLz4fAcceptLinked = 8;                               // LZ4HIP_LZ4F_ACCEPT_LINKED
constexpr unsigned kLz4fWithDict = 0x100;                               // internal: the call has a dictionary (no public call lets the bit through)
constexpr int kLz4fKindFrame = 0, kLz4fKindSkippable = 1;
constexpr int kLz4fCheckAbsent = 0, kLz4fCheckVerified = 1, kLz4fCheckSkipped = 2;   // info.checks: bits 0-1 the blocks', bits 2-3 the content's
constexpr uint8_t kLz4fRowRaw = 1, kLz4fRowBadSum = 2;
// a row of a frame with linked blocks: the rounds see a hole of its planned size; a dead one lies at or behind its item's first bad block
constexpr uint8_t kLz4fRowLinked = 4, kLz4fRowDead = 8;

// Device twin of lz4hip_lz4f_info_t (include/lz4hip.h; the API checks that the layouts agree).
struct Lz4fInfo {
    int64_t blocks, decoded_bytes, good_bytes, error_offset, content_size, frame_bytes;
    int32_t error, kind, block_max, flg, bd, checks;
};

// what the walk found: int64 slots in caller scratch
constexpr int kLz4fWalkBlocks = 0, kLz4fWalkError = 1, kLz4fWalkErrorOff = 2, kLz4fWalkFullOff = 3, kLz4fWalkFlg = 4, kLz4fWalkBd = 5,
              kLz4fWalkContentSize = 6, kLz4fWalkFrameBytes = 7, kLz4fWalkKind = 8, kLz4fWalkTrailer = 9, kLz4fWalkBlockMax = 10,
              kLz4fWalkContentLen = 11, kLz4fWalkSlots = 12;

// The index: one table in caller scratch, max_blocks rows laid out as the arrays of a lz4hip_batch_t (src_off / dec_len / dst_off /
// result) plus each block's size field offset, its stored length, the length its checksum covers (0 without block checksums) and
// its raw / bad checksum bits.  One frame's table and the table of a batch of frames (lz4hip_lz4f_batch.hpp) are this struct: the one
// frame is the batch of one item, whose rows all belong to item 0 (item = nullptr) and whose walk record starts at walk[0].  In a
// batch src_off is absolute and hdr_off stays relative to the row's item.
struct Lz4fTables {
    int64_t max_blocks;
    int64_t* src_off; int64_t* hdr_off;
    int64_t* dst_off;                                                  // max_blocks + 1 entries: the compact decode's offsets
    int32_t* stored; int32_t* dec_len; int32_t* sum_len; int32_t* result;
    uint32_t* sums;                                                    // max_blocks block checksums as computed; one frame: then the content's
    uint8_t* row;                                                      // kLz4fRow* bits
    int32_t* plan;                                                     // a linked row's size, known before the rounds (lz4hip_lz4f_linked.hpp)
    int32_t* item;                                                     // each row's item; nullptr: one item
    int64_t* walk;                                                     // kLz4fWalk* slots per item
};

LZ4HIP_DEVICE int64_t lz4f_row_item(const int32_t* item, int64_t k) { return item ? item[k] : 0; }

// what one walk found: the kLz4fWalk* slots before they are stored
struct Lz4fWalk {
    int64_t pos, blocks, err_off, content_size, trailer;
    int err, kind, flg, bd;
    int32_t block_max;
};

// A row as the walk leaves it: its bits, and the length the ring decoder is handed -- 0 for a raw row and for a linked one, which it
// sees as empty rows
LZ4HIP_DEVICE uint8_t lz4f_row_bits(bool raw, bool linked) { return (uint8_t)((raw ? kLz4fRowRaw : 0) | (linked ? kLz4fRowLinked : 0)); }
LZ4HIP_DEVICE int32_t lz4f_row_dec_len(uint8_t bits, int32_t size) { return bits ? 0 : size; }

// The walk over ONE frame at src[0, src_len), by every lane of a wavefront on the same (wave-uniform) position; it writes nothing itself:
// row(k, pos, size, bits, sum_bytes) is called for data block k, whose size field lies at pos (bits: lz4f_row_bits).  lz4f_walk_kernel and the batch's walk
// (lz4hip_lz4f_batch.hpp) are this walk with their own rows.  The descriptor's checks come in
// the order a sequential reader applies them: version, reserved bits and block size id; the descriptor's length against the frame's;
// HC; then what this decoder does not take (a dictionary ID, linked blocks unless `flags` has kLz4fAcceptLinked, a block maximum above
// the caller's slot).  With kLz4fWithDict a dictionary ID is taken, and compared in the same place: a frame whose ID is not `dict_id`
// (0: any) is kLz4fDictIdMismatch at the ID field.  With a descriptor error no block is walked.  Per size field: the EndMark (and the content checksum behind it),
// the size against the frame's block maximum, then the data and its checksum against the end of the frame.
template <class Row>
LZ4HIP_DEVICE Lz4fWalk lz4f_walk_frame(const uint8_t* src, int64_t src_len, int32_t slot_bytes, unsigned flags, Row row, uint32_t dict_id = 0)
{
    int64_t pos = 0, blocks = 0, err_off = -1, content_size = -1, trailer = -1;
    int err = kLz4fOk, kind = kLz4fKindFrame, flg = 0, bd = 0;
    int32_t block_max = 0;
    const uint32_t magic = src_len >= 4 ? wv::uniform(load_u32(src)) : 0u;
    if (src_len < 4) { err = kLz4fBadMagic; err_off = 0; }
    else if ((magic & 0xFFFFFFF0u) == kLz4fSkippableMagic) {
        kind = kLz4fKindSkippable;
        if (src_len < 8) { err = kLz4fTruncated; err_off = 4; }
        else {
            pos = 8 + (int64_t)wv::uniform(load_u32(src + 4));
            if (pos > src_len) { err = kLz4fTruncated; err_off = 4; }
        }
    } else if (magic != kLz4fMagic) { err = kLz4fBadMagic; err_off = 0; }
    else if (src_len < 7) { err = kLz4fTruncated; err_off = 4; }
    else {
        flg = (int)wv::uniform((uint32_t)src[4]); bd = (int)wv::uniform((uint32_t)src[5]);
        const int id = (bd >> 4) & 7, dlen = 3 + ((flg & 0x08) ? 8 : 0) + ((flg & 0x01) ? 4 : 0);
        if ((flg >> 6) != 1 || (flg & 0x02) || (bd & 0x8F) || id < 4) { err = kLz4fBadHeader; err_off = 4; }
        else if (4 + dlen > src_len) { err = kLz4fTruncated; err_off = 4; }
        else if ((uint32_t)src[4 + dlen - 1] != ((xxh32_serial(src + 4, dlen - 1, 0) >> 8) & 0xFFu)) { err = kLz4fHeaderChecksum; err_off = 4 + dlen - 1; }
        else {
            block_max = lz4f_block_bytes(id);
            if (flg & 0x08) content_size = (int64_t)wv::uniform(load_u64(src + 6));
            if ((flg & 0x01) && !(flags & kLz4fWithDict)) { err = kLz4fUnsupportedDict; err_off = 4; }
            else if ((flg & 0x01) && dict_id != 0 && wv::uniform(load_u32(src + 4 + dlen - 5)) != dict_id) { err = kLz4fDictIdMismatch; err_off = 4 + dlen - 5; }
            else if (!(flg & 0x20) && !(flags & kLz4fAcceptLinked)) { err = kLz4fUnsupportedLinked; err_off = 4; }
            else if (block_max > slot_bytes) { err = kLz4fSlotTooSmall; err_off = 5; }
            pos = 4 + dlen;
        }
        const int64_t sum_bytes = (flg & 0x10) ? 4 : 0;
        while (err == kLz4fOk) {
            if (pos + 4 > src_len) { err = kLz4fTruncated; err_off = pos; break; }
            const uint32_t field = wv::uniform(load_u32(src + pos));
            if (field == 0) {
                pos += 4;
                if (flg & 0x04) {
                    if (pos + 4 > src_len) { err = kLz4fTruncated; err_off = pos; break; }
                    trailer = pos;
                    pos += 4;
                }
                break;
            }
            const int64_t size = (int64_t)(field & ~kLz4fRawBit);
            if (size > block_max) { err = kLz4fBadBlockSize; err_off = pos; break; }
            if (pos + 4 + size + sum_bytes > src_len) { err = kLz4fTruncated; err_off = pos; break; }
            row(blocks, pos, (int32_t)size, lz4f_row_bits((field & kLz4fRawBit) != 0, !(flg & 0x20)), (int32_t)sum_bytes);
            blocks++;
            pos += 4 + size + sum_bytes;
        }
    }
    Lz4fWalk r;
    r.pos = pos; r.blocks = blocks; r.err_off = err_off; r.content_size = content_size; r.trailer = trailer;
    r.err = err; r.kind = kind; r.flg = flg; r.bd = bd; r.block_max = block_max;
    return r;
}

// the walk's record in its slots; full_off: the size field of the first block that did not fit the table, -1 if all did
LZ4HIP_DEVICE void lz4f_walk_store(int64_t* w, const Lz4fWalk& r, int64_t full_off)
{
    w[kLz4fWalkBlocks] = r.blocks; w[kLz4fWalkError] = r.err; w[kLz4fWalkErrorOff] = r.err_off; w[kLz4fWalkFullOff] = full_off;
    w[kLz4fWalkFlg] = r.flg; w[kLz4fWalkBd] = r.bd; w[kLz4fWalkContentSize] = r.content_size; w[kLz4fWalkFrameBytes] = r.pos;
    w[kLz4fWalkKind] = r.kind; w[kLz4fWalkTrailer] = r.trailer; w[kLz4fWalkBlockMax] = r.block_max; w[kLz4fWalkContentLen] = 0;
}

// One wavefront; every lane runs the same walk on the same (wave-uniform) position and lane 0 writes: row k of the table for block k
// while the table has rows, the record at the end.
__global__ void __launch_bounds__(64) lz4f_walk_kernel(const uint8_t* src, int64_t src_len, int32_t slot_bytes, unsigned flags, Lz4fTables t, uint32_t dict_id)
{
    const int lane = wv::lane();
    int64_t full_off = -1;
    const Lz4fWalk r = lz4f_walk_frame(src, src_len, slot_bytes, flags, [&](int64_t k, int64_t pos, int32_t size, uint8_t bits, int32_t sum_bytes) {
        if (k < t.max_blocks) {
            if (lane == 0) {
                t.src_off[k] = pos + 4; t.hdr_off[k] = pos; t.stored[k] = size;
                t.dec_len[k] = lz4f_row_dec_len(bits, size); t.sum_len[k] = sum_bytes ? size : 0;
                t.row[k] = bits;
            }
        } else if (k == t.max_blocks) {
            full_off = pos;
        }
    }, dict_id);
    if (lane == 0) lz4f_walk_store(t.walk, r, full_off);
}

// after xxh32_rows_kernel over the rows' stored bytes: a row whose checksum does not match is a bad block, and the decoder is handed an
// empty row in its place.  The rows that were tabled: total[0] of them, none if they did not all fit; total == nullptr: one frame, tabled
// while the table had rows.  Whether a row's frame carries block checksums is its item's FLG.4.
__global__ void __launch_bounds__(kStreamThreads) lz4f_verify_kernel(const uint8_t* src, Lz4fTables t, const int64_t* total)
{
    const int64_t rows = total ? total[0] : t.walk[kLz4fWalkBlocks];
    const int64_t n = rows <= t.max_blocks ? rows : (total ? 0 : t.max_blocks);
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < n; k += (int64_t)gridDim.x * kStreamThreads) {
        if (!(t.walk[lz4f_row_item(t.item, k) * kLz4fWalkSlots + kLz4fWalkFlg] & 0x10)) continue;
        if (t.sums[k] != load_u32(src + t.src_off[k] + t.stored[k])) { t.row[k] |= kLz4fRowBadSum; t.dec_len[k] = 0; }
    }
}

// One round of the compact decode (PackedRound: its caps, scan, rebase and state block are the packed paths') with what its own sizes
// step and pack layout look at: the source, the table's columns at row 0 of the round, and the per-item arrays whole.
struct Lz4fRound {
    PackedRound a;
    const uint8_t* src;
    const int64_t* src_off; const int32_t* stored; const uint8_t* row;
    const int32_t* plan;
    const int32_t* item;                                               // nullptr: one item
    const int64_t* walk;
    unsigned long long* item_bad;                                      // per item: its lowest bad row (~0: none); one frame: the state block's kPackedBad
};

// The bytes row k of the round takes, or -1 for a bad block: a row with a bad checksum; a raw row its stored size; a compressed row the
// decoder's result, if it is one and within the block maximum of the ROW's frame (it fits the slot either way).  A linked row takes
// its planned size (0 for a dead one; its item's bad block is the plan's to report).
LZ4HIP_DEVICE int32_t lz4f_row_bytes(const Lz4fRound& r, int64_t k)
{
    const uint8_t bits = r.row[k];
    if (bits & kLz4fRowLinked) return r.plan[k];
    if (bits & kLz4fRowBadSum) return -1;
    if (bits & kLz4fRowRaw) return r.stored[k];
    const int32_t res = r.a.result[k];
    return res < 0 || res > (int32_t)r.walk[lz4f_row_item(r.item, k) * kLz4fWalkSlots + kLz4fWalkBlockMax] || res > r.a.limit ? -1 : res;
}

// The rounds' sizes step, in compact_sizes_kernel's place: the lowest bad row is kept PER ITEM (a round may begin and end in the middle
// of one)
__global__ void __launch_bounds__(kStreamThreads) lz4f_round_sizes_kernel(Lz4fRound r)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < r.a.cnt; k += (int64_t)gridDim.x * kStreamThreads) {
        const int32_t len = lz4f_row_bytes(r, k);
        r.a.offs[k] = len < 0 ? 0 : len;
        if (len < 0) atomicMin(&r.item_bad[lz4f_row_item(r.item, k)], (unsigned long long)(r.a.first + k));
    }
}

// The rounds' pack layout, in PackedLayout's place: a raw row's payload lies in the source; a linked row has none (its bytes up to the
// next row's start are the linked decode's to write)
struct Lz4fRoundLayout {
    Lz4fRound r;
    LZ4HIP_DEVICE int64_t count() const { return r.a.cnt; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return r.a.offs[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        const int32_t len = (r.row[k] & kLz4fRowLinked) ? 0 : lz4f_row_bytes(r, k);
        s.start = s.pbegin = r.a.offs[k];
        s.pend = s.start + (len < 0 ? 0 : len);
        s.payload = (r.row[k] & kLz4fRowRaw) ? r.src + r.src_off[k] : r.a.ring + k * r.a.slot;
        s.flags = s.original = s.clen = 0;
        return s;
    }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg&, int64_t) const { return 0; }   // (no header bytes)
};

__global__ void __launch_bounds__(kStreamThreads) lz4f_round_pack_kernel(Lz4fRoundLayout L, uint8_t* dst, int64_t cap)
{
    const int64_t begin = L.r.a.offs[0], end = L.r.a.state[kPackedBase + (L.r.a.parity ^ 1)];
    copy_spans_from(L, dst, begin, end < cap ? end : cap);
}

// One item's record after the rounds, all but the content checksum's verdict, from its walk slots w, its lowest bad row and its bytes
// [begin, end) of the output; every offset in it is relative to the item.  Precedence, as a sequential reader meets them: a table too
// small (`full`: error_offset -1, which the one-frame call replaces); a descriptor error (no block was walked); the lowest bad block;
// the walk's error (it lies after every tabled block); the content size.  Returns whether the content checksum's row is to be summed:
// that checksum is there, asked for, and the item was wholly written without an error.
LZ4HIP_DEVICE bool lz4f_item_record(Lz4fInfo& r, const int64_t* w, unsigned long long bad, const Lz4fTables& t, bool full, int64_t begin, int64_t end,
                                    unsigned flags, int64_t dst_cap)
{
    const int flg = (int)w[kLz4fWalkFlg];
    r.blocks = w[kLz4fWalkBlocks];
    r.decoded_bytes = r.good_bytes = end - begin;
    r.error = (int32_t)w[kLz4fWalkError];
    r.error_offset = w[kLz4fWalkErrorOff];
    r.content_size = w[kLz4fWalkContentSize];
    r.frame_bytes = w[kLz4fWalkFrameBytes];
    r.kind = (int32_t)w[kLz4fWalkKind];
    r.block_max = (int32_t)w[kLz4fWalkBlockMax];
    r.flg = flg; r.bd = (int32_t)w[kLz4fWalkBd];
    r.checks = 0;
    if (full) {
        r.error = kLz4fTableFull;
        r.error_offset = -1;
    } else if (bad != ~0ull) {
        r.error = (t.row[bad] & kLz4fRowBadSum) ? kLz4fBlockChecksumError : kLz4fCorruptBlock;
        r.error_offset = t.hdr_off[bad];
        r.good_bytes = t.dst_off[bad] - begin;
    } else if (r.error == kLz4fOk && r.kind == kLz4fKindFrame && r.content_size >= 0 && r.content_size != r.decoded_bytes) {
        r.error = kLz4fContentSizeError;
        r.error_offset = 6;
    }
    const bool content = r.error == kLz4fOk && (flg & 0x04) && (flags & kLz4fVerifyContent) && end <= dst_cap;
    if (r.block_max > 0) {                                             // (a descriptor that parsed)
        r.checks = (flg & 0x10) ? ((flags & kLz4fVerifyBlocks) ? kLz4fCheckVerified : kLz4fCheckSkipped) : kLz4fCheckAbsent;
        r.checks |= ((flg & 0x04) ? (content ? kLz4fCheckVerified : kLz4fCheckSkipped) : kLz4fCheckAbsent) << 2;
    }
    return content;
}

// The one frame's record: the item at [0, the decoded total); a table too small is reported at the size field of the first block that
// did not fit.  It also sets the length of the content checksum's row: the decoded total, or 0 if it is not to be summed.
__global__ void __launch_bounds__(64) lz4f_info_kernel(Lz4fTables t, const unsigned long long* bad, unsigned flags, int64_t dst_cap, Lz4fInfo* info)
{
    if (threadIdx.x != 0) return;
    const bool full = t.walk[kLz4fWalkBlocks] > t.max_blocks;
    Lz4fInfo r;
    const bool content = lz4f_item_record(r, t.walk, *bad, t, full, 0, t.dst_off[t.max_blocks], flags, dst_cap);
    if (full) r.error_offset = t.walk[kLz4fWalkFullOff];
    t.walk[kLz4fWalkContentLen] = content ? r.decoded_bytes : 0;
    *info = r;
}

// The content checksum's verdict, after its row was summed: `sum` against the four bytes at frame[trailer].  True if it turned the
// record into an error.
LZ4HIP_DEVICE bool lz4f_content_verdict(Lz4fInfo* info, uint32_t sum, const uint8_t* frame, int64_t trailer)
{
    if (((info->checks >> 2) & 3) != kLz4fCheckVerified || sum == load_u32(frame + trailer)) return false;
    info->error = kLz4fContentChecksumError;
    info->error_offset = trailer;
    return true;
}

// after the content's row: the last verdict
__global__ void __launch_bounds__(64) lz4f_final_kernel(const uint8_t* src, Lz4fTables t, Lz4fInfo* info)
{
    if (threadIdx.x == 0) lz4f_content_verdict(info, t.sums[t.max_blocks], src, t.walk[kLz4fWalkTrailer]);
}

}  // namespace lz4hip
