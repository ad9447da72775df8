// lz4hip_lz4f_linked.hpp -- LZ4 frames whose blocks are LINKED (FLG.5 clear: what LZ4F_compressFrame, python-lz4 and Arrow's LZ4_FRAME
// codec write by default for content above one block), for callers that accept them (kLz4fAcceptLinked).  A match of block k may start
// anywhere in the bytes of its frame already produced, up to 65 535 back, so the blocks of ONE frame decode only in order -- but n
// frames of a batch are n independent chains.  One wavefront takes one frame and decodes its blocks in order, STRAIGHT TO THEIR FINAL
// PLACE in the output: that is where the bytes of the blocks before lie.  So a block's place must be known before it is decoded, and
// with it the size of every block in front of it in the whole batch.  Hence, around the rounds of lz4hip_lz4f.hpp / lz4hip_lz4f_batch.hpp:
//
//   the walk marks every row of a linked frame kLz4fRowLinked and hands the ring decoder an empty row in its place ->
//   [block checksums, as for every row] ->
//   lz4f_linked_sizes_kernel (ONE LANE PER ROW: decoded_size_block of lz4hip_sizes.hpp with the format's 65 535 bytes of history, a
//       raw row its stored size, a row with a bad checksum -1) ->
//   lz4f_linked_plan_kernel (one lane per linked item, over its rows in order: the first bad one -- checksum, a walk that fails, a size
//       above the frame's block maximum -- becomes the item's lowest bad row; it and every row behind it take 0 bytes and are dead) ->
//   the rounds, unchanged: a linked row reports its planned size and is a segment without payload, a hole the pack leaves alone ->
//   lz4f_linked_decode_kernel (ONE WAVEFRONT PER ITEM; the hot path) -> offsets, records, content checksums as for every item
//
// The size walk cannot know a block's real history (that needs the sizes before it); the decoder does, and refuses a match that starts
// before the frame's first byte whatever dst holds there.  A row the decoder refuses keeps its planned place: the item ends there, its
// lowest bad row is that row, and the rows behind it are not touched.  The one-frame call is the batch of one item: the same kernels
// over Lz4fLinked, which either path fills from its own tables.
//
// A linked frame is a serial chain on ONE wavefront: a lone large frame decodes far slower than on a host core (INTEGRATION.md 4 has a
// lone wavefront's figures).  This path pays only in batches of many items.
//
// The dictionary calls (lz4hip_lz4f_*_dict_*) run the same three kernels, the last in its dictionary form: the size walk already allows
// every row 65 535 bytes in front of it, so the plan is the same, and the decoder is where a source before the dictionary is refused.
#pragma once
#include "lz4hip_decode.hpp"
#include "lz4hip_sizes.hpp"
#include "lz4hip_lz4f.hpp"

namespace lz4hip {

constexpr int32_t kLz4fLinkedHistory = 65535;                          // the furthest a match reaches back

// what the three kernels look at, of either path's tables
struct Lz4fLinked {
    const uint8_t* src;
    uint8_t* dst;
    int64_t dst_cap;
    int64_t n, max_blocks;
    const int64_t* walk;                                               // kLz4fWalkSlots slots per item
    const int64_t* base;                                               // the item's first row; nullptr: one item, whose rows start at 0
    const int64_t* total;                                              // [0]: the rows all items need -- above max_blocks nothing was tabled; nullptr:
                                                                       // one item, tabled while the table had rows
    const int64_t* src_off; const int32_t* stored;
    const int64_t* dst_off;                                            // max_blocks + 1 offsets into dst, final after the last round
    uint8_t* row;
    int32_t* plan;
    unsigned long long* item_bad;                                      // per item: its lowest bad row (~0: none)
};

LZ4HIP_DEVICE bool lz4f_linked_full(const Lz4fLinked& a) { return a.total && a.total[0] > a.max_blocks; }

// item i's rows [first, first + count) if it is a frame with linked blocks whose descriptor the walk accepted
LZ4HIP_DEVICE bool lz4f_linked_item(const Lz4fLinked& a, int64_t i, int64_t& first, int64_t& count)
{
    const int64_t* w = a.walk + i * kLz4fWalkSlots;
    first = a.base ? a.base[i] : 0;
    const int64_t room = a.max_blocks - first;
    count = w[kLz4fWalkBlocks] < room ? w[kLz4fWalkBlocks] : (room < 0 ? 0 : room);
    return w[kLz4fWalkKind] == kLz4fKindFrame && w[kLz4fWalkBlockMax] > 0 && !(w[kLz4fWalkFlg] & 0x20) && count > 0;
}

// The size of every linked row before anything is decoded.  Rows that are not linked (and the rows past the walks' count, whose bits
// are 0) are skipped; any grid of kSizesThreads-wide workgroups covers the table.
__global__ void __launch_bounds__(kSizesThreads) lz4f_linked_sizes_kernel(Lz4fLinked a)
{
    LZ4HIP_STATIC_LDS(lds_raw, kSizesLdsBytes);
    uint32_t* const col = (uint32_t*)lds_raw + threadIdx.x;
    for (int64_t k = (int64_t)blockIdx.x * kSizesThreads + threadIdx.x; k < a.max_blocks; k += (int64_t)gridDim.x * kSizesThreads) {
        const uint8_t bits = a.row[k];
        if (!(bits & kLz4fRowLinked)) continue;
        a.plan[k] = (bits & kLz4fRowBadSum) ? -1 : ((bits & kLz4fRowRaw) ? a.stored[k] : decoded_size_block(a.src + a.src_off[k], a.stored[k], col, kLz4fLinkedHistory));
    }
}

// One lane per item: a sequential reader stops at the first bad block, so that row and all behind it take no bytes.
__global__ void __launch_bounds__(kStreamThreads) lz4f_linked_plan_kernel(Lz4fLinked a)
{
    if (lz4f_linked_full(a)) return;
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        int64_t first, count;
        if (!lz4f_linked_item(a, i, first, count)) continue;
        const int32_t block_max = (int32_t)a.walk[i * kLz4fWalkSlots + kLz4fWalkBlockMax];
        bool dead = false;
        for (int64_t k = first; k < first + count; k++) {
            if (!dead && (a.plan[k] < 0 || a.plan[k] > block_max)) {
                dead = true;
                atomicMin(&a.item_bad[i], (unsigned long long)k);
            }
            if (dead) { a.plan[k] = 0; a.row[k] |= kLz4fRowDead; }
        }
    }
}

// One wavefront per item, in workgroups of kWaveDecodeWavesPerGroup; a wavefront whose item is not linked takes the next one at once.
// The item's live rows in order, each at its final place dst + dst_off[row]: a raw row is copied, a compressed row decoded with the
// wavefront decoder at its planned size as capacity and the item's bytes in front of it as history; the result must be that size.
// mem_sync between rows: the next row reads what this one stored, through global memory.  Rows that do not lie wholly inside dst_cap
// end the item (the clip of a linked item is at a block boundary), and so does a row the decoder refuses, which becomes the item's
// lowest bad row.  Nothing is written outside the planned bytes of the item's rows, and nothing at or past dst_cap.
// DICT (the dictionary calls, lz4hip_lz4f_*_dict_*): the call's dictionary, whose dict_len <= 65 535 bytes end at dict_end, counts as
// lying in front of EVERY item's first byte.  A row with `history` bytes of its item in front of it reaches the dictionary's last
// min(dict_len, 65 535 - history) bytes behind them: a source before those is what a source before the frame is without a dictionary.
// The plain form is the instantiation without it, whose code does not know the two arguments.
template <bool DICT>
LZ4HIP_DEVICE void lz4f_linked_decode_items(const Lz4fLinked& a, unsigned char* const ring, const uint8_t* dict_end, int32_t dict_len)
{
    const int64_t waves = (int64_t)gridDim.x * kWaveDecodeWavesPerGroup;
    for (int64_t i = (int64_t)blockIdx.x * kWaveDecodeWavesPerGroup + wv::wave_in_block(); i < a.n; i += waves) {
        int64_t first, count;
        if (!lz4f_linked_item(a, i, first, count)) continue;
        first = wv::uniform(first); count = wv::uniform(count);
        const int64_t begin = wv::uniform(a.dst_off[first]);
        for (int64_t k = first; k < first + count; k++) {
            const uint32_t bits = wv::uniform((uint32_t)a.row[k]);
            if (bits & kLz4fRowDead) break;
            const int64_t at = wv::uniform(a.dst_off[k]);
            const int32_t size = wv::uniform(a.plan[k]), stored = wv::uniform(a.stored[k]);
            if (at + size > a.dst_cap) break;
            const uint8_t* in = a.src + wv::uniform(a.src_off[k]);
            if (bits & kLz4fRowRaw) {
                wave_copy(a.dst + at, in, size);
            } else {
                const int64_t before = at - begin;
                const int history = before < kLz4fLinkedHistory ? (int)before : kLz4fLinkedHistory;
                const int dict_reach = dict_len < kLz4fLinkedHistory - history ? dict_len : kLz4fLinkedHistory - history;
                const int r = decode_block<false, true, DICT>(in, stored, a.dst + at, size, ring, history, dict_end, dict_reach);
                if (r != size) {
                    if (wv::lane() == 0) atomicMin(&a.item_bad[i], (unsigned long long)k);
                    break;
                }
            }
            wv::mem_sync();
        }
    }
}

__global__ void __launch_bounds__(64 * kWaveDecodeWavesPerGroup) lz4f_linked_decode_kernel(Lz4fLinked a)
{
    LZ4HIP_STATIC_LDS(rings, kWaveDecodeWavesPerGroup * kWaveLdsBytes);
    unsigned char* const ring = rings + wv::wave_in_block() * kWaveLdsBytes;
    if (lz4f_linked_full(a)) return;
    lz4f_linked_decode_items<false>(a, ring, nullptr, 0);
}

__global__ void __launch_bounds__(64 * kWaveDecodeWavesPerGroup) lz4f_linked_decode_dict_kernel(Lz4fLinked a, const uint8_t* dict_end, int32_t dict_len)
{
    LZ4HIP_STATIC_LDS(rings, kWaveDecodeWavesPerGroup * kWaveLdsBytes);
    unsigned char* const ring = rings + wv::wave_in_block() * kWaveLdsBytes;
    if (lz4f_linked_full(a)) return;
    lz4f_linked_decode_items<true>(a, ring, dict_end, dict_len);
}

}  // namespace lz4hip
