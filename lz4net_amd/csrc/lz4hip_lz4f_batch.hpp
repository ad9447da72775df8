// lz4hip_lz4f_batch.hpp -- many independent LZ4 frames (lz4hip_lz4f.hpp) in one call.  A batch is one byte buffer plus int64 offsets
// off[n + 1]: item i is src[off[i], off[i + 1]).  Encode turns every item into the frame lz4hip_lz4f.hpp writes for that item alone and
// lays the frames back to back; decode reads that layout, one frame per item.  Everything here goes AROUND pieces that exist: the block
// codecs, the int64 scan, the position-driven copy routine, the rounds' caps and rebase steps and the row checksum kernel:
//
//   encode: lz4f_batch_counts_kernel (blocks per item, the item's span; bad offsets: no blocks) -> stream_scan_* (the first block of every
//           item, the block total K) -> lz4f_batch_blocks_kernel (the block table: row k finds its item by bisection; rows >= K are empty
//           blocks, the host sizes the table by the bound K <= src_len / block + n) -> [launch_encode, ONE batch: every block into scratch
//           at its own source position, capacity length - 1] -> lz4f_batch_rows_kernel + xxh32_rows_kernel (the stored bytes of every
//           block) -> xxh32_rows_kernel (n rows: the items' contents) -> lz4f_batch_head_kernel (n descriptors) -> lz4f_batch_sizes_kernel
//           (every segment's item and size) -> stream_scan_* (ONE scan: the frames are concatenated, so the global layout is each item's
//           local one) -> lz4f_batch_offsets_kernel (dst_off) -> lz4f_batch_pack_kernel (copy_spans over Lz4fBatchLayout)
//           With a dictionary (lz4hip_lz4f_batch_encode_dict_*) the block call is launch_encode_dict_prime + launch_encode_dict, and
//           the three kernels that know a descriptor's length are lz4f_batch_dict_head_kernel, lz4f_batch_dict_sizes_kernel and
//           lz4f_batch_dict_pack_kernel (Lz4fDictHead: the dictionary ID, 24 bytes of storage per item); everything else is the same.
//
//   decode: lz4f_batch_walk_kernel<false> (ONE WAVEFRONT PER ITEM runs lz4f_walk_frame: the item's record and its block count) ->
//           stream_scan_* (the first row of every item, the row total) -> lz4f_batch_walk_kernel<true> (the same walk again, writing
//           rows at the item's base with absolute source offsets and the item's index) -> [xxh32_rows_kernel over all rows +
//           lz4f_verify_kernel] -> the one-frame decode's rounds over ALL max_blocks rows, the SAME kernels (packed_caps_kernel, the
//           block decoder, lz4f_round_sizes_kernel, the scan, packed_rebase_kernel, lz4f_round_pack_kernel): a round may begin and
//           end in the middle of an item; the lowest bad row is kept PER ITEM -> [the linked items, each on one wavefront:
//           lz4hip_lz4f_linked.hpp, which also sizes their rows before the rounds] -> lz4f_batch_offsets_out_kernel (dst_off) ->
//           lz4f_batch_info_kernel (one thread per item: lz4f_item_record, the item's content row) -> xxh32_rows_kernel (n rows of
//           the output) -> lz4f_batch_final_kernel -> lz4f_batch_record_kernel
//
// The one-frame decode is the batch of one item: the table's rows (Lz4fTables), the round view, the sizes step, the pack layout, the
// block checksum verdict, the item record and the content checksum's verdict are lz4hip_lz4f.hpp's, written once for both.  The walks
// stay two kernels: the batch needs a count pass, a scan and a fill pass, and running a lone large frame's walk twice would double a
// serial chain of dependent loads.
//
// A lane-per-item walk is the alternative should the walk dominate a measured profile; it is not built.
// Every kernel here is launch-only work on the caller's stream over caller scratch; every table value is an ordinary store.
#pragma once
#include "lz4hip_lz4f.hpp"
#include "lz4hip_streams.hpp"

namespace lz4hip {

constexpr int32_t kLz4fBatchBadOffsets = -2000000002;    // LZ4HIP_E_ARGUMENT as an item's outcome (the API checks that the values agree)

// Device twin of lz4hip_lz4f_batch_info_t (include/lz4hip.h; the API checks that the layouts agree).
struct Lz4fBatchInfo {
    int64_t items, blocks, decoded_bytes, first_error, error_offset;
    int32_t error, reserved;
};

// ---- encode ---------------------------------------------------------------------------------------------------------------------
// Segments of the output, per item: its descriptor, its blocks, its tail ([checksum of the last block] EndMark [content checksum]).
// Item i's descriptor is segment first[i] + 2 * i; the segments past the last item's tail are padding of no bytes.
struct Lz4fBatchEncodeArgs {
    const uint8_t* src;
    const uint8_t* comp;         // the block encoder's output: every block at its own source position, at most its length - 1
    const int64_t* off;          // the caller's offsets, n + 1
    int64_t src_len, n;
    int64_t cap;                 // rows of the block table: src_len / block + n >= K
    int32_t block;               // the block maximum size
    int32_t block_id;            // 4 .. 7
    uint32_t flags;              // kLz4fBlockChecksum | kLz4fContentChecksum | kLz4fContentSize (an empty item's frame drops the last)
    int64_t* item_at;            // per item: where it starts, and its length (-1: bad offsets, the item takes no bytes)
    int64_t* item_len;
    int64_t* first;              // blocks per item, then (scanned in place) the item's first block; n entries
    const int64_t* total;        // K: the blocks of all items (device)
    int64_t* c_at;               // block table: source position (also its position in comp), length, capacity, encoder result
    int32_t* c_len;
    int32_t* c_cap;
    const int32_t* result;
    uint32_t* sums;              // cap block checksums, then n content checksums
    uint8_t* head;               // kLz4fHeadMax bytes per item (the dictionary encode: kLz4fDictHeadMax)
    int32_t* seg_item;           // per segment: its item, -1 for padding
    int64_t* offs;               // cap + 2 n segment sizes, scanned in place to their offsets; offs[cap + 2 n] = the total
};

LZ4HIP_DEVICE int64_t lz4f_batch_segments(const Lz4fBatchEncodeArgs& a) { return a.cap + 2 * a.n; }
LZ4HIP_DEVICE int64_t lz4f_batch_blocks(const Lz4fBatchEncodeArgs& a) { return *a.total < a.cap ? *a.total : a.cap; }
LZ4HIP_DEVICE uint32_t lz4f_batch_item_flags(const Lz4fBatchEncodeArgs& a, int64_t i) { return a.item_len[i] > 0 ? a.flags : a.flags & ~kLz4fContentSize; }
// blocks of item i that lie in the table (offsets that decrease can make K exceed it: the blocks past it are dropped)
LZ4HIP_DEVICE int64_t lz4f_batch_item_blocks(const Lz4fBatchEncodeArgs& a, int64_t i)
{
    const int64_t K = lz4f_batch_blocks(a), b = a.first[i] < K ? a.first[i] : K, e = i + 1 < a.n ? a.first[i + 1] : K;
    return (e < K ? e : K) - b < 0 ? 0 : (e < K ? e : K) - b;
}
LZ4HIP_DEVICE bool lz4f_batch_compressed(const Lz4fBatchEncodeArgs& a, int64_t k) { const int32_t r = a.result[k]; return r > 0 && r < a.c_len[k]; }
LZ4HIP_DEVICE int32_t lz4f_batch_stored_len(const Lz4fBatchEncodeArgs& a, int64_t k) { return lz4f_batch_compressed(a, k) ? a.result[k] : a.c_len[k]; }
LZ4HIP_DEVICE const uint8_t* lz4f_batch_stored(const Lz4fBatchEncodeArgs& a, int64_t k) { return (lz4f_batch_compressed(a, k) ? a.comp : a.src) + a.c_at[k]; }

__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_counts_kernel(Lz4fBatchEncodeArgs a)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        int64_t at, len;
        const bool valid = streams_item(a.off, i, a.src_len, at, len);
        a.item_at[i] = at;
        a.item_len[i] = valid ? len : -1;
        a.first[i] = len <= 0 ? 0 : (len - 1) / a.block + 1;
    }
}

// Row k of the block table, as streams_chunks_kernel finds it: the last item whose first block is <= k owns block k.
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_blocks_kernel(Lz4fBatchEncodeArgs a)
{
    const int64_t K = lz4f_batch_blocks(a);
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.cap; k += (int64_t)gridDim.x * kStreamThreads) {
        int64_t at = 0;
        int32_t len = 0;
        if (k < K) {
            int64_t lo = 0, hi = a.n - 1;
            while (lo < hi) {
                const int64_t mid = hi - (hi - lo) / 2;
                if (a.first[mid] <= k) lo = mid; else hi = mid - 1;
            }
            const int64_t done = (k - a.first[lo]) * a.block, left = a.item_len[lo] - done;
            if (left > 0) {
                at = a.item_at[lo] + done;
                len = left < a.block ? (int32_t)left : a.block;
            }
        }
        a.c_at[k] = at;
        a.c_len[k] = len;
        a.c_cap[k] = len > 0 ? len - 1 : 0;                            // the format library's rule: one byte less than the block
    }
}

// the checksum kernel's rows: where every block's stored bytes lie, relative to the source
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_rows_kernel(Lz4fBatchEncodeArgs a, int64_t* row_off, int32_t* row_len)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.cap; k += (int64_t)gridDim.x * kStreamThreads) {
        row_off[k] = (int64_t)((uintptr_t)lz4f_batch_stored(a, k) - (uintptr_t)a.src);
        row_len[k] = lz4f_batch_stored_len(a, k);
    }
}

// lz4f_head_kernel per item, one thread each: the magic, FLG, BD, the content size if asked for (not for an empty item) and HC, as the
// two little-endian words of the item's kLz4fHeadMax bytes
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_head_kernel(Lz4fBatchEncodeArgs a)
{
    static_assert(kLz4fHeadMax == 16, "two 64-bit words per descriptor");
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        const uint32_t flags = lz4f_batch_item_flags(a, i);
        const bool sized = (flags & kLz4fContentSize) != 0;
        const uint64_t size = sized ? (uint64_t)a.item_len[i] : 0;
        const uint32_t flg = 0x60u | ((flags & kLz4fBlockChecksum) ? 0x10u : 0u) | (sized ? 0x08u : 0u) | ((flags & kLz4fContentChecksum) ? 0x04u : 0u);
        const uint32_t bd = (uint32_t)a.block_id << 4;
        const uint64_t hc = lz4f_batch_hc(flg, bd, sized, size);
        uint64_t* head = (uint64_t*)(a.head + i * kLz4fHeadMax);       // (the descriptors start at a multiple of 256 bytes)
        head[0] = (uint64_t)kLz4fMagic | (uint64_t)flg << 32 | (uint64_t)bd << 40 | (sized ? size << 48 : hc << 48);
        head[1] = sized ? (size >> 16 | hc << 48) : 0;
    }
}

// ... and of the dictionary encode: three words of the item's kLz4fDictHeadMax bytes; without an ID the plain descriptor
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_dict_head_kernel(Lz4fBatchEncodeArgs a, Lz4fDictHead d)
{
    static_assert(kLz4fDictHeadMax == 24, "three 64-bit words per descriptor");
    // (the descriptors start at a multiple of 256 bytes)
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads)
        lz4f_dict_head_words((uint64_t*)(a.head + i * kLz4fDictHeadMax), lz4f_batch_item_flags(a, i), a.block_id, (uint64_t)a.item_len[i], d.dict_id);
}

// One segment: whose it is and which of the item's it is (0: the descriptor, 1 .. blocks: a block, blocks + 1: the tail).
struct Lz4fBatchSeg { int64_t item, local, blocks, row; };              // row: the block's table row (for the tail: one past the item's last)

LZ4HIP_DEVICE Lz4fBatchSeg lz4f_batch_seg_of(const Lz4fBatchEncodeArgs& a, int64_t s, int64_t item)
{
    Lz4fBatchSeg g;
    g.item = item;
    g.blocks = lz4f_batch_item_blocks(a, item);
    g.local = s - (a.first[item] + 2 * item);
    g.row = a.first[item] + g.local - 1;
    return g;
}

// the segment's bytes; lead: the checksum of the block before it opens a segment (a block's checksum FOLLOWS its data)
template <class H = Lz4fPlainHead>
LZ4HIP_DEVICE int64_t lz4f_batch_seg_bytes(const Lz4fBatchEncodeArgs& a, const Lz4fBatchSeg& g, const H& head = H())
{
    if (a.item_len[g.item] < 0 || g.local < 0 || g.local > g.blocks + 1) return 0;
    const uint32_t flags = lz4f_batch_item_flags(a, g.item);
    if (g.local == 0) return head.len(flags);
    int64_t bytes = (g.local >= 2 && (flags & kLz4fBlockChecksum) ? 4 : 0) + 4;
    if (g.local <= g.blocks) bytes += lz4f_batch_stored_len(a, g.row);
    else if (flags & kLz4fContentChecksum) bytes += 4;
    return bytes;
}

// every segment's item (bisection over first[i] + 2 i, which grows with i) and size
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_sizes_kernel(Lz4fBatchEncodeArgs a)
{
    const int64_t S = lz4f_batch_segments(a), used = lz4f_batch_blocks(a) + 2 * a.n;
    for (int64_t s = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; s < S; s += (int64_t)gridDim.x * kStreamThreads) {
        int64_t bytes = 0;
        int32_t item = -1;
        if (s < used) {
            int64_t lo = 0, hi = a.n - 1;
            while (lo < hi) {
                const int64_t mid = hi - (hi - lo) / 2;
                if (a.first[mid] + 2 * mid <= s) lo = mid; else hi = mid - 1;
            }
            item = (int32_t)lo;
            bytes = lz4f_batch_seg_bytes(a, lz4f_batch_seg_of(a, s, lo));
        }
        a.seg_item[s] = item;
        a.offs[s] = bytes;
    }
}

// ... with the dictionary encode's descriptors (the loop is written twice: as one function of both kernels it changed the plain kernel's
// listing, profiles/lz4f_dict_encode/listing_parent_vs_new.txt)
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_dict_sizes_kernel(Lz4fBatchEncodeArgs a, Lz4fDictHead d)
{
    const int64_t S = lz4f_batch_segments(a), used = lz4f_batch_blocks(a) + 2 * a.n;
    for (int64_t s = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; s < S; s += (int64_t)gridDim.x * kStreamThreads) {
        int64_t bytes = 0;
        int32_t item = -1;
        if (s < used) {
            int64_t lo = 0, hi = a.n - 1;
            while (lo < hi) {
                const int64_t mid = hi - (hi - lo) / 2;
                if (a.first[mid] + 2 * mid <= s) lo = mid; else hi = mid - 1;
            }
            item = (int32_t)lo;
            bytes = lz4f_batch_seg_bytes(a, lz4f_batch_seg_of(a, s, lo), d);
        }
        a.seg_item[s] = item;
        a.offs[s] = bytes;
    }
}

// dst_off[i] = the offset of item i's descriptor, dst_off[n] = the total
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_offsets_kernel(Lz4fBatchEncodeArgs a, int64_t* dst_off)
{
    const int64_t S = lz4f_batch_segments(a);
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i <= a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        const int64_t s = i < a.n ? a.first[i] + 2 * i : S;
        dst_off[i] = a.offs[s < S ? s : S];
    }
}

// Lz4fLayout's twin over the segments of all items.  flags: 1 = the checksum that opens the segment is there (in `original`), 4 = a
// descriptor, whose bytes are the payload pointer's; a tail's content checksum lies behind the payload pointer too.
template <class H>
LZ4HIP_DEVICE CopySeg lz4f_batch_layout_seg(const Lz4fBatchEncodeArgs& a, int64_t k, const H& head)
{
    CopySeg s;
    s.start = s.pbegin = s.pend = a.offs[k];
    s.flags = 0; s.original = s.clen = 0;
    s.payload = a.src;
    const int32_t item = a.seg_item[k];
    if (item < 0) return s;
    const Lz4fBatchSeg g = lz4f_batch_seg_of(a, k, item);
    if (lz4f_batch_seg_bytes(a, g, head) == 0) return s;
    const uint32_t flags = lz4f_batch_item_flags(a, item);
    if (g.local == 0) {
        s.flags = 4;
        s.payload = a.head + (int64_t)item * H::kBytes;
        s.pbegin = s.pend = s.start + head.len(flags);
        return s;
    }
    if (g.local >= 2 && (flags & kLz4fBlockChecksum)) { s.flags = 1; s.original = a.sums[g.row - 1]; }
    s.pbegin = s.start + (s.flags ? 8 : 4);
    if (g.local > g.blocks) {
        s.payload = (const uint8_t*)(a.sums + a.cap + item);
        s.pbegin += (flags & kLz4fContentChecksum) ? 4 : 0;
        s.pend = s.pbegin;
        return s;
    }
    const int32_t stored = lz4f_batch_stored_len(a, g.row);
    s.clen = (uint32_t)stored | (lz4f_batch_compressed(a, g.row) ? 0u : kLz4fRawBit);
    s.pend = s.pbegin + stored;
    s.payload = lz4f_batch_stored(a, g.row);
    return s;
}
LZ4HIP_DEVICE uint8_t lz4f_batch_layout_head_byte(const CopySeg& s, int64_t x)
{
    int i = (int)(x - s.start);
    if (s.flags & 4) return s.payload[i];
    if (s.flags & 1) {
        if (i < 4) return (uint8_t)(s.original >> (8 * i));
        i -= 4;
    }
    if (i < 4) return (uint8_t)(s.clen >> (8 * i));
    return s.payload[i - 4];                                        // (only a tail has header bytes here: its content checksum)
}
struct Lz4fBatchLayout {
    Lz4fBatchEncodeArgs a;
    LZ4HIP_DEVICE int64_t count() const { return lz4f_batch_segments(a); }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.offs[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const { return lz4f_batch_layout_seg(a, k, Lz4fPlainHead()); }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg& s, int64_t x) const { return lz4f_batch_layout_head_byte(s, x); }
};
// ... of the dictionary encode: the descriptors are Lz4fDictHead's
struct Lz4fBatchDictLayout {
    Lz4fBatchEncodeArgs a;
    Lz4fDictHead d;
    LZ4HIP_DEVICE int64_t count() const { return lz4f_batch_segments(a); }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.offs[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const { return lz4f_batch_layout_seg(a, k, d); }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg& s, int64_t x) const { return lz4f_batch_layout_head_byte(s, x); }
};

// output bytes [0, min(total, cap)): the total exceeds the bound only for offsets that decrease, and nothing past cap is written
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_pack_kernel(Lz4fBatchLayout L, uint8_t* dst, int64_t cap)
{
    const int64_t total = L.a.offs[lz4f_batch_segments(L.a)];
    copy_spans(L, dst, total < cap ? total : cap);
}
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_dict_pack_kernel(Lz4fBatchDictLayout L, uint8_t* dst, int64_t cap)
{
    const int64_t total = L.a.offs[lz4f_batch_segments(L.a)];
    copy_spans(L, dst, total < cap ? total : cap);
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------
// The index of ALL items: the rows of every item in one Lz4fTables (absolute source offsets, each row's item, kLz4fWalkSlots walk slots
// per item), plus what is kept per item.
struct Lz4fBatchTables {
    Lz4fTables rows;
    int64_t n;
    int64_t* item_at;                                                  // where the item starts in the source
    int64_t* base;                                                     // blocks per item, then (scanned in place) its first row
    int64_t* total;                                                    // [0]: the rows all items need
    unsigned long long* item_bad;                                      // per item: its lowest bad row (~0: none)
    unsigned long long* min_bad;                                       // the lowest failing item (~0: none)
    int64_t* content_off; int64_t* content_len;                        // the n rows of the content checksums in the output
    uint32_t* content_sums;
};

struct Lz4fBatchDecodeArgs {
    const uint8_t* src;
    const int64_t* off;
    int64_t src_len, n;
    int32_t slot_bytes;
    unsigned flags;
    int64_t dst_cap;
    int64_t* dst_off;                                                  // n + 1
    Lz4fInfo* item_info;                                               // n
    int64_t* written_items;
    uint32_t dict_id;                                                  // with kLz4fWithDict in flags: the ID a frame's must equal (0: any)
};

LZ4HIP_DEVICE bool lz4f_batch_full(const Lz4fBatchTables& t) { return t.total[0] > t.rows.max_blocks; }

// One wavefront per item runs the one-frame walk on it.  The count pass (kFill = false) leaves the item's record and its block count;
// the fill pass, after the scan, writes the item's rows at its base.  An item whose offsets decrease or leave [0, src_len] is not
// walked: no blocks, LZ4HIP_E_ARGUMENT.  With more rows than the table has nothing is filled.
template <bool kFill>
__global__ void __launch_bounds__(64) lz4f_batch_walk_kernel(Lz4fBatchDecodeArgs a, Lz4fBatchTables t)
{
    const int lane = wv::lane();
    if (kFill && lz4f_batch_full(t)) return;
    for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        int64_t at, len;
        const bool valid = streams_item(a.off, i, a.src_len, at, len);
        const int64_t base = kFill ? t.base[i] : 0;
        Lz4fWalk r;
        if (valid) {
            r = lz4f_walk_frame(a.src + at, len, a.slot_bytes, a.flags, [&](int64_t k, int64_t pos, int32_t size, uint8_t bits, int32_t sum_bytes) {
                if (kFill && lane == 0 && base + k < t.rows.max_blocks) {
                    const int64_t j = base + k;
                    t.rows.src_off[j] = at + pos + 4; t.rows.hdr_off[j] = pos; t.rows.stored[j] = size;
                    t.rows.dec_len[j] = lz4f_row_dec_len(bits, size); t.rows.sum_len[j] = sum_bytes ? size : 0;
                    t.rows.row[j] = bits; t.rows.item[j] = (int32_t)i;
                }
            }, a.dict_id);
        } else {
            r.pos = r.blocks = 0; r.err_off = r.content_size = r.trailer = -1;
            r.err = kLz4fBatchBadOffsets; r.kind = kLz4fKindFrame; r.flg = r.bd = 0; r.block_max = 0;
        }
        if (!kFill && lane == 0) {
            lz4f_walk_store(t.rows.walk + i * kLz4fWalkSlots, r, -1);
            t.item_at[i] = at;
            t.base[i] = r.blocks;
        }
    }
}

// dst_off[i] = the table's offset at the item's first row, dst_off[n] = the total
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_offsets_out_kernel(Lz4fBatchDecodeArgs a, Lz4fBatchTables t)
{
    const int64_t m = t.rows.max_blocks;
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i <= a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        const int64_t k = i < a.n && !lz4f_batch_full(t) ? t.base[i] : m;
        a.dst_off[i] = t.rows.dst_off[k < m ? k : m];
    }
}

// One thread per item: its record (lz4f_item_record over its bytes of the output), the length of the item's content row, the prefix of
// items that lie wholly inside dst_cap, the lowest failing item.  With a table that is too small every item's outcome is
// LZ4HIP_LZ4F_TABLE_FULL.
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_info_kernel(Lz4fBatchDecodeArgs a, Lz4fBatchTables t)
{
    const bool full = lz4f_batch_full(t);
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        const int64_t begin = a.dst_off[i], end = a.dst_off[i + 1];
        Lz4fInfo r;
        const bool content = lz4f_item_record(r, t.rows.walk + i * kLz4fWalkSlots, t.item_bad[i], t.rows, full, begin, end, a.flags, a.dst_cap);
        t.content_off[i] = begin;
        t.content_len[i] = content ? r.decoded_bytes : 0;
        a.item_info[i] = r;
        // the last item that fits: the offsets do not decrease, so there is one such item at most
        if (!full && end <= a.dst_cap && (i + 1 == a.n || a.dst_off[i + 2] > a.dst_cap)) *a.written_items = i + 1;
        if (r.error != kLz4fOk && !full) atomicMin(t.min_bad, (unsigned long long)i);
    }
}

// after the content rows: the items' last verdict
__global__ void __launch_bounds__(kStreamThreads) lz4f_batch_final_kernel(Lz4fBatchDecodeArgs a, Lz4fBatchTables t)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads)
        if (lz4f_content_verdict(a.item_info + i, t.content_sums[i], a.src + t.item_at[i], t.rows.walk[i * kLz4fWalkSlots + kLz4fWalkTrailer]))
            atomicMin(t.min_bad, (unsigned long long)i);
}

// The batch record: the counts, and the lowest failing item with its outcome (what a sequential loop over the items raises first); a
// batch that needs more than max_blocks rows is LZ4HIP_LZ4F_TABLE_FULL with the count needed, whatever its items hold.
__global__ void __launch_bounds__(64) lz4f_batch_record_kernel(Lz4fBatchDecodeArgs a, Lz4fBatchTables t, Lz4fBatchInfo* info)
{
    if (threadIdx.x != 0) return;
    const unsigned long long bad = *t.min_bad;
    Lz4fBatchInfo r;
    r.items = a.n;
    r.blocks = t.total[0];
    r.decoded_bytes = a.dst_off[a.n];
    r.first_error = bad == ~0ull ? -1 : (int64_t)bad;
    r.error_offset = bad == ~0ull ? -1 : a.item_info[bad].error_offset;
    r.error = bad == ~0ull ? kLz4fOk : a.item_info[bad].error;
    r.reserved = 0;
    if (lz4f_batch_full(t)) { r.error = kLz4fTableFull; r.first_error = -1; r.error_offset = -1; }
    *info = r;
}

// the record of a batch without items (no table to read it from)
__global__ void __launch_bounds__(64) lz4f_batch_empty_record_kernel(Lz4fBatchInfo* info)
{
    if (threadIdx.x != 0) return;
    Lz4fBatchInfo r = {};
    r.first_error = r.error_offset = -1;
    *info = r;
}

}  // namespace lz4hip
