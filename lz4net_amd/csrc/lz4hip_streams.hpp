// lz4hip_streams.hpp -- many independent LZ4Stream buffers in one call.  A batch of streams is one byte buffer plus int64 offsets
// off[n + 1]: item i is src[off[i], off[i + 1]).  Encode turns every item into the stream lz4hip_stream.hpp writes for that item alone
// and lays the streams back to back; decode reads that layout.  Everything here goes AROUND the merged pieces -- the block codecs
// (launch_encode / launch_decode), the int64 scan, the position-driven copy routine and the header step of lz4hip_stream.hpp:
//
//   encode: streams_counts_kernel (chunks per item, 0 for bad offsets) -> stream_scan_* (first chunk of every item, the chunk total K)
//           -> streams_chunks_kernel (the chunk table: entry k finds its item by bisection; entries >= K are empty blocks at offset 0,
//           the host sizes the table by the bound K <= src_len / block + n) -> [launch_encode into scratch at each chunk's own source
//           position, outputLength = inputLength] -> streams_sizes_kernel -> stream_scan_* (ONE scan over all chunks of all items: the
//           streams are concatenated, so the global layout is each item's local one) -> streams_offsets_kernel (dst_off) ->
//           streams_pack_kernel (copy_spans over StreamsEncodeLayout)
//   index:  streams_walk_kernel<false> (ONE WAVEFRONT PER ITEM counts its chunks, compressed chunks and bytes and finds its header
//           error) -> three scans -> streams_walk_kernel<true> (the same walk again, now writing the compressed and the raw table at
//           the scanned bases) -> streams_info_kernel
//   decode: [launch_decode, known size, on the compressed table of all items] -> stream_raw_copy_kernel (RawLayout over the raw table
//           of all items) -> streams_check_kernel (per item, the header offset of its first corrupt block) -> streams_finish_kernel
//           (final statuses, lowest failing item) -> streams_info_kernel
//   spans:  chosen items of an arena, [begin[j], end[j]) in any order: the walk alone reads an item's end, so the span form is the same
//           sequence behind streams_walk_spans_kernel<false / true>
//
// Every kernel here is launch-only work on the caller's stream over caller scratch.
#pragma once
#include "lz4hip_stream.hpp"

namespace lz4hip {

constexpr int32_t kStreamsBadOffsets = -2000000002;      // LZ4HIP_E_ARGUMENT as an item's status (the API checks that the values agree)

// Device twin of lz4hip_streams_info_t (include/lz4hip.h; the API checks that the layouts agree).
struct StreamsInfo {
    int64_t items, chunks, compressed_chunks, decoded_bytes, first_error, error_offset;
    int32_t error, reserved;
};

// the item src[a, b): false (and an empty item at 0) for bounds that decrease or fall outside [0, src_len]
LZ4HIP_DEVICE bool streams_span(int64_t a, int64_t b, int64_t src_len, int64_t& at, int64_t& len)
{
    at = 0;
    len = 0;
    if (a < 0 || b < a || b > src_len) return false;
    at = a;
    len = b - a;
    return true;
}

// item i of the batch: the span [off[i], off[i + 1])
LZ4HIP_DEVICE bool streams_item(const int64_t* off, int64_t i, int64_t src_len, int64_t& at, int64_t& len)
{
    return streams_span(off[i], off[i + 1], src_len, at, len);
}

// ---- encode ----------------------------------------------------------------------------------------------------------------
struct StreamsEncodeArgs {
    const uint8_t* src;
    const uint8_t* comp;         // launch_encode's output: every chunk at its own source position, at most its length
    const int64_t* off;          // the caller's offsets, n + 1
    int64_t src_len, n;
    int64_t cap;                 // entries of the chunk table: src_len / block + n >= K
    int32_t block;
    uint32_t hc_flag;            // kChunkHighCompression on EVERY chunk of an LZ4HC stream
    int64_t* first;              // chunks per item, then (scanned in place) the item's first chunk; n entries
    const int64_t* total;        // K: the chunks of all items (device)
    int64_t* c_at;               // chunk table: source position (also its position in comp), length, encoder result
    int32_t* c_len;
    const int32_t* result;
    int64_t* offs;               // framed size per chunk, then (scanned in place) its output offset; offs[cap] = the total
};

__global__ void __launch_bounds__(kStreamThreads) streams_counts_kernel(StreamsEncodeArgs a)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        int64_t at, len;
        streams_item(a.off, i, a.src_len, at, len);
        a.first[i] = len <= 0 ? 0 : (len - 1) / a.block + 1;
    }
}

// Entry k of the chunk table.  Offsets that decrease can make items overlap and K exceed the table: the chunks past it are dropped
// (the output is then unspecified, as for lz4hip_wrap_device), nothing outside the table is touched.
__global__ void __launch_bounds__(kStreamThreads) streams_chunks_kernel(StreamsEncodeArgs a)
{
    const int64_t K = *a.total < a.cap ? *a.total : a.cap;
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.cap; k += (int64_t)gridDim.x * kStreamThreads) {
        int64_t at = 0;
        int32_t len = 0;
        if (k < K) {
            int64_t lo = 0, hi = a.n - 1;                             // the last item whose first chunk is <= k owns chunk k
            while (lo < hi) {
                const int64_t mid = hi - (hi - lo) / 2;
                if (a.first[mid] <= k) lo = mid; else hi = mid - 1;
            }
            int64_t item_at, item_len;
            streams_item(a.off, lo, a.src_len, item_at, item_len);
            const int64_t done = (k - a.first[lo]) * a.block, left = item_len - done;
            if (left > 0) {                                           // (always, unless the offsets changed under the call)
                at = item_at + done;
                len = left < a.block ? (int32_t)left : a.block;
            }
        }
        a.c_at[k] = at;
        a.c_len[k] = len;
    }
}

__global__ void __launch_bounds__(kStreamThreads) streams_sizes_kernel(StreamsEncodeArgs a)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.cap; k += (int64_t)gridDim.x * kStreamThreads) {
        const int32_t len = a.c_len[k], r = a.result[k];
        if (len == 0) { a.offs[k] = 0; continue; }                     // padding: no bytes
        const bool c = chunk_compressed(r, len);
        const uint32_t flags = (c ? kChunkCompressed : 0u) | a.hc_flag;
        a.offs[k] = header_len(flags, (uint32_t)len, (uint32_t)r) + (int64_t)(c ? r : len);
    }
}

// dst_off[i] = the offset of item i's first chunk (an empty item: of whatever comes next), dst_off[n] = the total
__global__ void __launch_bounds__(kStreamThreads) streams_offsets_kernel(StreamsEncodeArgs a, int64_t* dst_off)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i <= a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        const int64_t k = i < a.n ? a.first[i] : a.cap;
        dst_off[i] = a.offs[k < a.cap ? k : a.cap];
    }
}

struct StreamsEncodeLayout {
    StreamsEncodeArgs a;
    LZ4HIP_DEVICE int64_t count() const { return a.cap; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.offs[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        const int32_t len = a.c_len[k], r = a.result[k];
        const bool c = len > 0 && chunk_compressed(r, len);
        s.flags = (c ? kChunkCompressed : 0u) | a.hc_flag;
        s.original = (uint32_t)len;
        s.clen = (uint32_t)r;
        s.start = a.offs[k];
        s.pbegin = s.start + (len > 0 ? header_len(s.flags, s.original, s.clen) : 0);
        s.pend = s.pbegin + (c ? r : len);
        s.payload = (c ? a.comp : a.src) + a.c_at[k];
        return s;
    }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg& s, int64_t x) const { return header_byte(s.flags, s.original, s.clen, (int)(x - s.start)); }
};

// output bytes [0, min(total, cap)): the total exceeds the bound only for offsets that decrease, and nothing past cap is written
__global__ void __launch_bounds__(kStreamThreads) streams_pack_kernel(StreamsEncodeLayout L, uint8_t* dst, int64_t cap)
{
    const int64_t total = L.a.offs[L.a.cap];
    copy_spans(L, dst, total < cap ? total : cap);
}

// ---- decode ----------------------------------------------------------------------------------------------------------------
// Scratch of the index and the decode (same scratch for both calls).  `t` holds the two chunk tables of ALL items in the layout of the
// one-stream path (offsets into the whole buffers; c_hdr_off relative to the chunk's item), so launch_decode and RawLayout take them as
// they are; c_item names each compressed chunk's item.
struct StreamsTables {
    StreamTables t;                     // (t.min_bad: the lowest failing item index, ~0: none)
    int64_t* totals;                    // [0] non-empty chunks, [1] compressed chunks of the batch
    int64_t* chunk_base;                // per item: non-empty chunks, then (scanned in place) its first slot among all chunks
    int64_t* comp_base;                 // per item: compressed chunks, then its first row of the compressed table
    unsigned long long* item_bad;       // per item: header offset of its first corrupt block (~0: none)
    int64_t* partial;                   // tile sums of the scans
    int32_t* c_item;
};

struct StreamsDecodeArgs {
    const uint8_t* src;
    const int64_t* off;
    int64_t src_len, n;
    int64_t* dst_off;                   // decoded bytes per item, then (scanned in place) its output offset; dst_off[n] = the total
    int32_t* status;
    int64_t* error_offset;
};

// One wavefront per item walks its headers like stream_index_kernel walks a lone stream.  The count pass (kFill = false) leaves the
// item's three counts, its header status and the failing header's offset; the fill pass, after the scans, writes the tables.
// Item i is src[a.off[i], end[i]): the walk is the only step that reads an item's end, everything after it reads the tables.
template <bool kFill>
LZ4HIP_DEVICE void streams_walk_items(const StreamsDecodeArgs& a, const StreamsTables& t, const int64_t* end)
{
    const int lane = wv::lane();
    if (kFill && t.totals[0] > t.t.max_chunks) return;                 // (TABLE_FULL: the caller grows the tables and indexes again)
    for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        int64_t at, len;
        const bool valid = streams_span(a.off[i], end[i], a.src_len, at, len);
        const uint8_t* const src = a.src + at;
        int64_t pos = 0, out = 0, ncomp = 0, nraw = 0;
        int64_t out_base = 0, comp_base = 0, raw_base = 0;
        if (kFill) { out_base = a.dst_off[i]; comp_base = t.comp_base[i]; raw_base = t.chunk_base[i] - comp_base; }
        int err = kStreamOk;
        while (pos < len) {
            const ChunkHeader h = stream_read_header(src, len, pos, lane);
            if (h.err != kStreamOk) { err = h.err; break; }
            if (h.original != 0) {
                if (kFill && lane == 0) {
                    if (h.compressed) {
                        const int64_t j = comp_base + ncomp;
                        t.t.c_src_off[j] = at + h.payload; t.t.c_dst_off[j] = out_base + out; t.t.c_hdr_off[j] = pos;
                        t.t.c_src_len[j] = h.clen; t.t.c_dst_cap[j] = h.original; t.c_item[j] = (int32_t)i;
                    } else {
                        const int64_t j = raw_base + nraw;
                        t.t.r_dst_off[j] = out_base + out; t.t.r_src_off[j] = at + h.payload; t.t.r_len[j] = h.original;
                    }
                }
                if (h.compressed) ncomp++; else nraw++;
                out += h.original;
            }
            pos = h.payload + h.clen;
        }
        if (!kFill && lane == 0) {
            const int32_t st = valid ? err : kStreamsBadOffsets;
            t.chunk_base[i] = ncomp + nraw;
            t.comp_base[i] = ncomp;
            a.dst_off[i] = out;
            a.status[i] = st;
            a.error_offset[i] = err != kStreamOk ? pos : -1;
            if (st != kStreamOk) atomicMin(t.t.min_bad, (unsigned long long)i);
        }
    }
}

// consecutive items: a.off has n + 1 entries and item i ends where item i + 1 begins
template <bool kFill>
__global__ void __launch_bounds__(64) streams_walk_kernel(StreamsDecodeArgs a, StreamsTables t)
{
    streams_walk_items<kFill>(a, t, a.off + 1);
}

// chosen items: a.off holds the n begins and `end` the n ends, in any order, with repeats, overlaps and holes
template <bool kFill>
__global__ void __launch_bounds__(64) streams_walk_spans_kernel(StreamsDecodeArgs a, StreamsTables t, const int64_t* end)
{
    streams_walk_items<kFill>(a, t, end);
}

// Decode64's check (src/LZ4pn/LZ4Codec.Unsafe.cs:373-378) per chunk; per item, the corrupt block FIRST in its stream
__global__ void __launch_bounds__(kStreamThreads) streams_check_kernel(StreamsTables t, int64_t ncomp)
{
    for (int64_t j = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; j < ncomp; j += (int64_t)gridDim.x * kStreamThreads)
        if (t.t.c_result[j] != t.t.c_src_len[j]) atomicMin(&t.item_bad[t.c_item[j]], (unsigned long long)t.t.c_hdr_off[j]);
}

// every chunk in the tables lies before its item's header error (if any), so an item's corrupt block comes first
__global__ void __launch_bounds__(kStreamThreads) streams_finish_kernel(StreamsDecodeArgs a, StreamsTables t)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        const unsigned long long bad = t.item_bad[i];
        if (bad != ~0ull) { a.status[i] = kStreamCorruptBlock; a.error_offset[i] = (int64_t)bad; }
        if (a.status[i] != kStreamOk) atomicMin(t.t.min_bad, (unsigned long long)i);
    }
}

// info from the tables: the counts, and the lowest failing item with its status (what a sequential loop over the items raises first);
// a batch that needs more than max_chunks table entries is LZ4HIP_STREAM_TABLE_FULL, whatever its items hold
__global__ void __launch_bounds__(64) streams_info_kernel(StreamsDecodeArgs a, StreamsTables t, StreamsInfo* info)
{
    if (threadIdx.x != 0) return;
    const unsigned long long bad = *t.t.min_bad;
    StreamsInfo r;
    r.items = a.n;
    r.chunks = t.totals[0];
    r.compressed_chunks = t.totals[1];
    r.decoded_bytes = a.dst_off[a.n];
    r.first_error = bad == ~0ull ? -1 : (int64_t)bad;
    r.error_offset = bad == ~0ull ? -1 : a.error_offset[bad];
    r.error = bad == ~0ull ? kStreamOk : a.status[bad];
    r.reserved = 0;
    if (r.chunks > t.t.max_chunks) { r.error = kStreamTableFull; r.first_error = -1; r.error_offset = -1; }
    *info = r;
}

// ---- decode in one call, into a buffer of any capacity (see lz4hip_stream.hpp) ---------------------------------------------------
// The items that fit dst_cap are a prefix of the batch: item i is written iff dst_off[i + 1] <= dst_cap.
struct StreamsClip {
    StreamsTables t;
    int32_t* s_src_len; int32_t* s_dst_cap;                            // the decoder's columns, max_chunks rows
    int64_t dst_cap;
    int64_t* written_items; int64_t* written_end;                      // the prefix's length and dst_off[that]; both 0 before the launch
};

__global__ void __launch_bounds__(kStreamThreads) streams_clip_kernel(StreamsDecodeArgs a, StreamsClip c)
{
    const int64_t rows = c.t.t.max_chunks, most = rows > a.n ? rows : a.n;
    const bool full = c.t.totals[0] > rows;
    int64_t ncomp, nraw;
    stream_clip_counts(c.t.totals, full, rows, ncomp, nraw);
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < most; i += (int64_t)gridDim.x * kStreamThreads) {
        if (i < rows) {
            int32_t len = 0, cap = 0;
            if (i < ncomp && a.dst_off[c.t.c_item[i] + 1] <= c.dst_cap) { len = c.t.t.c_src_len[i]; cap = c.t.t.c_dst_cap[i]; }
            c.s_src_len[i] = len;
            c.s_dst_cap[i] = cap;
        }
        // the last item that fits: the offsets do not decrease, so there is one such item at most
        if (!full && i < a.n && a.dst_off[i + 1] <= c.dst_cap && (i + 1 == a.n || a.dst_off[i + 2] > c.dst_cap)) {
            *c.written_items = i + 1;
            *c.written_end = a.dst_off[i + 1];
        }
    }
}

// streams_check_kernel over the rows the decoder was given
__global__ void __launch_bounds__(kStreamThreads) streams_check_into_kernel(StreamsTables t, const int32_t* s_dst_cap)
{
    int64_t ncomp, nraw;
    stream_clip_counts(t.totals, t.totals[0] > t.t.max_chunks, t.t.max_chunks, ncomp, nraw);
    for (int64_t j = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; j < ncomp; j += (int64_t)gridDim.x * kStreamThreads)
        if (s_dst_cap[j] != 0 && t.t.c_result[j] != t.t.c_src_len[j]) atomicMin(&t.item_bad[t.c_item[j]], (unsigned long long)t.t.c_hdr_off[j]);
}

// the info of a batch without items (no table to read it from)
__global__ void streams_empty_info_kernel(StreamsInfo* info)
{
    if (threadIdx.x != 0) return;
    StreamsInfo r = {};
    r.first_error = r.error_offset = -1;
    *info = r;
}

}  // namespace lz4hip
