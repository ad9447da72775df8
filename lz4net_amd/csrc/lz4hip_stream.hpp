// lz4hip_stream.hpp -- device-side framing of lz4net's LZ4Stream wire format (src/LZ4/LZ4Stream.cs:239-312) around the block
// kernels: a stream is a run of chunks
//
//     varint(flags)  varint(originalLength)  [varint(compressedLength) if flags & Compressed]  payload
//
// (lz4net_amd/stream.py has the host twin and the citations).  The block codecs themselves are the batch kernels of the library;
// this header holds only what goes around them:
//
//   encode: stream_lens_kernel (chunk lengths) -> [launch_encode into scratch, outputLength = inputLength] -> stream_sizes_kernel
//           (framed size per chunk) -> stream_scan_* (exclusive scan of the sizes, total to the caller's device int64) ->
//           stream_pack_kernel (headers + payloads, driven by output position)
//   decode: stream_index_kernel (ONE wavefront walks the headers, one dependent global round trip per chunk, and writes the
//           compressed and the raw chunks to two separate tables) -> [launch_decode on the compressed table] ->
//           stream_raw_copy_kernel (same copy routine as the pack) -> stream_check_kernel (the first corrupt block in stream order)
//   directory: stream_directory_kernel (the index's walk, writing every chunk's header and output offset to the caller's arrays)
//
// Every kernel here is launch-only work on the caller's stream over caller scratch.
#pragma once
#include "lz4hip_common.hpp"

namespace lz4hip {

constexpr int kStreamOk = 0, kStreamEndOfStream = 1, kStreamPasses = 2, kStreamCorruptBlock = 3, kStreamTableFull = 4;
constexpr uint32_t kChunkCompressed = 1, kChunkHighCompression = 2;     // ChunkFlags (src/LZ4/LZ4Stream.cs:43-59)
constexpr int kStreamThreads = 256;
constexpr int kScanItems = 16, kScanTile = kStreamThreads * kScanItems; // elements per workgroup of the scan

// Device twin of lz4hip_stream_info_t (include/lz4hip.h; the API checks that the layouts agree).
struct StreamInfo {
    int64_t chunks, compressed_chunks, decoded_bytes, error_offset;
    int32_t error, reserved;
};

__host__ __device__ inline int varint_len(uint64_t v)
{
    int n = 1;
    while (v >= 0x80) { v >>= 7; n++; }
    return n;
}

// ---- encode ------------------------------------------------------------------------------------------------------------
struct StreamEncodeArgs {
    const uint8_t* src;          // the source run [0, src_len)
    const uint8_t* comp;         // launch_encode's output: chunk k at k * block, at most its length
    int64_t src_len;
    int64_t n;                   // chunks = ceil(src_len / block)
    int32_t block;
    uint32_t hc_flag;            // kChunkHighCompression on EVERY chunk of an LZ4HC stream, raw chunks included (as the reference writes it)
    const int32_t* result;       // launch_encode's per-chunk results
    int64_t* offs;               // framed size per chunk, then (scanned in place) its output offset
};

LZ4HIP_DEVICE int32_t chunk_len(const StreamEncodeArgs& a, int64_t k)
{
    const int64_t left = a.src_len - k * a.block;
    return left < a.block ? (int32_t)left : a.block;
}

// FlushCurrentChunk: compressed iff the encoder returned 0 < r < length
LZ4HIP_DEVICE bool chunk_compressed(int32_t r, int32_t len) { return r > 0 && r < len; }

LZ4HIP_DEVICE int header_len(uint32_t flags, uint32_t original, uint32_t clen)
{
    return varint_len(flags) + varint_len(original) + ((flags & kChunkCompressed) ? varint_len(clen) : 0);
}

// byte j of varint(v) (WriteVarInt, src/LZ4/LZ4Stream.cs:162-178)
LZ4HIP_DEVICE uint8_t varint_byte(uint32_t v, int j, int n) { return (uint8_t)(((v >> (7 * j)) & 0x7F) | (j + 1 < n ? 0x80 : 0)); }

// byte j of varint(flags) varint(original) [varint(clen)]
LZ4HIP_DEVICE uint8_t header_byte(uint32_t flags, uint32_t original, uint32_t clen, int j)
{
    const int n0 = varint_len(flags);
    if (j < n0) return varint_byte(flags, j, n0);
    j -= n0;
    const int n1 = varint_len(original);
    if (j < n1) return varint_byte(original, j, n1);
    j -= n1;
    return varint_byte(clen, j, varint_len(clen));
}

__global__ void __launch_bounds__(kStreamThreads) stream_lens_kernel(int32_t* lens, int64_t n, int64_t src_len, int32_t block)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < n; k += (int64_t)gridDim.x * kStreamThreads) {
        const int64_t left = src_len - k * block;
        lens[k] = left < block ? (int32_t)left : block;
    }
}

__global__ void __launch_bounds__(kStreamThreads) stream_sizes_kernel(StreamEncodeArgs a)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.n; k += (int64_t)gridDim.x * kStreamThreads) {
        const int32_t len = chunk_len(a, k), r = a.result[k];
        const bool c = chunk_compressed(r, len);
        const uint32_t flags = (c ? kChunkCompressed : 0u) | a.hc_flag;
        a.offs[k] = header_len(flags, (uint32_t)len, (uint32_t)r) + (int64_t)(c ? r : len);
    }
}

// ---- exclusive scan of int64 values in place (reduce, scan of the tile sums, rescan of the tiles) --------------------------
// Exclusive scan over the workgroup of one value per thread (Hillis-Steele in LDS); returns the workgroup's total too.
LZ4HIP_DEVICE int64_t block_exclusive_scan(int64_t v, int64_t* lds, int64_t& total)
{
    const int t = (int)threadIdx.x;
    lds[t] = v;
    wv::block_sync();
    for (int d = 1; d < kStreamThreads; d *= 2) {
        const int64_t add = t >= d ? lds[t - d] : 0;
        wv::block_sync();
        lds[t] += add;
        wv::block_sync();
    }
    total = lds[kStreamThreads - 1];
    const int64_t incl = lds[t];
    wv::block_sync();                                                  // (lds is reused by the caller's next round)
    return incl - v;
}

__global__ void __launch_bounds__(kStreamThreads) stream_scan_reduce_kernel(const int64_t* x, int64_t n, int64_t* partial)
{
    LZ4HIP_STATIC_LDS(lds_raw, kStreamThreads * 8);
    int64_t* lds = (int64_t*)lds_raw;
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    int64_t s = 0;
    for (int j = 0; j < kScanItems; j++) {
        const int64_t i = base + (int64_t)j * kStreamThreads + threadIdx.x;
        if (i < n) s += x[i];
    }
    int64_t total;
    block_exclusive_scan(s, lds, total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: the tile sums, scanned in place; the grand total goes to *total
__global__ void __launch_bounds__(kStreamThreads) stream_scan_partials_kernel(int64_t* partial, int64_t tiles, int64_t* total)
{
    LZ4HIP_STATIC_LDS(lds_raw, kStreamThreads * 8);
    int64_t* lds = (int64_t*)lds_raw;
    int64_t carry = 0;
    for (int64_t b = 0; b < tiles; b += kStreamThreads) {
        const int64_t i = b + threadIdx.x;
        const int64_t v = i < tiles ? partial[i] : 0;
        int64_t round_total;
        const int64_t ex = block_exclusive_scan(v, lds, round_total);
        if (i < tiles) partial[i] = carry + ex;
        carry += round_total;
    }
    if (threadIdx.x == 0) *total = carry;
}

// each thread owns kScanItems consecutive elements of the tile
__global__ void __launch_bounds__(kStreamThreads) stream_scan_apply_kernel(int64_t* x, int64_t n, const int64_t* partial)
{
    LZ4HIP_STATIC_LDS(lds_raw, kStreamThreads * 8);
    int64_t* lds = (int64_t*)lds_raw;
    const int64_t first = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int64_t v[kScanItems];
    int64_t s = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        v[j] = first + j < n ? x[first + j] : 0;
        s += v[j];
    }
    int64_t total;
    int64_t run = partial[blockIdx.x] + block_exclusive_scan(s, lds, total);
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        if (first + j < n) x[first + j] = run;
        run += v[j];
    }
}

// ---- the copy routine shared by the encode pack and the decode raw copy ------------------------------------------------------
// The output is cut into aligned 16-byte pieces.  A Layout describes a sorted list of segments: segment k starts at start(k) in the
// output, may begin with header bytes (head_byte), and owns its payload bytes [pbegin, pend), read from `payload`; bytes from pend up
// to the next segment's start belong to nobody and are not written.  A workgroup owns a contiguous span of kCopySpan output bytes
// (each pass of its threads covers 4 KiB, coalesced); a thread keeps a cursor -- its current segment and the next one's start -- and
// searches (gallop, then bisection over the starts) only when a piece has passed that start, so a span inside one chunk costs no
// search at all and a stream of tiny chunks one short search per piece.  A piece inside one payload is ONE 16-byte load at the
// payload's alignment (gfx950 global loads take any alignment; a dwordx4 at an odd address splits into more requests in the memory
// pipeline, not into more instructions) and one 16-byte store; pieces that straddle a header or a segment boundary go by bytes.
constexpr int kCopyPiecesPerThread = 16;
constexpr int64_t kCopySpan = (int64_t)kStreamThreads * 16 * kCopyPiecesPerThread;   // 64 KiB per workgroup and pass

struct CopySeg {
    int64_t start, pbegin, pend;
    const uint8_t* payload;
    uint32_t flags, original, clen;
};

template <class Layout>
struct CopyCursor {
    int64_t k, next;                  // current segment (-1: before the first), start of segment k + 1 (INT64_MAX: none)
    CopySeg s;
    LZ4HIP_DEVICE explicit CopyCursor(const Layout& L) : k(-1), next(L.count() > 0 ? L.start(0) : INT64_MAX), s() {}
    // move to the last segment whose start is <= x; x never decreases
    LZ4HIP_DEVICE void seek(const Layout& L, int64_t x)
    {
        if (x < next) return;
        const int64_t n = L.count();
        int64_t lo = k, hi, step = 1;                                 // start(lo) <= x (or lo == -1)
        for (;;) {
            const int64_t p = lo + step;
            if (p >= n) { hi = n - 1; break; }
            if (L.start(p) <= x) { lo = p; step *= 2; } else { hi = p - 1; break; }
        }
        while (lo < hi) {
            const int64_t mid = hi - (hi - lo) / 2;
            if (L.start(mid) <= x) lo = mid; else hi = mid - 1;
        }
        k = lo;
        s = L.seg(k);
        next = k + 1 < n ? L.start(k + 1) : INT64_MAX;
    }
};

template <class Layout>
LZ4HIP_DEVICE void copy_piece(const Layout& L, CopyCursor<Layout>& c, uint8_t* dst, int64_t o, int64_t end)
{
    c.seek(L, o);
    if ((c.k < 0 || o >= c.s.pend) && o + 16 <= c.next) return;       // the whole piece lies between two segments: nothing to write
    if (c.k >= 0 && o >= c.s.pbegin && o + 16 <= c.s.pend && o + 16 <= end) {
        uint32_t w0, w1, w2, w3;
        wv::load_global16((uint64_t)(c.s.payload + (o - c.s.pbegin)), w0, w1, w2, w3);
        wv::store_global16((uint64_t)(dst + o), w0, w1, w2, w3);
        return;
    }
    for (int j = 0; j < 16; j++) {
        const int64_t x = o + j;
        if (x >= end) break;
        c.seek(L, x);
        if (c.k < 0 || x >= c.s.pend) continue;
        dst[x] = x < c.s.pbegin ? L.head_byte(c.s, x) : c.s.payload[x - c.s.pbegin];
    }
}

// output bytes [0, end): workgroup g takes spans g, g + grid, ...
template <class Layout>
LZ4HIP_DEVICE void copy_spans(const Layout& L, uint8_t* dst, int64_t end)
{
    CopyCursor<Layout> c(L);
    for (int64_t base = (int64_t)blockIdx.x * kCopySpan; base < end; base += (int64_t)gridDim.x * kCopySpan)
        for (int j = 0; j < kCopyPiecesPerThread; j++) {
            const int64_t o = base + ((int64_t)j * kStreamThreads + threadIdx.x) * 16;
            if (o >= end) break;
            copy_piece(L, c, dst, o, end);
        }
}

struct EncodeLayout {
    StreamEncodeArgs a;
    LZ4HIP_DEVICE int64_t count() const { return a.n; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.offs[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        const int32_t len = chunk_len(a, k), r = a.result[k];
        const bool c = chunk_compressed(r, len);
        s.flags = (c ? kChunkCompressed : 0u) | a.hc_flag;
        s.original = (uint32_t)len;
        s.clen = (uint32_t)r;
        s.start = a.offs[k];
        s.pbegin = s.start + header_len(s.flags, s.original, s.clen);
        s.pend = s.pbegin + (c ? r : len);
        s.payload = (c ? a.comp : a.src) + k * a.block;
        return s;
    }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg& s, int64_t x) const { return header_byte(s.flags, s.original, s.clen, (int)(x - s.start)); }
};

__global__ void __launch_bounds__(kStreamThreads) stream_pack_kernel(EncodeLayout L, uint8_t* dst, const int64_t* total)
{
    copy_spans(L, dst, *total);
}

// ---- decode ------------------------------------------------------------------------------------------------------------
// The index: two tables in caller scratch, max_chunks entries each.  The compressed table is laid out as the arrays of a
// lz4hip_batch_t (src_off / src_len / dst_off / dst_cap / result) plus the header offset of each chunk (error reports).
struct StreamTables {
    int64_t max_chunks;
    int64_t* c_src_off; int64_t* c_dst_off; int64_t* c_hdr_off;
    int32_t* c_src_len; int32_t* c_dst_cap; int32_t* c_result;
    int64_t* r_dst_off; int64_t* r_src_off; int32_t* r_len;
    unsigned long long* min_bad;                                       // header offset of the first corrupt block (decode)
};

// One step of the header walk, exactly as stream.parse_chunks / TryReadVarInt do (src/LZ4/LZ4Stream.cs:180-218, 274-312): ONE
// wavefront-wide load of the <= 30 header bytes at pos, the three varints' ends from a ballot of the continuation bits (a varint
// ends at a clear bit or after 10 bytes: count >= 64), the low 32 bits of their values (all the reference keeps of the lengths
// and of the flags: it casts them to int) from one prefix sum of the lanes' 7-bit groups, and every
// check in the order AcquireNextChunk applies them.  Called by all 64 lanes of a wavefront with the same arguments; the result is
// the same in every lane.  err != kStreamOk: the other fields are not meaningful.
struct ChunkHeader {
    int err;
    bool compressed;
    int32_t original, clen;      // clen = original for a raw chunk: the payload's length either way
    int64_t payload;             // offset of the payload; the next header is at payload + clen
};

LZ4HIP_DEVICE ChunkHeader stream_read_header(const uint8_t* src, int64_t src_len, int64_t pos, int lane)
{
    ChunkHeader h;
    h.err = kStreamEndOfStream; h.compressed = false; h.original = h.clen = 0; h.payload = pos;
    const int avail = src_len - pos < 30 ? (int)(src_len - pos) : 30;
    const uint32_t b = lane < avail ? src[pos + lane] : 0u;
    const uint64_t stop = wv::ballot(lane < avail && (b & 0x80u) == 0);
    // a varint starting at lane s ends at the first stop at or after s, or at s + 9; it is complete iff that lane exists
    auto vend = [&](int s) -> int {
        const uint64_t m = s < 64 ? stop & (~0ull << s) : 0ull;
        const int e = m ? __builtin_ctzll(m) : 64;
        return e < s + 9 ? e : s + 9;
    };
    const int e1 = vend(0), e2 = vend(e1 + 1), e3 = vend(e2 + 1);
    // the low 32 bits of each varint: lane i of a varint starting at s contributes (b & 0x7F) << 7 (i - s); the groups do not
    // overlap, so a prefix sum adds them without carries and varint [s, e] = sum[e] - sum[s - 1]
    const int s_mine = lane <= e1 ? 0 : (lane <= e2 ? e1 + 1 : e2 + 1);
    const int sh = 7 * (lane - s_mine);
    const uint32_t contrib = lane < avail && lane <= e3 && sh < 32 ? (b & 0x7Fu) << sh : 0u;
    const uint32_t sum = wv::scan_add(contrib);
    auto value = [&](int s, int e) -> uint32_t { return wv::readlane(sum, e) - (s > 0 ? wv::readlane(sum, s - 1) : 0u); };
    if (e1 >= avail || e2 >= avail) return h;                                  // inside a varint / missing chunk length
    const uint32_t flags = value(0, e1);
    h.compressed = (flags & kChunkCompressed) != 0;
    if (h.compressed && e3 >= avail) return h;                                 // missing compressed length
    h.original = (int32_t)value(e1 + 1, e2);
    h.clen = h.compressed ? (int32_t)value(e2 + 1, e3) : h.original;
    if (h.clen > h.original || h.clen < 0) return h;                           // corrupted chunk header
    h.payload = pos + (h.compressed ? e3 : e2) + 1;
    if (h.payload + h.clen > src_len) return h;                                // truncated payload
    // multiple passes: (int)flags >> 2 != 0 -- the reference casts the varint to an int-based enum, so only bits 2..31 of it count
    h.err = h.compressed && (flags >> 2) != 0 ? kStreamPasses : kStreamOk;
    return h;
}

// One wavefront walks the headers in stream order, one dependent global round trip per chunk: a header, then a jump past its
// payload.  Empty chunks (original == 0) are skipped like AcquireNextChunk skips them.
__global__ void __launch_bounds__(64) stream_index_kernel(const uint8_t* src, int64_t src_len, StreamTables t, StreamInfo* info)
{
    const int lane = wv::lane();
    int64_t pos = 0, out = 0, chunks = 0, ncomp = 0, nraw = 0, err_off = -1;
    int err = kStreamOk;
    while (pos < src_len) {
        const ChunkHeader h = stream_read_header(src, src_len, pos, lane);
        if (h.err != kStreamOk) { err = h.err; break; }
        if (h.original != 0) {
            if (chunks < t.max_chunks) {                                        // (ncomp + nraw == chunks: both lists fit)
                if (lane == 0) {
                    if (h.compressed) {
                        t.c_src_off[ncomp] = h.payload; t.c_dst_off[ncomp] = out; t.c_hdr_off[ncomp] = pos;
                        t.c_src_len[ncomp] = h.clen; t.c_dst_cap[ncomp] = h.original;
                    } else {
                        t.r_dst_off[nraw] = out; t.r_src_off[nraw] = h.payload; t.r_len[nraw] = h.original;
                    }
                }
            } else if (chunks == t.max_chunks) {
                err_off = pos;                                                  // (TABLE_FULL: the first chunk that did not fit)
            }
            if (h.compressed) ncomp++; else nraw++;
            chunks++;
            out += h.original;
        }
        pos = h.payload + h.clen;
    }
    // (a full table wins over a later header error: the caller grows the table to `chunks` and walks again)
    if (chunks > t.max_chunks) err = kStreamTableFull;
    else if (err != kStreamOk) err_off = pos;
    if (lane == 0) {
        StreamInfo r;
        r.chunks = chunks; r.compressed_chunks = ncomp; r.decoded_bytes = out; r.error_offset = err_off; r.error = err; r.reserved = 0;
        *info = r;
    }
}

// The same walk, kept: the directory of a stream that is decoded more than once, or in parts.  hdr_off[k] is the header offset of
// non-empty chunk k and out_off[k] its decoded offset; the closing entry (hdr_off[chunks], out_off[chunks]) is where the walk ended
// (src_len, or the header error's offset) and the decoded size.  Both arrays have max_chunks + 1 entries.  src[hdr_off[k],
// hdr_off[k + 1]) is chunk k and the empty chunks behind it: a one-chunk stream, an item of the batch decoder's span form
// (lz4hip_streams.hpp).  The stop rules, the error codes and *info are stream_index_kernel's; on TABLE_FULL the entries [0, max_chunks)
// are valid and no closing entry is written.
__global__ void __launch_bounds__(64) stream_directory_kernel(const uint8_t* src, int64_t src_len, int64_t max_chunks, int64_t* hdr_off,
                                                              int64_t* out_off, StreamInfo* info)
{
    const int lane = wv::lane();
    int64_t pos = 0, out = 0, chunks = 0, ncomp = 0, err_off = -1;
    int err = kStreamOk;
    while (pos < src_len) {
        const ChunkHeader h = stream_read_header(src, src_len, pos, lane);
        if (h.err != kStreamOk) { err = h.err; break; }
        if (h.original != 0) {
            if (chunks < max_chunks) {
                if (lane == 0) { hdr_off[chunks] = pos; out_off[chunks] = out; }
            } else if (chunks == max_chunks) {
                err_off = pos;                                                  // (TABLE_FULL: the first chunk that did not fit)
            }
            if (h.compressed) ncomp++;
            chunks++;
            out += h.original;
        }
        pos = h.payload + h.clen;
    }
    if (chunks > max_chunks) err = kStreamTableFull;
    else if (err != kStreamOk) err_off = pos;
    if (lane == 0) {
        if (chunks <= max_chunks) { hdr_off[chunks] = pos; out_off[chunks] = out; }
        StreamInfo r;
        r.chunks = chunks; r.compressed_chunks = ncomp; r.decoded_bytes = out; r.error_offset = err_off; r.error = err; r.reserved = 0;
        *info = r;
    }
}

struct RawLayout {
    const uint8_t* src;
    StreamTables t;
    int64_t n;
    LZ4HIP_DEVICE int64_t count() const { return n; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return t.r_dst_off[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        s.start = s.pbegin = t.r_dst_off[k];
        s.pend = s.start + t.r_len[k];
        s.payload = src + t.r_src_off[k];
        s.flags = s.original = s.clen = 0;
        return s;
    }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg&, int64_t) const { return 0; }   // (raw segments have no header bytes)
};

__global__ void __launch_bounds__(kStreamThreads) stream_raw_copy_kernel(RawLayout L, uint8_t* dst, int64_t end)
{
    copy_spans(L, dst, end);
}

// the decode's info starts as what the index reported; no corrupt block yet
__global__ void __launch_bounds__(64) stream_info_init_kernel(StreamInfo from_index, StreamInfo* info, unsigned long long* min_bad)
{
    if (threadIdx.x == 0) { *info = from_index; *min_bad = ~0ull; }
}

// Decode64's check (src/LZ4pn/LZ4Codec.Unsafe.cs:373-378): a chunk whose consumed count is not its payload length is corrupt;
// the one FIRST in stream order is what a sequential LZ4Stream.Read raises
__global__ void __launch_bounds__(kStreamThreads) stream_check_kernel(StreamTables t, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kStreamThreads)
        if (t.c_result[i] != t.c_src_len[i]) atomicMin(t.min_bad, (unsigned long long)t.c_hdr_off[i]);
}

// every chunk in the tables lies before the index's header error (if any), so any corrupt block comes first
__global__ void __launch_bounds__(64) stream_info_finish_kernel(StreamInfo* info, const unsigned long long* min_bad)
{
    if (threadIdx.x == 0 && *min_bad != ~0ull) { info->error = kStreamCorruptBlock; info->error_offset = (int64_t)*min_bad; }
}

// ---- decode in one call, into a buffer of any capacity ------------------------------------------------------------------------
// Nothing of the index is read on the host: the decoder runs over ALL max_chunks rows of the compressed table, and what the two-call
// decode took from the host's copy of the info -- the counts, the end of the output -- these kernels read on the device.  The output
// offsets are monotone, so the chunks that fit dst_cap are a prefix of the stream; the decoder is handed a copy of the length and
// capacity columns in which every other row (past the count, clipped, or all of them on TABLE_FULL) is an empty block of capacity 0.
// The table's own columns stay: the check compares against them.
struct StreamClip {
    StreamTables t;
    int32_t* s_src_len; int32_t* s_dst_cap;                            // the decoder's columns, max_chunks rows
    int64_t dst_cap;
    unsigned long long* written;                                       // end of the last chunk that fits, 0 before the launch
};

// `counts`: [non-empty chunks, compressed chunks] as the index left them (a StreamInfo's first fields); `full`: TABLE_FULL
LZ4HIP_DEVICE void stream_clip_counts(const int64_t* counts, bool full, int64_t max_chunks, int64_t& ncomp, int64_t& nraw)
{
    ncomp = full ? 0 : counts[1];
    nraw = full ? 0 : counts[0] - counts[1];
    if (ncomp > max_chunks) ncomp = max_chunks;                        // (never, for an index's counts: no row outside the table is read)
    if (nraw > max_chunks) nraw = max_chunks;
    if (ncomp < 0) ncomp = 0;
    if (nraw < 0) nraw = 0;
}

__global__ void __launch_bounds__(kStreamThreads) stream_clip_kernel(StreamClip c, const StreamInfo* info)
{
    int64_t ncomp, nraw;
    stream_clip_counts(&info->chunks, info->error == kStreamTableFull, c.t.max_chunks, ncomp, nraw);
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < c.t.max_chunks; i += (int64_t)gridDim.x * kStreamThreads) {
        // the last row of either table that fits speaks for its table (the offsets do not decrease): two atomics a call at most
        int32_t len = 0, cap = 0;
        if (i < ncomp) {
            const int64_t end = c.t.c_dst_off[i] + c.t.c_dst_cap[i];
            if (end <= c.dst_cap) {
                len = c.t.c_src_len[i]; cap = c.t.c_dst_cap[i];
                if (i + 1 == ncomp || c.t.c_dst_off[i + 1] + c.t.c_dst_cap[i + 1] > c.dst_cap) atomicMax(c.written, (unsigned long long)end);
            }
        }
        c.s_src_len[i] = len;
        c.s_dst_cap[i] = cap;
        if (i < nraw) {
            const int64_t end = c.t.r_dst_off[i] + c.t.r_len[i];
            if (end <= c.dst_cap && (i + 1 == nraw || c.t.r_dst_off[i + 1] + c.t.r_len[i + 1] > c.dst_cap)) atomicMax(c.written, (unsigned long long)end);
        }
    }
}

// the raw chunks that start before *end: a chunk that does not fit starts at *end or later, so the copy clips at a chunk boundary
__global__ void __launch_bounds__(kStreamThreads) stream_raw_copy_into_kernel(RawLayout L, uint8_t* dst, const int64_t* counts, const int64_t* end)
{
    const int64_t to = *end;
    int64_t ncomp;
    stream_clip_counts(counts, to <= 0, L.t.max_chunks, ncomp, L.n);
    if (L.n > 0) copy_spans(L, dst, to);
}

// stream_check_kernel over the rows the decoder was given (a chunk in the table has original > 0: capacity 0 means clipped)
__global__ void __launch_bounds__(kStreamThreads) stream_check_into_kernel(StreamTables t, const int32_t* s_dst_cap, const int64_t* counts)
{
    int64_t ncomp, nraw;
    stream_clip_counts(counts, false, t.max_chunks, ncomp, nraw);
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < ncomp; i += (int64_t)gridDim.x * kStreamThreads)
        if (s_dst_cap[i] != 0 && t.c_result[i] != t.c_src_len[i]) atomicMin(t.min_bad, (unsigned long long)t.c_hdr_off[i]);
}

}  // namespace lz4hip
