// lz4hip_wrap.hpp -- device-side framing of lz4net's self-describing messages, LZ4Codec.Wrap / WrapHC / Unwrap
// (src/LZ4/LZ4Codec.cs:471-599), for batches of many independent messages:
//
//     int32 originalLength (little-endian)  int32 payloadLength  payload
//
// A batch is one byte buffer plus int64 offsets off[n + 1]: message i is src[off[i], off[i + 1]).  Wrap writes that layout and Unwrap
// reads it.  The block codecs are the batch kernels of the library; this header holds only what goes around them, and reuses the
// int64 scan and the position-driven copy routine of lz4hip_stream.hpp:
//
//   wrap:   wrap_lens_kernel (message lengths, bad offsets) -> [launch_encode into scratch at the source's own offsets,
//           outputLength = inputLength] -> wrap_sizes_kernel (8 + payload per message) -> stream_scan_* (dst_off, total in dst_off[n])
//           -> wrap_pack_kernel (copy_spans over WrapLayout: 8 header bytes, then the compressed or the raw payload)
//   index:  unwrap_index_kernel (one thread per message reads its header and classifies it) -> stream_scan_* of the output sizes
//           (dst_off, decoded_bytes) -> stream_scan_* of the "compressed" flags -> unwrap_compact_kernel (the compressed messages as
//           the arrays of a lz4hip_batch_t) -> unwrap_info_kernel
//   decode: [launch_decode, known size, on the compacted table] -> wrap_raw_copy_kernel (copy_spans over UnwrapRawLayout) ->
//           unwrap_check_kernel (consumed != payloadLength: corrupt block) -> unwrap_info_kernel
//   spans:  chosen messages of an arena, [begin[j], end[j]) in any order: the index alone reads a message's end, so the span form is
//           the same sequence behind unwrap_index_spans_kernel; spans_select_kernel makes the spans from offsets and indices
//
// Every kernel here is launch-only work on the caller's stream over caller scratch.
#pragma once
#include "lz4hip_stream.hpp"

namespace lz4hip {

// per-message statuses (LZ4HIP_WRAP_* of include/lz4hip.h); bad offsets report LZ4HIP_E_ARGUMENT (the API checks that the values agree)
constexpr int32_t kWrapOk = 0, kWrapSizeInvalid = 1, kWrapCorruptHeader = 2, kWrapCorruptBlock = 3;
constexpr int32_t kWrapBadOffsets = -2000000002;
constexpr int64_t kWrapHeader = 8;

// Device twin of lz4hip_unwrap_info_t (include/lz4hip.h; the API checks that the layouts agree).
struct UnwrapInfo {
    int64_t messages, compressed, decoded_bytes, first_error;
    int32_t error, reserved;
};

// the message src[a, b): false for bounds that decrease, fall outside [0, src_len] or give a length above INT32_MAX
LZ4HIP_DEVICE bool wrap_span(int64_t a, int64_t b, int64_t src_len, int64_t& at, int32_t& len)
{
    at = 0;
    len = 0;
    if (a < 0 || b < a || b > src_len || b - a > 0x7FFFFFFF) return false;
    at = a;
    len = (int32_t)(b - a);
    return true;
}

// message i of the batch: the span [off[i], off[i + 1])
LZ4HIP_DEVICE bool wrap_message(const int64_t* off, int64_t i, int64_t src_len, int64_t& at, int32_t& len)
{
    return wrap_span(off[i], off[i + 1], src_len, at, len);
}

LZ4HIP_DEVICE int32_t load_le32(const uint8_t* p)
{
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// ---- wrap -------------------------------------------------------------------------------------------------------------------
struct WrapArgs {
    const uint8_t* src;
    const uint8_t* comp;         // launch_encode's output: message i at off[i], at most its length
    const int64_t* off;          // the caller's offsets, n + 1
    int64_t src_len, n;
    const int32_t* enc;          // launch_encode's per-message results
    int64_t* dst_off;            // framed size per message, then (scanned in place) its output offset; dst_off[n] = the total
};

// Wrap (src/LZ4/LZ4Codec.cs:527-533): the encoder's output is used iff 0 < r < inputLength
LZ4HIP_DEVICE bool wrap_compressed(int32_t r, int32_t len) { return r > 0 && r < len; }

// the encoder's view of the batch: bad messages are empty blocks at offset 0 (they read and write nothing)
__global__ void __launch_bounds__(kStreamThreads) wrap_lens_kernel(const int64_t* off, int64_t n, int64_t src_len, int64_t* at, int32_t* lens)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kStreamThreads) {
        int64_t a;
        int32_t len;
        wrap_message(off, i, src_len, a, len);
        at[i] = a;
        lens[i] = len;
    }
}

// result[i]: the payload size of a compressed message, 0 for a raw one, kWrapBadOffsets (and no output bytes) for bad offsets
__global__ void __launch_bounds__(kStreamThreads) wrap_sizes_kernel(WrapArgs a, int32_t* result)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        int64_t at;
        int32_t len;
        if (!wrap_message(a.off, i, a.src_len, at, len)) {
            a.dst_off[i] = 0;
            if (result) result[i] = kWrapBadOffsets;
            continue;
        }
        const int32_t r = a.enc[i];
        const bool c = wrap_compressed(r, len);
        a.dst_off[i] = kWrapHeader + (c ? r : len);
        if (result) result[i] = c ? r : 0;
    }
}

struct WrapLayout {
    WrapArgs a;
    LZ4HIP_DEVICE int64_t count() const { return a.n; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.dst_off[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        int64_t at;
        int32_t len;
        s.start = a.dst_off[k];
        s.flags = 0;
        if (!wrap_message(a.off, k, a.src_len, at, len)) {          // no bytes at all
            s.pbegin = s.pend = s.start;
            s.payload = a.src;
            s.original = s.clen = 0;
            return s;
        }
        const int32_t r = a.enc[k];
        const bool c = wrap_compressed(r, len);
        s.original = (uint32_t)len;                                  // an empty message: 8 zero bytes
        s.clen = (uint32_t)(c ? r : len);
        s.pbegin = s.start + kWrapHeader;
        s.pend = s.pbegin + s.clen;
        s.payload = (c ? a.comp : a.src) + at;
        return s;
    }
    // Poke4(original), Poke4(payload length)
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg& s, int64_t x) const
    {
        const int j = (int)(x - s.start);
        return (uint8_t)((j < 4 ? s.original : s.clen) >> (8 * (j & 3)));
    }
};

// output bytes [0, min(dst_off[n], cap)): the total exceeds the bound only for offsets that decrease, and nothing past cap is written
__global__ void __launch_bounds__(kStreamThreads) wrap_pack_kernel(WrapLayout L, uint8_t* dst, int64_t cap)
{
    const int64_t total = L.a.dst_off[L.a.n];
    copy_spans(L, dst, total < cap ? total : cap);
}

// ---- unwrap ----------------------------------------------------------------------------------------------------------------
// Scratch of the index and the decode (same scratch for both calls).  The compressed messages form the arrays of a lz4hip_batch_t
// (c_src_off / c_src_len / c_dst_off / c_dst_cap / c_result) plus each one's message index.  raw_len[i] is the payload length of a
// message stored raw, -1 for a compressed one, 0 for a failed one.
struct UnwrapTables {
    int64_t n;
    unsigned long long* min_bad;        // lowest failing message index (~0: none)
    int64_t* ncomp;                     // compressed messages (the scan's total)
    int64_t* cidx;                      // 1 per compressed message, then (scanned in place) its row of the table
    int64_t* partial;                   // tile sums of the scans
    int64_t* c_src_off; int64_t* c_dst_off; int64_t* c_msg;
    int32_t* c_src_len; int32_t* c_dst_cap; int32_t* c_result;
    int32_t* raw_len;
};

struct UnwrapArgs {
    const uint8_t* src;
    const int64_t* off;
    int64_t src_len, n;
    int64_t* dst_off;
    int32_t* status;
};

// Unwrap's checks in its order (src/LZ4/LZ4Codec.cs:574-599), with signed fields: < 8 bytes, payloadLength past the end (or negative),
// payloadLength >= originalLength: the payload as it is, else a known-size decode of originalLength bytes.
// Message i is src[a.off[i], end[i]): the index is the only step that reads a message's end, everything after it reads a.off[i] as
// the message's begin, a.dst_off and the tables.
LZ4HIP_DEVICE void unwrap_index_items(const UnwrapArgs& a, const UnwrapTables& t, const int64_t* end)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        int64_t at;
        int32_t len;
        int32_t st = kWrapOk, raw = 0;
        int64_t size = 0, comp = 0;
        if (!wrap_span(a.off[i], end[i], a.src_len, at, len)) {
            st = kWrapBadOffsets;
        } else if (len < kWrapHeader) {
            st = kWrapSizeInvalid;
        } else {
            const int32_t original = load_le32(a.src + at), payload = load_le32(a.src + at + 4);
            if (payload < 0 || payload > len - kWrapHeader) st = kWrapCorruptHeader;
            else if (payload >= original) { raw = payload; size = payload; }
            else { raw = -1; size = original; comp = 1; }
        }
        a.status[i] = st;
        a.dst_off[i] = size;
        t.cidx[i] = comp;
        t.raw_len[i] = raw;
        if (st != kWrapOk) atomicMin(t.min_bad, (unsigned long long)i);
    }
}

// consecutive messages: a.off has n + 1 entries and message i ends where message i + 1 begins
__global__ void __launch_bounds__(kStreamThreads) unwrap_index_kernel(UnwrapArgs a, UnwrapTables t)
{
    unwrap_index_items(a, t, a.off + 1);
}

// chosen messages: a.off holds the n begins and `end` the n ends, in any order, with repeats, overlaps and holes
__global__ void __launch_bounds__(kStreamThreads) unwrap_index_spans_kernel(UnwrapArgs a, UnwrapTables t, const int64_t* end)
{
    unwrap_index_items(a, t, end);
}

// after both scans: the compressed messages, in message order, into the table
__global__ void __launch_bounds__(kStreamThreads) unwrap_compact_kernel(UnwrapArgs a, UnwrapTables t)
{
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        if (t.raw_len[i] >= 0) continue;
        const int64_t j = t.cidx[i], at = a.off[i];
        t.c_src_off[j] = at + kWrapHeader;
        t.c_src_len[j] = load_le32(a.src + at + 4);
        t.c_dst_off[j] = a.dst_off[i];
        t.c_dst_cap[j] = (int32_t)(a.dst_off[i + 1] - a.dst_off[i]);
        t.c_msg[j] = i;
    }
}

// the payloads of the messages stored raw; compressed and failed messages are gaps of the layout
struct UnwrapRawLayout {
    UnwrapArgs a;
    UnwrapTables t;
    LZ4HIP_DEVICE int64_t count() const { return a.n; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.dst_off[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        const int32_t raw = t.raw_len[k];
        s.start = s.pbegin = a.dst_off[k];
        s.pend = s.start + (raw > 0 ? raw : 0);
        s.payload = raw > 0 ? a.src + a.off[k] + kWrapHeader : a.src;
        s.flags = s.original = s.clen = 0;
        return s;
    }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg&, int64_t) const { return 0; }   // (no header bytes in the output)
};

__global__ void __launch_bounds__(kStreamThreads) wrap_raw_copy_kernel(UnwrapRawLayout L, uint8_t* dst, int64_t end)
{
    copy_spans(L, dst, end);
}

// Decode64's check (src/LZ4pn/LZ4Codec.Unsafe.cs:373-378): a message whose consumed count is not its payload length is corrupt
__global__ void __launch_bounds__(kStreamThreads) unwrap_check_kernel(UnwrapTables t, int64_t ncomp, int32_t* status)
{
    for (int64_t j = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; j < ncomp; j += (int64_t)gridDim.x * kStreamThreads)
        if (t.c_result[j] != t.c_src_len[j]) {
            status[t.c_msg[j]] = kWrapCorruptBlock;
            atomicMin(t.min_bad, (unsigned long long)t.c_msg[j]);
        }
}

// ---- unwrap in one call, into a buffer of any capacity (see lz4hip_stream.hpp) ---------------------------------------------------
// The messages that fit dst_cap are a prefix of the batch: message i is written iff dst_off[i + 1] <= dst_cap.  The decoder runs over
// all n rows of the table with a copy of its length and capacity columns in which the rows past the count and the clipped ones are
// empty blocks of capacity 0 (a compressed message decodes to at least one byte: capacity 0 means "not given to the decoder").
struct UnwrapClip {
    UnwrapTables t;
    int32_t* s_src_len; int32_t* s_dst_cap;                            // the decoder's columns, n rows
    int64_t dst_cap;
    int64_t* written_messages; int64_t* written_end;                   // the prefix's length and dst_off[that]; both 0 before the launch
};

__global__ void __launch_bounds__(kStreamThreads) unwrap_clip_kernel(UnwrapArgs a, UnwrapClip c)
{
    int64_t ncomp = *c.t.ncomp;
    if (ncomp > a.n) ncomp = a.n;
    for (int64_t i = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kStreamThreads) {
        int32_t len = 0, cap = 0;
        if (i < ncomp && a.dst_off[c.t.c_msg[i] + 1] <= c.dst_cap) { len = c.t.c_src_len[i]; cap = c.t.c_dst_cap[i]; }
        c.s_src_len[i] = len;
        c.s_dst_cap[i] = cap;
        // the last message that fits: the offsets do not decrease, so there is one such message at most
        if (a.dst_off[i + 1] <= c.dst_cap && (i + 1 == a.n || a.dst_off[i + 2] > c.dst_cap)) {
            *c.written_messages = i + 1;
            *c.written_end = a.dst_off[i + 1];
        }
    }
}

// a message that does not fit starts at *end or later, so the copy clips at a message boundary
__global__ void __launch_bounds__(kStreamThreads) wrap_raw_copy_into_kernel(UnwrapRawLayout L, uint8_t* dst, const int64_t* end)
{
    const int64_t to = *end;
    if (to > 0) copy_spans(L, dst, to);
}

// unwrap_check_kernel over the rows the decoder was given
__global__ void __launch_bounds__(kStreamThreads) unwrap_check_into_kernel(UnwrapTables t, const int32_t* s_dst_cap, int32_t* status)
{
    int64_t ncomp = *t.ncomp;
    if (ncomp > t.n) ncomp = t.n;
    for (int64_t j = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; j < ncomp; j += (int64_t)gridDim.x * kStreamThreads)
        if (s_dst_cap[j] != 0 && t.c_result[j] != t.c_src_len[j]) {
            status[t.c_msg[j]] = kWrapCorruptBlock;
            atomicMin(t.min_bad, (unsigned long long)t.c_msg[j]);
        }
}

// info from the tables: the counts, and the lowest failing message with its status (what a sequential Unwrap loop raises first)
__global__ void __launch_bounds__(64) unwrap_info_kernel(UnwrapArgs a, UnwrapTables t, UnwrapInfo* info)
{
    if (threadIdx.x != 0) return;
    const unsigned long long bad = *t.min_bad;
    UnwrapInfo r;
    r.messages = a.n;
    r.compressed = *t.ncomp;
    r.decoded_bytes = a.dst_off[a.n];
    r.first_error = bad == ~0ull ? -1 : (int64_t)bad;
    r.error = bad == ~0ull ? kWrapOk : a.status[bad];
    r.reserved = 0;
    *info = r;
}

// ---- spans of chosen items ----------------------------------------------------------------------------------------------------
// begin[j] = off[sel[j]], end[j] = off[sel[j] + 1] for the span forms of the one-call decodes (wrapped messages and LZ4Stream buffers
// alike); a sel[j] outside [0, n) gives (-1, -1), which those calls answer with a bad-offsets status for item j alone.
__global__ void __launch_bounds__(kStreamThreads) spans_select_kernel(const int64_t* off, int64_t n, const int64_t* sel, int64_t m,
                                                                      int64_t* begin, int64_t* end)
{
    for (int64_t j = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; j < m; j += (int64_t)gridDim.x * kStreamThreads) {
        const int64_t i = sel[j];
        const bool inside = i >= 0 && i < n;
        begin[j] = inside ? off[i] : -1;
        end[j] = inside ? off[i + 1] : -1;
    }
}

}  // namespace lz4hip
