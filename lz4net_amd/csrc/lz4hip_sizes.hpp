// lz4hip_sizes.hpp -- the decoded size of every block of a batch, without decoding it: what LZ4_uncompress_unknownOutputSize
// (original/lz4.c:916-1044) returns for a block when its output limit never binds -- the bytes produced, or -(error position in the
// source) -- found by walking the block's tokens and writing nothing but that number.
//
// With an unbounded output the reference reduces to this walk (ip: source position, iend = src_len, produced: a 64-bit count):
//
//   src_len == 0                          0                                   (:946 returns -(0))
//   token; ll = token >> 4; ll == 15:     add bytes while ip < iend and the byte just read was 255          (:956-960)
//   ip + ll > iend - 8  (last sequence)   ip + ll != iend ? -ip : produced + ll                              (:965-975)
//   produced += ll; ip += ll; LE16 offset; ip += 2; offset > produced: -ip  (offset 0 is no error)           (:979-980)
//   ml = token & 15; ml == 15:            while ip < iend - 6: s = src[ip++]; ml += s; stop at s != 255      (:983-996)
//   produced += ml + 4
//
// and a count above INT32_MAX, where the reference's int would have wrapped, is LZ4HIP_E_ARGUMENT.
//
// Mapping: ONE LANE PER BLOCK.  The chain token -> length bytes -> next token is serial inside a block and there is nothing to copy,
// so the batch is the only parallelism and a wavefront that owned one block would spend 64 lanes on one scalar chain.  A lane's
// state is a handful of registers; its view of the input is a window of kSizesWindow bytes in LDS, refilled by four 16-byte loads
// (one 64-byte piece of its block per lane: the widest fetch there is when every lane reads another block) and peeked four bytes at
// a time.  The window is laid out transposed -- dword k of lane l at (k * 64 + l) * 4 -- so a lane only ever touches its own LDS bank,
// whichever dword it looks at.  Literals are skipped, never read: a block of incompressible data costs its length bytes (one per 255
// literals, taken four at a time) and two windows.  Workgroups are single wavefronts with 4 KiB of LDS, so a batch spreads over the
// CUs from 64 blocks per CU on and residency is bounded by the wavefront slots alone.
//
// sizes_walk_kernel also leaves what the scan and the info need: max(result, 0) as int64 and the lowest failing index.
#pragma once
#include "lz4hip_common.hpp"

namespace lz4hip {

constexpr int kSizesWindow = 64;                                   // bytes of input a lane sees at a time
constexpr int kSizesThreads = 64;                                  // one wavefront per workgroup
constexpr int kSizesLdsBytes = kSizesThreads * kSizesWindow;
constexpr int32_t kSizesTooLarge = -2000000002;                    // LZ4HIP_E_ARGUMENT as a block's result (the API checks that the values agree)

// Device twin of lz4hip_sizes_info_t (include/lz4hip.h; the API checks that the layouts agree).
struct SizesInfo {
    int64_t blocks, decoded_bytes, first_error;
    int32_t error, reserved;
};

struct SizesArgs {
    const uint8_t* src;
    const int64_t* src_off;      // as in Batch: block i at src + (src_off ? src_off[i] : i * src_stride)
    int64_t src_stride;
    const int32_t* src_len;      // or nullptr: every block has src_len_all bytes
    int32_t src_len_all;
    int64_t n;
    int32_t* result;             // the reference's return value per block (never nullptr: the caller's array or scratch)
    int32_t* dst_cap;            // max(result, 0), or nullptr
    int64_t* offs;               // max(result, 0) as int64, scanned in place afterwards; n + 1 entries
    unsigned long long* min_bad; // lowest index with a negative result (~0: none)
};

// A lane's window over its block: bytes [base, base + kSizesWindow) of src[0, len), in the lane's column of the LDS array.  A block
// of at least kSizesWindow bytes is only ever read in whole windows that end at or before its end (the last one is pulled back),
// a shorter one byte by byte, once: no byte outside the block is touched.
struct SizesWindow {
    uint32_t* col;               // this lane's dword k at col[k * kSizesThreads]
    const uint8_t* src;
    int64_t len, base;

    LZ4HIP_DEVICE void fill(int64_t p)
    {
        if (len >= kSizesWindow) {
            base = p < len - kSizesWindow ? p : len - kSizesWindow;
#pragma unroll
            for (int j = 0; j < kSizesWindow / 16; j++) {
                uint32_t w0, w1, w2, w3;
                wv::load_global16((uint64_t)(src + base + 16 * j), w0, w1, w2, w3);
                col[(4 * j + 0) * kSizesThreads] = w0; col[(4 * j + 1) * kSizesThreads] = w1;
                col[(4 * j + 2) * kSizesThreads] = w2; col[(4 * j + 3) * kSizesThreads] = w3;
            }
        } else {
            base = 0;
            for (int k = 0; 4 * k < len; k++) {
                uint32_t w = 0;
                for (int j = 0; j < 4 && 4 * k + j < len; j++) w |= (uint32_t)src[4 * k + j] << (8 * j);
                col[k * kSizesThreads] = w;
            }
        }
    }
    // makes src[p, p + n) -- what there is of it before the block's end -- part of the window; p never decreases, n <= 8
    LZ4HIP_DEVICE void need(int64_t p, int n)
    {
        if (p + n > base + kSizesWindow && base + kSizesWindow < len) fill(p);
    }
    // the bytes at p .. p + 3 (those before the block's end are meaningful), after need(p, 4)
    LZ4HIP_DEVICE uint32_t peek4(int64_t p) const
    {
        const int idx = (int)(p - base), k = idx >> 2, k1 = k + 1 < kSizesWindow / 4 ? k + 1 : k;
        const uint32_t lo = col[k * kSizesThreads], hi = col[k1 * kSizesThreads];
        return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (idx & 3)));
    }
};

// the walk of one block; every lane has a block of its own (no collective operations: lanes finish when they finish).  `history`: bytes
// of output that exist before the block and that its matches may reach into -- 0 for a block that stands alone; the linked blocks of
// an LZ4 frame (lz4hip_lz4f_linked.hpp) are sized with the format's 65 535, and their decoder checks the real history
LZ4HIP_DEVICE int32_t decoded_size_block(const uint8_t* src, int64_t iend, uint32_t* col, int32_t history = 0)
{
    if (iend == 0) return 0;
    if (iend < 0) return kSizesTooLarge;
    SizesWindow win;
    win.col = col; win.src = src; win.len = iend; win.base = 0;
    win.fill(0);
    int64_t ip = 0, produced = 0;
    for (;;) {
        // ---- token + literal length ----
        win.need(ip, 4);
        const uint32_t t4 = win.peek4(ip);
        const uint32_t token = t4 & 255u;
        ip++;
        int64_t ll = token >> 4;
        if (ll == 15) {
            // whole dwords of 255s first (each of the four bytes passes `ip < iend` and asks for the next), then byte by byte
            while (ip + 4 <= iend) {
                win.need(ip, 4);
                if (win.peek4(ip) != 0xFFFFFFFFu) break;
                ll += 4 * 255; ip += 4;
            }
            uint32_t s = 255;
            while (ip < iend && s == 255u) { win.need(ip, 1); s = win.peek4(ip) & 255u; ip++; ll += s; }
        }
        // ---- last sequence: literals only ----
        if (ip + ll > iend - 8) {
            if (ip + ll != iend) return (int32_t)-ip;
            produced += ll;
            break;
        }
        produced += ll;
        ip += ll;                                                      // the literals themselves are never looked at
        // ---- offset: in the token's dword when at most one literal lies between them ----
        uint32_t o4;
        if (token < 0x20u) o4 = t4 >> (8 * (1 + (int)ll));
        else { win.need(ip, 4); o4 = win.peek4(ip); }
        ip += 2;
        if ((int64_t)(o4 & 0xFFFFu) > produced + history) return (int32_t)-ip;
        // ---- match length ----
        int64_t ml = token & 15u;
        if (ml == 15) {
            while (ip + 4 <= iend - 6) {
                win.need(ip, 4);
                if (win.peek4(ip) != 0xFFFFFFFFu) break;
                ml += 4 * 255; ip += 4;
            }
            while (ip < iend - 6) {
                win.need(ip, 1);
                const uint32_t s = win.peek4(ip) & 255u;
                ip++; ml += s;
                if (s != 255u) break;
            }
        }
        produced += ml + kMinMatch;
    }
    return produced > 0x7FFFFFFF ? kSizesTooLarge : (int32_t)produced;
}

// grid-stride over the blocks: any grid of kSizesThreads-wide workgroups covers the batch
__global__ void __launch_bounds__(kSizesThreads) sizes_walk_kernel(SizesArgs a)
{
    LZ4HIP_STATIC_LDS(lds_raw, kSizesLdsBytes);
    uint32_t* const col = (uint32_t*)lds_raw + threadIdx.x;
    for (int64_t i = (int64_t)blockIdx.x * kSizesThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kSizesThreads) {
        const uint8_t* src = a.src + (a.src_off ? a.src_off[i] : i * a.src_stride);
        const int32_t r = decoded_size_block(src, a.src_len ? a.src_len[i] : a.src_len_all, col);
        const int32_t cap = r < 0 ? 0 : r;
        a.result[i] = r;
        if (a.dst_cap) a.dst_cap[i] = cap;
        a.offs[i] = cap;
        if (r < 0) atomicMin(a.min_bad, (unsigned long long)i);
    }
}

// the same walk for blocks that are decoded against a dictionary (lz4hip_decoded_sizes_dict_*): a match may start up to `history` bytes
// before its block -- the dictionary's length, at most the format's 65 535; no byte of the dictionary is needed
__global__ void __launch_bounds__(kSizesThreads) sizes_walk_dict_kernel(SizesArgs a, int32_t history)
{
    LZ4HIP_STATIC_LDS(lds_raw, kSizesLdsBytes);
    uint32_t* const col = (uint32_t*)lds_raw + threadIdx.x;
    for (int64_t i = (int64_t)blockIdx.x * kSizesThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kSizesThreads) {
        const uint8_t* src = a.src + (a.src_off ? a.src_off[i] : i * a.src_stride);
        const int32_t r = decoded_size_block(src, a.src_len ? a.src_len[i] : a.src_len_all, col, history);
        const int32_t cap = r < 0 ? 0 : r;
        a.result[i] = r;
        if (a.dst_cap) a.dst_cap[i] = cap;
        a.offs[i] = cap;
        if (r < 0) atomicMin(a.min_bad, (unsigned long long)i);
    }
}

// after the scan: offs[n] is the total
__global__ void __launch_bounds__(64) sizes_info_kernel(SizesArgs a, SizesInfo* info)
{
    if (threadIdx.x != 0) return;
    const unsigned long long bad = *a.min_bad;
    SizesInfo r;
    r.blocks = a.n;
    r.decoded_bytes = a.offs[a.n];
    r.first_error = bad == ~0ull ? -1 : (int64_t)bad;
    r.error = bad == ~0ull ? 0 : a.result[bad];
    r.reserved = 0;
    *info = r;
}

// the info of a batch without blocks (no scratch to read it from)
__global__ void sizes_empty_info_kernel(SizesInfo* info)
{
    if (threadIdx.x != 0) return;
    SizesInfo r = {};
    r.first_error = -1;
    *info = r;
}

}  // namespace lz4hip
