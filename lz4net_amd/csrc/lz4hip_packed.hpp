// lz4hip_packed.hpp -- the pack step of a plain block batch: n independent blocks encoded into ONE buffer of exactly the bytes they
// produced, block i at dst[dst_off[i], dst_off[i + 1]), no slot per block.  The block encoders are the batch kernels of the library;
// this header holds only what goes around them, and reuses the int64 scan and the position-driven copy routine of lz4hip_stream.hpp.
//
// The batch runs in ROUNDS of at most K blocks through one ring of K slots, so the scratch does not grow with the batch.  Per round:
//
//   packed_caps_kernel (the round's per-block limits: min(dst_cap[i], slot width); and the round's lengths with every negative one
//   turned into 0: the block encoders do not look at a length's sign) -> [launch_encode on the round's rows into the ring, row k at
//   k * slot, with those lengths] -> packed_sizes_kernel (a block whose length was negative gets LZ4HIP_E_ARGUMENT as its result;
//   max(result, 0) into the round's stretch of dst_off and of packed_len; the lowest failed index) -> stream_scan_* over that
//   stretch (the round's total to the state block) -> packed_rebase_kernel (adds the running base: dst_off holds GLOBAL offsets; the
//   base advances) -> packed_pack_kernel (copy_spans_from over PackedLayout: the round's own bytes, clipped at dst_cap)
//
// and after the last round packed_info_kernel.  The running base lives in TWO slots of the state block that alternate by round: the
// rebase kernel of round r reads slot r & 1 in every thread and writes slot (r + 1) & 1 in one, so no thread of a launch reads what
// another thread of the same launch writes.
//
// Every kernel here is launch-only work on the caller's stream over caller scratch.
#pragma once
#include "lz4hip_stream.hpp"

namespace lz4hip {

// Device twin of lz4hip_packed_info_t (include/lz4hip.h; the API checks that the layouts agree).
struct PackedInfo {
    int64_t blocks, packed_bytes, written_blocks, first_failed;
    int32_t error, reserved;
};

// the state block: int64 slots in caller scratch, zeroed (kPackedBad: ~0) before the first round
constexpr int kPackedBase = 0;           // and 1: the running base of round r in slot r & 1
constexpr int kPackedTotal = 2;          // the scan's total of the current round
constexpr int kPackedBad = 3;            // lowest global index whose encoder result is <= 0 (~0: none)
constexpr int kPackedError = 4;          // that block's result
constexpr int64_t kPackedStateBytes = 256;
constexpr int32_t kPackedBadLength = -2000000002;   // LZ4HIP_E_ARGUMENT (checked where the C header is seen): a negative length's result

// One round: rows [first, first + cnt) of the batch, row k in ring slot k.
struct PackedRound {
    int64_t first, cnt;
    int64_t slot;                // bytes between ring slots (the slot width, 16-byte aligned)
    int32_t limit;               // the slot width: the per-block output limit where the caller gave none
    int32_t parity;              // round & 1
    const int32_t* cap_in;       // the caller's per-block limits at row 0 of the round, or nullptr
    int32_t* caps;               // the encoder's dst_cap for the round (scratch)
    const int32_t* len_in;       // the caller's per-block lengths at row 0 of the round, or nullptr (one length for all, checked on the host)
    int32_t* lens_enc;           // the encoder's src_len for the round (scratch): len_in with negative lengths as 0; unused without len_in
    int32_t* result;             // the encoder's results, row 0 of the round first; the sizes kernel overrides those of negative lengths
    const uint8_t* ring;
    int64_t* offs;               // dst_off + first: cnt sizes, scanned and rebased in place, then [cnt] = the next round's base
    int32_t* lens;               // packed_len + first, or nullptr
    int64_t* state;
};

// The bytes block k takes: its result, nothing for a block that failed its limit (0) or its arguments (negative).  A limited encoder
// returns at most its limit; a result above it is held inside the slot all the same, so that the pack stays inside the ring.
LZ4HIP_DEVICE int32_t packed_block_len(int32_t r, int32_t limit) { return r < 0 ? 0 : (r > limit ? limit : r); }

__global__ void __launch_bounds__(kStreamThreads) packed_caps_kernel(PackedRound a)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.cnt; k += (int64_t)gridDim.x * kStreamThreads) {
        const int32_t c = a.cap_in ? a.cap_in[k] : a.limit;
        a.caps[k] = c < 0 ? 0 : (c > a.limit ? a.limit : c);
        if (a.len_in) a.lens_enc[k] = a.len_in[k] < 0 ? 0 : a.len_in[k];
    }
}

__global__ void __launch_bounds__(kStreamThreads) packed_sizes_kernel(PackedRound a)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.cnt; k += (int64_t)gridDim.x * kStreamThreads) {
        int32_t r = a.result[k];
        if (a.len_in && a.len_in[k] < 0) a.result[k] = r = kPackedBadLength;   // (the encoder saw an empty block in its place)
        const int32_t len = packed_block_len(r, a.limit);
        a.offs[k] = len;
        if (a.lens) a.lens[k] = len;
        if (r <= 0) atomicMin((unsigned long long*)(a.state + kPackedBad), (unsigned long long)(a.first + k));
    }
}

// after the scan: the round's offsets become global ones.  One thread moves the base on -- into the OTHER slot -- leaves it as the
// entry after the round's last (the next round's first size overwrites it; after the last round it is dst_off[n]) and, when the lowest
// failed index so far lies in this round, keeps its result: the rounds run in index order, so no later round can lower it.
__global__ void __launch_bounds__(kStreamThreads) packed_rebase_kernel(PackedRound a)
{
    const int64_t base = a.state[kPackedBase + a.parity];
    const int64_t t = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
    for (int64_t k = t; k < a.cnt; k += (int64_t)gridDim.x * kStreamThreads) a.offs[k] += base;
    if (t == 0) {
        const int64_t next = base + a.state[kPackedTotal];
        a.state[kPackedBase + (a.parity ^ 1)] = next;
        a.offs[a.cnt] = next;
        const unsigned long long bad = (unsigned long long)a.state[kPackedBad];
        if (bad != ~0ull && (int64_t)bad >= a.first) a.state[kPackedError] = a.result[(int64_t)bad - a.first];
    }
}

// The round's rows as segments of the output: no header, the payload in ring slot k.  start(k) is one load of the global offsets.
struct PackedLayout {
    PackedRound a;
    LZ4HIP_DEVICE int64_t count() const { return a.cnt; }
    LZ4HIP_DEVICE int64_t start(int64_t k) const { return a.offs[k]; }
    LZ4HIP_DEVICE CopySeg seg(int64_t k) const
    {
        CopySeg s;
        s.start = s.pbegin = a.offs[k];
        s.pend = s.start + packed_block_len(a.result[k], a.limit);
        s.payload = a.ring + k * a.slot;
        s.flags = s.original = s.clen = 0;
        return s;
    }
    LZ4HIP_DEVICE uint8_t head_byte(const CopySeg&, int64_t) const { return 0; }   // (no header bytes)
};

// copy_spans over output bytes [begin, end) instead of [0, end): the spans start at the aligned piece that holds `begin`, so a round
// costs its own bytes and not the whole buffer's.  The bytes of that first piece below `begin` lie before the layout's first segment
// (they are an earlier round's): the cursor finds no segment for them and they are not written.
template <class Layout>
LZ4HIP_DEVICE void copy_spans_from(const Layout& L, uint8_t* dst, int64_t begin, int64_t end)
{
    CopyCursor<Layout> c(L);
    for (int64_t base = (begin & ~(int64_t)15) + (int64_t)blockIdx.x * kCopySpan; base < end; base += (int64_t)gridDim.x * kCopySpan)
        for (int j = 0; j < kCopyPiecesPerThread; j++) {
            const int64_t o = base + ((int64_t)j * kStreamThreads + threadIdx.x) * 16;
            if (o >= end) break;
            copy_piece(L, c, dst, o, end);
        }
}

// output bytes [the round's first offset, min(the next round's base, cap)): nothing at or past cap is written
__global__ void __launch_bounds__(kStreamThreads) packed_pack_kernel(PackedLayout L, uint8_t* dst, int64_t cap)
{
    const int64_t begin = L.a.offs[0], end = L.a.state[kPackedBase + (L.a.parity ^ 1)];
    copy_spans_from(L, dst, begin, end < cap ? end : cap);
}

// The record, after the last round.  The offsets are monotone, so the blocks that lie wholly inside cap are a prefix: its length is the
// largest w with dst_off[w] <= cap, found by bisection (dst_off[0] = 0 <= cap).
__global__ void __launch_bounds__(64) packed_info_kernel(const int64_t* dst_off, int64_t n, int64_t cap, const int64_t* state, PackedInfo* info)
{
    if (threadIdx.x != 0) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = hi - (hi - lo) / 2;
        if (dst_off[mid] <= cap) lo = mid; else hi = mid - 1;
    }
    const unsigned long long bad = (unsigned long long)state[kPackedBad];
    PackedInfo r;
    r.blocks = n;
    r.packed_bytes = dst_off[n];
    r.written_blocks = lo;
    r.first_failed = bad == ~0ull ? -1 : (int64_t)bad;
    r.error = bad == ~0ull ? 0 : (int32_t)state[kPackedError];
    r.reserved = 0;
    *info = r;
}

// no block: no state block to read
__global__ void __launch_bounds__(64) packed_empty_info_kernel(PackedInfo* info)
{
    if (threadIdx.x != 0) return;
    PackedInfo r;
    r.blocks = r.packed_bytes = r.written_blocks = 0;
    r.first_failed = -1;
    r.error = r.reserved = 0;
    *info = r;
}

}  // namespace lz4hip
