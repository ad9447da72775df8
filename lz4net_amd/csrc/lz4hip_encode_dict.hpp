// lz4hip_encode_dict.hpp -- block batches encoded against ONE shared dictionary (lz4hip_encode_batch_dict_*), fast mode, one
// wavefront per block.
//
// The reference has no such parse, so the bytes are defined here: the generic encoder (LZ4_compressCtx,
// original/lz4.c:345-562, which encode_fast_block<true> restates) run over the VIRTUAL buffer V = tail || block, where tail is the
// last T = min(dict_len, 65 535) bytes of the dictionary, with its U32[4096] table PRIMED: bucket h holds the highest position
// p <= T - 4 whose word hashes to h (0 where there is none -- position 0, a legitimate candidate, as in the reference).  The parse
// starts at T (table[hash(V[T..])] = T, anchor = T, first probe at T + 1); every limit of the reference is taken over N = T + n.
// Literals always come from the block, offsets are ip - ref <= 65 535, and a block's bytes are legal input for
// lz4hip_decode_batch_dict_device and LZ4_decompress_safe_usingDict.
//
// Two kernels: encode_dict_prime_kernel builds the primed table once per call (it depends on the dictionary alone), and
// encode_dict_kernel copies it into each wavefront's LDS in place of the zero fill and runs encode_fast_block<true> over a
// two-segment VIEW of V: position p < T reads dict_end - T + p, any other src + p - T.
#pragma once
#include "lz4hip_encode.hpp"

namespace lz4hip {

constexpr int kEncDictPrimeThreads = 256;
constexpr int kEncDictMaxInput = 0x7E000000;                         // LZ4_MAX_INPUT_SIZE

// V = tail || block.  `src` is the block, `dict_end` one past the dictionary's last byte, T >= 1 the reachable bytes before it.
struct DictInput {
    const uint8_t* dict_end;
    const uint8_t* src;
    int T;
    const uint8_t* primed;                                            // the primed table (encode_dict_prime_kernel), 16 KiB
    // the address of V[p] (any p in [0, N))
    LZ4HIP_DEVICE const uint8_t* at(int p) const { return p < T ? dict_end - (T - p) : src + (p - T); }
    LZ4HIP_DEVICE uint8_t operator[](int p) const
    {
        LZ4HIP_STAT_ENCDICT(kEncDictByteInDict, p < T ? 1 : 0);
        return *at(p);
    }
};
struct DictAt { DictInput v; int p; };                               // "in + p"
LZ4HIP_DEVICE DictAt operator+(const DictInput& v, int p) { return DictAt{ v, p }; }
LZ4HIP_DEVICE DictAt operator+(const DictAt& a, int d) { return DictAt{ a.v, a.p + d }; }
LZ4HIP_DEVICE DictAt operator-(const DictAt& a, int d) { return DictAt{ a.v, a.p - d }; }

// The dword V[p .. p + 4).  Inside one segment it is ONE load, issued unconditionally (a load under a condition needs its register
// zeroed first, which waits for whatever is in flight: lz4hip_encode.hpp, round 6); a dword that straddles T -- the ref side of a count
// or a candidate word, T < 4 included -- takes the block's first dword with that load (the parse only runs on blocks of 13 bytes and
// more) and, under a rare branch, its 1 .. 3 bytes of the dictionary one by one.
LZ4HIP_DEVICE uint32_t load_u32(const DictAt& a)
{
    const int p = a.p, T = a.v.T;
    const int k = T - p;                                              // bytes of the dword that lie in the dictionary, if 1 .. 3
    const bool straddles = k > 0 && k < 4;
    LZ4HIP_STAT_ENCDICT(kEncDictWordInDict, k >= 4 ? 1 : 0);
    LZ4HIP_STAT_ENCDICT(kEncDictWordStraddles, straddles ? 1 : 0);
    uint32_t w = load_u32(straddles ? a.v.src : a.v.at(p));
    if (straddles) {
        uint32_t head = 0;
        for (int j = 0; j < k; j++) head |= (uint32_t)a.v.dict_end[j - k] << (8 * j);
        w = head | (w << (8 * k));
    }
    return w;
}
// (the re-seed's qword at ip - 2: ip is the end of a match that began at or behind `anchor` >= T and has 4 bytes or more -- inside the block)
LZ4HIP_DEVICE uint64_t load_u64(const DictAt& a) { return load_u64(a.v.src + (a.p - a.v.T)); }
// (literals: anchor >= T)
LZ4HIP_DEVICE void wave_copy(uint8_t* dst, const DictAt& a, int n) { wave_copy(dst, a.v.src + (a.p - a.v.T), n); }

LZ4HIP_DEVICE int input_start(const DictInput& v) { return v.T; }

// the primed table into the wavefront's LDS, 16 bytes per lane and step, in place of the zero fill
LZ4HIP_DEVICE void fast_table_init(const DictInput& v, unsigned char* table_bytes)
{
    for (int k = wv::lane() * 16; k < kFastTableBytes; k += 64 * 16) *(Vec16*)(table_bytes + k) = load_v16(v.primed + k);
}

// ---- the primed table: bucket h = the highest p in [0, T - 4] with hash(read32(V, p)) == h, 0 where there is none ---------------------
// ONE workgroup: a maximum over positions in LDS (order does not matter: deterministic), then the table leaves in 16-byte vector
// stores.  Positions p <= T - 4 lie wholly inside the tail, so no block byte is read; T < 4 gives the zero table.
__global__ void __launch_bounds__(kEncDictPrimeThreads) encode_dict_prime_kernel(const uint8_t* dict_end, int T, uint8_t* primed)
{
    LZ4HIP_STATIC_LDS(lds, kFastTableBytes);
    uint32_t* const table = (uint32_t*)lds;
    const int t = (int)threadIdx.x;
    for (int k = t * 16; k < kFastTableBytes; k += kEncDictPrimeThreads * 16) {
        Vec16 z = { { 0, 0, 0, 0 } };
        *(Vec16*)(lds + k) = z;
    }
    wv::block_sync();
    const uint8_t* const tail = dict_end - T;
    for (int p = t; p <= T - 4; p += kEncDictPrimeThreads) atomicMax(&table[FastTable<true>::hash(load_u32(tail + p))], (uint32_t)p);
    wv::block_sync();
    for (int k = t * 16; k < kFastTableBytes; k += kEncDictPrimeThreads * 16) store_v16(primed + k, *(const Vec16*)(lds + k));
}

// ---- one wavefront per block, WAVES blocks per workgroup, 16 KiB of dynamic LDS each (as encode_fast_kernel; no barrier) ----------------
template <int WAVES = 1>
__global__ void __launch_bounds__(64 * WAVES) encode_dict_kernel(Batch b, const uint8_t* dict_end, int T, const uint8_t* primed)
{
    LZ4HIP_DYN_LDS(lds_all);
    unsigned char* const lds = lds_all + (WAVES > 1 ? (size_t)wv::wave_in_block() * kFastTableBytes : 0);
    const int64_t blk = WAVES > 1 ? (int64_t)blockIdx.x * WAVES + wv::wave_in_block() : (int64_t)blockIdx.x;
    if (blk >= b.n_blocks) return;
    const int n = wv::uniform(batch_src_len(b, blk));
    const int cap = wv::uniform(batch_dst_cap(b, blk));
    const DictInput in = { dict_end, batch_src(b, blk), T, primed };
    LZ4HIP_STAT_ENCDICT(kEncDictBlocks, wv::lane() == 0 && n >= kMinLength ? 1 : 0);
    // (N = T + n must stay an int: a block beyond the reference's LZ4_MAX_INPUT_SIZE gets its result for one, 0)
    const int r = n > kEncDictMaxInput ? 0 : encode_fast_block<true>(in, T + n, batch_dst(b, blk), cap, lds);
    if (wv::lane() == 0) b.result[blk] = r;
}

}  // namespace lz4hip
