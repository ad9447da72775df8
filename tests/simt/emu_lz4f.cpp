// emu_lz4f.cpp -- TEST INFRASTRUCTURE ONLY.
// The xxHash32 row kernel and the LZ4 frame path (lz4net_amd/csrc/lz4hip_lz4f.hpp) under the SIMT emulator, for tests/test_simt_lz4f.py
// and tests/test_lz4f_interop.py: the real kernels, the library's own fronts and launch sequences (lz4hip_framing.hpp: xxh32_rows_run,
// lz4f_encode, lz4f_decode) and its host-pointer calls (lz4f_encode_host / lz4f_decode_host) over the emulated device of
// emu_framing.hpp.  The block codec is a stand-in, as in emu_frame.cpp: results and bytes the test computed with the oracle -- the
// encoder's by row, the decoder's keyed by GLOBAL table row, because the sequence hands the decoder one round's rows at a time.  Built
// with g++ by build_emu_lz4f.py into a library of its own, never shipped.
#include "simt_wave.hpp"

// the quad exchanges of lz4hip_wave.hpp (DPP quad_perm): lane i receives v from lane i ^ 1 / i ^ 2, and that lane must take part
#define LZ4HIP_WAVE_QUAD 1
namespace wv {
inline uint32_t quad_xor(uint32_t v, int x, int site)
{
    unsigned p, tag;
    const simt::Lane* w = simt::exchange(v, site, &p, &tag);
    const int from = lane() ^ x;
    if (from >= simt::wave_width(simt::rt().cur) || !simt::took_part(w[from], p, tag)) simt::die("wv::quad_xor() with an inactive lane in the quad", from);
    return (uint32_t)w[from].slot[p];
}
inline uint32_t quad_xor1(uint32_t v) { return quad_xor(v, 1, 160); }
inline uint32_t quad_xor2(uint32_t v) { return quad_xor(v, 2, 161); }
}  // namespace wv

#include "lz4hip_common.hpp"

using namespace lz4hip;

#include "emu_framing.hpp"

// what the emulated device is to do, and what it did
struct Lz4fEmuRun {
    const int32_t* enc_results;  // the block encoder's stand-in: block j gets enc_results[j] and its bytes from enc_bytes at j * stride
    const uint8_t* enc_bytes;
    const int32_t* enc_len;      // ... the length the encoder must be handed for block j; its capacity must be that length - 1
    const int32_t* dec_results;  // the block decoder's, per table row: what LZ4_uncompress_unknownOutputSize returns at the slot's capacity
    const int32_t* dec_len;      // ... the length the decoder must be handed for the row (0: raw, bad checksum, past the count)
    const int64_t* dec_at;       // ... and where its max(result, 0) bytes start in dec_bytes
    const uint8_t* dec_bytes;
    int64_t dec_rows;
    int32_t grid, intact;        // grid > 0 replaces every formula's answer; intact: EmuBackend::intact() after a host call
    int64_t calls, shape_errors; // decoder calls; rows or descriptors that were not as promised
    int64_t reserves, moves, uploads, downloads, syncs;
    char error[160];
};

namespace {

constexpr uint8_t kJunk = 0xBD;  // what a decoder may leave inside its capacity

struct Lz4fBackend : emu_framing::EmuBackend {
    Lz4fEmuRun* r = nullptr;
    int64_t done = 0;

    template <class... P, class... A>
    void launch(void (*kernel)(P...), framing::Grid grid, unsigned threads, A&&... a)
    {
        if (emu_framing::same_kernel(kernel, lz4f_walk_kernel)) done = 0;    // (a host call that decodes again starts at row 0 again)
        const int mine = grid.kind == framing::kGridItems || grid.kind == framing::kGridCopy ? r->grid : 0;
        simt::launch(dim3(mine > 0 ? (unsigned)mine : grid.groups), dim3(threads), kStreamThreads * 8,
                     emu_framing::KernelCall<P...>{ kernel, std::tuple<P...>{ P(a)... } });
    }
    // LZ4_compress_limitedOutput per block at length - 1: the batch must be the frame's blocks, each with its own length (the last one
    // ragged) and one byte less of room; the results and bytes are the test's
    int encode(const lz4hip_batch_t* b, int)
    {
        if (!b->src_len || !b->dst_cap || !b->result || !b->dst || b->src_off || b->dst_off) { r->shape_errors++; return 0; }
        for (int64_t j = 0; j < b->n_blocks; j++) {
            const int32_t len = b->src_len[j], cap = b->dst_cap[j];
            if (len != r->enc_len[j] || cap != len - 1 || cap > b->dst_stride || len > b->src_stride) { r->shape_errors++; b->result[j] = 0; continue; }
            const int32_t res = r->enc_results[j];
            if (res > cap) { r->shape_errors++; b->result[j] = 0; continue; }
            if (res > 0) memcpy((uint8_t*)b->dst + j * b->dst_stride, r->enc_bytes + j * b->dst_stride, (size_t)res);
            b->result[j] = res;
        }
        return 0;
    }
    int decode(const lz4hip_batch_t* b, int known)
    {
        r->calls++;
        if (known || !b->dst_cap || !b->result || !b->dst || b->dst_off || !b->src_off || !b->src_len || b->dst_stride % 16 != 0) { r->shape_errors++; return 0; }
        for (int64_t j = 0; j < b->n_blocks; j++) {
            const int64_t g = done + j;
            const int32_t len = b->src_len[j], cap = b->dst_cap[j];
            uint8_t* out = (uint8_t*)b->dst + j * b->dst_stride;
            if (len == 0) { b->result[j] = 0; continue; }                    // an empty block decodes to nothing
            if (g >= r->dec_rows || len != r->dec_len[g] || cap < 0 || cap > b->dst_stride) { r->shape_errors++; b->result[j] = -1; continue; }
            const int32_t res = r->dec_results[g];
            const int64_t wrote = res > 0 ? res : 0, junk = wrote + 64 < cap ? wrote + 64 : cap;
            if (wrote > cap) { r->shape_errors++; b->result[j] = -1; continue; }
            memset(out, kJunk, (size_t)junk);
            memcpy(out, r->dec_bytes + r->dec_at[g], (size_t)wrote);
            b->result[j] = res;
        }
        done += b->n_blocks;
        return 0;
    }
};

Lz4fBackend backend_of(Lz4fEmuRun* r)
{
    Lz4fBackend be;
    be.r = r; be.results = r->enc_results; be.bytes = r->enc_bytes;
    return be;
}

int finish(const Lz4fBackend& be, int rc, Lz4fEmuRun* r)
{
    r->intact = be.intact();
    r->reserves = be.reserves; r->moves = be.moves; r->uploads = be.uploads; r->downloads = be.downloads; r->syncs = be.syncs;
    snprintf(r->error, sizeof r->error, "%s", be.error.c_str());
    return rc;
}

}  // namespace

extern "C" {

int64_t emu_lz4f_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(Lz4fInfo);
    case 1: return sizeof(Lz4fEmuRun);
    case 2: return sizeof(lz4hip_lz4f_info_t);
    case 100: return kXxhRowsPerWave * (kXxhThreads / 64);
    case 101: return 64 * kXxhDepth;
    default: return -1;
    }
}

uint32_t emu_xxh32_serial(const uint8_t* p, int64_t len, uint32_t seed) { return xxh32_serial(p, len, seed); }

// the row kernel through the library's launch: grid > 0 replaces the formula's answer
int emu_xxh32_rows(const void* data, const int64_t* off, int64_t stride, const int32_t* len, int64_t len_all, uint32_t seed, uint32_t* sums,
                   int64_t n, int grid)
{
    Lz4fEmuRun r = {};
    r.grid = grid;
    Lz4fBackend be = backend_of(&r);
    if (int rc = framing::xxh32_rows_check(be, data, off, stride, len, len_all, sums, n)) return rc;
    const XxhRows rows = { (const uint8_t*)data, off, stride, len, nullptr, len_all, seed, sums, n };
    return framing::xxh32_rows_run(be, rows);
}

int64_t emu_lz4f_bound(int64_t src_len, int id, unsigned flags) { return framing::lz4f_bound(src_len, id, flags); }
int64_t emu_lz4f_encode_scratch_bytes(int64_t src_len, int id)
{
    return framing::lz4f_encode_scratch(nullptr, src_len, lz4f_block_bytes(framing::lz4f_id(id))).bytes;
}
int64_t emu_lz4f_decode_scratch_bytes(int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    return framing::lz4f_decode_scratch_bytes(slot_bytes, max_blocks, round_blocks);
}

// ---- the fronts with their sequences: the library's argument lists, then the run record ------------------------------------------------
int emu_lz4f_encode(const void* src, int64_t src_len, int id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len, void* scratch,
                    int64_t scratch_bytes, Lz4fEmuRun* r)
{
    Lz4fBackend be = backend_of(r);
    return finish(be, framing::lz4f_encode(be, src, src_len, id, mode, flags, dst, dst_cap, dst_len, scratch, scratch_bytes), r);
}

int emu_lz4f_decode(const void* src, int64_t src_len, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch,
                    int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, Lz4fEmuRun* r)
{
    Lz4fBackend be = backend_of(r);
    return finish(be, framing::lz4f_decode(be, src, src_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info), r);
}

// ---- the host-pointer calls ----------------------------------------------------------------------------------------------------------
int emu_lz4f_encode_host(const void* src, int64_t src_len, int id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len, Lz4fEmuRun* r)
{
    Lz4fBackend be = backend_of(r);
    return finish(be, framing::lz4f_encode_host(be, src, src_len, id, mode, flags, dst, dst_cap, dst_len), r);
}

int emu_lz4f_decode_host(const void* src, int64_t src_len, unsigned flags, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, Lz4fEmuRun* r)
{
    Lz4fBackend be = backend_of(r);
    return finish(be, framing::lz4f_decode_host(be, src, src_len, flags, dst, dst_cap, info), r);
}

}  // extern "C"
