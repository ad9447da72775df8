// emu_lz4f.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The xxHash32 row kernel and the LZ4 frame path (lz4net_amd/csrc/lz4hip_lz4f.hpp) under the SIMT emulator, for tests/test_simt_lz4f.py
// and tests/test_lz4f_interop.py: the real kernels, the library's own fronts and launch sequences (lz4hip_framing.hpp: xxh32_rows_run,
// lz4f_encode, lz4f_decode) and its host-pointer calls (lz4f_encode_host / lz4f_decode_host) over the emulated device of
// emu_framing.hpp.  The block codec is a stand-in, as in emu_frame.inc: results and bytes the test computed with the oracle -- the
// encoder's by row, the decoder's keyed by GLOBAL table row, because the sequence hands the decoder one round's rows at a time.

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
    int32_t grid, pad;           // grid > 0 replaces the item and copy formulas' answers
    int64_t calls, shape_errors; // decoder calls; rows or descriptors that were not as promised
    EmuCounters counters;
};

namespace {

// The stand-in block decoder keyed by global table row, of this part's backend and of the batch's (emu_lz4f_batch.inc): `Run` is the
// run record, of which it reads dec_results, dec_len, dec_at, dec_bytes and dec_rows and counts calls and shape_errors.  It is what
// decides whether a decode sequence kept its promises, so it is written once.
template <class Run>
struct RowKeyedDecoder : EmuBackend {
    Run* r = nullptr;
    int64_t done = 0, walk = 0;  // rows the decoder was given since walk number `walk` (EmuBackend::passes)

    int decode(const lz4hip_batch_t* b, int known)
    {
        r->calls++;
        if (walk != passes) { walk = passes; done = 0; }                     // (a host call that decodes again starts at row 0 again)
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

struct Lz4fBackend : RowKeyedDecoder<Lz4fEmuRun> {
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
};

Lz4fBackend backend_of(Lz4fEmuRun* r)
{
    Lz4fBackend be = backend<Lz4fBackend>(r->grid, r->grid, 0, r->enc_results, r->enc_bytes);
    be.r = r;
    return be;
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
    return finish(be, framing::lz4f_encode(be, src, src_len, id, mode, flags, dst, dst_cap, dst_len, scratch, scratch_bytes), &r->counters);
}

int emu_lz4f_decode(const void* src, int64_t src_len, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch,
                    int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, Lz4fEmuRun* r)
{
    Lz4fBackend be = backend_of(r);
    return finish(be, framing::lz4f_decode(be, src, src_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info), &r->counters);
}

// ---- the host-pointer calls ----------------------------------------------------------------------------------------------------------
int emu_lz4f_encode_host(const void* src, int64_t src_len, int id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len, Lz4fEmuRun* r)
{
    Lz4fBackend be = backend_of(r);
    return finish(be, framing::lz4f_encode_host(be, src, src_len, id, mode, flags, dst, dst_cap, dst_len), &r->counters);
}

int emu_lz4f_decode_host(const void* src, int64_t src_len, unsigned flags, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, Lz4fEmuRun* r)
{
    Lz4fBackend be = backend_of(r);
    return finish(be, framing::lz4f_decode_host(be, src, src_len, flags, dst, dst_cap, info), &r->counters);
}

}  // extern "C"
