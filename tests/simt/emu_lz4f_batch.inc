// emu_lz4f_batch.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The batch of LZ4 frames (lz4net_amd/csrc/lz4hip_lz4f_batch.hpp and its host code in lz4hip_framing.hpp: lz4f_batch_encode,
// lz4f_batch_decode and the host-pointer calls lz4f_batch_encode_host / lz4f_batch_decode_host) under the SIMT emulator, for
// tests/test_simt_lz4f_batch.py and tests/cpp/lz4f_batch_asan_main.cpp, and the decode of frames with linked blocks
// (lz4net_amd/csrc/lz4hip_lz4f_linked.hpp inside the sequences lz4f_decode and lz4f_batch_decode) over the same backend, for
// tests/test_simt_lz4f_linked.py and tests/cpp/lz4f_linked_asan_main.cpp.  The block codec is a stand-in, as in emu_lz4f.inc: results
// and bytes the test computed with the oracle, keyed by GLOBAL table row -- the encoder's table spans all items, and the decoder is
// emu_lz4f.inc's RowKeyedDecoder.

// what the emulated device is to do, and what it did
struct Lz4fBatchEmuRun {
    const int32_t* enc_results;  // the block encoder's stand-in: table row j gets enc_results[j] and its bytes from enc_bytes at enc_at[j]
    const uint8_t* enc_bytes;
    const int64_t* enc_at;
    const int32_t* enc_len;      // ... the length the encoder must be handed for row j; its capacity must be that length - 1 (0 for an empty row)
    const int64_t* enc_src;      // ... and where the row's source (and its output in scratch) must lie
    int64_t enc_rows;            // rows past these must be empty
    const int32_t* dec_results;  // the block decoder's, per table row: what LZ4_uncompress_unknownOutputSize returns at the slot's capacity
    const int32_t* dec_len;      // ... the length the decoder must be handed for the row (0: raw, bad checksum, past the count)
    const int64_t* dec_at;       // ... and where its max(result, 0) bytes start in dec_bytes
    const uint8_t* dec_bytes;
    int64_t dec_rows;
    int32_t grid, pad;           // grid > 0 replaces the item, copy and walk formulas' answers
    int64_t calls, shape_errors; // decoder calls; rows that were not as promised
    EmuCounters counters;
};

namespace {

struct Lz4fBatchBackend : RowKeyedDecoder<Lz4fBatchEmuRun> {
    template <class... P, class... A>
    void launch(void (*kernel)(P...), framing::Grid grid, unsigned threads, A&&... a)
    {
        passes += same_kernel(kernel, lz4f_batch_walk_kernel<false>);
        EmuBackend::launch(kernel, grid, threads, a...);
    }

    // ONE call over the blocks of all items: every block at its own source position, into scratch at the same position, with one byte less
    // of room than it is long
    int encode(const lz4hip_batch_t* b, int)
    {
        if (!b->src_len || !b->dst_cap || !b->result || !b->dst || !b->src_off || !b->dst_off) { r->shape_errors++; return 0; }
        for (int64_t j = 0; j < b->n_blocks; j++) {
            const int32_t len = b->src_len[j], cap = b->dst_cap[j];
            const bool live = j < r->enc_rows;
            if (len != (live ? r->enc_len[j] : 0) || cap != (len > 0 ? len - 1 : 0) || b->src_off[j] != b->dst_off[j] ||
                (live && len > 0 && b->src_off[j] != r->enc_src[j])) { r->shape_errors++; b->result[j] = 0; continue; }
            const int32_t res = live ? r->enc_results[j] : 0;
            if (res > cap) { r->shape_errors++; b->result[j] = 0; continue; }
            if (res > 0) memcpy((uint8_t*)b->dst + b->dst_off[j], r->enc_bytes + r->enc_at[j], (size_t)res);
            b->result[j] = res;
        }
        return 0;
    }
};

Lz4fBatchBackend backend_of(Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = backend<Lz4fBatchBackend>(r->grid, r->grid, r->grid);
    be.r = r;
    return be;
}

// The linked decode needs what the plain launches do not have: a workgroup's LDS as large as the wavefront decoder's rings.  The linked
// rows are decoded by the real decode_block under the emulator; the stand-in sees them as the empty rows the sequence promises, and the
// INDEPENDENT rows keep it.
Lz4fBatchBackend linked_backend_of(Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = backend_of(r);
    be.lds_bytes = kWaveDecodeLdsBytes;
    return be;
}

}  // namespace

extern "C" {

int64_t emu_lz4f_batch_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(Lz4fInfo);
    case 1: return sizeof(Lz4fBatchEmuRun);
    case 2: return sizeof(lz4hip_lz4f_batch_info_t);
    case 3: return sizeof(EmuCounters);
    case 100: return kScanTile;
    default: return -1;
    }
}

int64_t emu_lz4f_batch_bound(int64_t n, int64_t src_len, int id, unsigned flags) { return framing::lz4f_batch_bound(n, src_len, id, flags); }
int64_t emu_lz4f_batch_encode_scratch_bytes(int64_t n, int64_t src_len, int id)
{
    return framing::lz4f_batch_encode_scratch(nullptr, n, src_len, lz4f_block_bytes(framing::lz4f_id(id))).bytes;
}
int64_t emu_lz4f_batch_decode_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    return framing::lz4f_batch_decode_scratch_bytes(n, slot_bytes, max_blocks, round_blocks);
}

// ---- the fronts with their sequences: the library's argument lists, then the run record ------------------------------------------------
int emu_lz4f_batch_encode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int id, int mode, unsigned flags, void* dst, int64_t dst_cap,
                          int64_t* dst_off, void* scratch, int64_t scratch_bytes, Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = backend_of(r);
    return finish(be, framing::lz4f_batch_encode(be, src, src_len, src_off, n, id, mode, flags, dst, dst_cap, dst_off, scratch, scratch_bytes), &r->counters);
}

int emu_lz4f_batch_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks,
                          unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info,
                          lz4hip_lz4f_batch_info_t* info, int64_t* written_items, Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = backend_of(r);
    return finish(be, framing::lz4f_batch_decode(be, src, src_len, src_off, n, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap,
                                                 dst_off, item_info, info, written_items), &r->counters);
}

// ---- the host-pointer calls ----------------------------------------------------------------------------------------------------------
int emu_lz4f_batch_encode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int id, int mode, unsigned flags, void* dst,
                               int64_t dst_cap, int64_t* dst_off, Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = backend_of(r);
    return finish(be, framing::lz4f_batch_encode_host(be, src, src_len, src_off, n, id, mode, flags, dst, dst_cap, dst_off), &r->counters);
}

int emu_lz4f_batch_decode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, unsigned flags, void* dst, int64_t dst_cap,
                               int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = backend_of(r);
    return finish(be, framing::lz4f_batch_decode_host(be, src, src_len, src_off, n, flags, dst, dst_cap, dst_off, item_info, info), &r->counters);
}

// ---- frames with linked blocks: the one-frame and the batch decode with the wavefront decoder's LDS -------------------------------------
int64_t emu_lz4f_linked_decode_scratch_bytes(int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    return framing::lz4f_decode_scratch_bytes(slot_bytes, max_blocks, round_blocks);
}

int emu_lz4f_linked_decode(const void* src, int64_t src_len, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch,
                           int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = linked_backend_of(r);
    return finish(be, framing::lz4f_decode(be, src, src_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info), &r->counters);
}

int emu_lz4f_linked_decode_host(const void* src, int64_t src_len, unsigned flags, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = linked_backend_of(r);
    return finish(be, framing::lz4f_decode_host(be, src, src_len, flags, dst, dst_cap, info), &r->counters);
}

int emu_lz4f_linked_batch_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t slot_bytes, int64_t max_blocks,
                                 int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off,
                                 lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, int64_t* written_items, Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = linked_backend_of(r);
    return finish(be, framing::lz4f_batch_decode(be, src, src_len, src_off, n, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap,
                                                 dst_off, item_info, info, written_items), &r->counters);
}

int emu_lz4f_linked_batch_decode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, unsigned flags, void* dst, int64_t dst_cap,
                                      int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = linked_backend_of(r);
    return finish(be, framing::lz4f_batch_decode_host(be, src, src_len, src_off, n, flags, dst, dst_cap, dst_off, item_info, info), &r->counters);
}

}  // extern "C"
