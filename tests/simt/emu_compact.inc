// emu_compact.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The compact decode of a block batch (lz4net_amd/csrc/lz4hip_compact.hpp) and the legacy frame's one-call decode on top of it under the
// SIMT emulator, for tests/test_simt_compact.py: the real kernels, the library's own fronts and launch sequences (lz4hip_framing.hpp:
// decode_compact, frame_decode_compact and their _plan / _run halves) and its host-pointer call (lz4hip_hostbatch.hpp:
// decode_compact_host) over the emulated device of emu_framing.hpp.  The block decoder is a stand-in keyed by GLOBAL block index: the
// sequence hands the decoder one round's rows at a time, so the backend counts the rows it has been given.  Results and bytes are the
// test's, computed with the oracle.  The size field walks are the counters' passes.

// what the emulated device is to do, and what it did
struct CompactEmuRun {
    const int32_t* results;      // per global block: what LZ4_uncompress_unknownOutputSize returns for it at its limit
    const int32_t* limits;       // ... that limit: the capacity the decoder must be handed for the block
    const int64_t* at;           // ... and where its max(result, 0) bytes start in `bytes`
    const uint8_t* bytes;
    const uint8_t* src;          // the source rows, block g at src_at[g]: every row the decoder is handed is compared with it
    const int64_t* src_at;
    const int32_t* src_len;      // per global block: the length the decoder must see (0 where the caller's is negative)
    int64_t n;
    int32_t grid, pad;           // grid > 0 replaces the item and copy formulas' answers
    int64_t calls, max_rows, shape_errors;                               // decoder calls, the most rows in one, rows or descriptors that were not as promised
    EmuCounters counters;
};

namespace {

struct CompactBackend : EmuBackend {
    CompactEmuRun* r = nullptr;
    int64_t done = 0;

    // LZ4_uncompress_unknownOutputSize per row at the row's capacity: the oracle's result and, inside the capacity and nowhere else, its
    // bytes; what lies between them and the capacity is junk, as after a decoder that failed or stopped short
    int decode(const lz4hip_batch_t* b, int known)
    {
        r->calls++;
        if (b->n_blocks > r->max_rows) r->max_rows = b->n_blocks;
        if (known || !b->dst_cap || !b->result || !b->dst || b->dst_off || b->dst_stride % 16 != 0 || done + b->n_blocks > r->n) { r->shape_errors++; return 0; }
        for (int64_t j = 0; j < b->n_blocks; j++) {
            const int64_t g = done + j;
            const uint8_t* row = (const uint8_t*)b->src + (b->src_off ? b->src_off[j] : j * b->src_stride);
            const int32_t len = b->src_len ? b->src_len[j] : b->src_len_all, cap = b->dst_cap[j], res = r->results[g];
            uint8_t* out = (uint8_t*)b->dst + j * b->dst_stride;
            if (cap < 0 || cap > b->dst_stride || cap != r->limits[g]) { r->shape_errors++; continue; }
            if (len != r->src_len[g]) { r->shape_errors++; continue; }   // (a negative length must arrive as an empty block)
            if (len > 0 && memcmp(row, r->src + r->src_at[g], (size_t)len) != 0) r->shape_errors++;
            const int64_t wrote = res > 0 ? res : 0, junk = wrote + 64 < cap ? wrote + 64 : cap;
            if (wrote > cap) { r->shape_errors++; continue; }
            memset(out, kJunk, (size_t)junk);
            memcpy(out, r->bytes + r->at[g], (size_t)wrote);
            b->result[j] = res;
        }
        done += b->n_blocks;
        return 0;
    }
};

CompactBackend backend_of(CompactEmuRun* r)
{
    CompactBackend be = backend<CompactBackend>(r->grid, r->grid);
    be.r = r;
    return be;
}

}  // namespace

extern "C" {

int64_t emu_compact_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(PackedInfo);
    case 1: return sizeof(CompactEmuRun);
    case 2: return sizeof(lz4hip_batch_t);
    case 3: return sizeof(lz4hip_compact_info_t);
    case 4: return sizeof(FrameTables);
    case 5: return sizeof(FrameInfo);
    case 100: return kScanTile;
    case 101: return kCopySpan;
    default: return -1;
    }
}

int64_t emu_compact_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t round_blocks) { return framing::decode_compact_scratch_bytes(n, slot_bytes, round_blocks); }
int64_t emu_frame_compact_scratch_bytes(int32_t chunk_size, int64_t max_chunks, int64_t round_chunks)
{
    return framing::frame_decode_compact_scratch_bytes(chunk_size, max_chunks, round_chunks);
}

// where the frame call keeps its table in a scratch buffer
void emu_frame_compact_tables(void* scratch, int32_t chunk_size, int64_t max_chunks, int64_t round_chunks, FrameTables* t)
{
    *t = framing::frame_compact_scratch(scratch, framing::frame_chunk(chunk_size), max_chunks, round_chunks).t;
}

// framing::decode_compact, front and sequence, on a scratch buffer the test brings
int emu_decode_compact(const lz4hip_batch_t* b, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* decoded_len,
                       void* scratch, int64_t scratch_bytes, lz4hip_compact_info_t* info, CompactEmuRun* r)
{
    CompactBackend be = backend_of(r);
    return finish(be, framing::decode_compact(be, b, round_blocks, dst, dst_cap, dst_off, decoded_len, scratch, scratch_bytes, info), &r->counters);
}

// hostbatch::decode_compact_host over the emulated image; pool_floor < 0: the library's limit for gathering on the row pool
int emu_decode_compact_host(const lz4hip_batch_t* b, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* decoded_len,
                            lz4hip_compact_info_t* info, int64_t pool_floor, CompactEmuRun* r)
{
    CompactBackend be = backend_of(r);
    hostbatch::HostLimits limits;
    if (pool_floor >= 0) limits.pool_floor = pool_floor;
    return finish(be, hostbatch::decode_compact_host(be, b, round_blocks, dst, dst_cap, dst_off, decoded_len, info, 2, limits), &r->counters);
}

// framing::frame_decode_compact, front and sequence: block g of the run record is row g of the table
int emu_frame_decode_compact(const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, int64_t round_chunks, void* scratch,
                             int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_frame_info_t* info, CompactEmuRun* r)
{
    CompactBackend be = backend_of(r);
    return finish(be, framing::frame_decode_compact(be, src, src_len, chunk_size, max_chunks, round_chunks, scratch, scratch_bytes, dst, dst_cap, info), &r->counters);
}

}  // extern "C"
