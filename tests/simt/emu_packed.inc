// emu_packed.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The packed encode of a block batch (lz4net_amd/csrc/lz4hip_packed.hpp) under the SIMT emulator, for tests/test_simt_packed.py: the real
// kernels, the library's own front and launch sequence (lz4hip_framing.hpp: encode_packed and its _plan / _run halves) and its
// host-pointer call (lz4hip_hostbatch.hpp: encode_packed_host) over the emulated device of emu_framing.hpp.  The block codec is a
// stand-in keyed by GLOBAL block index: the sequence hands the encoder one round's rows at a time, so the backend counts the rows it
// has been given.  Results and bytes are the test's, computed with the oracle.

// what the emulated device is to do, and what it did
struct PackedEmuRun {
    const int32_t* sizes;        // per global block: the size of the encoder's output for it
    const int64_t* at;           // ... and where those bytes start in `bytes`
    const uint8_t* bytes;
    const uint8_t* src;          // the source rows back to back, block g at src_at[g]: every row the encoder is handed is compared with it
    const int64_t* src_at;
    const uint8_t* bad_len;      // per global block: 1 where the caller's length is negative (the encoder must see an empty block there), or NULL
    int64_t n;
    int32_t grid, pad;           // grid > 0 replaces the item and copy formulas' answers
    int64_t calls, max_rows, shape_errors;                               // encoder calls, the most rows in one, rows or descriptors that were not as promised
    EmuCounters counters;
};

namespace {

struct PackedBackend : EmuBackend {
    PackedEmuRun* r = nullptr;
    int64_t done = 0;

    // LZ4_compress_limitedOutput per row: the oracle's bytes where they fit the row's capacity, else 0 and junk inside the capacity
    int encode(const lz4hip_batch_t* b, int)
    {
        r->calls++;
        if (b->n_blocks > r->max_rows) r->max_rows = b->n_blocks;
        if (!b->dst_cap || !b->result || !b->dst || b->dst_off || b->dst_stride % 16 != 0 || done + b->n_blocks > r->n) { r->shape_errors++; return 0; }
        for (int64_t j = 0; j < b->n_blocks; j++) {
            const int64_t g = done + j;
            const uint8_t* row = (const uint8_t*)b->src + (b->src_off ? b->src_off[j] : j * b->src_stride);
            const int32_t len = b->src_len ? b->src_len[j] : b->src_len_all, cap = b->dst_cap[j];
            uint8_t* out = (uint8_t*)b->dst + j * b->dst_stride;
            if (cap < 0 || cap > b->dst_stride) { r->shape_errors++; continue; }
            if (len < 0) { r->shape_errors++; continue; }           // the sequence must keep a negative length from the encoders: they do not check it
            if (len > 0 && memcmp(row, r->src + r->src_at[g], (size_t)len) != 0) r->shape_errors++;
            memset(out, kJunk, (size_t)cap);
            if (r->bad_len && r->bad_len[g]) {                             // the block arrives as an empty one: the one-byte block
                if (len != 0) r->shape_errors++;
                if (cap < 1) { b->result[j] = 0; continue; }
                out[0] = 0; b->result[j] = 1;
                continue;
            }
            if (r->sizes[g] > cap) { b->result[j] = 0; continue; }
            memcpy(out, r->bytes + r->at[g], (size_t)r->sizes[g]);
            b->result[j] = r->sizes[g];
        }
        done += b->n_blocks;
        return 0;
    }
};

PackedBackend backend_of(PackedEmuRun* r)
{
    PackedBackend be = backend<PackedBackend>(r->grid, r->grid);
    be.r = r;
    return be;
}

}  // namespace

extern "C" {

int64_t emu_packed_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(PackedInfo);
    case 1: return sizeof(PackedEmuRun);
    case 2: return sizeof(lz4hip_batch_t);
    case 100: return kScanTile;
    case 101: return kCopySpan;
    default: return -1;
    }
}

int64_t emu_packed_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t round_blocks) { return framing::encode_packed_scratch_bytes(n, slot_bytes, round_blocks); }
int emu_packed_copy_grid(int64_t bytes) { return (int)framing::copy_grid(bytes).groups; }

// framing::encode_packed, front and sequence, on a scratch buffer the test brings
int emu_encode_packed(const lz4hip_batch_t* b, int mode, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* packed_len,
                      void* scratch, int64_t scratch_bytes, lz4hip_packed_info_t* info, PackedEmuRun* r)
{
    PackedBackend be = backend_of(r);
    return finish(be, framing::encode_packed(be, b, mode, round_blocks, dst, dst_cap, dst_off, packed_len, scratch, scratch_bytes, info), &r->counters);
}

// hostbatch::encode_packed_host over the emulated image; pool_floor < 0: the library's limit for gathering on the row pool
int emu_encode_packed_host(const lz4hip_batch_t* b, int mode, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* packed_len,
                           lz4hip_packed_info_t* info, int64_t pool_floor, PackedEmuRun* r)
{
    PackedBackend be = backend_of(r);
    hostbatch::HostLimits limits;
    if (pool_floor >= 0) limits.pool_floor = pool_floor;
    return finish(be, hostbatch::encode_packed_host(be, b, mode, round_blocks, dst, dst_cap, dst_off, packed_len, info, 2, limits), &r->counters);
}

}  // extern "C"
