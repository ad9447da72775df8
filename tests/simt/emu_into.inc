// emu_into.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The one-call decodes of an LZ4Stream buffer, of a batch of them and of wrapped messages (lz4net_amd/csrc/lz4hip_framing.hpp:
// stream_decode_into, streams_decode_into, unwrap_into -- fronts and sequences -- over the clip, check and copy kernels of
// lz4hip_stream.hpp, lz4hip_streams.hpp and lz4hip_wrap.hpp) under the SIMT emulator, for tests/test_simt_into.py.  The block decoder
// is a stand-in fed the test's results and bytes; it also VERIFIES what it is handed: one known-size call over the whole table, every
// row past the count and every clipped row an empty block of capacity 0, every other row with its own offsets, length and capacity.

// what the emulated device is to do, and what it did
struct IntoEmuRun {
    const int32_t* results;      // per row of the compressed table below `count`: what the known-size decoder returns for it
    const uint8_t* bytes;        // the decoder's output, every row's at the row's own output offset
    const int64_t* src_off;      // per row below `count`: the offsets the decoder must be handed ...
    const int64_t* dst_off;
    const int32_t* len;          // ... and, for ALL `rows` rows, the length and capacity: (0, 0) for a clipped row and past the count
    const int32_t* cap;
    int64_t rows, count;         // the table's size; the rows the index fills (0 on TABLE_FULL)
    int32_t grid_items, grid_copy, grid_walk, pad;   // > 0 replaces the formula's answer
    int64_t calls, shape_errors, decoded_rows;       // decoder calls, rows or descriptors that were not as promised, rows given bytes
    EmuCounters counters;
};

namespace {

struct IntoBackend : EmuBackend {
    IntoEmuRun* r = nullptr;

    // a (0, 0) row gets -1 and not a byte, as the known-size decoders answer it
    int decode(const lz4hip_batch_t* b, int known)
    {
        r->calls++;
        if (known != 1 || b->n_blocks != r->rows || !b->src || !b->dst || !b->src_off || !b->dst_off || !b->src_len || !b->dst_cap || !b->result ||
            b->src_stride || b->dst_stride) { r->shape_errors++; return 0; }
        for (int64_t j = 0; j < b->n_blocks; j++) {
            const int32_t len = b->src_len[j], cap = b->dst_cap[j];
            if (len != r->len[j] || cap != r->cap[j]) { r->shape_errors++; continue; }
            if (j >= r->count) {
                if (len != 0 || cap != 0 || b->src_off[j] != 0 || b->dst_off[j] != 0) r->shape_errors++;
                b->result[j] = -1;
                continue;
            }
            if (b->src_off[j] != r->src_off[j] || b->dst_off[j] != r->dst_off[j]) { r->shape_errors++; continue; }
            if (len == 0 && cap == 0) { b->result[j] = -1; continue; }
            memcpy((uint8_t*)b->dst + b->dst_off[j], r->bytes + b->dst_off[j], (size_t)cap);
            b->result[j] = r->results[j];
            r->decoded_rows++;
        }
        return 0;
    }
};

IntoBackend backend_of(IntoEmuRun* r)
{
    IntoBackend be = backend<IntoBackend>(r->grid_items, r->grid_copy, r->grid_walk);
    be.r = r;
    return be;
}

}  // namespace

extern "C" {

int64_t emu_into_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(IntoEmuRun);
    case 1: return sizeof(StreamInfo);
    case 2: return sizeof(StreamsInfo);
    case 3: return sizeof(UnwrapInfo);
    default: return -1;
    }
}

// 0: the one stream (max_chunks), 1: the batch of streams (n, max_chunks), 2: unwrap (n); 10 .. 12: the two-call forms' sizes
int64_t emu_into_scratch_bytes(int which, int64_t a, int64_t b)
{
    switch (which) {
    case 0: return framing::stream_decode_into_scratch_bytes(a);
    case 1: return framing::streams_decode_into_scratch_bytes(a, b);
    case 2: return framing::unwrap_into_scratch_bytes(a);
    case 10: return framing::stream_decode_scratch_bytes(a);
    case 11: return framing::streams_decode_scratch_bytes(a, b);
    case 12: return framing::unwrap_scratch_bytes(a);
    default: return -1;
    }
}

int emu_stream_decode_into(const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                           lz4hip_stream_info_t* info, int64_t* written_bytes, IntoEmuRun* r)
{
    IntoBackend be = backend_of(r);
    return finish(be, framing::stream_decode_into(be, src, src_len, max_chunks, scratch, scratch_bytes, dst, dst_cap, info, written_bytes), &r->counters);
}

int emu_streams_decode_into(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks, void* scratch,
                            int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status, int64_t* error_offset,
                            lz4hip_streams_info_t* info, int64_t* written_items, IntoEmuRun* r)
{
    IntoBackend be = backend_of(r);
    return finish(be, framing::streams_decode_into(be, src, src_len, src_off, n, max_chunks, scratch, scratch_bytes, dst, dst_cap, dst_off, status,
                                                   error_offset, info, written_items), &r->counters);
}

int emu_unwrap_into(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* scratch, int64_t scratch_bytes, void* dst,
                    int64_t dst_cap, int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info, int64_t* written_messages, IntoEmuRun* r)
{
    IntoBackend be = backend_of(r);
    return finish(be, framing::unwrap_into(be, src, src_len, src_off, n, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info, written_messages), &r->counters);
}

}  // extern "C"
