// emu_stream.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// C entry points that run the framing kernels (lz4hip_stream.hpp, lz4hip_wrap.hpp, lz4hip_streams.hpp) under the SIMT emulator
// for tests/test_simt_framing.py: single kernels, and the library's own host code for the framing paths (lz4hip_framing.hpp: layouts,
// grids, kernel sequences and the staging of the host-pointer calls) over EmuBackend, with the block codec step replaced by arrays the
// test hands in and the device image served from host memory.  The argument structs are passed by pointer; tests/emu_helpers.py mirrors
// them with ctypes and checks the sizes against emu_framing_sizeof().  A grid argument of 0 means "the library's formula".

template <class Call>
int emu_host_run(EmuHostRun* r, Call call)
{
    EmuBackend be = backend(r->grid_items, r->grid_copy, r->grid_walk, r->results, r->bytes);
    return finish(be, call(be), &r->counters);
}

extern "C" {

int64_t emu_framing_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(StreamEncodeArgs);
    case 1: return sizeof(StreamTables);
    case 2: return sizeof(StreamInfo);
    case 3: return sizeof(WrapArgs);
    case 4: return sizeof(UnwrapTables);
    case 5: return sizeof(UnwrapArgs);
    case 6: return sizeof(UnwrapInfo);
    case 7: return sizeof(StreamsEncodeArgs);
    case 8: return sizeof(StreamsTables);
    case 9: return sizeof(StreamsDecodeArgs);
    case 10: return sizeof(StreamsInfo);
    case 11: return sizeof(EmuHostRun);
    case 12: return sizeof(EmuCounters);
    case 100: return kScanTile;
    case 101: return kCopySpan;
    default: return -1;
    }
}

// the library's grid formulas, for the entries below that take an explicit grid
int emu_items_grid(int64_t items) { return (int)framing::stream_grid(items).groups; }
int emu_copy_grid(int64_t bytes) { return (int)framing::copy_grid(bytes).groups; }
int emu_walk_grid(int64_t n) { return (int)framing::walk_grid(n).groups; }

// ---- single kernels ----------------------------------------------------------------------------------------------------------
void emu_scan(int64_t* x, int64_t n, int64_t* partial, int64_t* total)
{
    EmuBackend be;
    framing::launch_scan(be, x, n, partial, total);
}

void emu_stream_index(const uint8_t* src, int64_t src_len, const StreamTables* t, StreamInfo* info)
{
    const StreamTables tt = *t;
    simt::launch(dim3(1), dim3(64), 0, [=] { stream_index_kernel(src, src_len, tt, info); });
}

void emu_copy_encode(const StreamEncodeArgs* a, uint8_t* dst, const int64_t* total, int grid)
{
    EncodeLayout L = { *a };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { stream_pack_kernel(L, dst, total); });
}

void emu_copy_raw(const uint8_t* src, const StreamTables* t, int64_t n, uint8_t* dst, int64_t end, int grid)
{
    RawLayout L = { src, *t, n };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { stream_raw_copy_kernel(L, dst, end); });
}

void emu_copy_wrap(const WrapArgs* a, uint8_t* dst, int64_t cap, int grid)
{
    WrapLayout L = { *a };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { wrap_pack_kernel(L, dst, cap); });
}

void emu_copy_unwrap_raw(const UnwrapArgs* a, const UnwrapTables* t, uint8_t* dst, int64_t end, int grid)
{
    UnwrapRawLayout L = { *a, *t };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { wrap_raw_copy_kernel(L, dst, end); });
}

void emu_copy_streams(const StreamsEncodeArgs* a, uint8_t* dst, int64_t cap, int grid)
{
    StreamsEncodeLayout L = { *a };
    simt::launch(dim3((unsigned)grid), dim3(kStreamThreads), 0, [=] { streams_pack_kernel(L, dst, cap); });
}

void emu_streams_walk(int fill, const StreamsDecodeArgs* a, const StreamsTables* t, int grid)
{
    const StreamsDecodeArgs aa = *a;
    const StreamsTables tt = *t;
    const unsigned g = grid > 0 ? (unsigned)grid : framing::walk_grid(aa.n).groups;
    if (fill) simt::launch(dim3(g), dim3(64), 0, [=] { streams_walk_kernel<true>(aa, tt); });
    else      simt::launch(dim3(g), dim3(64), 0, [=] { streams_walk_kernel<false>(aa, tt); });
}

void emu_stream_check(const StreamTables* t, int64_t n, int grid)
{
    const StreamTables tt = *t;
    simt::launch(dim3(grid > 0 ? (unsigned)grid : framing::stream_grid(n).groups), dim3(kStreamThreads), 0, [=] { stream_check_kernel(tt, n); });
}

// ---- the sequences of lz4hip_framing.hpp over the test's own arrays ------------------------------------------------------------------
// stream_encode without the block encoder: a->result and a->comp are the test's
void emu_stream_encode(const StreamEncodeArgs* a, int32_t* lens, int64_t* partial, uint8_t* dst, int64_t* dst_len, int64_t bound,
                       int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy);
    framing::stream_encode_run(be, *a, LZ4HIP_MODE_FAST, lens, partial, dst, dst_len);
}

// stream_index + stream_decode: results[j] / decoded stand for the block decoder on row j.  Returns 0, or 1 when the index reported a
// full table (stream_decode refuses that info).
int emu_stream_decode(const uint8_t* src, int64_t src_len, const StreamTables* t, const int32_t* results, const uint8_t* decoded,
                      uint8_t* dst, StreamInfo* index_info, StreamInfo* info, int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy, 0, results, decoded);
    framing::stream_index_run(be, src, src_len, *t, index_info);
    if (index_info->error == kStreamTableFull) return 1;
    framing::stream_decode_run(be, src, *index_info, *t, dst, info);
    return 0;
}

// wrap_encode without the block encoder: a->enc and a->comp are the test's
void emu_wrap(const WrapArgs* a, int64_t* at, int32_t* lens, int32_t* result, int64_t* partial, uint8_t* dst, int64_t cap, int64_t bound,
              int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy);
    framing::wrap_encode_run(be, *a, LZ4HIP_MODE_FAST, at, lens, result, partial, dst, cap);
}

void emu_unwrap_index(const UnwrapArgs* a, const UnwrapTables* t, UnwrapInfo* info, int grid_items)
{
    EmuBackend be = backend(grid_items, 0);
    framing::unwrap_index_run(be, *a, *t, info);
}

// unwrap_decode on the tables emu_unwrap_index left
void emu_unwrap_decode(const UnwrapArgs* a, const UnwrapTables* t, const UnwrapInfo* index_info, const int32_t* results, const uint8_t* decoded,
                       uint8_t* dst, UnwrapInfo* info, int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy, 0, results, decoded);
    framing::unwrap_decode_run(be, *a, *t, *index_info, dst, info);
}

// streams_encode in its two parts: the chunk table, then (a->result and a->comp filled by the test) the pack
void emu_streams_plan(const StreamsEncodeArgs* a, int64_t* partial, int grid_items)
{
    EmuBackend be = backend(grid_items, 0);
    framing::streams_encode_plan(be, *a, partial);
}

void emu_streams_pack(const StreamsEncodeArgs* a, int64_t* partial, int64_t* dst_off, uint8_t* dst, int64_t cap, int64_t bound,
                      int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy);
    framing::streams_encode_pack(be, *a, partial, dst_off, dst, cap);
}

void emu_streams_index(const StreamsDecodeArgs* a, const StreamsTables* t, StreamsInfo* info, int grid_walk)
{
    EmuBackend be = backend(0, 0, grid_walk);
    framing::streams_index_run(be, *a, *t, info);
}

// streams_decode on the tables emu_streams_index left; returns 1 for a full table
int emu_streams_decode(const StreamsDecodeArgs* a, const StreamsTables* t, const StreamsInfo* index_info, const int32_t* results,
                       const uint8_t* decoded, uint8_t* dst, StreamsInfo* info, int grid_items, int grid_copy)
{
    if (index_info->error == kStreamTableFull) return 1;
    EmuBackend be = backend(grid_items, grid_copy, 0, results, decoded);
    framing::streams_decode_run(be, *a, *t, *index_info, dst, info);
    return 0;
}

// ---- the whole functions of lz4hip_framing.hpp (front and sequence) on a scratch buffer the test brings -----------------------------
// The library's argument lists, then the block codec's stand-in (results, bytes) and the grids.
int64_t emu_scratch_bytes(int which, int64_t a, int64_t b, int64_t c)
{
    switch (which) {
    case 0: return framing::stream_encode_scratch(nullptr, a, framing::stream_block((int32_t)b)).bytes;      // (src_len, block_size)
    case 1: return framing::stream_decode_scratch_bytes(a);                                                   // (max_chunks)
    case 2: return framing::wrap_scratch(nullptr, a, b).bytes;                                                // (n, src_len)
    case 3: return framing::unwrap_scratch_bytes(a);                                                          // (n)
    case 4: return framing::streams_encode_scratch(nullptr, a, b, framing::stream_block((int32_t)c)).bytes;  // (n, src_len, block_size)
    case 5: return framing::streams_decode_scratch_bytes(a, b);                                               // (n, max_chunks)
    default: return -1;
    }
}

int emu_lib_stream_encode(const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len,
                          void* scratch, int64_t scratch_bytes, const int32_t* results, const uint8_t* bytes, int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy, 0, results, bytes);
    return framing::stream_encode(be, src, src_len, block_size, mode, dst, dst_cap, dst_len, scratch, scratch_bytes);
}

int emu_lib_stream_index(const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes, lz4hip_stream_info_t* info)
{
    EmuBackend be;
    return framing::stream_index(be, src, src_len, max_chunks, scratch, scratch_bytes, info);
}

int emu_lib_stream_decode(const void* src, const lz4hip_stream_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                          void* dst, int64_t dst_cap, lz4hip_stream_info_t* info, const int32_t* results, const uint8_t* bytes,
                          int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy, 0, results, bytes);
    return framing::stream_decode(be, src, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, info);
}

int emu_lib_wrap(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode, void* dst, int64_t dst_cap, int64_t* dst_off,
                 int32_t* result, void* scratch, int64_t scratch_bytes, const int32_t* results, const uint8_t* bytes, int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy, 0, results, bytes);
    return framing::wrap_encode(be, src, src_len, src_off, n, mode, dst, dst_cap, dst_off, result, scratch, scratch_bytes);
}

int emu_lib_unwrap_index(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t* dst_off, int32_t* status,
                         void* scratch, int64_t scratch_bytes, lz4hip_unwrap_info_t* info, int grid_items)
{
    EmuBackend be = backend(grid_items, 0);
    return framing::unwrap_index(be, src, src_len, src_off, n, dst_off, status, scratch, scratch_bytes, info);
}

int emu_lib_unwrap_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const lz4hip_unwrap_info_t* info_host,
                          void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, const int64_t* dst_off, int32_t* status,
                          lz4hip_unwrap_info_t* info, const int32_t* results, const uint8_t* bytes, int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy, 0, results, bytes);
    return framing::unwrap_decode(be, src, src_len, src_off, n, info_host, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info);
}

int emu_lib_streams_encode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode, void* dst,
                           int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, const int32_t* results, const uint8_t* bytes,
                           int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy, 0, results, bytes);
    return framing::streams_encode(be, src, src_len, src_off, n, block_size, mode, dst, dst_cap, dst_off, scratch, scratch_bytes);
}

int emu_lib_streams_index(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks, int64_t* dst_off,
                          int32_t* status, int64_t* error_offset, void* scratch, int64_t scratch_bytes, lz4hip_streams_info_t* info, int grid_walk)
{
    EmuBackend be = backend(0, 0, grid_walk);
    return framing::streams_index(be, src, src_len, src_off, n, max_chunks, dst_off, status, error_offset, scratch, scratch_bytes, info);
}

int emu_lib_streams_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const lz4hip_streams_info_t* info_host,
                           int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, const int64_t* dst_off,
                           int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info, const int32_t* results, const uint8_t* bytes,
                           int grid_items, int grid_copy)
{
    EmuBackend be = backend(grid_items, grid_copy, 0, results, bytes);
    return framing::streams_decode(be, src, src_len, src_off, n, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, dst_off, status,
                                   error_offset, info);
}

// ---- the host-pointer calls of lz4hip_framing.hpp: the library's argument lists, then an EmuHostRun ------------------------------------
int emu_host_stream_encode(const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len, EmuHostRun* r)
{
    return emu_host_run(r, [&](EmuBackend& be) { return framing::stream_encode_host(be, src, src_len, block_size, mode, dst, dst_cap, dst_len); });
}

int emu_host_stream_decode(const void* src, int64_t src_len, void* dst, int64_t dst_cap, lz4hip_stream_info_t* info, EmuHostRun* r)
{
    return emu_host_run(r, [&](EmuBackend& be) { return framing::stream_decode_host(be, src, src_len, dst, dst_cap, info); });
}

int emu_host_wrap(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode, void* dst, int64_t dst_cap, int64_t* dst_off,
                  int32_t* result, EmuHostRun* r)
{
    return emu_host_run(r, [&](EmuBackend& be) { return framing::wrap_host(be, src, src_len, src_off, n, mode, dst, dst_cap, dst_off, result); });
}

int emu_host_unwrap(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status,
                    lz4hip_unwrap_info_t* info, EmuHostRun* r)
{
    return emu_host_run(r, [&](EmuBackend& be) { return framing::unwrap_host(be, src, src_len, src_off, n, dst, dst_cap, dst_off, status, info); });
}

int emu_host_streams_encode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode, void* dst,
                            int64_t dst_cap, int64_t* dst_off, EmuHostRun* r)
{
    return emu_host_run(r, [&](EmuBackend& be) {
        return framing::streams_encode_host(be, src, src_len, src_off, n, block_size, mode, dst, dst_cap, dst_off);
    });
}

int emu_host_streams_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* dst, int64_t dst_cap, int64_t* dst_off,
                            int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info, EmuHostRun* r)
{
    return emu_host_run(r, [&](EmuBackend& be) {
        return framing::streams_decode_host(be, src, src_len, src_off, n, dst, dst_cap, dst_off, status, error_offset, info);
    });
}

}  // extern "C"
