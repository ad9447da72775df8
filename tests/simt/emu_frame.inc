// emu_frame.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The legacy frame path (lz4net_amd/csrc/lz4hip_frame.hpp) under the SIMT emulator, for tests/test_simt_frame.py: the real kernels, the
// library's own fronts and launch sequences (lz4hip_framing.hpp: frame_encode / frame_index / frame_decode and their _plan / _run
// halves) and its host-pointer calls (frame_encode_host / frame_decode_host) over the emulated device of emu_framing.hpp with its moving
// image.  The block codec is EmuBackend's stand-in: results and bytes the test computed with the oracle.

namespace {

// EmuBackend with the LDS the size walk's workgroup has on the device; `grid` > 0 replaces every formula's answer: the item kernels',
// the copy kernels' and (handed to the front) the size walk's
EmuBackend frame_backend(int grid, const int32_t* results, const uint8_t* bytes)
{
    EmuBackend be = backend(grid, grid, 0, results, bytes);
    be.lds_bytes = kSizesLdsBytes;
    return be;
}

}  // namespace

extern "C" {

int64_t emu_frame_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(FrameTables);
    case 1: return sizeof(FrameInfo);
    case 2: return sizeof(EmuHostRun);
    default: return -1;
    }
}

int64_t emu_frame_bound(int64_t src_len, int32_t chunk_size) { return framing::frame_bound(src_len, chunk_size); }
int64_t emu_frame_encode_scratch_bytes(int64_t src_len, int32_t chunk_size)
{
    return framing::frame_encode_scratch(nullptr, src_len, framing::frame_chunk(chunk_size)).bytes;
}
int64_t emu_frame_decode_scratch_bytes(int64_t max_chunks) { return framing::frame_decode_scratch_bytes(max_chunks); }

// where the index keeps its table in a scratch buffer
void emu_frame_tables(void* scratch, int64_t max_chunks, FrameTables* t)
{
    framing::Carver c(scratch);
    *t = framing::frame_tables(c, max_chunks);
}

// ---- the fronts with their sequences: the library's argument lists, then the codec's stand-in, the grid and the failure text ----------
int emu_frame_encode(const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len, void* scratch,
                     int64_t scratch_bytes, const int32_t* results, const uint8_t* bytes, int grid, char* error, int error_bytes)
{
    EmuBackend be = frame_backend(grid, results, bytes);
    return finish(be, framing::frame_encode(be, src, src_len, chunk_size, mode, dst, dst_cap, dst_len, scratch, scratch_bytes), error, error_bytes);
}

int emu_frame_index(const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                    lz4hip_frame_info_t* info, int grid, char* error, int error_bytes)
{
    EmuBackend be = frame_backend(grid, nullptr, nullptr);
    return finish(be, framing::frame_index(be, src, src_len, chunk_size, max_chunks, scratch, scratch_bytes, info, grid), error, error_bytes);
}

// results[k] / bytes + dst_off[k] stand for the block decoder on row k
int emu_frame_decode(const void* src, const lz4hip_frame_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst,
                     int64_t dst_cap, lz4hip_frame_info_t* info, const int32_t* results, const uint8_t* bytes, int grid, char* error, int error_bytes)
{
    EmuBackend be = frame_backend(grid, results, bytes);
    return finish(be, framing::frame_decode(be, src, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, info), error, error_bytes);
}

// ---- the sequences alone, over a table the test laid out (emu_frame_tables) --------------------------------------------------------------
int emu_frame_index_run(const uint8_t* src, int64_t src_len, int32_t chunk, const FrameTables* t, FrameInfo* info, int grid)
{
    EmuBackend be = frame_backend(grid, nullptr, nullptr);
    const framing::FrameIndexPlan p = { src, src_len, chunk, *t, info, grid };
    return framing::frame_index_run(be, p);
}

int emu_frame_decode_run(const uint8_t* src, const FrameInfo* index_info, const FrameTables* t, uint8_t* dst, FrameInfo* info, const int32_t* results,
                         const uint8_t* bytes, int grid)
{
    EmuBackend be = frame_backend(grid, results, bytes);
    const framing::FrameDecodePlan p = { src, *index_info, *t, dst, info };
    return framing::frame_decode_run(be, p);
}

// ---- the host-pointer calls: the library's argument lists, then an EmuHostRun (grid_items: the grid of every formula) ---------------------
int emu_host_frame_encode(const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len, EmuHostRun* r)
{
    EmuBackend be = frame_backend(r->grid_items, r->results, r->bytes);
    return finish(be, framing::frame_encode_host(be, src, src_len, chunk_size, mode, dst, dst_cap, dst_len), &r->counters);
}

int emu_host_frame_decode(const void* src, int64_t src_len, int32_t chunk_size, void* dst, int64_t dst_cap, lz4hip_frame_info_t* info, EmuHostRun* r)
{
    EmuBackend be = frame_backend(r->grid_items, r->results, r->bytes);
    return finish(be, framing::frame_decode_host(be, src, src_len, chunk_size, dst, dst_cap, info), &r->counters);
}

}  // extern "C"
