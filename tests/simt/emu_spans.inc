// emu_spans.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The span forms of the one-call decodes (lz4net_amd/csrc/lz4hip_framing.hpp: unwrap_spans_into, streams_decode_spans_into), the
// selection kernel (spans_select) and the chunk directory of one stream (stream_directory) under the SIMT emulator, for
// tests/test_simt_spans.py.  The decoder stand-in, its run record and the consecutive forms' entry points (emu_unwrap_into,
// emu_streams_decode_into) are emu_into.inc's: the identity cases compare the two forms under one emulator and one stand-in.

extern "C" {

int emu_unwrap_spans_into(const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m, void* scratch,
                          int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info,
                          int64_t* written_messages, IntoEmuRun* r)
{
    IntoBackend be = backend_of(r);
    return finish(be, framing::unwrap_spans_into(be, src, src_len, src_begin, src_end, m, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info,
                                                 written_messages), &r->counters);
}

int emu_streams_decode_spans_into(const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m,
                                  int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off,
                                  int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info, int64_t* written_items, IntoEmuRun* r)
{
    IntoBackend be = backend_of(r);
    return finish(be, framing::streams_decode_spans_into(be, src, src_len, src_begin, src_end, m, max_chunks, scratch, scratch_bytes, dst, dst_cap,
                                                         dst_off, status, error_offset, info, written_items), &r->counters);
}

// grid > 0 replaces the formula's answer
int emu_spans_select(const int64_t* src_off, int64_t n, const int64_t* sel, int64_t m, int64_t* src_begin, int64_t* src_end, int grid)
{
    EmuBackend be = backend(grid, 0);
    return framing::spans_select(be, src_off, n, sel, m, src_begin, src_end);
}

int emu_stream_directory(const void* src, int64_t src_len, int64_t max_chunks, int64_t* hdr_off, int64_t* out_off, lz4hip_stream_info_t* info)
{
    EmuBackend be;
    return framing::stream_directory(be, src, src_len, max_chunks, hdr_off, out_off, info);
}

// the index's info for the same stream: what the directory's must equal
int emu_spans_stream_index(const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes, lz4hip_stream_info_t* info)
{
    EmuBackend be;
    return framing::stream_index(be, src, src_len, max_chunks, scratch, scratch_bytes, info);
}

}  // extern "C"
