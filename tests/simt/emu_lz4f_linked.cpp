// emu_lz4f_linked.cpp -- TEST INFRASTRUCTURE ONLY.
// libsimt_lz4f_linked.so: the decode of LZ4 frames with linked blocks (lz4net_amd/csrc/lz4hip_lz4f_linked.hpp inside the sequences
// lz4f_decode and lz4f_batch_decode of lz4hip_framing.hpp, and their host-pointer calls) compiled against the SIMT emulator, for
// tests/test_simt_lz4f_linked.py and tests/cpp/lz4f_linked_asan_main.cpp.  It is emu_lz4f_batch.cpp -- its emulated device, its run
// record, its stand-in block codec keyed by global table row, which the INDEPENDENT rows keep -- with the one thing the linked decode
// needs and that unit's launches do not have: a workgroup's LDS as large as the wavefront decoder's rings.  The linked rows are decoded
// by the real decode_block under the emulator; the stand-in sees them as the empty rows the sequence promises.  Also the one-frame
// sequence over the same backend.  Built with g++ by tests/lz4f_linked_cases.py through build_emu._build, never shipped.
#include "emu_lz4f_batch.cpp"

namespace {

static_assert(kWaveDecodeWavesPerGroup * kWaveLdsBytes >= kSizesLdsBytes && kWaveDecodeWavesPerGroup * kWaveLdsBytes >= kStreamThreads * 8,
              "one LDS size serves every kernel of the sequences");

Lz4fBatchBackend linked_backend_of(Lz4fBatchEmuRun* r)
{
    Lz4fBatchBackend be = backend_of(r);
    be.lds_bytes = (size_t)kWaveDecodeWavesPerGroup * kWaveLdsBytes;
    return be;
}

}  // namespace

extern "C" {

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
