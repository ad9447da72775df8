// emu_sizes.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The size query of a block batch (lz4net_amd/csrc/lz4hip_sizes.hpp) under the SIMT emulator, for tests/test_decoded_sizes.py: the real
// kernels, the library's own launch sequence and argument checks (lz4hip_framing.hpp: decoded_sizes) and its host-pointer call
// (lz4hip_hostbatch.hpp: decoded_sizes_host) over the emulated device of emu_framing.hpp.

namespace {

// EmuBackend with the LDS the walk's workgroup has on the device (the scan kernels need less)
EmuBackend sizes_backend()
{
    EmuBackend be;
    be.lds_bytes = kSizesLdsBytes;
    return be;
}

}  // namespace

extern "C" {

int64_t emu_sizes_window(void) { return kSizesWindow; }
int64_t emu_sizes_scratch_bytes(int64_t n) { return framing::sizes_scratch_bytes(n); }

// framing::decoded_sizes, front and sequence, on a scratch buffer the test brings; groups = 0: the library's grid
int emu_decoded_sizes(const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap, void* scratch, int64_t scratch_bytes, lz4hip_sizes_info_t* info,
                      int groups, char* error, int error_bytes)
{
    EmuBackend be = sizes_backend();
    return finish(be, framing::decoded_sizes(be, b, dst_off, dst_cap, scratch, scratch_bytes, info, groups), error, error_bytes);
}

// hostbatch::decoded_sizes_host over the emulated stage; pool_floor < 0: the library's limit for gathering on the row pool
int emu_decoded_sizes_host(const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap, lz4hip_sizes_info_t* info, int groups, int64_t pool_floor,
                           EmuHostRun* r)
{
    EmuBackend be = sizes_backend();
    hostbatch::HostLimits limits;
    if (pool_floor >= 0) limits.pool_floor = pool_floor;
    return finish(be, hostbatch::decoded_sizes_host(be, b, dst_off, dst_cap, info, groups, 2, limits), &r->counters);
}

}  // extern "C"
