// emu_sizes.cpp -- TEST INFRASTRUCTURE ONLY.
// The size query of a block batch (lz4net_amd/csrc/lz4hip_sizes.hpp) under the SIMT emulator, for tests/test_decoded_sizes.py: the real
// kernels, the library's own launch sequence and argument checks (lz4hip_framing.hpp: decoded_sizes) and its host-pointer call
// (lz4hip_hostbatch.hpp: decoded_sizes_host) over the emulated device of emu_framing.hpp.  Built with g++ by build_emu_sizes.py into a
// library of its own, never shipped.
#include "simt_wave.hpp"

#include "lz4hip_common.hpp"

using namespace lz4hip;

#include "emu_framing.hpp"
#include "lz4hip_hostbatch.hpp"

namespace {

// EmuBackend with the LDS the walk's workgroup has on the device (the scan kernels need less)
struct SizesBackend : emu_framing::EmuBackend {
    template <class... P, class... A>
    void launch(void (*kernel)(P...), framing::Grid grid, unsigned threads, A&&... a)
    {
        simt::launch(dim3(grid.groups), dim3(threads), kSizesLdsBytes, emu_framing::KernelCall<P...>{ kernel, std::tuple<P...>{ P(a)... } });
    }
};

}  // namespace

extern "C" {

int64_t emu_sizes_window(void) { return kSizesWindow; }
int64_t emu_sizes_scratch_bytes(int64_t n) { return framing::sizes_scratch_bytes(n); }

// framing::decoded_sizes, front and sequence, on a scratch buffer the test brings; groups = 0: the library's grid
int emu_decoded_sizes(const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap, void* scratch, int64_t scratch_bytes, lz4hip_sizes_info_t* info,
                      int groups, char* error, int error_bytes)
{
    SizesBackend be;
    const int rc = framing::decoded_sizes(be, b, dst_off, dst_cap, scratch, scratch_bytes, info, groups);
    snprintf(error, (size_t)error_bytes, "%s", be.error.c_str());
    return rc;
}

// hostbatch::decoded_sizes_host over the emulated stage; pool_floor < 0: the library's limit for gathering on the row pool
int emu_decoded_sizes_host(const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap, lz4hip_sizes_info_t* info, int groups, int64_t pool_floor,
                           EmuHostRun* r)
{
    SizesBackend be;
    hostbatch::HostLimits limits;
    if (pool_floor >= 0) limits.pool_floor = pool_floor;
    const int rc = hostbatch::decoded_sizes_host(be, b, dst_off, dst_cap, info, groups, 2, limits);
    r->intact = be.intact();
    r->reserves = be.reserves; r->moves = be.moves; r->uploads = be.uploads; r->downloads = be.downloads; r->syncs = be.syncs; r->passes = be.passes;
    r->image_bytes = be.blocks.empty() ? 0 : (int64_t)be.blocks.back().bytes;
    snprintf(r->error, sizeof r->error, "%s", be.error.c_str());
    return rc;
}

}  // extern "C"
