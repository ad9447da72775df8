// emu_dict.cpp -- TEST INFRASTRUCTURE ONLY.
// libsimt_dict.so: the decode of block batches against a shared dictionary (decode_block's DICT mode and decode_dict_kernel of
// lz4net_amd/csrc/lz4hip_decode.hpp, sizes_walk_dict_kernel through framing::decoded_sizes, and the host-pointer call's upload and slice
// loop of lz4hip_hostbatch.hpp) compiled against the SIMT emulator, for tests/test_simt_dict_decode.py and
// tests/cpp/dict_decode_asan_main.cpp.  It is emu_kernels.cpp -- its kernels, its counters, its EmuStage -- with the counters of the DICT
// mode behind LZ4HIP_STAT_DICT, which expands to nothing in every other build.  Built with g++ by build_emu.py (build_dict), never
// shipped.
static unsigned long long g_dict_stat[16];    // lz4hip::DictStat: where the bytes before the block came from, per lane
#define LZ4HIP_STAT_DICT(slot, n) do { g_dict_stat[slot] += (unsigned long long)(n); } while (0)

#include "emu_kernels.cpp"
#include "emu_framing.hpp"

// what the stage of an emu_dict_host call saw of the dictionary
struct EmuDictHost {
    int64_t uploads, bytes;                   // dict_upload calls, and the bytes of the last one
    int64_t log_at_upload, kernels_at_upload; // the stage's records and kernels calls when it came: before everything else is 0 and 0
    int64_t intact;                           // the guard bytes around the dictionary's device copy after the call
    int64_t first_byte_offset;                // which byte of the caller's dictionary the copy starts with
};

namespace emu_dict {

using namespace lz4hip;

static_assert(kDictStats <= 16, "g_dict_stat");

// the library's launch (launch_decode_dict of lz4hip_api.hip): the reachable bytes, the dictionary's end, four wavefronts a workgroup
inline void launch(const Batch& d, const uint8_t* dict, int64_t dict_len, int known, unsigned wpg)
{
    const int reach = (int)hostbatch::dict_reach(dict_len);
    const uint8_t* dict_end = reach > 0 ? dict + dict_len : nullptr;
    dim3 grid((unsigned)((d.n_blocks + wpg - 1) / wpg)), block(64 * wpg);
    const size_t lds = (size_t)wpg * kWaveLdsBytes;
    if (known) simt::launch(grid, block, lds, [=] { decode_dict_kernel<true>(d, dict_end, reach); });
    else       simt::launch(grid, block, lds, [=] { decode_dict_kernel<false>(d, dict_end, reach); });
}

// EmuStage with the dictionary's staging: exactly the bytes asked for between guard bytes
struct DictStage : emu_hostbatch::EmuStage {
    EmuDictHost& d;
    const uint8_t* caller_dict;
    std::vector<uint8_t> store;
    DictStage(EmuHostBatch& run, EmuDictHost& dict_run, const uint8_t* dict) : emu_hostbatch::EmuStage(run), d(dict_run), caller_dict(dict) { memset(&d, 0, sizeof d); d.intact = 1; }
    int dict_upload(const uint8_t* from, int64_t bytes, uint8_t*& dev)
    {
        d.uploads++; d.bytes = bytes; d.log_at_upload = r.log_n; d.kernels_at_upload = r.kernel_calls;
        d.first_byte_offset = from - caller_dict;
        store.assign((size_t)bytes + 2 * kGuard, kGuardByte);
        memcpy(store.data() + kGuard, from, (size_t)bytes);
        dev = store.data() + kGuard;
        return 0;
    }
    bool dict_intact() const
    {
        for (size_t g = 0; g < kGuard && !store.empty(); g++)
            if (store[g] != kGuardByte || store[store.size() - 1 - g] != kGuardByte) return false;
        return true;
    }
};

}  // namespace emu_dict

extern "C" {

void emu_dict_decode(int known, const uint8_t* src, int64_t src_stride, const int32_t* src_len, uint8_t* dst, int64_t dst_stride, const int32_t* dst_cap,
                     int32_t* result, int64_t n, int waves_per_group, const uint8_t* dict, int64_t dict_len)
{
    emu_dict::launch(make_batch(src, src_stride, src_len, dst, dst_stride, dst_cap, result, n), dict, dict_len, known, (unsigned)waves_per_group);
}

// the same over rows at offsets (every row in an allocation of its own)
void emu_dict_decode_at(int known, const uint8_t* src, const int64_t* src_off, const int32_t* src_len, uint8_t* dst, const int64_t* dst_off,
                        const int32_t* dst_cap, int32_t* result, int64_t n, int waves_per_group, const uint8_t* dict, int64_t dict_len)
{
    Batch b = make_batch(src, 0, src_len, dst, 0, dst_cap, result, n);
    b.src_off = src_off; b.dst_off = dst_off;
    emu_dict::launch(b, dict, dict_len, known, (unsigned)waves_per_group);
}

void emu_dict_stats(unsigned long long* out, int reset)
{
    for (int i = 0; i < lz4hip::kDictStats; i++) { out[i] = g_dict_stat[i]; if (reset) g_dict_stat[i] = 0; }
}

int64_t emu_dict_sizes_scratch_bytes(int64_t n) { return lz4hip::framing::sizes_scratch_bytes(n); }

// lz4hip_decoded_sizes_dict_device over the emulated device
int emu_dict_sizes(const lz4hip_batch_t* b, int64_t dict_len, int64_t* dst_off, int32_t* dst_cap, void* scratch, int64_t scratch_bytes,
                   lz4hip_sizes_info_t* info, int groups, char* error)
{
    emu_framing::EmuBackend be;
    be.lds_bytes = lz4hip::kSizesLdsBytes;
    return emu_framing::finish(be, lz4hip::framing::decoded_sizes(be, b, dst_off, dst_cap, scratch, scratch_bytes, info, groups, dict_len), error, 160);
}

// lz4hip_decode_batch_dict_host: the library's upload and slice loop over the stage, the slices' kernels under the emulator
int emu_dict_host(const lz4hip_batch_t* hb, const uint8_t* dict, int64_t dict_len, int known, int waves_per_group, EmuHostBatch* r, EmuDictHost* d)
{
    using namespace lz4hip;
    emu_dict::DictStage st(*r, *d, dict);
    r->error[0] = 0;
    const unsigned wpg = (unsigned)waves_per_group;
    auto make_run = [known, wpg](const uint8_t* d_dict, int64_t reach) {
        return [=](const lz4hip_batch_t* db, int64_t) { emu_dict::launch(emu_framing::device_batch(db), d_dict, reach, known, wpg); return 0; };
    };
    const int rc = hostbatch::run_host_batch_dict(st, hb, dict, dict_len, !known, make_run, r->slices_knob, 1, emu_hostbatch::limits_of(*r));
    r->intact = st.intact();
    d->intact = st.dict_intact();
    snprintf(r->error, sizeof r->error, "%s", st.error.c_str());
    return rc;
}

int64_t emu_dict_sizeof(int which) { return which == 0 ? (int64_t)sizeof(EmuDictHost) : (int64_t)sizeof(EmuHostBatch); }

}  // extern "C"
