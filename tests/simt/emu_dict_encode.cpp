// emu_dict_encode.cpp -- TEST INFRASTRUCTURE ONLY.
// libsimt_dict_encode.so: the encode of block batches against a shared dictionary (encode_dict_prime_kernel, encode_dict_kernel and
// encode_fast_block's DICT mode of lz4net_amd/csrc/lz4hip_encode_dict.hpp / lz4hip_encode.hpp, and the host-pointer call's upload, priming
// and slice loop of lz4hip_hostbatch.hpp) compiled against the SIMT emulator, for tests/test_simt_dict_encode.py and
// tests/cpp/dict_encode_asan_main.cpp.  It is emu_kernels.cpp -- its kernels, its EmuStage -- with the counters of the DICT mode behind
// LZ4HIP_STAT_ENCDICT, which expands to nothing in every other build.  Built with g++ by tests/dict_encode_lib.py, never shipped.
static unsigned long long g_encdict_stat[16];    // lz4hip::EncDictStat
#define LZ4HIP_STAT_ENCDICT(slot, n) do { g_encdict_stat[slot] += (unsigned long long)(n); } while (0)

#include "emu_kernels.cpp"
#include "lz4hip_encode_dict.hpp"
#include "emu_framing.hpp"

// what the stage of an emu_encdict_host call saw of the dictionary and its table
struct EmuEncDictHost {
    int64_t uploads, bytes;                   // dict_upload calls, and the bytes of the last one
    int64_t log_at_upload, kernels_at_upload; // the stage's records and kernels calls when it came: before everything else is 0 and 0
    int64_t first_byte_offset;                // which byte of the caller's dictionary the copy starts with
    int64_t primes, log_at_prime, kernels_at_prime, uploads_at_prime;
    int64_t intact;                           // the guard bytes around the dictionary's copy and around the table after the call
    int64_t table_unchanged;                  // the table after the call is the table dict_prime left
};

namespace emu_encdict {

using namespace lz4hip;

static_assert(kEncDictStats <= 16, "g_encdict_stat");

inline void prime(const uint8_t* dict, int64_t dict_len, uint8_t* table)
{
    const int reach = (int)hostbatch::dict_reach(dict_len);
    const uint8_t* dict_end = dict + dict_len;
    simt::launch(dim3(1), dim3(kEncDictPrimeThreads), kFastTableBytes, [=] { encode_dict_prime_kernel(dict_end, reach, table); });
}

// the library's launch (launch_encode_dict of lz4hip_api.hip) over a table already primed; wpg: 1 or 5 wavefronts a workgroup
inline void launch(const Batch& d, const uint8_t* dict, int64_t dict_len, const uint8_t* table, unsigned wpg)
{
    const int reach = (int)hostbatch::dict_reach(dict_len);
    const uint8_t* dict_end = dict + dict_len;
    if (wpg == 5) simt::launch(dim3((unsigned)((d.n_blocks + 4) / 5)), dim3(64 * 5), 5 * kFastTableBytes, [=] { encode_dict_kernel<5>(d, dict_end, reach, table); });
    else          simt::launch(dim3((unsigned)d.n_blocks), dim3(64), kFastTableBytes, [=] { encode_dict_kernel<1>(d, dict_end, reach, table); });
}

// lz4hip_encode_batch_dict_device: dict_len == 0 IS the plain call
inline void encode(const Batch& d, const uint8_t* dict, int64_t dict_len, uint8_t* table, unsigned wpg)
{
    if (d.n_blocks == 0) return;
    if (dict_len == 0) {
        if (wpg == 5) simt::launch(dim3((unsigned)((d.n_blocks + 4) / 5)), dim3(64 * 5), 5 * kFastTableBytes, [=] { encode_fast_kernel<2, 5>(d, 0); });
        else          simt::launch(dim3((unsigned)d.n_blocks), dim3(64), kFastTableBytes, [=] { encode_fast_kernel(d, 0); });
        return;
    }
    prime(dict, dict_len, table);
    launch(d, dict, dict_len, table, wpg);
}

// EmuStage with the dictionary's staging and the table's: exactly the bytes asked for between guard bytes
struct Stage : emu_hostbatch::EmuStage {
    EmuEncDictHost& d;
    const uint8_t* caller_dict;
    std::vector<uint8_t> store, table, table_then;
    Stage(EmuHostBatch& run, EmuEncDictHost& dict_run, const uint8_t* dict) : emu_hostbatch::EmuStage(run), d(dict_run), caller_dict(dict) { memset(&d, 0, sizeof d); d.intact = 1; }
    int dict_upload(const uint8_t* from, int64_t bytes, uint8_t*& dev)
    {
        d.uploads++; d.bytes = bytes; d.log_at_upload = r.log_n; d.kernels_at_upload = r.kernel_calls;
        d.first_byte_offset = from - caller_dict;
        store.assign((size_t)bytes + 2 * kGuard, kGuardByte);
        memcpy(store.data() + kGuard, from, (size_t)bytes);
        dev = store.data() + kGuard;
        return 0;
    }
    int dict_prime(const uint8_t* d_dict, int64_t reach, uint8_t*& dev)
    {
        d.primes++; d.log_at_prime = r.log_n; d.kernels_at_prime = r.kernel_calls; d.uploads_at_prime = d.uploads;
        table.assign((size_t)kFastTableBytes + 2 * kGuard + 16, kGuardByte);
        uint8_t* t = table.data() + kGuard;
        t += (16 - (uintptr_t)t % 16) % 16;
        prime(d_dict, reach, t);
        table_then.assign(t, t + kFastTableBytes);
        dev = t;
        return 0;
    }
    bool dict_intact() const
    {
        for (size_t g = 0; g < kGuard && !store.empty(); g++)
            if (store[g] != kGuardByte || store[store.size() - 1 - g] != kGuardByte) return false;
        for (size_t g = 0; g < kGuard && !table.empty(); g++)
            if (table[g] != kGuardByte || table[table.size() - 1 - g] != kGuardByte) return false;
        return true;
    }
    bool table_unchanged() const
    {
        if (table.empty()) return true;
        const uint8_t* t = table.data() + kGuard;
        t += (16 - (uintptr_t)t % 16) % 16;
        return memcmp(t, table_then.data(), kFastTableBytes) == 0;
    }
};

}  // namespace emu_encdict

extern "C" {

// the primed table alone: `table` gets 4096 x u32
void emu_encdict_prime(const uint8_t* dict, int64_t dict_len, uint8_t* table) { emu_encdict::prime(dict, dict_len, table); }

// lz4hip_encode_batch_dict_device over rows at a stride (src_off / dst_off NULL) or at offsets; `table`: the call's scratch
void emu_encdict_encode(const uint8_t* src, const int64_t* src_off, int64_t src_stride, const int32_t* src_len, uint8_t* dst, const int64_t* dst_off,
                        int64_t dst_stride, const int32_t* dst_cap, int32_t* result, int64_t n, int waves_per_group, const uint8_t* dict, int64_t dict_len,
                        uint8_t* table)
{
    Batch b = make_batch(src, src_stride, src_len, dst, dst_stride, dst_cap, result, n);
    b.src_off = src_off; b.dst_off = dst_off;
    emu_encdict::encode(b, dict, dict_len, table, (unsigned)waves_per_group);
}

int emu_encdict_stats(unsigned long long* out, int reset)
{
    for (int i = 0; i < lz4hip::kEncDictStats; i++) { out[i] = g_encdict_stat[i]; if (reset) g_encdict_stat[i] = 0; }
    return lz4hip::kEncDictStats;
}

// lz4hip_encode_batch_dict_host (dict_len > 0): the library's upload, priming and slice loop over the stage, the slices' kernels under the emulator
int emu_encdict_host(const lz4hip_batch_t* hb, const uint8_t* dict, int64_t dict_len, int waves_per_group, EmuHostBatch* r, EmuEncDictHost* d)
{
    using namespace lz4hip;
    emu_encdict::Stage st(*r, *d, dict);
    r->error[0] = 0;
    const unsigned wpg = (unsigned)waves_per_group;
    auto make_run = [wpg](const uint8_t* d_dict, int64_t reach, const uint8_t* table) {
        return [=](const lz4hip_batch_t* db, int64_t) { emu_encdict::launch(emu_framing::device_batch(db), d_dict, reach, table, wpg); return 0; };
    };
    const int rc = hostbatch::run_host_batch_encode_dict(st, hb, dict, dict_len, make_run, r->slice_hint, r->slices_knob, 1, emu_hostbatch::limits_of(*r));
    r->intact = st.intact();
    d->intact = st.dict_intact();
    d->table_unchanged = st.table_unchanged();
    snprintf(r->error, sizeof r->error, "%s", st.error.c_str());
    return rc;
}

int64_t emu_encdict_sizeof(int which) { return which == 0 ? (int64_t)sizeof(EmuEncDictHost) : (int64_t)sizeof(EmuHostBatch); }

}  // extern "C"
