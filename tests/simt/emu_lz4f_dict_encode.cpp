// emu_lz4f_dict_encode.cpp -- TEST INFRASTRUCTURE ONLY.
// libsimt_lz4f_dict_encode.so: the encode of LZ4 frames with a dictionary (lz4hip_lz4f_encode_dict_* and lz4hip_lz4f_batch_encode_dict_*:
// the dictionary forms of lz4hip_framing.hpp's sequences lz4f_encode_run and lz4f_batch_encode_run, the head kernels of the descriptor
// with a dictionary ID, and the host-pointer calls with the dictionary's staging) under the SIMT emulator, for
// tests/test_simt_lz4f_dict_encode.py and tests/cpp/lz4f_dict_encode_asan_main.cpp.  The block codec is NO stand-in: encode_dict_prime
// and encode_dict run the real encode_dict_prime_kernel and encode_dict_kernel<1> / <5> under the emulator, as the library's launches
// do, and encode (the plain sequences, which a call without a dictionary is) the real encode_fast_kernel; the framing kernels are the
// real ones throughout.  Built with g++ by tests/lz4f_dict_encode_lib.py, never shipped.
#include "simt_wave.hpp"

#include "lz4hip_common.hpp"
#include "lz4hip_encode.hpp"
#include "lz4hip_encode_dict.hpp"

using namespace lz4hip;

#include "emu_framing.hpp"

using emu_framing::EmuBackend;
using emu_framing::backend;
using emu_framing::finish;
using emu_framing::device_batch;

// what the emulated device is to do, and what it did
struct Lz4fDictEncEmuRun {
    int32_t grid, waves_per_group;        // grid > 0 replaces the item and copy formulas' answers; blocks per workgroup of the encoders: 1 or 5
    int64_t plain_calls, dict_calls;      // block batches handed to encode / to encode_dict
    int64_t primes, primes_before_dict;   // encode_dict_prime calls, and how many had run when the (last) encode_dict came
    int64_t dict_uploads, dict_bytes;     // dict_upload calls, and the bytes of the last one
    int64_t dict_first_byte;              // which byte of the caller's dictionary the copy starts with
    int64_t dict_intact;                  // the guard bytes around the dictionary's device copy after the call
    int64_t uploads_before_dict;          // the image's uploads when the dictionary went up: 0, it comes first
    EmuCounters counters;
};

namespace {

struct Lz4fDictEncBackend : EmuBackend {
    Lz4fDictEncEmuRun* r = nullptr;
    const uint8_t* caller_dict = nullptr;
    std::vector<uint8_t> dict_store;

    unsigned wpg() const { return r->waves_per_group == 5 ? 5u : 1u; }
    // the library's launches (launch_encode with the wavefront mapping, launch_encode_dict_prime, launch_encode_dict)
    int encode(const lz4hip_batch_t* b, int)
    {
        r->plain_calls++;
        if (b->n_blocks == 0) return 0;
        const Batch d = device_batch(b);
        if (wpg() == 5) simt::launch(dim3((unsigned)((d.n_blocks + 4) / 5)), dim3(64 * 5), 5 * kFastTableBytes, [=] { encode_fast_kernel<2, 5>(d, 0); });
        else            simt::launch(dim3((unsigned)d.n_blocks), dim3(64), kFastTableBytes, [=] { encode_fast_kernel(d, 0); });
        return 0;
    }
    int encode_dict_prime(const uint8_t* dict_end, int32_t reach, uint8_t* primed)
    {
        r->primes++;
        simt::launch(dim3(1), dim3(kEncDictPrimeThreads), kFastTableBytes, [=] { encode_dict_prime_kernel(dict_end, reach, primed); });
        return 0;
    }
    int encode_dict(const lz4hip_batch_t* b, const uint8_t* dict_end, int32_t reach, const uint8_t* primed)
    {
        r->dict_calls++; r->primes_before_dict = r->primes;
        if (b->n_blocks == 0) return 0;
        const Batch d = device_batch(b);
        if (wpg() == 5) simt::launch(dim3((unsigned)((d.n_blocks + 4) / 5)), dim3(64 * 5), 5 * kFastTableBytes, [=] { encode_dict_kernel<5>(d, dict_end, reach, primed); });
        else            simt::launch(dim3((unsigned)d.n_blocks), dim3(64), kFastTableBytes, [=] { encode_dict_kernel<1>(d, dict_end, reach, primed); });
        return 0;
    }
    // the dictionary's staging: exactly the bytes asked for between guard bytes, apart from the image
    int dict_upload(const uint8_t* from, int64_t bytes, uint8_t*& dev)
    {
        r->dict_uploads++; r->dict_bytes = bytes; r->dict_first_byte = from - caller_dict; r->uploads_before_dict = uploads;
        dict_store.assign((size_t)bytes + 2 * kGuard, kGuardByte);
        memcpy(dict_store.data() + kGuard, from, (size_t)bytes);
        dev = dict_store.data() + kGuard;
        return 0;
    }
    bool dict_intact() const
    {
        for (size_t g = 0; g < kGuard && !dict_store.empty(); g++)
            if (dict_store[g] != kGuardByte || dict_store[dict_store.size() - 1 - g] != kGuardByte) return false;
        return true;
    }
};

Lz4fDictEncBackend backend_of(Lz4fDictEncEmuRun* r, const void* dict)
{
    Lz4fDictEncBackend be = backend<Lz4fDictEncBackend>(r->grid, r->grid, r->grid);
    be.r = r; be.caller_dict = (const uint8_t*)dict;
    r->plain_calls = r->dict_calls = r->primes = r->primes_before_dict = r->dict_uploads = r->dict_bytes = r->dict_first_byte = r->uploads_before_dict = 0;
    return be;
}

int done(const Lz4fDictEncBackend& be, int rc, Lz4fDictEncEmuRun* r)
{
    r->dict_intact = be.dict_intact();
    return finish(be, rc, &r->counters);
}

}  // namespace

extern "C" {

int64_t emu_lz4f_dict_encode_sizeof(int which) { return which == 0 ? (int64_t)sizeof(Lz4fDictEncEmuRun) : (which == 1 ? (int64_t)sizeof(EmuCounters) : -1); }

// ---- the queries, as lz4hip_api.hip has them ----------------------------------------------------------------------------------------------
int64_t emu_lz4f_dict_bound(int64_t src_len, int id, unsigned flags, int64_t dict_len, uint32_t dict_id) { return framing::lz4f_dict_bound(src_len, id, flags, dict_len, dict_id); }
int64_t emu_lz4f_batch_dict_bound(int64_t n, int64_t src_len, int id, unsigned flags, int64_t dict_len, uint32_t dict_id)
{
    return framing::lz4f_batch_dict_bound(n, src_len, id, flags, dict_len, dict_id);
}
int64_t emu_lz4f_encode_dict_scratch_bytes(int64_t src_len, int id, int64_t dict_len)
{
    if (dict_len < 0 || !framing::lz4f_id_valid(id)) return LZ4HIP_E_ARGUMENT;
    return framing::lz4f_encode_scratch(nullptr, src_len < 0 ? 0 : src_len, lz4f_block_bytes(framing::lz4f_id(id)), dict_len).bytes;
}
int64_t emu_lz4f_batch_encode_dict_scratch_bytes(int64_t n, int64_t src_len, int id, int64_t dict_len)
{
    if (dict_len < 0 || !framing::lz4f_id_valid(id)) return LZ4HIP_E_ARGUMENT;
    return n <= 0 ? 0 : framing::lz4f_batch_encode_scratch(nullptr, n, src_len < 0 ? 0 : src_len, lz4f_block_bytes(framing::lz4f_id(id)), dict_len).bytes;
}
int64_t emu_lz4f_plain_bound(int64_t src_len, int id, unsigned flags) { return framing::lz4f_bound(src_len, id, flags); }
int64_t emu_lz4f_plain_batch_bound(int64_t n, int64_t src_len, int id, unsigned flags) { return framing::lz4f_batch_bound(n, src_len, id, flags); }
int64_t emu_lz4f_plain_encode_scratch_bytes(int64_t src_len, int id)
{
    return framing::lz4f_encode_scratch(nullptr, src_len < 0 ? 0 : src_len, lz4f_block_bytes(framing::lz4f_id(id))).bytes;
}
int64_t emu_lz4f_plain_batch_encode_scratch_bytes(int64_t n, int64_t src_len, int id)
{
    return n <= 0 ? 0 : framing::lz4f_batch_encode_scratch(nullptr, n, src_len < 0 ? 0 : src_len, lz4f_block_bytes(framing::lz4f_id(id))).bytes;
}

// ---- the device calls: the library's argument lists (plan, then run, as lz4hip_api.hip has them), then the run record ------------------
int emu_lz4f_encode_dict(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int id, unsigned flags, void* dst, int64_t dst_cap,
                         int64_t* dst_len, void* scratch, int64_t scratch_bytes, Lz4fDictEncEmuRun* r)
{
    Lz4fDictEncBackend be = backend_of(r, dict);
    framing::Lz4fEncodePlan p;
    framing::Lz4fDict d;
    int rc = framing::lz4f_encode_dict_plan(be, src, src_len, dict, dict_len, dict_id, id, flags, dst, dst_cap, dst_len, scratch, scratch_bytes, p, d);
    if (rc == 0) rc = framing::lz4f_encode_dict_run(be, p, d);
    return done(be, rc, r);
}

int emu_lz4f_batch_encode_dict(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id, int id,
                               unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, Lz4fDictEncEmuRun* r)
{
    Lz4fDictEncBackend be = backend_of(r, dict);
    framing::Lz4fBatchEncodePlan p;
    framing::Lz4fDict d;
    int rc = framing::lz4f_batch_encode_dict_plan(be, src, src_len, src_off, n, dict, dict_len, dict_id, id, flags, dst, dst_cap, dst_off, scratch, scratch_bytes, p, d);
    if (rc == 0) rc = framing::lz4f_batch_encode_dict_run(be, p, d);
    return done(be, rc, r);
}

// ---- the plain calls in fast mode over the same backend: what a call with dict_len == 0 must equal ---------------------------------------
int emu_lz4f_plain_encode(const void* src, int64_t src_len, int id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len, void* scratch,
                          int64_t scratch_bytes, Lz4fDictEncEmuRun* r)
{
    Lz4fDictEncBackend be = backend_of(r, nullptr);
    return done(be, framing::lz4f_encode(be, src, src_len, id, LZ4HIP_MODE_FAST, flags, dst, dst_cap, dst_len, scratch, scratch_bytes), r);
}

int emu_lz4f_plain_batch_encode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int id, unsigned flags, void* dst, int64_t dst_cap,
                                int64_t* dst_off, void* scratch, int64_t scratch_bytes, Lz4fDictEncEmuRun* r)
{
    Lz4fDictEncBackend be = backend_of(r, nullptr);
    return done(be, framing::lz4f_batch_encode(be, src, src_len, src_off, n, id, LZ4HIP_MODE_FAST, flags, dst, dst_cap, dst_off, scratch, scratch_bytes), r);
}

// ---- the host-pointer calls ----------------------------------------------------------------------------------------------------------
int emu_lz4f_encode_dict_host(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int id, unsigned flags, void* dst,
                              int64_t dst_cap, int64_t* dst_len, Lz4fDictEncEmuRun* r)
{
    Lz4fDictEncBackend be = backend_of(r, dict);
    return done(be, framing::lz4f_encode_dict_host(be, src, src_len, dict, dict_len, dict_id, id, flags, dst, dst_cap, dst_len), r);
}

int emu_lz4f_batch_encode_dict_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                    int id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, Lz4fDictEncEmuRun* r)
{
    Lz4fDictEncBackend be = backend_of(r, dict);
    return done(be, framing::lz4f_batch_encode_dict_host(be, src, src_len, src_off, n, dict, dict_len, dict_id, id, flags, dst, dst_cap, dst_off), r);
}

}  // extern "C"
