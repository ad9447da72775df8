// emu_lz4f_dict.inc -- TEST INFRASTRUCTURE ONLY, a part of emu_framing.cpp.
// The decode of LZ4 frames with a dictionary (lz4hip_lz4f_decode_dict_* and lz4hip_lz4f_batch_decode_dict_*: the dictionary forms of
// lz4hip_framing.hpp's sequences lz4f_decode and lz4f_batch_decode, the walk's dictionary ID, the linked decode's dictionary form of
// lz4hip_lz4f_linked.hpp, and the host-pointer calls with the dictionary's staging) under the SIMT emulator, for
// tests/test_simt_lz4f_dict.py and tests/cpp/lz4f_dict_asan_main.cpp.  The block codec of the rounds is NO stand-in here: decode_dict
// runs the real decode_dict_kernel under the emulator, as the library's launch does, and decode (the plain sequences, which a call
// without a dictionary is) the real decode_kernel.

// what the emulated device is to do, and what it did
struct Lz4fDictEmuRun {
    int32_t grid, pad;                    // grid > 0 replaces the item, copy and walk formulas' answers
    int64_t plain_calls, dict_calls;      // rounds handed to decode / to decode_dict
    int64_t dict_uploads, dict_bytes;     // dict_upload calls, and the bytes of the last one
    int64_t dict_first_byte;              // which byte of the caller's dictionary the copy starts with
    int64_t dict_intact;                  // the guard bytes around the dictionary's device copy after the call
    int64_t uploads_before_dict;          // the image's uploads when the dictionary went up: 0, it comes first
    EmuCounters counters;
};

namespace {

struct Lz4fDictBackend : EmuBackend {
    Lz4fDictEmuRun* r = nullptr;
    const uint8_t* caller_dict = nullptr;
    std::vector<uint8_t> dict_store;

    // the library's launches (launch_decode with the wavefront mapping, launch_decode_dict): four wavefronts a workgroup
    int decode(const lz4hip_batch_t* b, int known)
    {
        r->plain_calls++;
        if (b->n_blocks == 0) return 0;
        const Batch d = device_batch(b);
        const unsigned wpg = kWaveDecodeWavesPerGroup;
        dim3 grid((unsigned)((d.n_blocks + wpg - 1) / wpg)), block(64 * wpg);
        if (known) simt::launch(grid, block, kWaveDecodeLdsBytes, [=] { decode_kernel<true>(d, kAllBlocks); });
        else       simt::launch(grid, block, kWaveDecodeLdsBytes, [=] { decode_kernel<false>(d, kAllBlocks); });
        return 0;
    }
    int decode_dict(const lz4hip_batch_t* b, const uint8_t* dict_end, int32_t reach, int known)
    {
        r->dict_calls++;
        if (b->n_blocks == 0) return 0;
        const Batch d = device_batch(b);
        const unsigned wpg = kWaveDecodeWavesPerGroup;
        dim3 grid((unsigned)((d.n_blocks + wpg - 1) / wpg)), block(64 * wpg);
        if (known) simt::launch(grid, block, kWaveDecodeLdsBytes, [=] { decode_dict_kernel<true>(d, dict_end, reach); });
        else       simt::launch(grid, block, kWaveDecodeLdsBytes, [=] { decode_dict_kernel<false>(d, dict_end, reach); });
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

Lz4fDictBackend backend_of(Lz4fDictEmuRun* r, const void* dict)
{
    Lz4fDictBackend be = backend<Lz4fDictBackend>(r->grid, r->grid, r->grid);
    be.r = r; be.caller_dict = (const uint8_t*)dict;
    be.lds_bytes = kWaveDecodeLdsBytes;
    r->plain_calls = r->dict_calls = r->dict_uploads = r->dict_bytes = r->dict_first_byte = r->uploads_before_dict = 0;
    return be;
}

int done(const Lz4fDictBackend& be, int rc, Lz4fDictEmuRun* r)
{
    r->dict_intact = be.dict_intact();
    return finish(be, rc, &r->counters);
}

}  // namespace

extern "C" {

int64_t emu_lz4f_dict_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(Lz4fInfo);
    case 1: return sizeof(Lz4fDictEmuRun);
    case 2: return sizeof(lz4hip_lz4f_batch_info_t);
    case 3: return sizeof(EmuCounters);
    default: return -1;
    }
}

int64_t emu_lz4f_dict_decode_scratch_bytes(int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    return framing::lz4f_decode_scratch_bytes(slot_bytes, max_blocks, round_blocks);
}
int64_t emu_lz4f_dict_batch_decode_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    return framing::lz4f_batch_decode_scratch_bytes(n, slot_bytes, max_blocks, round_blocks);
}

// ---- the device calls: the library's argument lists (plan, then run, as lz4hip_api.hip has them), then the run record ------------------
int emu_lz4f_dict_decode(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int32_t slot_bytes, int64_t max_blocks,
                         int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info,
                         Lz4fDictEmuRun* r)
{
    Lz4fDictBackend be = backend_of(r, dict);
    framing::Lz4fDecodePlan p;
    int rc = framing::lz4f_decode_dict_plan(be, src, src_len, dict, dict_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info, p);
    if (rc == 0) rc = framing::lz4f_decode_dict_run(be, p, dict, dict_len, dict_id);
    return done(be, rc, r);
}

int emu_lz4f_dict_batch_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                               int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst,
                               int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, int64_t* written_items,
                               Lz4fDictEmuRun* r)
{
    Lz4fDictBackend be = backend_of(r, dict);
    framing::Lz4fBatchDecodePlan p;
    int rc = framing::lz4f_batch_decode_dict_plan(be, src, src_len, src_off, n, dict, dict_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes,
                                                  dst, dst_cap, dst_off, item_info, info, written_items, p);
    if (rc == 0) rc = framing::lz4f_batch_decode_dict_run(be, p, dict, dict_len, dict_id);
    return done(be, rc, r);
}

// ---- the plain calls over the same backend: what a call with dict_len == 0 must equal ---------------------------------------------------
int emu_lz4f_dict_plain_decode(const void* src, int64_t src_len, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch,
                               int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, Lz4fDictEmuRun* r)
{
    Lz4fDictBackend be = backend_of(r, nullptr);
    return done(be, framing::lz4f_decode(be, src, src_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info), r);
}

int emu_lz4f_dict_plain_batch_decode(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t slot_bytes, int64_t max_blocks,
                                     int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off,
                                     lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, int64_t* written_items, Lz4fDictEmuRun* r)
{
    Lz4fDictBackend be = backend_of(r, nullptr);
    return done(be, framing::lz4f_batch_decode(be, src, src_len, src_off, n, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap,
                                               dst_off, item_info, info, written_items), r);
}

// ---- the host-pointer calls ----------------------------------------------------------------------------------------------------------
int emu_lz4f_dict_decode_host(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, unsigned flags, void* dst, int64_t dst_cap,
                              lz4hip_lz4f_info_t* info, Lz4fDictEmuRun* r)
{
    Lz4fDictBackend be = backend_of(r, dict);
    return done(be, framing::lz4f_decode_dict_host(be, src, src_len, dict, dict_len, dict_id, flags, dst, dst_cap, info), r);
}

int emu_lz4f_dict_batch_decode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                    unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info,
                                    Lz4fDictEmuRun* r)
{
    Lz4fDictBackend be = backend_of(r, dict);
    return done(be, framing::lz4f_batch_decode_dict_host(be, src, src_len, src_off, n, dict, dict_len, dict_id, flags, dst, dst_cap, dst_off, item_info, info), r);
}

}  // extern "C"
