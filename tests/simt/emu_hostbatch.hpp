// emu_hostbatch.hpp -- TEST INFRASTRUCTURE ONLY, included by emu_kernels.cpp.
// C entry points that run the library's own host code for the host-pointer block batch calls (lz4hip_hostbatch.hpp: the plan, the row
// work, the slice loop, the shards) for tests/test_simt_hostbatch.py, over EmuStage: a stage without any asynchrony that is built to
// show ordering mistakes all the same.  tests/emu_helpers.py mirrors EmuHostBatch with ctypes (size checked: emu_hostbatch_sizeof).
#pragma once
#include "lz4hip_hostbatch.hpp"

#include <string>
#include <vector>

// what an emu_host_batch call is to do, and what the stage saw
struct EmuHostBatch {
    const int32_t* results; const uint8_t* bytes; int64_t bytes_stride;   // the block codec's stand-in: the r-th row the kernels see gets
                                                                          // results[r] and, over its whole capacity, the bytes at r * bytes_stride
    int64_t row0;                                    // r of the call's first row (shards: the rows of the shards before it)
    int32_t decoder;                                 // 0: the stand-in; 1 / 2: decode_kernel<true / false> under the emulator
    int32_t fail_at;                                 // the kernels call that fails (0-based; -1: none)
    int32_t lag;                                     // how often out_done answers "not yet" about a slice before its copies land
    int32_t slices_knob, dst_len_is_result, pad;
    int64_t slice_hint, slice_floor, slice_ceiling, hinted_ceiling, pool_floor;     // (a limit < 0: the library's)
    uint8_t* seen_src; int64_t seen_stride; int32_t* seen_len; int32_t* seen_cap;   // what the kernels found staged for row r (NULL: not kept)
    int64_t* log; int64_t log_cap;                   // records of 8: kind, slot, a .. f (EmuStage::Kind)
    int64_t log_n, rows_seen, kernel_calls, quiesces, reserves;
    int32_t violations, intact;                      // EmuStage::violations; the guard bytes around all images after the call
    char error[160];                                 // what fail() recorded
};

namespace emu_hostbatch {

using namespace lz4hip;
using namespace lz4hip::hostbatch;

inline HostLimits limits_of(const EmuHostBatch& r)
{
    HostLimits l;
    if (r.slice_floor >= 0) l.slice_floor = r.slice_floor;
    if (r.slice_ceiling >= 0) l.slice_ceiling = r.slice_ceiling;
    if (r.hinted_ceiling >= 0) l.hinted_ceiling = r.hinted_ceiling;
    if (r.pool_floor >= 0) l.pool_floor = r.pool_floor;
    return l;
}

// The stage of hostbatch::run_host_batch, faked: all four images of a slot are host memory of exactly the bytes asked for between
// guard bytes.  Nothing runs asynchronously, but a copy out is only RECORDED and carried out when out_done or wait_out reports it
// complete -- until then pin_out holds kStale -- out_done says "not yet" `lag` times per slice, pin_in is overwritten with kSpent as
// soon as it was copied in, and the device images start out as kFresh (dev_out again before every slice's kernels).  A slot that is
// written while its previous slice has not been drained is refused.
struct EmuStage {
    enum Kind { kReserve = 1, kCopyIn, kKernels, kCopyOut, kOutDone, kWaitOut, kBegin, kQuiesce };
    enum { kSlotBusy = 1, kNothingPending = 2, kOutOfImage = 4, kReserveTwice = 8, kNotABatch = 16 };
    static constexpr size_t kGuard = 64;
    static constexpr uint8_t kGuardByte = 0xC3, kFresh = 0xEE, kStale = 0xDD, kSpent = 0xBB;
    struct Image { std::vector<uint8_t> store; uint8_t* base = nullptr; int64_t bytes = 0; };
    struct Copy { int64_t offset, bytes; };
    struct Out { int state = 0 /* 0 drained, 1 queued, 2 landed */, asked = 0; std::vector<Copy> copies; };

    EmuHostBatch& r;
    Image pin_i[kHostSlots], dev_i[kHostSlots], dev_o[kHostSlots], pin_o[kHostSlots];
    Out out[kHostSlots];
    int slots = 0;
    std::string error;
    explicit EmuStage(EmuHostBatch& run) : r(run) { r.log_n = 0; r.rows_seen = r.row0; r.kernel_calls = r.quiesces = r.reserves = 0; r.violations = 0; }

    void note(int kind, int slot, int64_t a = 0, int64_t b = 0, int64_t c = 0, int64_t d = 0, int64_t e = 0, int64_t f = 0)
    {
        if (r.log && r.log_n < r.log_cap) {
            int64_t* at = r.log + 8 * r.log_n;
            at[0] = kind; at[1] = slot; at[2] = a; at[3] = b; at[4] = c; at[5] = d; at[6] = e; at[7] = f;
        }
        r.log_n++;
    }
    int fail(int code, const char* what) { error = what; return code; }
    int violation(int which, const char* what) { r.violations |= which; return fail(LZ4HIP_E_DEVICE, what); }
    static void make(Image& im, int64_t bytes, uint8_t fill)
    {
        im.store.assign((size_t)bytes + 2 * kGuard, kGuardByte);
        im.base = im.store.data() + kGuard; im.bytes = bytes;
        memset(im.base, fill, (size_t)bytes);
    }
    int reserve(int n_slots, int64_t in_bytes, int64_t out_bytes)
    {
        note(kReserve, n_slots, in_bytes, out_bytes);
        if (r.reserves++) return violation(kReserveTwice, "EmuStage: reserve called twice");
        slots = n_slots;
        for (int k = 0; k < slots; k++) { make(pin_i[k], in_bytes, kSpent); make(dev_i[k], in_bytes, kFresh); make(dev_o[k], out_bytes, kFresh); make(pin_o[k], out_bytes, kStale); }
        return 0;
    }
    uint8_t* pin_in(int k) { return pin_i[k].base; }
    uint8_t* pin_out(int k) { return pin_o[k].base; }
    uint8_t* dev_in(int k) { return dev_i[k].base; }
    uint8_t* dev_out(int k) { return dev_o[k].base; }
    int begin() { note(kBegin, 0); return 0; }
    bool inside(const Image& im, int64_t offset, int64_t bytes) const { return offset >= 0 && bytes >= 0 && offset + bytes <= im.bytes; }
    int copy_in(int slot, int64_t offset, int64_t bytes)
    {
        note(kCopyIn, slot, offset, bytes);
        if (slot >= slots || !inside(dev_i[slot], offset, bytes)) return violation(kOutOfImage, "EmuStage: copy_in outside the image");
        if (out[slot].state != 0) return violation(kSlotBusy, "EmuStage: copy_in into a slot whose previous slice was not drained");
        memcpy(dev_i[slot].base + offset, pin_i[slot].base + offset, (size_t)bytes);
        memset(pin_i[slot].base + offset, kSpent, (size_t)bytes);
        return 0;
    }
    template <class Run>
    int kernels(int slot, Run& run, const lz4hip_batch_t& db)
    {
        const int flags = (db.src_off == nullptr) | (db.dst_off == nullptr) << 1 | (db.src == dev_i[slot].base) << 2 | (db.dst == dev_o[slot].base) << 3;
        note(kKernels, slot, db.n_blocks, db.src_stride, db.dst_stride, db.src_len_all, db.dst_cap_all, flags);
        if (out[slot].state != 0) return violation(kSlotBusy, "EmuStage: kernels on a slot whose previous slice was not drained");
        if (r.kernel_calls++ == r.fail_at) {
            snprintf(r.error, sizeof r.error, "EmuStage: the kernels failed at row %lld", (long long)r.rows_seen);
            error = r.error;
            return LZ4HIP_E_DEVICE;
        }
        for (int64_t j = 0; j < db.n_blocks; j++)
            if (db.src_len[j] < 0 || db.src_len[j] > db.src_stride || db.dst_cap[j] < 0 || db.dst_cap[j] > db.dst_stride)
                return violation(kNotABatch, "EmuStage: the staged lengths and capacities are not those of rows at these strides");
        memset(dev_o[slot].base, kFresh, (size_t)dev_o[slot].bytes);
        for (int64_t j = 0; j < db.n_blocks; j++) {
            const int64_t at = r.rows_seen + j;
            if (r.seen_len) r.seen_len[at] = db.src_len[j];
            if (r.seen_cap) r.seen_cap[at] = db.dst_cap[j];
            if (r.seen_src) memcpy(r.seen_src + at * r.seen_stride, (const uint8_t*)db.src + j * db.src_stride, (size_t)(db.src_len[j] < r.seen_stride ? db.src_len[j] : r.seen_stride));
        }
        const int rc = run(&db, r.rows_seen);
        r.rows_seen += db.n_blocks;
        return rc;
    }
    int copy_out(int slot, int64_t offset, int64_t bytes)
    {
        note(kCopyOut, slot, offset, bytes);
        if (slot >= slots || !inside(dev_o[slot], offset, bytes)) return violation(kOutOfImage, "EmuStage: copy_out outside the image");
        if (out[slot].state == 2) return violation(kSlotBusy, "EmuStage: copy_out into a slot whose previous slice was not drained");
        if (out[slot].state == 0) { out[slot] = Out(); out[slot].state = 1; memset(pin_o[slot].base, kStale, (size_t)pin_o[slot].bytes); }
        out[slot].copies.push_back({ offset, bytes });
        return 0;
    }
    void land(int slot)
    {
        for (const Copy& c : out[slot].copies) memcpy(pin_o[slot].base + c.offset, dev_o[slot].base + c.offset, (size_t)c.bytes);
        out[slot].state = 2;
    }
    bool out_done(int slot)
    {
        Out& o = out[slot];
        if (o.state == 0) r.violations |= kNothingPending;
        const bool done = o.state != 1 || o.asked++ >= r.lag;
        if (done && o.state == 1) land(slot);
        note(kOutDone, slot, done);
        return done;
    }
    int wait_out(int slot)
    {
        note(kWaitOut, slot);
        if (out[slot].state == 0) return violation(kNothingPending, "EmuStage: wait_out on a slot with no copy out queued");
        if (out[slot].state == 1) land(slot);
        out[slot].state = 0;                                              // (drained: the loop scatters it now)
        return 0;
    }
    void quiesce() { note(kQuiesce, 0); r.quiesces++; }
    bool intact() const
    {
        for (const Image* set : { pin_i, dev_i, dev_o, pin_o })
            for (int k = 0; k < slots; k++)
                for (size_t g = 0; g < kGuard; g++)
                    if (set[k].store[g] != kGuardByte || set[k].store[kGuard + (size_t)set[k].bytes + g] != kGuardByte) return false;
        return true;
    }
};

// the whole call: the library's loop over an EmuStage, threads_knob 1 -- the row pool starts no thread, so a scatter job that was
// queued (rows of pool_floor bytes or more) is carried out by whoever waits for it, and not before
inline int run(const lz4hip_batch_t* hb, EmuHostBatch& r)
{
    EmuStage st(r);
    r.error[0] = 0;
    auto stand_in = [&r](const lz4hip_batch_t* b, int64_t row) {
        for (int64_t j = 0; j < b->n_blocks; j++) {
            b->result[j] = r.results[row + j];
            if (b->dst_cap[j] > 0) memcpy((uint8_t*)b->dst + j * b->dst_stride, r.bytes + (row + j) * r.bytes_stride, (size_t)b->dst_cap[j]);
        }
        return 0;
    };
    auto decoder = [&r](const lz4hip_batch_t* b, int64_t) {
        Batch d;
        memset(&d, 0, sizeof d);
        d.src = (const uint8_t*)b->src; d.src_stride = b->src_stride; d.src_len = b->src_len; d.src_len_all = b->src_len_all;
        d.dst = (uint8_t*)b->dst; d.dst_stride = b->dst_stride; d.dst_cap = b->dst_cap; d.dst_cap_all = b->dst_cap_all;
        d.result = b->result; d.n_blocks = b->n_blocks;
        if (r.decoder == 1) simt::launch(dim3((unsigned)d.n_blocks), dim3(64), kWaveLdsBytes, [=] { decode_kernel<true>(d, 0); });
        else                simt::launch(dim3((unsigned)d.n_blocks), dim3(64), kWaveLdsBytes, [=] { decode_kernel<false>(d, 0); });
        return 0;
    };
    const HostLimits limits = limits_of(r);
    const int rc = r.decoder ? run_host_batch(st, hb, r.dst_len_is_result != 0, decoder, r.slice_hint, r.slices_knob, 1, limits)
                             : run_host_batch(st, hb, r.dst_len_is_result != 0, stand_in, r.slice_hint, r.slices_knob, 1, limits);
    r.intact = st.intact();
    snprintf(r.error, sizeof r.error, "%s", st.error.c_str());
    return rc;
}

}  // namespace emu_hostbatch

extern "C" {

int64_t emu_hostbatch_sizeof(void) { return sizeof(EmuHostBatch); }

// which: 0 encode_host_slice_blocks(n_blocks, mode, cus), 1 host_workers_for(n_blocks, hc, knob), 2 kHostSlots
int64_t emu_host_rule(int which, int64_t a, int64_t b, int64_t c)
{
    switch (which) {
    case 0: return lz4hip::hostbatch::encode_host_slice_blocks(a, (int)b, (int)c);
    case 1: return lz4hip::hostbatch::host_workers_for(a, b != 0, (int)c);
    case 2: return lz4hip::hostbatch::kHostSlots;
    default: return -1;
    }
}

// plan_host_batch; out[0 .. 18]: n, max_src, max_dst, s_stride, d_stride, per_slice, n_slices, slots, in_lens, in_caps, in_bytes, out_res,
// out_bytes, the last slice's first row and count, then the four copies of that slice: rows in, tail in, rows out, tail out.
// Returns the plan's error; its text goes to `text` (160 bytes).
int emu_host_plan(const lz4hip_batch_t* hb, int slices_knob, int64_t slice_hint, const EmuHostBatch* limits, int64_t* out, char* text)
{
    using namespace lz4hip::hostbatch;
    const HostPlan p = plan_host_batch(hb, slices_knob, slice_hint, emu_hostbatch::limits_of(*limits));
    snprintf(text, 160, "%s", p.error_text ? p.error_text : "");
    const int64_t last = p.n_slices - 1, cnt = p.n_slices > 0 ? p.count(last) : 0;
    const int64_t v[19] = { p.n, p.max_src, p.max_dst, p.s_stride, p.d_stride, p.per_slice, p.n_slices, p.slots, p.in_lens, p.in_caps, p.in_bytes,
                            p.out_res, p.out_bytes, p.n_slices > 0 ? p.first(last) : 0, cnt, p.rows_in(cnt), p.tail_in(), p.rows_out(cnt), p.tail_out() };
    memcpy(out, v, sizeof v);
    return p.error;
}

int emu_host_batch(const lz4hip_batch_t* hb, EmuHostBatch* r) { return emu_hostbatch::run(hb, *r); }

// shard_batch, every shard through emu_host_batch (r->row0 moves on by each shard's rows; the shards of the mask fail_shards fail at
// their first kernels call), merge_shards with shard k on "device" devs[k].  shard_rows[k]: the shard's blocks; shard_reserves[k]:
// whether it reserved a stage.  The merged failure text goes to r->error.
int emu_host_shards(const lz4hip_batch_t* hb, int nd, const int* devs, unsigned fail_shards, EmuHostBatch* r, int64_t* shard_rows, int64_t* shard_reserves)
{
    using namespace lz4hip::hostbatch;
    std::vector<Shard> shards = shard_batch(hb, nd);
    int32_t violations = 0, intact = 1;
    int64_t row0 = r->row0;
    for (int k = 0; k < nd; k++) {
        Shard& sh = shards[(size_t)k];
        r->row0 = row0;
        r->fail_at = (fail_shards >> k & 1u) ? 0 : -1;
        sh.rc = emu_hostbatch::run(&sh.b, *r);
        sh.err = r->error;
        shard_rows[k] = sh.b.n_blocks; shard_reserves[k] = r->reserves;
        if (!sh.rc) { violations |= r->violations; intact &= r->intact; }
        row0 += sh.b.n_blocks;
    }
    std::string text;
    const int rc = merge_shards(hb, shards, devs, text);
    r->violations = violations; r->intact = intact;
    snprintf(r->error, sizeof r->error, "%s", text.c_str());
    return rc;
}

}  // extern "C"
