// lz4hip_hostbatch.hpp -- host side of the host-pointer BLOCK batch calls (lz4hip_*_batch_host, *_host_multi and, through them, the seven
// single-block calls; lz4hip_decoded_sizes_host, decoded_sizes_host below, over the framing backend instead of the stage): how a batch of caller rows is cut into slices, the two staging images of a slice, the gather and scatter of
// rows, the order in which slices travel through kHostSlots sets of buffers, and the round-robin shards of the multi-device form,
// written ONCE for the library (lz4hip_api.hip, HostContext) and for the CPU tests (tests/simt/emu_hostbatch.hpp, EmuStage).  Host code
// only: nothing here calls the HIP runtime; everything that touches a device goes through the stage S of run_host_batch, which has
//
//     int      reserve(slots, in_bytes, out_bytes)    per slot: a pinned and a device "in" image, a device and a pinned "out" image
//     uint8_t* pin_in(slot), pin_out(slot)            the pinned images: host memory the rows are gathered into / scattered from
//     uint8_t* dev_in(slot), dev_out(slot)            the device images (addresses only: never dereferenced here)
//     int      begin()                                whatever the caller queued before this call comes first
//     int      copy_in(slot, offset, bytes)           pin_in -> dev_in, [offset, offset + bytes), queued behind every earlier copy_in
//     int      kernels(slot, run, batch)              `run` over `batch` (device addresses) once the slot's copies in have landed
//     int      copy_out(slot, offset, bytes)          dev_out -> pin_out, queued behind the slot's kernels and every earlier copy_out
//     bool     out_done(slot)                         the slot's copies out have landed (does not block)
//     int      wait_out(slot)                         waits until they have
//     void     quiesce()                              waits for everything queued (the error path)
//     int      fail(code, text)                       records the text, returns the code
//
// Every int is 0 or the code of a recorded failure.  The loop promises the stage: a slot's images are touched again only after its
// previous slice's wait_out (or a true out_done), and pin_out(slot) is read only between that and the slot's next copy_out.
#pragma once
#include "lz4hip_framing.hpp"

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

namespace lz4hip {
namespace hostbatch __attribute__((visibility("hidden"))) {          // (the library exports its C ABI, nothing of this)

using framing::Carver;

constexpr int kHostSlots = 4;
constexpr int64_t kHcHostSliceBlocks = 16384;     // host-pointer LZ4HC batches: blocks per slice
constexpr int64_t kHostWorkersMinBlocks = 8192;
constexpr int kHostEncodeBlocksPerCu = 10;        // the wavefront-mapped fast encoder's residency: two workgroups of five blocks

// A single-device host-pointer batch of kHostWorkersMinBlocks blocks or more runs as TWO staging pipelines on the same device (the persistent
// workers of the multi-device path, block i -> worker i mod 2): one pipeline's kernels and copies fill the gaps of the other's -- a 16 384-block
// D2 decode 23.6 -> 33.5 GB/s on the driver's box of round 5/6 (profiles/r06/bench_driver_style_call1.json, host_pointer_batch_multi_device).
// Knob host_workers: 1 = the calling thread's pipeline alone.  (Concurrent callers queue on those two workers: ADVICE.md, open.)
inline int host_workers_for(int64_t n_blocks, bool mode_is_hc, int workers_knob)      // (decode; fast encode only where the knob is set)
{
    if (n_blocks < kHostWorkersMinBlocks || mode_is_hc) return 1;
    return workers_knob > 0 ? (workers_knob > 8 ? 8 : workers_knob) : 2;
}

// Slices of a host-pointer FAST encode: the wavefront-mapped encoder holds ten blocks per CU (workgroups of five) and a slice's kernel time goes by
// whole residency rounds -- 2 731 blocks (a sixth of 16 384) are 10.7 per CU = two rounds, 12.5 ms, where 2 560 blocks take 7.6 ms.  So a batch is cut
// into the fewest EQUAL slices of at most one round each (16 384 blocks: 7 x 2 341), and it runs as ONE pipeline: the kernels are the bottleneck, a
// second pipeline's slices only compete for the same ten places per CU (16 384 blocks 15.7-16.4 against 11.1-13.8 GB/s with two pipelines and 11.9-14.4
// with round 5's six equal slices, three runs each on one box: profiles/r06/host_encode_one_pipeline_equal_round_slices.txt; earlier forms of the rule:
// host_encode_slices_of_one_residency_round.txt, host_tapered_slices_ab.txt).  cus <= 0 (not known): no hint.
inline int64_t encode_host_slice_blocks(int64_t n_blocks, int mode, int cus)
{
    if (mode == LZ4HIP_MODE_HC) return kHcHostSliceBlocks;
    if (n_blocks < 4096 || cus <= 0) return 0;
    const int64_t round = (int64_t)kHostEncodeBlocksPerCu * cus, slices = (n_blocks + round - 1) / round;
    return (n_blocks + slices - 1) / slices;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// the byte limits of a slice; the CPU tests bring small ones (with these, a batch small enough for the emulator is one slice)
struct HostLimits {
    int64_t slice_floor = 32ll << 20;             // rows of a slice: at least this many bytes ...
    int64_t slice_ceiling = 512ll << 20;          // ... and at most this many,
    int64_t hinted_ceiling = 4ll << 30;           // or this many where the caller's hint asks for more
    int64_t pool_floor = 4ll << 20;               // rows of fewer bytes are copied on the calling thread, not on the row pool
};

// How a batch travels: rows in per-block places of the maximum length, 16-byte aligned, in equal slices of per_slice rows (the last
// one may be short) over `slots` sets of images.  "in" image: [src rows | src_len | dst_cap]; "out" image: [dst rows | result].
struct HostPlan {
    int error = 0;                                // 0, or the batch is refused with error_text
    const char* error_text = nullptr;
    int64_t n = 0, max_src = 0, max_dst = 0, s_stride = 0, d_stride = 0, per_slice = 0, n_slices = 0;
    int slots = 0;
    int64_t in_lens = 0, in_caps = 0, in_bytes = 0, out_res = 0, out_bytes = 0;
    int64_t first(int64_t slice) const { return slice * per_slice; }
    int64_t count(int64_t slice) const { return n - first(slice) < per_slice ? n - first(slice) : per_slice; }
    // the four copies of a slice of cnt rows: the rows it has, then the whole tail (a short slice does not pay for a full one's rows)
    int64_t rows_in(int64_t cnt) const { return s_stride * cnt; }
    int64_t tail_in() const { return in_bytes - in_lens; }
    int64_t rows_out(int64_t cnt) const { return d_stride * cnt; }
    int64_t tail_out() const { return out_bytes - out_res; }
};

inline int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

// slices_knob: the host_slices knob (0: automatic).  slice_hint > 0: blocks per slice wanted by the caller (LZ4HC: its lane kernels need
// ~0.35 s however few blocks a launch has, so a batch goes in slices of up to 16384 blocks instead of ~2048).
inline HostPlan plan_host_batch(const lz4hip_batch_t* hb, int slices_knob, int64_t slice_hint, const HostLimits& limits = HostLimits())
{
    HostPlan p;
    const int64_t n = p.n = hb->n_blocks;
    for (int64_t i = 0; i < n; i++) {
        const int32_t sl = hb->src_len ? hb->src_len[i] : hb->src_len_all;
        const int32_t dc = hb->dst_cap ? hb->dst_cap[i] : hb->dst_cap_all;
        if (sl < 0) { p.error = LZ4HIP_E_ARGUMENT; p.error_text = "negative source length"; return p; }
        p.max_src = sl > p.max_src ? sl : p.max_src;
        p.max_dst = dc > p.max_dst ? dc : p.max_dst;
    }
    if (n == 0) return p;
    p.s_stride = align16(p.max_src + 16); p.d_stride = align16(p.max_dst + 16);
    const int64_t row_bytes = p.s_stride + p.d_stride;
    // slices: the kernels of a slice take milliseconds however few blocks it has (a 64 KiB block of short sequences needs 2.6 ms
    // in the wavefront mapping), so small batches are cut less: 1 slice up to ~3 k blocks, 2 at 4 k, 6 from 12 k (knob host_slices;
    // profiles/r02/host_slices_sweep.txt, profiles/r03/host_slices_by_batch_size.txt: 4 096 blocks 19.4 GB/s with 2 slices, 14.7-18.4 with 6-8)
    const int64_t auto_slices = n / 2048 < 1 ? 1 : (n / 2048 > 6 ? 6 : n / 2048);
    const int64_t want_slices = slices_knob > 0 ? slices_knob : auto_slices;
    int64_t per_slice = (n + want_slices - 1) / want_slices;
    int64_t lo = limits.slice_floor / row_bytes, hi = limits.slice_ceiling / row_bytes;
    if (slice_hint > 0 && slices_knob <= 0 && p.max_src <= 65536) {
        // (the hint is for the LZ4HC kernels of blocks <= 64 KiB; whatever the rows are, a slice stays below 4 GiB of staging)
        const int64_t cap4g = limits.hinted_ceiling / row_bytes, most = hi > cap4g ? hi : cap4g;
        const int64_t hinted = slice_hint < most ? slice_hint : most;
        per_slice = hinted; hi = hi > hinted ? hi : hinted;
    }
    per_slice = per_slice < lo ? lo : per_slice;
    per_slice = per_slice > hi ? hi : per_slice;
    p.per_slice = per_slice < 1 ? 1 : (per_slice > n ? n : per_slice);
    // (equal slices; a quarter slice at both ends -- less time before the first kernel and after the last one -- measured no gain:
    // profiles/r06/host_tapered_slices_ab.txt, tools/ab/host_tapered_slices.patch)
    p.n_slices = (n + p.per_slice - 1) / p.per_slice;
    p.slots = p.n_slices < kHostSlots ? (int)p.n_slices : kHostSlots;
    Carver in, out;
    in.take(p.s_stride * p.per_slice);
    p.in_lens = in.take(4 * p.per_slice); p.in_caps = in.take(4 * p.per_slice); p.in_bytes = in.at;
    out.take(p.d_stride * p.per_slice);
    p.out_res = out.take(4 * p.per_slice); p.out_bytes = out.at;
    return p;
}

// ---- the row pool: gathers and scatters between caller memory and the pinned staging ------------------------------------
// Plain memcpy of rows, ~10 GB/s per core -- and with six slices per batch the calling thread used to spend more time in them
// than PCIe needs for the payload (round 3: 16 threads, started and joined per call: 24 GB/s for a 16 384-block decode).  Now
// ONE persistent pool per process, started on first use: min(hardware threads / 4, 64) threads (knob host_threads), shared by
// every caller -- the device workers of a multi-device call included: each of their jobs is cut into chunks that any pool
// thread (and the submitting thread) may take, so eight devices share the pool instead of getting two threads each.
struct RowJob {
    std::function<void(int64_t)> f;
    int64_t n = 0, chunk = 1;
    std::atomic<int64_t> next{ 0 }, remaining{ 0 };
    std::mutex m;
    std::condition_variable done_cv;
    bool exhausted() const { return next.load(std::memory_order_relaxed) >= n; }
    // runs one chunk; false when none was left
    bool work_one()
    {
        const int64_t lo = next.fetch_add(chunk, std::memory_order_relaxed);
        if (lo >= n) return false;
        const int64_t hi = lo + chunk < n ? lo + chunk : n;
        for (int64_t i = lo; i < hi; i++) f(i);
        if (remaining.fetch_sub(hi - lo, std::memory_order_acq_rel) == hi - lo) {
            std::lock_guard<std::mutex> lk(m);
            done_cv.notify_all();
        }
        return true;
    }
};
struct RowPool {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::shared_ptr<RowJob>> q;                            // in priority order: gathers (they feed the pipeline) before scatters
    unsigned started = 0;
    void loop()
    {
        for (;;) {
            std::shared_ptr<RowJob> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    while (!q.empty() && q.front()->exhausted()) q.pop_front();
                    for (auto& c : q) if (!c->exhausted()) { j = c; break; }
                    if (j) break;
                    cv.wait(lk);
                }
            }
            j->work_one();                                            // one chunk, then look again: a more urgent job may have arrived
        }
    }
    // threads_knob: the host_threads knob (0: automatic)
    static unsigned want_threads(int threads_knob)
    {
        if (threads_knob > 0) return (unsigned)threads_knob;
        // a quarter of the hardware threads, at least 8 where the host has them, at most 64 -- and never more than the host has
        const unsigned hc = std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 1u;
        unsigned t = hc / 4;
        t = t < 8 ? 8 : (t > 64 ? 64 : t);
        return t > hc ? hc : t;
    }
    // queues the job and returns at once; wait() (which also works on it) before anything it touches is reused
    std::shared_ptr<RowJob> submit(int64_t n, std::function<void(int64_t)> f, bool urgent, int threads_knob)
    {
        const unsigned want = want_threads(threads_knob);
        auto j = std::make_shared<RowJob>();
        j->f = std::move(f); j->n = n;
        j->chunk = n / ((int64_t)want * 4) > 0 ? n / ((int64_t)want * 4) : 1;
        j->remaining.store(n);
        {
            std::lock_guard<std::mutex> lk(mu);
            while (started + 1 < want) {                              // (the submitting thread works too)
                try { std::thread(&RowPool::loop, this).detach(); }
                catch (const std::system_error&) { break; }           // no more threads to be had: fewer helpers, same result
                started++;
            }
            if (urgent) q.push_front(j); else q.push_back(j);
        }
        cv.notify_all();
        return j;
    }
    void wait(const std::shared_ptr<RowJob>& j)
    {
        while (j->work_one()) {}
        std::unique_lock<std::mutex> lk(j->m);
        j->done_cv.wait(lk, [&] { return j->remaining.load(std::memory_order_acquire) == 0; });
    }
    void run(int64_t n, std::function<void(int64_t)> f, int threads_knob) { wait(submit(n, std::move(f), true, threads_knob)); }
};
inline RowPool* row_pool()
{
    static RowPool* p = new RowPool();                               // never destroyed: its threads outlive main()
    return p;
}

// the calling thread's to copy: too few bytes, or one row
inline bool rows_are_small(int64_t n, int64_t bytes, const HostLimits& limits) { return bytes < limits.pool_floor || n < 2; }

// f(i) for i in [0, n): on the calling thread for small jobs, on the row pool for large ones.
template <class F>
void for_rows(int64_t n, int64_t bytes, const HostLimits& limits, int threads_knob, F f)
{
    if (rows_are_small(n, bytes, limits)) { for (int64_t i = 0; i < n; i++) f(i); return; }
    try { row_pool()->run(n, std::function<void(int64_t)>(f), threads_knob); }
    catch (const std::bad_alloc&) { for (int64_t i = 0; i < n; i++) f(i); }   // (idempotent copies: doing them again is harmless)
}

// ---- the row work of a slice ---------------------------------------------------------------------------------------------------------
inline const uint8_t* src_row(const lz4hip_batch_t* hb, int64_t i) { return (const uint8_t*)hb->src + (hb->src_off ? hb->src_off[i] : i * hb->src_stride); }
inline uint8_t* dst_row(const lz4hip_batch_t* hb, int64_t i) { return (uint8_t*)hb->dst + (hb->dst_off ? hb->dst_off[i] : i * hb->dst_stride); }
inline int32_t src_len(const lz4hip_batch_t* hb, int64_t i) { return hb->src_len ? hb->src_len[i] : hb->src_len_all; }
inline int32_t dst_cap(const lz4hip_batch_t* hb, int64_t i) { return hb->dst_cap ? hb->dst_cap[i] : hb->dst_cap_all; }

// rows [first, first + cnt) into a pinned "in" image: lengths, capacities, the gathered rows
inline void stage_in(const lz4hip_batch_t* hb, const HostPlan& p, int64_t first, int64_t cnt, uint8_t* pi, const HostLimits& limits, int threads_knob)
{
    int32_t* lens = (int32_t*)(pi + p.in_lens);
    int32_t* caps = (int32_t*)(pi + p.in_caps);
    for (int64_t j = 0; j < cnt; j++) { lens[j] = src_len(hb, first + j); caps[j] = dst_cap(hb, first + j); }
    const int64_t s_stride = p.s_stride;
    for_rows(cnt, cnt * s_stride, limits, threads_knob, [=](int64_t j) {
        const int32_t sl = src_len(hb, first + j);
        if (sl > 0) memcpy(pi + s_stride * j, src_row(hb, first + j), (size_t)sl);
    });
}

// row first + j out of a pinned "out" image: the bytes the caller gets back are the result for encoders / unknown-size decode
// (dst_len_is_result), the full size for known-size decode -- nothing of a failed block, never more than the capacity
inline void scatter_row(const lz4hip_batch_t* hb, bool dst_len_is_result, int64_t d_stride, const uint8_t* po, const int32_t* res, int64_t first, int64_t j)
{
    const int32_t cap = dst_cap(hb, first + j);
    int64_t nbytes = dst_len_is_result ? res[j] : cap;
    if (!dst_len_is_result && res[j] < 0) nbytes = 0;
    if (nbytes > cap) nbytes = cap;
    if (nbytes > 0) memcpy(dst_row(hb, first + j), po + d_stride * j, (size_t)nbytes);
}

// Rows [first, first + cnt) out of a pinned "out" image into the caller's buffers.  The results are the caller's on return; the rows
// of a large slice are copied by the row pool WITHOUT the calling thread waiting for them -- that thread goes on gathering the next
// slice (round 3 did gather k+1 and scatter k-1 one after the other: ~23 of the 34 ms of a 16 384-block decode) -- and then the job
// comes back: the image may be reused only after RowPool::wait() on it.
inline std::shared_ptr<RowJob> scatter(const lz4hip_batch_t* hb, bool dst_len_is_result, const HostPlan& p, int64_t first, int64_t cnt, const uint8_t* po,
                                       const HostLimits& limits, int threads_knob)
{
    const int32_t* res = (const int32_t*)(po + p.out_res);
    for (int64_t j = 0; j < cnt; j++) hb->result[first + j] = res[j];
    const int64_t d_stride = p.d_stride;
    auto row = [=](int64_t j) { scatter_row(hb, dst_len_is_result, d_stride, po, res, first, j); };
    if (!rows_are_small(cnt, cnt * d_stride, limits)) {
        try { return row_pool()->submit(cnt, std::function<void(int64_t)>(row), false, threads_knob); }
        catch (const std::bad_alloc&) {}
    }
    for (int64_t j = 0; j < cnt; j++) row(j);
    return nullptr;
}

// the batch the kernels of a slice of cnt rows see: its rows at their strides in the slot's device images
inline lz4hip_batch_t device_batch(const HostPlan& p, uint8_t* d_in, uint8_t* d_out, int64_t cnt)
{
    lz4hip_batch_t db;
    db.src = d_in; db.src_off = nullptr; db.src_stride = p.s_stride; db.src_len = (const int32_t*)(d_in + p.in_lens);
    db.dst = d_out; db.dst_off = nullptr; db.dst_stride = p.d_stride; db.dst_cap = (const int32_t*)(d_in + p.in_caps);
    db.dst_cap_all = 0; db.src_len_all = (int32_t)p.max_src;   /* upper-bound hint */ db.result = (int32_t*)(d_out + p.out_res); db.n_blocks = cnt;
    return db;
}

// ---- the loop ------------------------------------------------------------------------------------------------------------------------
// Stage a host batch through device memory, run `run` on it, copy results (and dst payloads) back.
// The batch is cut into slices; per slice: rows are gathered into pinned memory (host threads), the copies in, the kernels, the
// copies out into pinned memory, rows scattered to the caller.  Copies in, kernels and copies out are queued independently over
// kHostSlots sets of images: slice k+1 travels in and slice k-1 out while slice k is being processed (PCIe is full duplex),
// kernels of neighbouring slices overlap, and the host gathers / scatters next to all that.  A slot is refilled only after its
// previous slice was drained (wait_out, or a true out_done) AND that slice's scatter job finished.
// The batch has passed check_batch.  slices_knob, threads_knob: the knobs host_slices and host_threads.
template <class Stage, class Run>
int run_host_batch(Stage& st, const lz4hip_batch_t* hb, bool dst_len_is_result, Run run, int64_t slice_hint, int slices_knob, int threads_knob,
                   const HostLimits& limits = HostLimits())
{
    if (hb->n_blocks == 0) return 0;
    const HostPlan p = plan_host_batch(hb, slices_knob, slice_hint, limits);
    if (p.error) return st.fail(p.error, p.error_text);
    if (int rc = st.reserve(p.slots, p.in_bytes, p.out_bytes)) return rc;

    std::shared_ptr<RowJob> scatter_job[kHostSlots];
    auto scatter_wait = [&](int slot) {
        if (scatter_job[slot]) { row_pool()->wait(scatter_job[slot]); scatter_job[slot].reset(); }
    };
    int err = 0;
    int64_t drained = 0;                                             // slices [0, drained) are back in the caller's buffers (or with their scatter job)
    auto drain_one = [&] {                                           // (blocking)
        const int slot = (int)(drained % p.slots);
        err = st.wait_out(slot);
        if (!err) scatter_job[slot] = scatter(hb, dst_len_is_result, p, p.first(drained), p.count(drained), st.pin_out(slot), limits, threads_knob);
        drained++;
    };
    err = st.begin();
    int64_t slice = 0;
    for (; slice < p.n_slices && !err; slice++) {
        const int64_t first = p.first(slice), cnt = p.count(slice);
        const int slot = (int)(slice % p.slots);
        while (!err && drained + p.slots <= slice) drain_one();   // the slot's previous slice must be out of its images
        scatter_wait(slot);                                          // ... and in the caller's
        if (err) break;
        stage_in(hb, p, first, cnt, st.pin_in(slot), limits, threads_knob);
        if ((err = st.copy_in(slot, 0, p.rows_in(cnt)))) break;
        if ((err = st.copy_in(slot, p.in_lens, p.tail_in()))) break;
        const lz4hip_batch_t db = device_batch(p, st.dev_in(slot), st.dev_out(slot), cnt);
        if ((err = st.kernels(slot, run, db))) break;
        if ((err = st.copy_out(slot, 0, p.rows_out(cnt)))) break;
        if ((err = st.copy_out(slot, p.out_res, p.tail_out()))) break;
        // slices that have already arrived are scattered while the later ones are in flight
        while (!err && drained < slice && st.out_done((int)(drained % p.slots))) drain_one();
    }
    while (!err && drained < slice) drain_one();
    for (int k = 0; k < kHostSlots; k++) scatter_wait(k);           // (also on error: the jobs read the stage's images and the caller's batch)
    if (err) st.quiesce();
    return err;
}

// ---- a host-pointer batch decoded against one dictionary ------------------------------------------------------------------------------
// lz4hip_decode_batch_dict_host: the bytes of the dictionary that a match can reach -- its last 65 535 -- are uploaded ONCE per call, into
// staging of the stage's that is the dictionary's alone, and the upload is complete before the slice loop starts: whichever stream a
// slice's kernels run on, and whichever pipeline they belong to, they find it there.  The stage has for this
//
//     int      dict_upload(from, bytes, dev)          reserves `bytes` of device memory (grow-only), copies the host bytes there, WAITS
//                                                     for the copy, and gives the device address
//
// and make_run(device dictionary, its length) gives the `run` of the slices.
inline int64_t dict_reach(int64_t dict_len) { return dict_len < 65535 ? dict_len : 65535; }

template <class Stage>
int upload_dictionary(Stage& st, const void* dict, int64_t dict_len, const uint8_t*& d_dict, int64_t& reach)
{
    reach = dict_reach(dict_len);
    d_dict = nullptr;
    if (reach == 0) return 0;
    uint8_t* dev = nullptr;
    if (int rc = st.dict_upload((const uint8_t*)dict + (dict_len - reach), reach, dev)) return rc;
    d_dict = dev;
    return 0;
}

template <class Stage, class MakeRun>
int run_host_batch_dict(Stage& st, const lz4hip_batch_t* hb, const void* dict, int64_t dict_len, bool dst_len_is_result, MakeRun make_run,
                        int slices_knob, int threads_knob, const HostLimits& limits = HostLimits())
{
    if (hb->n_blocks == 0) return 0;
    const uint8_t* d_dict = nullptr;
    int64_t reach = 0;
    if (int rc = upload_dictionary(st, dict, dict_len, d_dict, reach)) return rc;
    return run_host_batch(st, hb, dst_len_is_result, make_run(d_dict, reach), 0, slices_knob, threads_knob, limits);
}

// lz4hip_encode_batch_dict_host (dict_len > 0): the same upload, then the dictionary's primed table (lz4hip_encode_dict.hpp) ONCE per
// call, into staging of its own, complete before the slice loop starts as the upload is.  The stage has for this
//
//     int      dict_prime(device dictionary, bytes, table)   reserves the table's 16 KiB (grow-only), builds it from the uploaded bytes,
//                                                            WAITS for that, and gives its device address
//
// make_run(device dictionary, its length, the table) gives the `run` of the slices, which are the plain encode's (slice_hint:
// encode_host_slice_blocks).
template <class Stage, class MakeRun>
int run_host_batch_encode_dict(Stage& st, const lz4hip_batch_t* hb, const void* dict, int64_t dict_len, MakeRun make_run, int64_t slice_hint,
                               int slices_knob, int threads_knob, const HostLimits& limits = HostLimits())
{
    if (hb->n_blocks == 0) return 0;
    const uint8_t* d_dict = nullptr;
    int64_t reach = 0;
    if (int rc = upload_dictionary(st, dict, dict_len, d_dict, reach)) return rc;
    uint8_t* table = nullptr;
    if (int rc = st.dict_prime(d_dict, reach, table)) return rc;
    return run_host_batch(st, hb, true, make_run(d_dict, reach, (const uint8_t*)table), slice_hint, slices_knob, threads_knob, limits);
}

// ---- the decoded sizes of a host-pointer batch ---------------------------------------------------------------------------------------
// lz4hip_decoded_sizes_host: the rows are gathered back to back (the row work above), staged with their lengths in ONE device image of
// the framing backend B, sized by the device call (framing::decoded_sizes), and only result, dst_off, dst_cap and info come back -- no
// block payload travels in that direction.  Every row is needed before the offsets can be scanned, so there are no slices here.
template <class B>
int decoded_sizes_host(B& be, const lz4hip_batch_t* hb, int64_t* dst_off, int32_t* dst_cap, lz4hip_sizes_info_t* info, int groups, int threads_knob,
                       const HostLimits& limits = HostLimits(), int64_t dict_len = -1)       // (dict_len: framing::decoded_sizes)
{
    if (!hb) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: batch descriptor is NULL");
    const int64_t n = hb->n_blocks;
    if (n < 0) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: n_blocks < 0");
    if (n > 0x7FFFFFFF) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: more than 2^31 - 1 blocks");
    if (n == 0) {
        if (dst_off) dst_off[0] = 0;
        if (info) { lz4hip_sizes_info_t r = {}; r.first_error = -1; *info = r; }
        return 0;
    }
    if (!hb->src) return be.fail(LZ4HIP_E_ARGUMENT, "decoded sizes: src must be non-NULL");
    std::vector<int64_t> at;
    std::vector<int32_t> lens;
    std::vector<uint8_t> rows;
    int64_t total = 0;
    try {
        at.resize((size_t)n); lens.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int32_t sl = src_len(hb, i);
            if (sl < 0) return be.fail(LZ4HIP_E_ARGUMENT, "negative source length");
            at[(size_t)i] = total; lens[(size_t)i] = sl; total += sl;
        }
        rows.resize((size_t)total);
    } catch (const std::bad_alloc&) { return be.fail(LZ4HIP_E_MEMORY, "decoded sizes: no host memory to gather the rows in"); }
    uint8_t* const packed = rows.data();
    const int64_t* const at_p = at.data();
    const int32_t* const len_p = lens.data();
    for_rows(n, total, limits, threads_knob, [=](int64_t i) {
        if (len_p[i] > 0) memcpy(packed + at_p[i], src_row(hb, i), (size_t)len_p[i]);
    });
    // device image: [rows | offsets | lengths | results | sizes | output offsets | info | scratch]
    const int64_t scratch_bytes = framing::sizes_scratch_bytes(n);
    Carver c;
    c.take(total);
    const int64_t off_at = c.take(8 * n), len_at = c.take(4 * n), res_at = c.take(4 * n), cap_at = c.take(4 * n), doff_at = c.take(8 * (n + 1)),
                  info_at = c.take(256), scratch_at = c.take(scratch_bytes);
    framing::Image<B> im = { be };
    if (int rc = im.reserve(c.at)) return rc;
    if (int rc = im.upload_source(packed, total)) return rc;
    if (int rc = im.upload(off_at, at_p, 8 * n)) return rc;
    if (int rc = im.upload(len_at, len_p, 4 * n)) return rc;
    lz4hip_batch_t db = {};
    db.src = im.d; db.src_off = im.i64(off_at); db.src_len = im.i32(len_at); db.result = im.i32(res_at); db.n_blocks = n;
    if (int rc = framing::decoded_sizes(be, &db, im.i64(doff_at), im.i32(cap_at), im.d + scratch_at, scratch_bytes,
                                        (lz4hip_sizes_info_t*)(im.d + info_at), groups, dict_len)) return rc;
    if (hb->result) if (int rc = im.download(hb->result, res_at, 4 * n)) return rc;
    if (dst_off) if (int rc = im.download(dst_off, doff_at, 8 * (n + 1))) return rc;
    if (dst_cap) if (int rc = im.download(dst_cap, cap_at, 4 * n)) return rc;
    if (info) if (int rc = im.download(info, info_at, sizeof *info)) return rc;
    return be.sync();                                                  // (also what keeps the gathered rows alive until the upload has read them)
}

// ---- a host-pointer batch encoded into, or decoded into, one packed buffer -------------------------------------------------------------------
// lz4hip_encode_packed_host and lz4hip_decode_compact_host: the rows, strided or at offsets, are gathered back to back, once (the row work
// above, as decoded_sizes_host does), staged with their offsets, lengths and limits in ONE device image of the framing backend B and
// run through the device call (`device`: framing::encode_packed or framing::decode_compact on the image's batch, output, offsets, lengths,
// scratch and info).  The info comes back first; then the per-block arrays and only min(the bytes the batch took, dst_cap) bytes of
// output.  The image's output piece is min(dst_cap, the sum of the per-block limits): no batch can take more, so a generous dst_cap
// costs no device memory.  A negative src_len[i] travels as it is -- the device sequence keeps it from the block codec and gives that
// block its LZ4HIP_E_ARGUMENT result -- and gathers no bytes.  The batch has passed the call's argument checks and is not empty.
// `total`: the info's count of those bytes.
template <class B, class Info, class Device>
int packed_host_run(B& be, const lz4hip_batch_t* hb, int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* out_len,
                    Info* info, int64_t Info::*total_bytes, const char* no_memory, int threads_knob, const HostLimits& limits, Device device)
{
    const int64_t n = hb->n_blocks;
    Info h = {};
    std::vector<int64_t> at;
    std::vector<int32_t> lens;
    std::vector<uint8_t> rows;
    int64_t total = 0, most = 0;
    try {
        at.resize((size_t)n); lens.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int32_t sl = src_len(hb, i), lim = hb->dst_cap && hb->dst_cap[i] < hb->dst_cap_all ? hb->dst_cap[i] : hb->dst_cap_all;
            const int32_t cap = lim < 0 ? 0 : lim;
            at[(size_t)i] = total; lens[(size_t)i] = sl; total += sl > 0 ? sl : 0; most += cap;
        }
        rows.resize((size_t)total);
    } catch (const std::bad_alloc&) { return be.fail(LZ4HIP_E_MEMORY, no_memory); }
    uint8_t* const packed = rows.data();
    const int64_t* const at_p = at.data();
    const int32_t* const len_p = lens.data();
    for_rows(n, total, limits, threads_knob, [=](int64_t i) {
        if (len_p[i] > 0) memcpy(packed + at_p[i], src_row(hb, i), (size_t)len_p[i]);
    });
    // device image: [rows | offsets | lengths | limits | results | lengths out | output offsets | info | scratch | output]
    const int64_t out_bytes = dst_cap < most ? dst_cap : most;
    Carver c;
    c.take(total);
    const int64_t off_at = c.take(8 * n), len_at = c.take(4 * n), cap_at = c.take(4 * n), res_at = c.take(4 * n), plen_at = c.take(4 * n),
                  doff_at = c.take(8 * (n + 1)), info_at = c.take(256), scratch_at = c.take(scratch_bytes), out_at = c.take(out_bytes);
    framing::Image<B> im = { be };
    if (int rc = im.reserve(c.at)) return rc;
    if (int rc = im.upload_source(packed, total)) return rc;
    if (int rc = im.upload(off_at, at_p, 8 * n)) return rc;
    if (int rc = im.upload(len_at, len_p, 4 * n)) return rc;
    if (hb->dst_cap) if (int rc = im.upload(cap_at, hb->dst_cap, 4 * n)) return rc;
    lz4hip_batch_t db = {};
    db.src = im.d; db.src_off = im.i64(off_at); db.src_len = im.i32(len_at); db.src_len_all = hb->src_len_all;      /* upper-bound hint */
    db.dst_cap = hb->dst_cap ? im.i32(cap_at) : nullptr; db.dst_cap_all = hb->dst_cap_all; db.result = im.i32(res_at); db.n_blocks = n;
    if (int rc = device(&db, im.d + out_at, out_bytes, im.i64(doff_at), im.i32(plen_at), im.d + scratch_at, (Info*)(im.d + info_at))) return rc;
    if (int rc = im.download(&h, info_at, sizeof h)) return rc;
    if (int rc = be.sync()) return rc;                                 // (also what keeps the gathered rows alive until the upload has read them)
    if (info) *info = h;
    if (hb->result) if (int rc = im.download(hb->result, res_at, 4 * n)) return rc;
    if (int rc = im.download(dst_off, doff_at, 8 * (n + 1))) return rc;
    if (out_len) if (int rc = im.download(out_len, plen_at, 4 * n)) return rc;
    return im.download_encoded(dst, out_at, h.*total_bytes < out_bytes ? h.*total_bytes : out_bytes);
}

// the argument checks are the device call's and run first (framing::encode_packed_check); info may be NULL
template <class B>
int encode_packed_host(B& be, const lz4hip_batch_t* hb, int mode, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                       int32_t* packed_len, lz4hip_packed_info_t* info, int threads_knob, const HostLimits& limits = HostLimits())
{
    if (int rc = framing::encode_packed_check(be, hb, mode, round_blocks, dst, dst_cap, dst_off)) return rc;
    if (hb->n_blocks == 0) {
        lz4hip_packed_info_t h = {};
        dst_off[0] = 0;
        h.first_failed = -1;
        if (info) *info = h;
        return 0;
    }
    const int64_t scratch_bytes = framing::encode_packed_scratch_bytes(hb->n_blocks, hb->dst_cap_all, round_blocks);
    return packed_host_run(be, hb, scratch_bytes, dst, dst_cap, dst_off, packed_len, info, &lz4hip_packed_info_t::packed_bytes,
                           "encode packed: no host memory to gather the rows in", threads_knob, limits,
                           [&](const lz4hip_batch_t* db, uint8_t* out, int64_t out_bytes, int64_t* doff, int32_t* plen, uint8_t* scratch, lz4hip_packed_info_t* dinfo) {
                               return framing::encode_packed(be, db, mode, round_blocks, out, out_bytes, doff, plen, scratch, scratch_bytes, dinfo);
                           });
}

// lz4hip_decode_compact_host.  The caller has run the device call's argument checks (framing::decode_compact_check) before it looked
// for a device; info may be NULL.
template <class B>
int decode_compact_host(B& be, const lz4hip_batch_t* hb, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                        int32_t* decoded_len, lz4hip_compact_info_t* info, int threads_knob, const HostLimits& limits = HostLimits())
{
    if (int rc = framing::decode_compact_check(be, hb, round_blocks, dst, dst_cap, dst_off)) return rc;
    if (hb->n_blocks == 0) {
        lz4hip_compact_info_t h = {};
        dst_off[0] = 0;
        h.first_failed = -1;
        if (info) *info = h;
        return 0;
    }
    const int64_t scratch_bytes = framing::decode_compact_scratch_bytes(hb->n_blocks, hb->dst_cap_all, round_blocks);
    return packed_host_run(be, hb, scratch_bytes, dst, dst_cap, dst_off, decoded_len, info, &lz4hip_compact_info_t::decoded_bytes,
                           "decode compact: no host memory to gather the rows in", threads_knob, limits,
                           [&](const lz4hip_batch_t* db, uint8_t* out, int64_t out_bytes, int64_t* doff, int32_t* dlen, uint8_t* scratch, lz4hip_compact_info_t* dinfo) {
                               return framing::decode_compact(be, db, round_blocks, out, out_bytes, doff, dlen, scratch, scratch_bytes, dinfo);
                           });
}

// ---- the shards of the multi-device form -----------------------------------------------------------------------------------------------
// Block i belongs to shard i mod nd -- the partition of SURVEY.md 8e / BASELINE configs[4]: shard k holds blocks k, k + nd, ... as an
// offset-addressed batch over the caller's buffers with lengths, capacities and results of its own (none at all when n <= k).
struct Shard {
    std::vector<int64_t> src_off, dst_off;
    std::vector<int32_t> src_len, dst_cap, result;
    lz4hip_batch_t b;
    int rc = 0;                                                      // what the shard's run returned, and its text
    std::string err;
};

inline std::vector<Shard> shard_batch(const lz4hip_batch_t* hb, int nd)
{
    const int64_t n = hb->n_blocks;
    std::vector<Shard> shards((size_t)nd);
    for (int k = 0; k < nd; k++) {
        Shard& sh = shards[(size_t)k];
        const int64_t cnt = n > k ? (n - k + nd - 1) / nd : 0;
        sh.src_off.resize((size_t)cnt); sh.dst_off.resize((size_t)cnt);
        sh.src_len.resize((size_t)cnt); sh.dst_cap.resize((size_t)cnt); sh.result.assign((size_t)cnt, 0);
        for (int64_t j = 0; j < cnt; j++) {
            const int64_t i = j * nd + k;
            sh.src_off[(size_t)j] = hb->src_off ? hb->src_off[i] : i * hb->src_stride;
            sh.dst_off[(size_t)j] = hb->dst_off ? hb->dst_off[i] : i * hb->dst_stride;
            sh.src_len[(size_t)j] = src_len(hb, i);
            sh.dst_cap[(size_t)j] = dst_cap(hb, i);
        }
        sh.b = *hb;
        sh.b.src_off = sh.src_off.data(); sh.b.dst_off = sh.dst_off.data();
        sh.b.src_len = sh.src_len.data(); sh.b.dst_cap = sh.dst_cap.data();
        sh.b.result = sh.result.data(); sh.b.n_blocks = cnt;
    }
    return shards;
}

// The shards' results into the caller's array, in global order.  The first shard that failed ends it: its code is returned and
// `error` names its device (devs[k]: the device shard k ran on) and its text; the results of the shards before it have landed.
inline int merge_shards(const lz4hip_batch_t* hb, const std::vector<Shard>& shards, const int* devs, std::string& error)
{
    const int64_t nd = (int64_t)shards.size();
    for (int64_t k = 0; k < nd; k++) {
        const Shard& sh = shards[(size_t)k];
        if (sh.rc) { error = "device " + std::to_string(devs[k]) + ": " + sh.err; return sh.rc; }
        for (int64_t j = 0; j < sh.b.n_blocks; j++) hb->result[j * nd + k] = sh.result[(size_t)j];
    }
    return 0;
}

}  // namespace hostbatch
}  // namespace lz4hip
