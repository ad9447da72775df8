// lz4hip_api.hip -- host side of liblz4hip.so: the C ABI declared in include/lz4hip.h.
//
// Only launches the gfx950 kernels of this directory; there is deliberately NO CPU code path for
// the codec here (a missing/unsupported device is an error, never a fallback).
#include "lz4hip_wave.hpp"

#include "lz4hip_common.hpp"
#include "lz4hip_decode.hpp"
#include "lz4hip_decode_lane4.hpp"
#ifdef LZ4HIP_TUNING_BUILD            /* superseded generations, for same-box A/B runs only (tools/ab/) */
#include "../../tools/ab/lz4hip_decode_lane.hpp"
#include "../../tools/ab/lz4hip_decode_lane3.hpp"
#include "../../tools/ab/lz4hip_hc_lane.hpp"
#include "../../tools/ab/lz4hip_hc_nat_lane.hpp"
#endif
#include "lz4hip_encode.hpp"
#include "lz4hip_encode_dict.hpp"
#include "lz4hip_encode_lane.hpp"
#include "lz4hip_hc.hpp"
#include "lz4hip_hc_conv.hpp"
#include "lz4hip_hc_nat.hpp"
#include "lz4hip_hc_lcp.hpp"
#include "lz4hip_synth.hpp"
#include "lz4hip_stream.hpp"
#include "lz4hip_wrap.hpp"
#include "lz4hip_streams.hpp"
#include "lz4hip_framing.hpp"
#include "lz4hip_hostbatch.hpp"

#include "../../include/lz4hip.h"

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace lz4hip;
using namespace lz4hip::framing;
using lz4hip::hostbatch::kHostSlots;
using lz4hip::hostbatch::kHcHostSliceBlocks;

namespace {

thread_local std::string g_last_error;

// Launch counters per kernel family (lz4hip_dispatch_counts): what the tests assert so that a test that names a
// mapping is known to have run it.
std::atomic<uint64_t> g_dispatch[LZ4HIP_K_COUNT];
void count_dispatch(int k) { g_dispatch[k].fetch_add(1, std::memory_order_relaxed); }

// Named integer knobs (lz4hip_tuning_set / _get).  Each one takes its initial value from the environment ONCE, the
// first time any knob is looked at; after that the launch paths read an atomic and never call getenv().
// Mappings: 0 = automatic, 1 = one wavefront per block, 2 = one lane per block.
enum Knob { kKnobDecoder = 0, kKnobEncoder, kKnobHc, kKnobEncoderWavesPerCu, kKnobHcWavesPerCu, kKnobHcGroups,
            kKnobHostThreads, kKnobHostSlices, kKnobLogicalDevices, kKnobDecoderGen, kKnobDecoderRing, kKnobHcGen, kKnobHcCtrlEvery, kKnobHcCtrlLanes, kKnobHcSubChunks, kKnobDecoderPersist, kKnobDecoderGroups, kKnobEncoderSlabTries, kKnobEncoderWaveVersion, kKnobEncoderWg5, kKnobHostWorkers, kKnobDecoderWg4, kKnobDecoderWrappedStores, kKnobSizesGroups, kKnobCount };
struct KnobInfo { const char* name; const char* env; bool mapping; };
const KnobInfo kKnobInfo[kKnobCount] = {
    { "decoder", "LZ4HIP_DECODER", true }, { "encoder", "LZ4HIP_ENCODER", true }, { "hc", "LZ4HIP_HC", true },
    { "encoder_waves_per_cu", "LZ4HIP_ENCODER_WAVES_PER_CU", false }, { "hc_waves_per_cu", "LZ4HIP_HC_WAVES_PER_CU", false },
    { "hc_groups", "LZ4HIP_HC_GROUPS", false },                     // persistent grid of the LZ4HC lane kernel (tests: few lanes, many blocks each)
    { "host_threads", "LZ4HIP_HOST_THREADS", false }, { "host_slices", "LZ4HIP_HOST_SLICES", false },
    { "logical_devices", "LZ4HIP_LOGICAL_DEVICES", false },         // tests: N workers of the multi-device path over the visible devices (wrapping around)
    { "decoder_gen", "LZ4HIP_DECODER_GEN", false },                 // lane decoder: 0 default = 4 lz4hip_decode_lane4.hpp; 2 and 3 (tools/ab/) only in LZ4HIP_TUNING_BUILD libraries
    { "decoder_ring", "LZ4HIP_DECODER_RING", false },               // generation 4: ring bytes + 1000 x variant (0 default; other configurations only in LZ4HIP_TUNING_BUILD libraries)
    { "hc_gen", "LZ4HIP_HC_GEN", false },                           // LZ4HC lane mapping: 0 default; 4 lz4hip_hc_lcp.hpp (blocks <= 64 KiB), 2 lz4hip_hc_conv.hpp (larger blocks; <= 64 KiB in tuning builds); 1 lz4hip_hc_lane.hpp and 3 lz4hip_hc_nat.hpp in tuning builds only
    { "hc_ctrl_every", "LZ4HIP_HC_CTRL_EVERY", false }, { "hc_ctrl_lanes", "LZ4HIP_HC_CTRL_LANES", false },   // lz4hip_hc_lcp.hpp: control-flow batching (0 default)
    { "hc_sub_chunks", "LZ4HIP_HC_SUB_CHUNKS", false },             // LZ4HC lane launch: sub-chunks whose table builders and lane kernels overlap (0 default = 2, 1 = one after the other, max 8)
    { "decoder_persist", "LZ4HIP_DECODER_PERSIST", false },         // lane decoder, default configuration: 0 the device picks one block per lane or the persistent grid, 1 always persistent, 2 never
    { "decoder_groups", "LZ4HIP_DECODER_GROUPS", false },           // tests: wavefronts of the persistent lane decoder's grid (0 = the residency): few lanes, many restarts each
    { "encoder_slab_tries", "LZ4HIP_ENCODER_SLAB_TRIES", false },   // lane encoder's table slab: candidate placements that are built and measured (0 default = 4; 1 = the first one, unmeasured)
    { "encoder_wave_version", "LZ4HIP_ENCODER_WAVE_VERSION", false },   // wavefront-mapped fast encoder, blocks < 64 KiB + 11: 0 default = 2 (encode_fast_block64k); 1 = the first version, in LZ4HIP_TUNING_BUILD libraries only
    { "encoder_wg5", "LZ4HIP_ENCODER_WG5", false },                   // wavefront-mapped fast encoder: 0 default = workgroups of FIVE blocks (80 KiB of LDS: two per CU = ten blocks) wherever that saves a residency round against one-block workgroups (nine per CU: 16 KiB is thirteen of the CU's 128 LDS granules of 1 280 bytes); 1 = always one block per workgroup (rounds 1-5); 2 = five per workgroup whatever the batch size (tests, A/B runs)
    { "host_workers", "LZ4HIP_HOST_WORKERS", false },                 // single-device host-pointer batches of >= 8192 blocks: staging pipelines (persistent worker threads) that share the device, each taking every k-th block (0 default = 2 for decode, 1 for the encoders; 1 = the calling thread's pipeline alone, rounds 2-5)
    { "decoder_wg4", "LZ4HIP_DECODER_WG4", false },                   // lane decoder, batches of at most one residency round: 0 default = workgroups of FOUR wavefronts (one per SIMD of a CU) while the batch has more than one wavefront per CU and at most one residency round; 1 = always workgroups of one wavefront (rounds 1-5); 2 = the four-wavefront form from four wavefronts on (tests); 3 = whatever the batch size (A/B runs)
    { "decoder_wrapped_stores", "LZ4HIP_DECODER_WRAPPED_STORES", false },   // lane decoder: 1 = the instantiation that WRAPS its ring rows (no LDS store outside the allocation) whatever the device's probe said; 0 default = what the probe allows (read-only twin: "decoder_dual_store")
    { "sizes_groups", "LZ4HIP_SIZES_GROUPS", false },                 // lz4hip_decoded_sizes_*: wavefronts of the walk's grid (0 default = one wavefront per 64 blocks; tests: few wavefronts, many blocks per lane)
};
std::atomic<int> g_knob[kKnobCount];
std::once_flag g_knob_once;
void knobs_init()
{
    std::call_once(g_knob_once, [] {
        for (int k = 0; k < kKnobCount; k++) {
            const char* e = getenv(kKnobInfo[k].env);
            int v = 0;
            if (e && kKnobInfo[k].mapping) v = e[0] == 'w' ? 1 : (e[0] == 'l' ? 2 : 0);
            else if (e) v = atoi(e);
            g_knob[k].store(v < 0 ? 0 : v, std::memory_order_relaxed);
        }
    });
}
int knob(int k) { knobs_init(); return g_knob[k].load(std::memory_order_relaxed); }

// A lone wavefront of the lane mapping needs milliseconds for its 64 blocks, so the mapping only pays once the
// batch fills the GPU (measured crossover 13 k (D2) .. 28 k (D3) blocks, profiles/r01/decode_small_batches.txt).
constexpr int64_t kLaneDecodeMinBlocks = 16384;
constexpr int64_t kLaneEncodeMinBlocks = 49152;  // a lane needs 60 - 110 ms for its block whatever the batch: the wavefront mapping alone is faster up to ~46 k (D2) /
                                                // ~58 k (D3) blocks since its second version (profiles/r06/encoder_mapping_crossover.txt; round 5: 32768, until then 16384)
constexpr int kLaneDecodeGeneration = 4;
constexpr int kLane4Config = 59192;          // lane decoder: 192-byte ring, 32-byte input pieces out of whole 64-byte sectors, 128-byte flush units; iterations
                                              // alternate between flushing (two store instructions) and requesting input (four load instructions, one sector)
constexpr int kHcLaneGeneration = 4;           // blocks <= 64 KiB; larger ones: 2

int fail(int code, const std::string& what)
{
    g_last_error = what;
    return code;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(e_ == hipErrorOutOfMemory ? LZ4HIP_E_MEMORY : LZ4HIP_E_DEVICE,          \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                     \
    } while (0)

Batch to_device_batch(const lz4hip_batch_t& b)
{
    Batch d;
    d.src = (const uint8_t*)b.src; d.src_off = b.src_off; d.src_stride = b.src_stride; d.src_len = b.src_len;
    d.dst = (uint8_t*)b.dst; d.dst_off = b.dst_off; d.dst_stride = b.dst_stride; d.dst_cap = b.dst_cap;
    d.dst_cap_all = b.dst_cap_all; d.src_len_all = b.src_len_all; d.result = b.result; d.n_blocks = b.n_blocks;
    return d;
}

int check_batch(const lz4hip_batch_t* b)
{
    if (!b) return fail(LZ4HIP_E_ARGUMENT, "batch descriptor is NULL");
    if (b->n_blocks < 0) return fail(LZ4HIP_E_ARGUMENT, "n_blocks < 0");
    if (b->n_blocks > 0 && (!b->src || !b->dst || !b->result))
        return fail(LZ4HIP_E_ARGUMENT, "src, dst and result must be non-NULL");
    if (b->n_blocks > 0x7FFFFFFF) return fail(LZ4HIP_E_ARGUMENT, "n_blocks too large for one launch");
    return 0;
}

// ---- grow-only per-thread device scratch for the host-pointer entry points --------------------
struct Scratch {
    void* p = nullptr; size_t cap = 0; int dev = -1;
    int reserve(size_t n)
    {
        int dev_now = 0;
        HIP_TRY(hipGetDevice(&dev_now));
        if (p && (dev_now != dev || n > cap)) { (void)hipFree(p); p = nullptr; cap = 0; }
        if (!p) {
            size_t want = n < (1u << 20) ? (1u << 20) : n;
            HIP_TRY(hipMalloc(&p, want));
            cap = want; dev = dev_now;
        }
        return 0;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
    ~Scratch() { /* the HIP runtime may already be gone at thread exit: leak on purpose */ }
};

// Per-device kernel workspaces (hash tables of the lane encoder, LZ4HC heads/chains): grow-only, shared by every
// caller of the device.  Kernels that use one must not overlap, whatever streams they were queued on, so a user
// takes a LEASE: the mutex is held while its work is being queued, its stream first waits for the previous user's
// completion event, and the release records the new one.  (GPU-side ordering only; the host never blocks on it.)
struct HcWorkspace {
    void* p = nullptr; size_t cap = 0;
    hipEvent_t last = nullptr; bool busy = false;
    std::mutex mu;
};

struct Lease {
    HcWorkspace* w = nullptr;
    std::unique_lock<std::mutex> lock;
    void* p = nullptr;
    hipStream_t stream = nullptr;
    bool queued = false;         // kernels that use the workspace have been queued on `stream`
    std::vector<hipStream_t> side;   // ... and on these streams of the library's own (the LZ4HC sub-chunk pipeline)
    // An error return between the first launch and lease_end() must not leave those kernels unaccounted for: the next user
    // (possibly on another stream) would overwrite tables that are still being read.  Work on the side streams is not behind
    // `stream` yet on that path, so it is waited for here (an error path: blocking the host is acceptable).
    ~Lease()
    {
        if (!(w && lock.owns_lock() && queued)) return;
        for (hipStream_t s : side) (void)hipStreamSynchronize(s);
        if (w->last && hipEventRecord(w->last, stream) == hipSuccess) w->busy = true;
    }
};

// Takes the lock on the device's workspace and makes `stream` wait for its previous user.
int lease_begin(HcWorkspace& w, hipStream_t stream, Lease& l)
{
    l.w = &w;
    l.stream = stream;
    l.lock = std::unique_lock<std::mutex>(l.w->mu);
    if (!l.w->last) HIP_TRY(hipEventCreateWithFlags(&l.w->last, hipEventDisableTiming));
    if (l.w->busy) HIP_TRY(hipStreamWaitEvent(stream, l.w->last, 0));
    return 0;
}
// Makes the leased workspace at least `bytes` large (nonzero return: could not be allocated; the lease stays valid).
int lease_reserve(Lease& l, size_t bytes)
{
    HcWorkspace& w = *l.w;
    if (w.cap < bytes) {
        if (w.p) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(w.p); w.p = nullptr; w.cap = 0; w.busy = false; }
        if (hipMalloc(&w.p, bytes) != hipSuccess) { (void)hipGetLastError(); w.p = nullptr; return fail(LZ4HIP_E_MEMORY, "workspace allocation failed"); }
        w.cap = bytes;
    }
    l.p = w.p;
    return 0;
}
// Everything queued on `stream` so far is this user's work on the workspace.
int lease_end(Lease& l, hipStream_t stream)
{
    l.queued = false;                                                // (recorded here; nothing left for the destructor)
    HIP_TRY(hipEventRecord(l.w->last, stream));
    l.w->busy = true;
    l.lock.unlock();
    return 0;
}

// The lane encoder's table slab (lz4hip_encode_lane.hpp): equally sized chunks, separate allocations, because the kernel's rate is the
// device's rate of random sector read-modify-writes and that depends on how the slab is spread over device memory (20.5 G steps per second
// inside one contiguous 8 GiB allocation, 25-27 G spread out: profiles/r04/random_sectors_*.txt).  Where an allocation lands cannot be
// asked for, but it can be MEASURED: a candidate set of chunks is built and timed with slab_probe_kernel (a few milliseconds); if it is
// slower than a well spread slab, up to three more are built next to it and the fastest stays (fast_slab_reserve).
// One-time work per device and slab size; protected by the device's fast_ws lease.
struct FastSlab {
    std::vector<void*> chunks;
    unsigned tables_per_chunk = 0;   // a multiple of 64
    int64_t groups = 0;              // wavefronts the slab has tables for
    void* ctl = nullptr;             // device: the work counter (256 bytes), then the chunk pointers
    double probe = 0;                // G steps per second the placement measured (0: not measured)
    int tries = 0;
    int64_t failed_groups = 0;       // the smallest slab that could NOT be allocated, and the free device memory at that moment: a request of that
    size_t failed_free = 0;          // size or more is not tried again until more memory is free (or the workspaces were released)
    void release()
    {
        for (void* c : chunks) (void)hipFree(c);
        chunks.clear();
        if (ctl) { (void)hipFree(ctl); ctl = nullptr; }
        groups = 0; tables_per_chunk = 0; probe = 0; tries = 0; failed_groups = 0; failed_free = 0;
    }
};
constexpr int kFastSlabMaxChunks = 64;
constexpr size_t kFastSlabCtlBytes = 256 + 8 * kFastSlabMaxChunks;

// One candidate: n_chunks separate allocations of chunk_bytes.
bool fast_slab_candidate(int n_chunks, size_t chunk_bytes, std::vector<void*>& out)
{
    for (int k = 0; k < n_chunks; k++) {
        void* c = nullptr;
        if (hipMalloc(&c, chunk_bytes) != hipSuccess) {
            (void)hipGetLastError();
            for (void* q : out) (void)hipFree(q);
            out.clear();
            return false;
        }
        out.push_back(c);
    }
    return true;
}

// Makes the device's slab hold tables for `groups` wavefronts (nonzero return: could not be allocated; the lease stays valid).
int fast_slab_reserve(Lease& l, FastSlab& fs, int64_t groups)
{
    if (fs.groups >= groups && fs.ctl) return 0;
    // (a smaller slab that is already there stays until the larger one is built: a failure leaves the old one in place)
    if (fs.failed_groups > 0 && groups >= fs.failed_groups) {            // this size failed before: not again (multi-GiB hipMallocs) unless memory has been freed since
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
        if (free_b <= fs.failed_free + ((size_t)256 << 20)) return fail(LZ4HIP_E_MEMORY, "workspace allocation failed (not retried: no more device memory free than when it last failed)");
    }
    auto remember_failure = [&] {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
        if (fs.failed_groups == 0 || groups < fs.failed_groups) fs.failed_groups = groups;
        fs.failed_free = free_b;
    };
    const size_t tables = (size_t)groups * 64;
    const bool large = tables * (size_t)kLaneTableBytes >= ((size_t)2 << 30);   // below 2 GiB: one chunk, nothing to measure
    const int want_tries = !large ? 1 : (knob(kKnobEncoderSlabTries) > 0 ? knob(kKnobEncoderSlabTries) : 4);
    void* ctl = nullptr;
    if (hipMalloc(&ctl, kFastSlabCtlBytes) != hipSuccess) { (void)hipGetLastError(); return fail(LZ4HIP_E_MEMORY, "workspace allocation failed"); }
    hipStream_t ps = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    unsigned* sink = (unsigned*)((uint8_t*)ctl + 128);
    if (want_tries > 1 && (hipStreamCreateWithFlags(&ps, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) {
        (void)hipGetLastError();
        if (ps) (void)hipStreamDestroy(ps);
        if (e0) (void)hipEventDestroy(e0);
        ps = nullptr;                                                 // (no measurement then: the first candidate stays)
    }
    // Candidates: 16 chunks allocated back to back (64 for the third one).  A candidate that measures below the rate of a well spread slab
    // stays allocated while the next one is built -- so that the next one lands elsewhere -- and all but the best are freed at the end
    // (spacer allocations between the chunks spread further but cost seconds: tools/r04/call24.sh, first version).
    const double good = 24.0 * ((double)tables < 262144.0 ? (double)tables / 262144.0 : 1.0);   // G steps per second (profiles/r04/random_sectors_*.txt: 20.5 in one piece, 25-27 spread)
    std::vector<std::vector<void*>> held;
    std::vector<void*> best;
    unsigned best_tpc = 0;
    double best_rate = -1;
    int tried = 0;
    for (int r = 0; r < want_tries; r++) {
        const int n_chunks = !large ? 1 : (r == 2 ? 64 : 16);
        const unsigned tpc = (unsigned)(((groups + n_chunks - 1) / n_chunks) * 64);
        if (r > 0) {                                                   // a further candidate only while it leaves half of the free memory alone
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); break; }
            if ((size_t)n_chunks * tpc * (size_t)kLaneTableBytes > free_b / 2) break;
        }
        std::vector<void*> cand;
        if (!fast_slab_candidate(n_chunks, (size_t)tpc * (size_t)kLaneTableBytes, cand)) break;
        tried++;
        double rate = 0;
        if (ps && want_tries > 1) {
            bool ok = hipMemcpyAsync((uint8_t*)ctl + 256, cand.data(), 8 * cand.size(), hipMemcpyHostToDevice, ps) == hipSuccess
                   && hipStreamSynchronize(ps) == hipSuccess;
            const int steps = 300;
            if (ok) {
                hipLaunchKernelGGL(slab_probe_kernel, dim3((unsigned)groups), dim3(64), 0, ps, (uint8_t* const*)((uint8_t*)ctl + 256), tpc, 30, sink);   // (warm-up)
                ok = hipEventRecord(e0, ps) == hipSuccess;
                hipLaunchKernelGGL(slab_probe_kernel, dim3((unsigned)groups), dim3(64), 0, ps, (uint8_t* const*)((uint8_t*)ctl + 256), tpc, steps, sink);
                ok = ok && hipEventRecord(e1, ps) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
                float ms = 0;
                if (ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0) rate = (double)tables * steps / ms / 1e6;
            }
            if (!ok) (void)hipGetLastError();
        }
        if (rate > best_rate) { best.swap(cand); best_tpc = tpc; best_rate = rate; }   // (cand now holds the set that lost)
        if (!cand.empty()) held.push_back(std::move(cand));
        if (rate >= good || rate == 0) break;
    }
    for (auto& h : held) for (void* c : h) (void)hipFree(c);
    if (ps) { (void)hipStreamDestroy(ps); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
    if (best.empty()) { (void)hipFree(ctl); remember_failure(); return fail(LZ4HIP_E_MEMORY, "workspace allocation failed"); }
    if (hipMemcpy((uint8_t*)ctl + 256, best.data(), 8 * best.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        for (void* c : best) (void)hipFree(c);
        (void)hipFree(ctl);
        return fail(LZ4HIP_E_DEVICE, "workspace set-up failed");
    }
    if (fs.ctl) {                                                    // the old, smaller slab: its last user first
        if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
        fs.release();
        l.w->busy = false;
    }
    fs.chunks.swap(best); fs.tables_per_chunk = best_tpc; fs.groups = groups; fs.ctl = ctl; fs.probe = best_rate > 0 ? best_rate : 0; fs.tries = tried;
    fs.failed_groups = 0; fs.failed_free = 0;
    return 0;
}

// Streams and events of the pipelined LZ4HC lane launch (one set per device, created on first use; the workspace lease
// serialises its users).
constexpr int kHcSubChunks = 2, kHcMaxSubChunks = 8;   // measured at 2^18 blocks (profiles/r04/hc_sub_chunks.txt): 1 -> 15.9 / 20.8 GB/s (D2 / D3), 2 -> 16.8 / 23.2, 4 -> 15.1 / 21.0, 8 -> 11.6 / 16.7
constexpr size_t kHcCounterBytes = 256 * kHcMaxSubChunks;
struct HcPipe {
    bool ready = false;
    hipStream_t build = nullptr, lane[kHcMaxSubChunks] = {};
    hipEvent_t start = nullptr, built[kHcMaxSubChunks] = {}, done[kHcMaxSubChunks] = {};
    int init()
    {
        if (ready) return 0;
        HIP_TRY(hipStreamCreateWithFlags(&build, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&start, hipEventDisableTiming));
        for (int k = 0; k < kHcMaxSubChunks; k++) {
            HIP_TRY(hipStreamCreateWithFlags(&lane[k], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&built[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
        }
        ready = true;
        return 0;
    }
    // (lz4hip_release_workspaces, under the LZ4HC workspace's lock, after its last user's event)
    void release()
    {
        if (build) { (void)hipStreamDestroy(build); build = nullptr; }
        if (start) { (void)hipEventDestroy(start); start = nullptr; }
        for (int k = 0; k < kHcMaxSubChunks; k++) {
            if (lane[k]) { (void)hipStreamDestroy(lane[k]); lane[k] = nullptr; }
            if (built[k]) { (void)hipEventDestroy(built[k]); built[k] = nullptr; }
            if (done[k]) { (void)hipEventDestroy(done[k]); done[k] = nullptr; }
        }
        ready = false;
    }
};

// Work counters of the persistent lane decoder: a small per-device ring of 256-byte slots, one per launch in flight.  A slot comes
// back into use after 64 further launches on that device, possibly on another stream, so each slot carries an event that its
// user records after the last kernel that reads it: the next user's stream waits for that event before it zeroes the slot, and
// the slot's mutex is held from the zeroing to the record (a second host thread that draws the same slot waits for the
// first one's record, not just for its launch).  GPU-side ordering only; a stream never waits unless 64 launches are in flight.
struct CounterSlot { std::mutex mu; hipEvent_t done = nullptr; bool used = false; };
struct CounterRing { void* mem = nullptr; CounterSlot slot[64]; std::atomic<unsigned> next{ 0 }; std::mutex mu; };

// Everything the library keeps per device, shared by all its callers: facts and verdicts are kept for the life of the process once
// they are known; device memory, streams and events until lz4hip_release_workspaces().
constexpr int kMaxDevices = 64;
static_assert(kMaxDevices <= 64, "device masks (lz4hip_*_multi) are 64-bit");
struct DeviceState {
    std::atomic<int> cus{ 0 };                  // multiprocessors (0: not known yet)
    std::atomic<bool> gfx950{ false };          // ensure_device() has checked the architecture
    HcWorkspace hc_ws, fast_ws;
    FastSlab fast_slab;                         // under the fast_ws lease
    HcPipe hc_pipe;                             // under the hc_ws lease
    CounterRing counter_ring;
    std::atomic<int> lds_drop{ 0 };             // lds_drop_confirmed(): 0 not probed yet, 1 confirmed, 2 not confirmed (or the probe could not run)
    std::mutex lds_drop_mu;
    std::atomic<int> lds_encode_five{ 0 }, lds_encode_dict_five{ 0 }, lds_hc_lcp_fill{ 0 }, lds_encode_hc{ 0 };   // allow_dynamic_lds()
    std::atomic<int> persist_per_cu{ 0 };       // residency of the persistent lane decoder (0: not known yet)
};
DeviceState g_device[kMaxDevices];

// The current device's record (and ordinal), with its CU count known; a failed query is not kept.
int current_device(DeviceState*& ds, int* dev_out = nullptr)
{
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(LZ4HIP_E_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (dev < 0 || dev >= kMaxDevices) return fail(LZ4HIP_E_DEVICE, "device index out of range");
    ds = &g_device[dev];
    if (ds->cus <= 0) {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (cus <= 0) return fail(LZ4HIP_E_DEVICE, "device reports no multiprocessors");
        ds->cus = cus;
    }
    if (dev_out) *dev_out = dev;
    return 0;
}

// The library refuses to run anywhere but on the architecture its kernels were written for.
int ensure_device()
{
    DeviceState* ds = nullptr;
    int dev = -1, rc = current_device(ds, &dev);
    if (rc || ds->gfx950) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(LZ4HIP_E_DEVICE, std::string("liblz4hip is built for gfx950 only, device is ") + prop.gcnArchName);
    ds->gfx950 = true;
    return 0;
}

// Lets `kernel` use `bytes` of dynamic LDS, asked once per device; `state`: 0 not asked yet, 1 allowed, 2 refused.  keep_refusal: a
// refusal is kept (and taken off hipGetLastError) for a caller that falls back to a form without it; otherwise it is asked again next time.
hipError_t allow_dynamic_lds(std::atomic<int>& state, const void* kernel, int bytes, bool keep_refusal)
{
    if (int st = state.load(std::memory_order_acquire)) return st == 1 ? hipSuccess : hipErrorInvalidValue;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) state.store(1, std::memory_order_release);
    else if (keep_refusal) { (void)hipGetLastError(); state.store(2, std::memory_order_release); }
    return e;
}

// Whether the wavefront-mapped fast encoder runs as workgroups of kEncodeBlocksPerGroup blocks (ten blocks per CU) instead of one-block workgroups
// (nine per CU): whenever that saves a residency round -- 2 305 ... 2 560 blocks on 256 CUs, 16 384 (7 rounds instead of 8), every batch from 90 blocks
// per CU up.  With the same number of rounds one block per workgroup is the better form (finer placement, nine wavefronts per CU disturb one another
// less than ten): profiles/r06/wave_encoder_round_steps.txt.
constexpr int kEncodeBlocksPerGroup = 5;
static_assert(hostbatch::kHostEncodeBlocksPerCu == 2 * kEncodeBlocksPerGroup, "encode_host_slice_blocks: two workgroups per CU");
bool encoder_five_blocks_per_workgroup(int64_t n_blocks)
{
    const int k = knob(kKnobEncoderWg5);
    if (k == 1 || n_blocks < kEncodeBlocksPerGroup) return false;
    if (k == 2) return true;
    DeviceState* ds = nullptr;
    if (current_device(ds)) return false;
    const int cus = ds->cus;
    const int64_t rounds9 = (n_blocks + 9 * cus - 1) / (9 * cus), rounds10 = (n_blocks + 10 * cus - 1) / (10 * cus);
    return rounds10 < rounds9;
}

int launch_encode(const lz4hip_batch_t* b, int mode, hipStream_t stream)
{
    if (b->n_blocks == 0) return 0;
    const Batch d = to_device_batch(*b);
    DeviceState* ds = nullptr;
    int rc = current_device(ds);
    if (rc) return rc;
    const int cus = ds->cus;
    if (mode == LZ4HIP_MODE_FAST) {
        // Two mappings (lz4hip_encode.hpp: one wavefront per block, table in LDS, 64 probes of the match search per
        // step; lz4hip_encode_lane.hpp: one lane per block, tables in a global slab).  The first is several times
        // faster where matches are far between (incompressible data: 6x), the second where sequences are short (a
        // chain of dependent steps per sequence: 64 chains per wavefront instead of one).  A batch large enough to
        // fill the lanes is therefore encoded by two launches: the wavefront mapping over every block, which hands a
        // block over (kDeferredResult) as soon as 16 consecutive sequences cover less than 1 KiB, then the lane mapping
        // over the blocks handed over.  Small batches use the wavefront mapping only.
        // The "encoder" knob (LZ4HIP_ENCODER=wave|lane at load time, lz4hip_tuning_set) forces ONE mapping for every block.
        const int force = knob(kKnobEncoder);
        char pick = d.n_blocks >= kLaneEncodeMinBlocks ? 'a' : 'w';  // 'a': both launches
        if (force) pick = force == 1 ? 'w' : 'l';
        Lease lease;
        void* ws = nullptr;                                           // the slab's control block: work counter, then the chunk pointers
        unsigned slab_tpc = 0;
        int64_t groups = 0;
        if (pick != 'w') {
            int wpc = knob(kKnobEncoderWavesPerCu) > 0 ? knob(kKnobEncoderWavesPerCu) : kLaneEncodeWavesPerCu;
            if ((rc = lease_begin(ds->fast_ws, stream, lease))) return rc;
            // the slab holds one table per resident lane; if it cannot be had, halve the residency, and
            // in the end fall back to the wavefront mapping (which needs no workspace)
            for (; wpc >= 1; wpc /= 2) {
                groups = (int64_t)cus * wpc;
                if (groups > (d.n_blocks + 63) / 64) groups = (d.n_blocks + 63) / 64;
                if (fast_slab_reserve(lease, ds->fast_slab, groups) == 0) { ws = ds->fast_slab.ctl; slab_tpc = ds->fast_slab.tables_per_chunk; break; }
            }
            if (!ws) { lease.lock.unlock(); pick = 'w'; }
        }
        if (pick != 'l') {
            bool first_version = false;
#ifdef LZ4HIP_TUNING_BUILD
            first_version = knob(kKnobEncoderWaveVersion) == 1;
            if (first_version)
                hipLaunchKernelGGL(encode_fast_kernel<1>, dim3((unsigned)d.n_blocks), dim3(64), kFastTableBytes, stream, d, pick == 'a' ? (int)kEncodeMayDefer : 0);
#endif
            // gfx950 hands out LDS in granules of 1 280 bytes, 128 per CU: a 16 KiB table takes thirteen, so NINE one-block workgroups fit a CU;
            // five tables are exactly 64 granules, two such workgroups fill the CU with TEN blocks (profiles/r06/wave_encoder_round_steps.txt).
            // 80 KiB of dynamic LDS has to be allowed per device first; where that is refused the one-block form runs.
            bool five = !first_version && encoder_five_blocks_per_workgroup(d.n_blocks);
            five = five && allow_dynamic_lds(ds->lds_encode_five, (const void*)(encode_fast_kernel<2, kEncodeBlocksPerGroup>),
                                             kEncodeBlocksPerGroup * kFastTableBytes, true) == hipSuccess;
            if (five)
                hipLaunchKernelGGL((encode_fast_kernel<2, kEncodeBlocksPerGroup>), dim3((unsigned)((d.n_blocks + kEncodeBlocksPerGroup - 1) / kEncodeBlocksPerGroup)),
                                   dim3(64 * kEncodeBlocksPerGroup), kEncodeBlocksPerGroup * kFastTableBytes, stream, d, pick == 'a' ? (int)kEncodeMayDefer : 0);
            else if (!first_version)
                hipLaunchKernelGGL(encode_fast_kernel<2>, dim3((unsigned)d.n_blocks), dim3(64), kFastTableBytes, stream, d, pick == 'a' ? (int)kEncodeMayDefer : 0);
            HIP_TRY(hipGetLastError());
            count_dispatch(LZ4HIP_K_ENCODE_WAVE);
        }
        if (pick != 'w') {
            lease.queued = true;
            HIP_TRY(hipMemsetAsync(ws, 0, 256, stream));
            hipLaunchKernelGGL(encode_fast_lane_kernel, dim3((unsigned)groups), dim3(64), 0, stream, d,
                               (unsigned long long*)ws, (uint8_t* const*)((uint8_t*)ws + 256), slab_tpc, pick == 'a' ? 1 : 0);
            HIP_TRY(hipGetLastError());
            count_dispatch(LZ4HIP_K_ENCODE_LANE);
            if ((rc = lease_end(lease, stream))) return rc;
        }
    } else if (mode == LZ4HIP_MODE_HC) {
        // 16-bit heads (64 KiB of LDS, two workgroups per CU) when every block is known to be <= 64 KiB:
        // uniform length, or per-block lengths with src_len_all carrying an upper bound (0 = unknown).
        const bool small = b->src_len_all > 0 && b->src_len_all <= 65536;
        // Large batches: one lane per block -- blocks <= 64 KiB over tables built up front for a chunk of the batch
        // (lz4hip_hc_lcp.hpp: chain + shared length per position), larger blocks with the insert loop and a per-lane global slab
        // (lz4hip_hc_conv.hpp); if the workspace cannot be allocated, or the batch is small, one wavefront per block (lz4hip_hc.hpp).
        // The "hc" knob (LZ4HIP_HC=wave|lane at load time, lz4hip_tuning_set) overrides.
        const int force = knob(kKnobHc);
        // (a lane-mapped wavefront needs ~0.35 s for its 64 blocks <= 64 KiB however small the batch, the wavefront mapping does
        //  ~11 k blocks per second: measured crossover at 4096 blocks, profiles/r03/hc_small_batches.txt; blocks > 64 KiB take
        //  the kernel with the insert loop, 1.3 - 2.4 s: 16 k blocks, profiles/r01/hc_small_batches.txt)
        bool lane_per_block = d.n_blocks >= (small ? 4096 : 16384);
        if (force == 1) lane_per_block = false;
        if (force == 2) lane_per_block = true;
        Lease lease;
        if ((rc = lease_begin(ds->hc_ws, stream, lease))) return rc;
        if (lane_per_block) {
            int hc_gen = knob(kKnobHcGen) ? knob(kKnobHcGen) : kHcLaneGeneration;
            if (hc_gen >= 3 && !small) hc_gen = 2;                    // lz4hip_hc_nat.hpp / lz4hip_hc_lcp.hpp are for blocks <= 64 KiB
            const size_t slab = small ? kHcLaneSlab16 : kHcLaneSlab32;
            int wpc = knob(kKnobHcWavesPerCu) > 0 ? knob(kKnobHcWavesPerCu) : kHcLaneWavesPerCu;
            void* ws = nullptr;
            int64_t groups = 0, chunk = 0;
            for (; wpc >= 1; wpc /= 2) {
                groups = (int64_t)cus * wpc;
                if (knob(kKnobHcGroups) > 0) groups = knob(kKnobHcGroups);
                if (groups > (d.n_blocks + 63) / 64) groups = (d.n_blocks + 63) / 64;
                // generation 3: one chain table per block of a chunk; a chunk = at most one block per resident lane (but at least
                // 4096), the batch cut into equal chunks (a short last chunk would run at a fraction of the residency)
                chunk = groups * 64 < 4096 ? 4096 : groups * 64;
                const int64_t n_chunks = (d.n_blocks + chunk - 1) / chunk;
                chunk = ((d.n_blocks + n_chunks - 1) / n_chunks + 63) / 64 * 64;
                if (hc_gen >= 3) {
                    // tables: 256 KiB (generation 4) per block of a chunk, rebuilt chunk after chunk -- never more than half of what the
                    // device has free (a 2^18-block chunk is 64 GiB), and a chunk that cannot be had is halved, down to 4096 blocks
                    const size_t entry = hc_gen == 4 ? kHcLcpTableBytes : kHcNatChainBytes;
                    size_t free_b = 0, total_b = 0;
                    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)8 << 30; }
                    const size_t budget = (free_b + lease.w->cap) / 2;
                    int64_t c = chunk;
                    while (c > 4096 && (size_t)c * entry > budget) c = (c / 2 + 63) / 64 * 64;
                    for (;;) {
                        if (lease_reserve(lease, (size_t)c * entry + kHcCounterBytes) == 0) { ws = lease.p; chunk = c; break; }
                        if (c <= 4096) break;
                        c = (c / 2 + 63) / 64 * 64;
                    }
                    if (ws || knob(kKnobHcGroups) > 0) break;
                    continue;
                }
                const size_t bytes = (size_t)groups * 64 * slab;
                if (lease_reserve(lease, bytes + kHcCounterBytes) == 0) { ws = lease.p; break; }
            }
            if (ws && hc_gen >= 3) {
                // lz4hip_hc_nat.hpp / lz4hip_hc_lcp.hpp: per chunk, the table builders (one workgroup per block), then the lane kernel.
                // The builders need LDS and few registers, the lane kernel registers and no LDS, so they overlap well -- but one
                // after the other on one stream they did not overlap at all (round 3: 190 ms of builders in front of 850 ms of lane
                // kernel).  A chunk is therefore cut into up to kHcSubChunks SUB-CHUNKS: the builders run through them on a build
                // stream, and the lane kernel of a sub-chunk starts on its own stream as soon as its tables are there -- next to the
                // builders of the following ones and to the lane kernels of the earlier ones (each takes its share of the persistent
                // grid).  Same tables, same bytes; the table memory is what one chunk needs, as before.
                if (hc_gen == 4) HIP_TRY(allow_dynamic_lds(ds->lds_hc_lcp_fill, (const void*)hc_lcp_fill_kernel, kHcLcpFillLdsBytes, false));
                HcPipe& hp = ds->hc_pipe;
                if ((rc = hp.init())) return rc;
                const size_t entry = hc_gen == 4 ? kHcLcpTableBytes : kHcNatChainBytes;
                uint8_t* const tables = (uint8_t*)ws + kHcCounterBytes;
                lease.queued = true;
                lease.side.assign(hp.lane, hp.lane + kHcMaxSubChunks);
                lease.side.push_back(hp.build);
                HIP_TRY(hipMemsetAsync(ws, 0, kHcCounterBytes, stream));          // one work counter per sub-chunk (256 bytes apart)
                for (int64_t first = 0; first < d.n_blocks; first += chunk) {
                    const int64_t cnt = d.n_blocks - first < chunk ? d.n_blocks - first : chunk;
                    int subs = knob(kKnobHcSubChunks) > 0 ? knob(kKnobHcSubChunks) : kHcSubChunks;
                    subs = subs > kHcMaxSubChunks ? kHcMaxSubChunks : subs;
                    while (subs > 1 && cnt / subs < 4096) subs--;              // (a lane-mapped launch of fewer blocks is all latency)
                    const int64_t per = ((cnt + subs - 1) / subs + 63) / 64 * 64;
                    // everything queued on the caller's stream so far (the previous chunk's lane kernels included: they read the
                    // tables that are rebuilt now, and the counters that are zeroed again) comes first
                    if (first > 0) HIP_TRY(hipMemsetAsync(ws, 0, kHcCounterBytes, stream));
                    HIP_TRY(hipEventRecord(hp.start, stream));
                    HIP_TRY(hipStreamWaitEvent(hp.build, hp.start, 0));
                    int used = 0;
                    for (int64_t s0 = 0; s0 < cnt; s0 += per, used++) {
                        const int64_t sc = cnt - s0 < per ? cnt - s0 : per;
                        uint8_t* const tab = tables + (size_t)s0 * entry;
                        hipStream_t ls = subs > 1 ? hp.lane[used] : stream;
                        hipStream_t bs = subs > 1 ? hp.build : stream;
                        if (hc_gen == 4) {
                            hipLaunchKernelGGL(hc_nat_chain_kernel<uint32_t>, dim3((unsigned)sc), dim3(kHcNatChainThreads), kHcNatLdsBytes, bs, d, (long long)(first + s0), tab);
                            HIP_TRY(hipGetLastError());
                            hipLaunchKernelGGL(hc_lcp_fill_kernel, dim3((unsigned)sc), dim3(kHcLcpFillThreads), kHcLcpFillLdsBytes, bs, d, (long long)(first + s0), tab);
                            HIP_TRY(hipGetLastError());
                        } else {
#ifdef LZ4HIP_TUNING_BUILD
                            hipLaunchKernelGGL(hc_nat_chain_kernel<uint16_t>, dim3((unsigned)sc), dim3(kHcNatChainThreads), kHcNatLdsBytes, bs, d, (long long)(first + s0), tab);
                            HIP_TRY(hipGetLastError());
#else
                            return fail(LZ4HIP_E_ARGUMENT, "hc_gen: this library has no LZ4HC lane kernel of that generation");
#endif
                        }
                        if (subs > 1) {
                            HIP_TRY(hipEventRecord(hp.built[used], hp.build));
                            HIP_TRY(hipStreamWaitEvent(ls, hp.built[used], 0));
                            HIP_TRY(hipStreamWaitEvent(ls, hp.start, 0));        // (the counters' memset, the caller's earlier work)
                        }
                        int64_t g = (sc + 63) / 64 < groups ? (sc + 63) / 64 : groups;
                        unsigned long long* const counter = (unsigned long long*)((uint8_t*)ws + 256 * (size_t)used);
                        if (hc_gen == 4) {
                            int every = knob(kKnobHcCtrlEvery) > 0 ? knob(kKnobHcCtrlEvery) : kHcLcpCtrlEvery;
                            while (every & (every - 1)) every &= every - 1;          // (a power of two)
                            const int lanes = knob(kKnobHcCtrlLanes) > 0 ? knob(kKnobHcCtrlLanes) : kHcLcpCtrlLanes;
                            hipLaunchKernelGGL(encode_hc_lcp_kernel, dim3((unsigned)g), dim3(64), 0, ls, d, (long long)(first + s0), (long long)sc,
                                               counter, tab, every, lanes);
                        }
#ifdef LZ4HIP_TUNING_BUILD
                        else hipLaunchKernelGGL(encode_hc_nat_kernel, dim3((unsigned)g), dim3(64), 0, ls, d, (long long)(first + s0), (long long)sc, counter, tab);
#endif
                        HIP_TRY(hipGetLastError());
                        if (subs > 1) {
                            HIP_TRY(hipEventRecord(hp.done[used], ls));
                            HIP_TRY(hipStreamWaitEvent(stream, hp.done[used], 0));   // the caller's stream ends up behind every sub-chunk
                        }
                    }
                }
                count_dispatch(LZ4HIP_K_HC_LANE);
                return lease_end(lease, stream);
            }
            if (ws) {
                lease.queued = true;
                HIP_TRY(hipMemsetAsync(ws, 0, 256, stream));
                if (hc_gen == 2 && !small)
                    hipLaunchKernelGGL(encode_hc_conv_kernel<uint32_t>, dim3((unsigned)groups), dim3(64), 0, stream, d,
                                       (unsigned long long*)ws, (uint8_t*)ws + 256, (unsigned long long)slab);
#ifdef LZ4HIP_TUNING_BUILD                                              /* the kernels generation 3 replaced, for A/B runs (tools/hc_gen_ab.py) */
                else if (hc_gen == 2)
                    hipLaunchKernelGGL(encode_hc_conv_kernel<uint16_t>, dim3((unsigned)groups), dim3(64), 0, stream, d,
                                       (unsigned long long*)ws, (uint8_t*)ws + 256, (unsigned long long)slab);
                else if (hc_gen == 1)
                    hipLaunchKernelGGL(encode_hc_lane_kernel, dim3((unsigned)groups), dim3(64), 0, stream, d,
                                       (unsigned long long*)ws, (uint8_t*)ws + 256, (unsigned long long)slab);
#endif
                else return fail(LZ4HIP_E_ARGUMENT, "hc_gen: this library has no LZ4HC lane kernel of that generation");
                HIP_TRY(hipGetLastError());
                count_dispatch(LZ4HIP_K_HC_LANE);
                return lease_end(lease, stream);
            }
        }
        const int lds_bytes = small ? kHcLdsHeads16 : kHcLdsHeads32;
        int64_t groups = (int64_t)cus * (small ? kHcGroupsPerCu : 1);
        if (groups > d.n_blocks) groups = d.n_blocks;
        if ((rc = lease_reserve(lease, (size_t)groups * kHcGlobalBytesPerGroup + 256))) return rc;
        void* ws = lease.p;
        // first 8 bytes of the workspace: the work counter of the persistent grid
        lease.queued = true;
        HIP_TRY(hipMemsetAsync(ws, 0, 256, stream));
        if (!small) HIP_TRY(allow_dynamic_lds(ds->lds_encode_hc, (const void*)encode_hc_kernel, lds_bytes, false));
        hipLaunchKernelGGL(encode_hc_kernel, dim3((unsigned)groups), dim3(64), lds_bytes, stream, d,
                           (unsigned long long*)ws, (uint8_t*)ws + 256, lds_bytes);
        HIP_TRY(hipGetLastError());
        count_dispatch(LZ4HIP_K_HC_WAVE);
        if ((rc = lease_end(lease, stream))) return rc;
    } else {
        return fail(LZ4HIP_E_ARGUMENT, "mode must be LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The lane decoder's dual ring stores (lz4hip_decode_lane4.hpp, L4_APPEND) rest on one hardware rule: a DS store outside the workgroup's LDS
// allocation is dropped.  That rule is CHECKED here, once per device, before the first lane-mapped decode (lds_drop_probe_kernel: every CU
// full of workgroups of the decoder's LDS size issuing the decoder's kinds of out-of-range stores; ~1 ms); a device that does not confirm it --
// or a caller that sets the knob decoder_wrapped_stores -- gets the instantiation whose ring rows are wrapped (POL bit 5), same bytes, ~2 % slower.
bool lds_drop_confirmed(DeviceState& ds)
{
    int st = ds.lds_drop.load(std::memory_order_acquire);
    if (st == 0) {
        std::lock_guard<std::mutex> lk(ds.lds_drop_mu);
        st = ds.lds_drop.load(std::memory_order_acquire);
        if (st == 0) {
            st = 2;
            unsigned* d = nullptr;
            unsigned h = ~0u;
            hipStream_t ps = nullptr;
            if (hipStreamCreateWithFlags(&ps, hipStreamNonBlocking) == hipSuccess && hipMalloc(&d, 256) == hipSuccess) {
                bool ok = hipMemsetAsync(d, 0, 256, ps) == hipSuccess;
                if (ok) {
                    hipLaunchKernelGGL(lds_drop_probe_kernel, dim3((unsigned)ds.cus * 24u), dim3(64), 0, ps, d, 48);
                    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, ps) == hipSuccess && hipStreamSynchronize(ps) == hipSuccess;
                }
                if (ok && h == 0u) st = 1;
            }
            (void)hipGetLastError();
            if (d) (void)hipFree(d);
            if (ps) (void)hipStreamDestroy(ps);
            ds.lds_drop.store(st, std::memory_order_release);
        }
    }
    return st == 1;
}

struct CounterLease {
    CounterSlot* s = nullptr;
    std::unique_lock<std::mutex> lock;
    hipStream_t stream = nullptr;
    // (also on error returns: whatever was queued on `stream` so far is what may still touch the slot)
    ~CounterLease() { if (s && lock.owns_lock() && s->done && hipEventRecord(s->done, stream) == hipSuccess) s->used = true; }
};
int decoder_counter(CounterRing& r, hipStream_t stream, unsigned long long** out, CounterLease& lease)
{
    void* mem = nullptr;
    unsigned k = 0;
    {
        // the slot's lock is taken while the ring's is still held: lz4hip_release_workspaces() (ring lock, then every slot's lock) can then
        // neither free the ring between the two nor destroy the slot's event before this user has recorded it
        std::lock_guard<std::mutex> lk(r.mu);
        if (!r.mem) HIP_TRY(hipMalloc(&r.mem, 64 * 256));
        mem = r.mem;
        k = r.next.fetch_add(1) & 63u;
        lease.s = &r.slot[k];
        lease.stream = stream;
        lease.lock = std::unique_lock<std::mutex>(lease.s->mu);
        if (!lease.s->done) HIP_TRY(hipEventCreateWithFlags(&lease.s->done, hipEventDisableTiming));
    }
    if (lease.s->used) HIP_TRY(hipStreamWaitEvent(stream, lease.s->done, 0));
    uint8_t* slot = (uint8_t*)mem + 256 * (size_t)k;
    HIP_TRY(hipMemsetAsync(slot, 0, 16, stream));                   // work counter + selected-block count
    *out = (unsigned long long*)slot;
    return 0;
}

int launch_decode(const lz4hip_batch_t* b, int known, hipStream_t stream)
{
    if (b->n_blocks == 0) return 0;
    const Batch d = to_device_batch(*b);
    // Two mappings of the same decoder (lz4hip_decode.hpp: one wavefront per block, coalesced wide copies;
    // lz4hip_decode_lane4.hpp: one lane per block, 64 blocks in flight per wavefront).  A batch is
    // partitioned per block by block_selected(): two launches, each skipping the other's blocks.
    // Small batches cannot fill the lanes and use the wavefront mapping only.
    // The "decoder" knob (LZ4HIP_DECODER=wave|lane at load time, lz4hip_tuning_set) forces one mapping for EVERY block,
    // whatever the batch size (tests, A-B runs).
    const int force = knob(kKnobDecoder);
    int wave_filter = kStreamingBlocks, lane_filter = kFineGrainedBlocks;
    if (force == 1) { wave_filter = kAllBlocks; lane_filter = -1; }
    else if (force == 2) { lane_filter = kAllBlocks; wave_filter = -1; }
    else if (d.n_blocks < kLaneDecodeMinBlocks) { wave_filter = kAllBlocks; lane_filter = -1; }
    if (lane_filter >= 0) {
        const unsigned grid = (unsigned)((d.n_blocks + 63) / 64);
        // Generation 4 (lz4hip_decode_lane4.hpp): LDS per wavefront = 64 x ring + 256..512 bytes decides the residency (ring 192:
        // 12 wavefronts per CU); the configurations that were measured are in profiles/r04/decoder_gen4_*.txt.
        const int gen = knob(kKnobDecoderGen) ? knob(kKnobDecoderGen) : kLaneDecodeGeneration;
        if (gen == 4) {
            // decoder_ring = ring bytes + 1000 x variant (variant bit 0: 128-byte flush units, bit 1: 32-byte input pieces,
            // bit 2: one flush store instruction per iteration, bit 3: the flush runs in every second iteration only,
            // bit 4: input pieces are requested in the other iterations only, bit 5: sector input -- L holds a whole 64-byte sector
            // of the source and feeds the window one 32-byte half at a time)
            const int cfg = knob(kKnobDecoderRing) ? knob(kKnobDecoderRing) : kLane4Config;
            DeviceState* ds = nullptr;
            if (int rc = current_device(ds)) return rc;
            const int cus = ds->cus;
            // ring rows stored twice (out-of-range LDS stores dropped by the hardware) only where this device's probe confirmed the rule
            const bool wrapped = knob(kKnobDecoderWrappedStores) != 0 || !lds_drop_confirmed(*ds);
#define LZ4HIP_LAUNCH_LANE4_POL(RING, PIECE, FLUSH, FS, FE, IE, POL)                                                                \
            do {                                                                                                                \
                if (known) hipLaunchKernelGGL((decode_lane4_kernel<true, RING, PIECE, FLUSH, FS, FE, IE, POL>), dim3(grid), dim3(64), 0, stream, d, lane_filter);  \
                else       hipLaunchKernelGGL((decode_lane4_kernel<false, RING, PIECE, FLUSH, FS, FE, IE, POL>), dim3(grid), dim3(64), 0, stream, d, lane_filter); \
            } while (0)
#define LZ4HIP_LAUNCH_LANE4(RING, PIECE, FLUSH, FS, FE, IE, POL)                                                                    \
            do {                                                                                                                \
                if (wrapped) LZ4HIP_LAUNCH_LANE4_POL(RING, PIECE, FLUSH, FS, FE, IE, (POL) | 32);                                   \
                else         LZ4HIP_LAUNCH_LANE4_POL(RING, PIECE, FLUSH, FS, FE, IE, POL);                                          \
            } while (0)
#define LZ4HIP_LANE4_CASE(CFG) case CFG: LZ4HIP_LAUNCH_LANE4((CFG) % 1000, ((CFG) / 1000 & 2) ? 32 : 64, ((CFG) / 1000 & 1) ? 128 : 64, ((CFG) / 1000 & 4) ? 1 : 2, ((CFG) / 1000 & 8) ? 2 : 1, ((CFG) / 1000 & 16) ? 2 : 1, ((CFG) / 1000 & 32) ? 16 : 0); break
            // Default configuration: TWO forms of the same kernel.  One block per lane under hardware dispatch is the faster one for
            // a large batch whose blocks all take the lane mapping (2^20 D2 blocks: 980 vs 952 GB/s); the persistent grid, whose lanes pull
            // blocks from a counter and skip what the filter does not select, wins when a wavefront would idle otherwise -- a batch of
            // more than one but fewer than three residency rounds (2^18 blocks: 865 -> 938 GB/s) or a batch with many blocks routed to the
            // wavefront mapping (half zeros: 68 -> 44 ms).  Which one runs is decided ON THE DEVICE: a counting launch, then both kernels, each of which
            // returns at once unless the count says it is its turn (profiles/r04/decoder_persistent_lanes_ab.txt).
            // Knob decoder_persist: 0 automatic, 1 always the persistent form, 2 never.
            const int persist = knob(kKnobDecoderPersist);
            if (cfg == kLane4Config && persist != 2) {
                constexpr int R_ = kLane4Config % 1000, P_ = (kLane4Config / 1000 & 2) ? 32 : 64, FU_ = (kLane4Config / 1000 & 1) ? 128 : 64,
                              FS_ = (kLane4Config / 1000 & 4) ? 1 : 2, FE_ = (kLane4Config / 1000 & 8) ? 2 : 1, IE_ = (kLane4Config / 1000 & 16) ? 2 : 1,
                              POL_ = (kLane4Config / 1000 & 32) ? 16 : 0;
                int per_cu = ds->persist_per_cu.load(std::memory_order_relaxed);
                if (per_cu <= 0) {
                    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, decode_lane4_persistent_kernel<true, R_, P_, FU_, FS_, FE_, IE_, POL_>, 64, 0));
                    if (per_cu <= 0) per_cu = 1;
                    ds->persist_per_cu.store(per_cu, std::memory_order_relaxed);
                }
                const int64_t capacity = (int64_t)per_cu * cus;
                // 0: one block per lane only; 1: persistent only; 2: counted, one of the two
                // (a batch that fits the residency in one round gives every lane one block either way: nothing to refill, no counter needed)
                int mode = persist == 1 ? 1 : ((int64_t)grid <= capacity ? 0 : ((int64_t)grid < 3 * capacity ? 1 : (lane_filter == kAllBlocks ? 0 : 2)));
                unsigned long long* counter = nullptr;
                CounterLease counter_lease;                              // (its destructor records the slot's event behind the kernels queued below)
                if (mode != 0) { int rc = decoder_counter(ds->counter_ring, stream, &counter, counter_lease); if (rc) return rc; }
                const unsigned* gate = mode == 2 ? (const unsigned*)(counter + 1) : nullptr;       // (the slot's second qword: the count)
                const unsigned threshold = (unsigned)(d.n_blocks - d.n_blocks / 10);            // "nearly every block": 90 %
                if (mode == 2) {
                    const unsigned cg = (unsigned)((d.n_blocks + 255) / 256 < 512 ? (d.n_blocks + 255) / 256 : 512);   // (one atomic per wavefront on ONE address: few, fat wavefronts)
                    hipLaunchKernelGGL(count_selected_kernel, dim3(cg), dim3(256), 0, stream, d, lane_filter, (unsigned*)(counter + 1));
                    HIP_TRY(hipGetLastError());
                }
                unsigned pg = (unsigned)(capacity < (int64_t)grid ? capacity : (int64_t)grid);
                if (knob(kKnobDecoderGroups) > 0 && (unsigned)knob(kKnobDecoderGroups) < pg) pg = (unsigned)knob(kKnobDecoderGroups);
                // one residency round at most, and few wavefronts per CU: workgroups of four wavefronts, so that the SIMDs of a CU share them evenly
                // whatever ran before (decode_lane4_wg4_kernel)
                // (from more than one wavefront per CU on: with at most one, single-wavefront workgroups spread evenly by themselves and keep the
                //  dual ring stores, 8.19 vs 8.59 ms at 16 384 D2 blocks; knob decoder_wg4 = 2 takes the four-wavefront form from four wavefronts on: tests)
                const int wg4_knob = knob(kKnobDecoderWg4);
                const bool wg4 = mode == 0 && wg4_knob != 1 && (int64_t)grid >= 4 && (wg4_knob == 3 || ((int64_t)grid > (wg4_knob == 2 ? 0 : (int64_t)cus) && (int64_t)grid <= capacity));   // (up to one residency round; 3: whatever the batch size -- A/B runs)
                auto both_forms = [&](auto pol_tag) -> int {
                    constexpr int POLX = decltype(pol_tag)::value;
                    if (wg4) {
                        const unsigned g4 = (grid + 3u) / 4u;
                        if (known) hipLaunchKernelGGL((decode_lane4_wg4_kernel<true, R_, P_, FU_, FS_, FE_, IE_, POLX>), dim3(g4), dim3(256), 0, stream, d, lane_filter);
                        else       hipLaunchKernelGGL((decode_lane4_wg4_kernel<false, R_, P_, FU_, FS_, FE_, IE_, POLX>), dim3(g4), dim3(256), 0, stream, d, lane_filter);
                        HIP_TRY(hipGetLastError());
                        return 0;
                    }
                    if (mode != 1) {
                        if (known) hipLaunchKernelGGL((decode_lane4_kernel<true, R_, P_, FU_, FS_, FE_, IE_, POLX>), dim3(grid), dim3(64), 0, stream, d, lane_filter, gate, mode == 2 ? 1 : 0, threshold);
                        else       hipLaunchKernelGGL((decode_lane4_kernel<false, R_, P_, FU_, FS_, FE_, IE_, POLX>), dim3(grid), dim3(64), 0, stream, d, lane_filter, gate, mode == 2 ? 1 : 0, threshold);
                        HIP_TRY(hipGetLastError());
                    }
                    if (mode != 0) {
                        if (known) hipLaunchKernelGGL((decode_lane4_persistent_kernel<true, R_, P_, FU_, FS_, FE_, IE_, POLX>), dim3(pg), dim3(64), 0, stream, d, lane_filter, counter, gate, mode == 2 ? 2 : 0, threshold);
                        else       hipLaunchKernelGGL((decode_lane4_persistent_kernel<false, R_, P_, FU_, FS_, FE_, IE_, POLX>), dim3(pg), dim3(64), 0, stream, d, lane_filter, counter, gate, mode == 2 ? 2 : 0, threshold);
                    }
                    return 0;
                };
                const int rc2 = wrapped ? both_forms(std::integral_constant<int, POL_ | 32>{}) : both_forms(std::integral_constant<int, POL_>{});
                if (rc2) return rc2;
            } else
            switch (cfg) {
            LZ4HIP_LANE4_CASE(kLane4Config);
#ifdef LZ4HIP_TUNING_BUILD                                              /* residency / ring / piece / flush-unit sweeps (tools/ab_decoder_knobs.py) */
            LZ4HIP_LANE4_CASE(128); LZ4HIP_LANE4_CASE(2128); LZ4HIP_LANE4_CASE(6128); LZ4HIP_LANE4_CASE(3192); LZ4HIP_LANE4_CASE(192); LZ4HIP_LANE4_CASE(1192); LZ4HIP_LANE4_CASE(2192);
            LZ4HIP_LANE4_CASE(5192); LZ4HIP_LANE4_CASE(7192); LZ4HIP_LANE4_CASE(11192); LZ4HIP_LANE4_CASE(25192); LZ4HIP_LANE4_CASE(11256); LZ4HIP_LANE4_CASE(1256); LZ4HIP_LANE4_CASE(3256); LZ4HIP_LANE4_CASE(7256); LZ4HIP_LANE4_CASE(5256);
            LZ4HIP_LANE4_CASE(27192); LZ4HIP_LANE4_CASE(43192); LZ4HIP_LANE4_CASE(35192); LZ4HIP_LANE4_CASE(58128); LZ4HIP_LANE4_CASE(59256); LZ4HIP_LANE4_CASE(59224); LZ4HIP_LANE4_CASE(59208);
            LZ4HIP_LANE4_CASE(59384); LZ4HIP_LANE4_CASE(59512); LZ4HIP_LANE4_CASE(59768); LZ4HIP_LANE4_CASE(59960);   /* round 6: large rings for batches that leave the LDS idle anyway (tools/r06/call12.sh) */
#endif
            default: return fail(LZ4HIP_E_ARGUMENT, "decoder_ring: this library has no generation-4 lane decoder with that configuration");
            }
#undef LZ4HIP_LANE4_CASE
#undef LZ4HIP_LAUNCH_LANE4
#undef LZ4HIP_LAUNCH_LANE4_POL
        }
#ifdef LZ4HIP_TUNING_BUILD                                              /* the generations it replaced (tools/ab/), for same-box A/B runs */
        else if (gen == 2) {
            if (known) hipLaunchKernelGGL((decode_lane_kernel<true, 128, 64>), dim3(grid), dim3(64), 0, stream, d, lane_filter);
            else       hipLaunchKernelGGL((decode_lane_kernel<false, 128, 64>), dim3(grid), dim3(64), 0, stream, d, lane_filter);
        } else if (gen == 3) {
            const int ring = knob(kKnobDecoderRing) ? knob(kKnobDecoderRing) : 128;
#define LZ4HIP_LAUNCH_LANE3(RING)                                                                                               \
            do {                                                                                                                \
                if (known) hipLaunchKernelGGL((decode_lane3_kernel<true, RING, 64>), dim3(grid), dim3(64), 0, stream, d, lane_filter);  \
                else       hipLaunchKernelGGL((decode_lane3_kernel<false, RING, 64>), dim3(grid), dim3(64), 0, stream, d, lane_filter); \
            } while (0)
            switch (ring) {
            case 128: LZ4HIP_LAUNCH_LANE3(128); break;
            case 192: LZ4HIP_LAUNCH_LANE3(192); break;
            case 240: LZ4HIP_LAUNCH_LANE3(240); break;
            default: return fail(LZ4HIP_E_ARGUMENT, "decoder_ring: this library has no generation-3 lane decoder with that ring size");
            }
#undef LZ4HIP_LAUNCH_LANE3
        }
#endif
        else return fail(LZ4HIP_E_ARGUMENT, "decoder_gen: this library has no lane decoder of that generation");
        count_dispatch(LZ4HIP_K_DECODE_LANE);
    }
    if (wave_filter >= 0) {
        const unsigned waves = kWaveDecodeWavesPerGroup, grid = (unsigned)((d.n_blocks + waves - 1) / waves);
        if (known) hipLaunchKernelGGL(decode_kernel<true>, dim3(grid), dim3(64 * waves), 0, stream, d, wave_filter);
        else       hipLaunchKernelGGL(decode_kernel<false>, dim3(grid), dim3(64 * waves), 0, stream, d, wave_filter);
        count_dispatch(LZ4HIP_K_DECODE_WAVE);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// lz4hip_decode_batch_dict_*: every block against one dictionary in device memory, of which the kernel is given the bytes a match can
// reach -- the last 65 535.  The wavefront mapping at every batch size: the lane mapping has no dictionary mode (include/lz4hip.h).
int launch_decode_dict(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, int known, hipStream_t stream)
{
    if (b->n_blocks == 0) return 0;
    const Batch d = to_device_batch(*b);
    const int reach = (int)hostbatch::dict_reach(dict_len);
    const uint8_t* dict_end = reach > 0 ? (const uint8_t*)dict + dict_len : nullptr;
    const unsigned waves = kWaveDecodeWavesPerGroup, grid = (unsigned)((d.n_blocks + waves - 1) / waves);
    if (known) hipLaunchKernelGGL(decode_dict_kernel<true>, dim3(grid), dim3(64 * waves), 0, stream, d, dict_end, reach);
    else       hipLaunchKernelGGL(decode_dict_kernel<false>, dim3(grid), dim3(64 * waves), 0, stream, d, dict_end, reach);
    count_dispatch(LZ4HIP_K_DECODE_WAVE);
    HIP_TRY(hipGetLastError());
    return 0;
}

// lz4hip_encode_batch_dict_*: the primed table of the dictionary's reachable bytes into `primed` (16 KiB), once per call ...
int launch_encode_dict_prime(const void* dict, int64_t dict_len, void* primed, hipStream_t stream)
{
    const int reach = (int)hostbatch::dict_reach(dict_len);
    hipLaunchKernelGGL(encode_dict_prime_kernel, dim3(1), dim3(kEncDictPrimeThreads), 0, stream, (const uint8_t*)dict + dict_len, reach, (uint8_t*)primed);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ... and every block against it: the wavefront mapping at every batch size (no lane mapping, no hand-over), in workgroups of five
// blocks wherever launch_encode would pick them.  dict_len > 0.
int launch_encode_dict(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, const void* primed, hipStream_t stream)
{
    if (b->n_blocks == 0) return 0;
    const Batch d = to_device_batch(*b);
    DeviceState* ds = nullptr;
    int rc = current_device(ds);
    if (rc) return rc;
    const int reach = (int)hostbatch::dict_reach(dict_len);
    const uint8_t* dict_end = (const uint8_t*)dict + dict_len;
    bool five = encoder_five_blocks_per_workgroup(d.n_blocks);
    five = five && allow_dynamic_lds(ds->lds_encode_dict_five, (const void*)(encode_dict_kernel<kEncodeBlocksPerGroup>),
                                     kEncodeBlocksPerGroup * kFastTableBytes, true) == hipSuccess;
    if (five)
        hipLaunchKernelGGL((encode_dict_kernel<kEncodeBlocksPerGroup>), dim3((unsigned)((d.n_blocks + kEncodeBlocksPerGroup - 1) / kEncodeBlocksPerGroup)),
                           dim3(64 * kEncodeBlocksPerGroup), kEncodeBlocksPerGroup * kFastTableBytes, stream, d, dict_end, reach, (const uint8_t*)primed);
    else
        hipLaunchKernelGGL(encode_dict_kernel<1>, dim3((unsigned)d.n_blocks), dim3(64), kFastTableBytes, stream, d, dict_end, reach, (const uint8_t*)primed);
    HIP_TRY(hipGetLastError());
    count_dispatch(LZ4HIP_K_ENCODE_WAVE);
    return 0;
}

int check_dict(const void* dict, int64_t dict_len)
{
    if (dict_len < 0) return fail(LZ4HIP_E_ARGUMENT, "dictionary: dict_len < 0");
    if (dict_len > 0 && !dict) return fail(LZ4HIP_E_ARGUMENT, "dictionary: dict is NULL and dict_len > 0");
    return 0;
}

// Pinned (page-locked) host staging, grow-only, per calling thread: two slots so that the host can fill / drain
// one slice while the device works on the other.
struct Pinned {
    void* p = nullptr; size_t cap = 0;
    int reserve(size_t n)
    {
        if (n <= cap) return 0;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = n < (1u << 20) ? (1u << 20) : n;
        HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
        return 0;
    }
    void release() { if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; } }
    ~Pinned() { /* see ~Scratch */ }
};

// Per calling thread and device: the streams and events of the host pipeline (H2D | kernels | D2H).  A slice owns one of
// kHostSlots slots (pinned in/out images, device in/out images, a kernel stream): the kernels of consecutive slices run
// on DIFFERENT streams, so that a slice's kernels start as soon as its input has landed, next to those of the slices
// before it -- a launch over a thousand blocks cannot fill the device and takes the same few milliseconds as one over
// four thousand.
struct HostPipe {
    bool ready = false;
    int dev = -1;                // streams and events belong to a device: one set per (thread, device)
    hipStream_t s_in = nullptr, s_out = nullptr, s_k[kHostSlots];
    hipEvent_t e_in[kHostSlots], e_k[kHostSlots], e_out[kHostSlots], e_start;
    int init()
    {
        if (ready) return 0;
        HIP_TRY(hipGetDevice(&dev));
        HIP_TRY(hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&e_start, hipEventDisableTiming));
        for (int k = 0; k < kHostSlots; k++) {
            HIP_TRY(hipStreamCreateWithFlags(&s_k[k], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&e_in[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&e_k[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&e_out[k], hipEventDisableTiming));
        }
        ready = true;
        return 0;
    }
};
// Everything a calling thread needs to stage host batches through ONE device: scratch, pinned slots, pipeline.
// Indexed by the device that is current when the call is made, so a thread may hipSetDevice() between calls
// (and the multi-device entry points run one worker thread per device).
// It is the stage of hostbatch::run_host_batch (lz4hip_hostbatch.hpp): copies in on one stream, copies out on another, the
// kernels of a slot on the slot's own stream, events between them.
struct HostContext {
    Scratch scratch;
    Scratch dict;                                                    // lz4hip_decode_batch_dict_host: the call's dictionary, apart from the slots' images (which move when they grow)
    Scratch primed;                                                  // lz4hip_encode_batch_dict_host: the dictionary's primed table
    Pinned pinned_in[kHostSlots], pinned_out[kHostSlots];
    HostPipe pipe;
    uint8_t* d_in[kHostSlots] = {};
    uint8_t* d_out[kHostSlots] = {};

    int fail(int code, const std::string& what) { return ::fail(code, what); }
    int reserve(int slots, int64_t in_bytes, int64_t out_bytes)
    {
        int rc = scratch.reserve((size_t)slots * (size_t)(in_bytes + out_bytes));
        if (rc) return rc;
        for (int k = 0; k < slots; k++) {
            if ((rc = pinned_in[k].reserve((size_t)in_bytes))) return rc;
            if ((rc = pinned_out[k].reserve((size_t)out_bytes))) return rc;
        }
        if ((rc = pipe.init())) return rc;
        for (int k = 0; k < slots; k++) {
            d_in[k] = (uint8_t*)scratch.p + (size_t)k * (size_t)(in_bytes + out_bytes);
            d_out[k] = d_in[k] + in_bytes;
        }
        return 0;
    }
    // (pageable host memory: the runtime stages it; the wait is what lets kernels on any stream, of any pipeline, read it)
    int dict_upload(const uint8_t* from, int64_t bytes, uint8_t*& dev)
    {
        int rc = dict.reserve((size_t)bytes);
        if (rc) return rc;
        if ((rc = pipe.init())) return rc;
        HIP_TRY(hipMemcpyAsync(dict.p, from, (size_t)bytes, hipMemcpyHostToDevice, pipe.s_in));
        HIP_TRY(hipStreamSynchronize(pipe.s_in));
        dev = (uint8_t*)dict.p;
        return 0;
    }
    // lz4hip_encode_batch_dict_host: the primed table of the uploaded dictionary, built and WAITED for, as the upload is
    int dict_prime(const uint8_t* d_dict, int64_t reach, uint8_t*& table)
    {
        int rc = primed.reserve((size_t)kFastTableBytes);
        if (rc) return rc;
        if ((rc = pipe.init())) return rc;
        if ((rc = launch_encode_dict_prime(d_dict, reach, primed.p, pipe.s_in))) return rc;
        HIP_TRY(hipStreamSynchronize(pipe.s_in));
        table = (uint8_t*)primed.p;
        return 0;
    }
    uint8_t* pin_in(int slot) { return (uint8_t*)pinned_in[slot].p; }
    uint8_t* pin_out(int slot) { return (uint8_t*)pinned_out[slot].p; }
    uint8_t* dev_in(int slot) { return d_in[slot]; }
    uint8_t* dev_out(int slot) { return d_out[slot]; }
    // whatever the caller queued on its stream before this call comes first
    int begin()
    {
        HIP_TRY(hipEventRecord(pipe.e_start, hipStreamPerThread));
        HIP_TRY(hipStreamWaitEvent(pipe.s_in, pipe.e_start, 0));
        return 0;
    }
    // (the slot's previous kernels have finished: their slice has been drained)
    int copy_in(int slot, int64_t offset, int64_t bytes)
    {
        HIP_TRY(hipMemcpyAsync(d_in[slot] + offset, pin_in(slot) + offset, (size_t)bytes, hipMemcpyHostToDevice, pipe.s_in));
        return 0;
    }
    // on the slot's own stream, after its input has landed; the copies out wait for them
    template <class Run>
    int kernels(int slot, Run& run, const lz4hip_batch_t& db)
    {
        hipStream_t ks = pipe.s_k[slot];
        HIP_TRY(hipEventRecord(pipe.e_in[slot], pipe.s_in));
        HIP_TRY(hipStreamWaitEvent(ks, pipe.e_in[slot], 0));
        if (int rc = run(&db, ks)) return rc;
        HIP_TRY(hipEventRecord(pipe.e_k[slot], ks));
        HIP_TRY(hipStreamWaitEvent(pipe.s_out, pipe.e_k[slot], 0));
        return 0;
    }
    // (the slot's event is recorded behind each copy: it stands for the last one)
    int copy_out(int slot, int64_t offset, int64_t bytes)
    {
        HIP_TRY(hipMemcpyAsync(pin_out(slot) + offset, d_out[slot] + offset, (size_t)bytes, hipMemcpyDeviceToHost, pipe.s_out));
        HIP_TRY(hipEventRecord(pipe.e_out[slot], pipe.s_out));
        return 0;
    }
    bool out_done(int slot) { return hipEventQuery(pipe.e_out[slot]) == hipSuccess; }
    int wait_out(int slot) { HIP_TRY(hipEventSynchronize(pipe.e_out[slot])); return 0; }
    void quiesce()
    {
        (void)hipStreamSynchronize(pipe.s_in); (void)hipStreamSynchronize(pipe.s_out);
        for (int k = 0; k < kHostSlots; k++) (void)hipStreamSynchronize(pipe.s_k[k]);
    }
};
// One per (thread, device), created on first use and kept for the life of the thread.  The threads that call this are
// the callers' own (single-device entry points) and the library's PERSISTENT device workers (multi-device entry points,
// below) -- never a thread the library starts per call.
HostContext* host_context(int dev, bool create = true)
{
    static thread_local HostContext* ctx[kMaxDevices] = {};
    if (dev < 0 || dev >= kMaxDevices) return nullptr;
    if (!ctx[dev] && create) ctx[dev] = new HostContext();   // lives as long as the thread (see ~Scratch)
    return ctx[dev];
}
void release_host_context(int dev)
{
    if (HostContext* hc = host_context(dev, false)) {
        hc->scratch.release();
        hc->dict.release();
        hc->primed.release();
        for (int k = 0; k < kHostSlots; k++) { hc->pinned_in[k].release(); hc->pinned_out[k].release(); }
    }
}

// ---- persistent device workers of the multi-device entry points --------------------------------------------------------
// One thread per (logical) device, started on first use and kept until the process ends: its staging context (device
// images, pinned slots, streams, events) is allocated once and reused by every later call.  A caller posts one job per
// worker and waits for all of them; concurrent callers queue on the worker's `busy` mutex (taken in ascending worker order).
struct DeviceWorker {
    std::mutex busy;                 // held by the caller that owns the worker for one job
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, finished = false, started = false;
    void loop()
    {
        for (;;) {
            std::function<void()> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return has_job; });
                j = std::move(job); has_job = false;
            }
            try { j(); } catch (...) {}                              // (jobs report through their own state; see run_host_batch_multi)
            {
                std::lock_guard<std::mutex> lk(mu);
                finished = true;
            }
            cv.notify_all();
        }
    }
    // (caller holds `busy`)
    int post(std::function<void()> j)
    {
        std::unique_lock<std::mutex> lk(mu);
        if (!started) {
            try { std::thread(&DeviceWorker::loop, this).detach(); }
            catch (const std::system_error& e) { return fail(LZ4HIP_E_MEMORY, std::string("cannot start a device worker thread: ") + e.what()); }
            started = true;
        }
        job = std::move(j); has_job = true; finished = false;
        lk.unlock();
        cv.notify_all();
        return 0;
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return finished; });
    }
};
constexpr int kMaxWorkers = 64;
DeviceWorker* g_worker[kMaxWorkers];         // never freed: a worker blocked in cv.wait at process exit must keep its object
std::mutex g_worker_mu;
DeviceWorker* device_worker(int logical)
{
    std::lock_guard<std::mutex> lk(g_worker_mu);
    if (!g_worker[logical]) g_worker[logical] = new DeviceWorker();
    return g_worker[logical];
}

// Stage a host batch through device memory, run `run` on it, copy results (and dst payloads) back: hostbatch::run_host_batch
// (lz4hip_hostbatch.hpp: slices, images, gather and scatter, the order of it all) over the calling thread's context for the current device.
// slice_hint > 0: blocks per slice wanted by the caller.
template <class Run>
int run_host_batch(const lz4hip_batch_t* hb, bool dst_len_is_result, Run run, int64_t slice_hint = 0)
{
    int rc = check_batch(hb);
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    int dev_now = 0;
    HIP_TRY(hipGetDevice(&dev_now));
    HostContext* hc = host_context(dev_now);
    if (!hc) return fail(LZ4HIP_E_DEVICE, "device index out of range");
    return hostbatch::run_host_batch(*hc, hb, dst_len_is_result, run, slice_hint, knob(kKnobHostSlices), knob(kKnobHostThreads));
}

// Host-resident batch sharded over the devices of `device_mask` (bit d = HIP device d; 0 = every visible device):
// block i belongs to the (i mod N)-th selected device -- the partition of SURVEY.md 8e / BASELINE configs[4] -- one
// persistent worker thread per device, each with its own staging pipeline (run_host_batch on that device); no device ever
// sees another device's blocks and nothing is exchanged between them.  Results land in the caller's arrays in global order.
// (The "logical_devices" knob makes N workers out of fewer devices, wrapping around: how the threaded path is tested on
// a one-GPU box.)
template <class Run>
int run_host_batch_multi(const lz4hip_batch_t* hb, bool dst_len_is_result, uint64_t device_mask, Run run, int64_t slice_hint = 0, int workers_on_one_device = 0)
{
    int rc = check_batch(hb);
    if (rc) return rc;
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) return fail(LZ4HIP_E_DEVICE, "no HIP device");
    std::vector<int> devs;
    for (int d = 0; d < visible && d < kMaxDevices; d++)
        if (device_mask == 0 || ((device_mask >> d) & 1ull)) devs.push_back(d);
    if (devs.empty()) return fail(LZ4HIP_E_ARGUMENT, "device_mask selects no visible device");
    const int logical = workers_on_one_device > 0 ? workers_on_one_device : knob(kKnobLogicalDevices);
    if (logical > 0) {
        const std::vector<int> base = devs;
        devs.clear();
        for (int k = 0; k < logical && k < kMaxWorkers; k++) devs.push_back(base[(size_t)k % base.size()]);
    }
    const int64_t n = hb->n_blocks;
    if (n == 0) return 0;
    const int nd = (int)devs.size();

    using hostbatch::Shard;
    std::vector<Shard> shards = hostbatch::shard_batch(hb, nd);
    if (nd == 1) {                                                   // one device: on the calling thread, with its own context
        int prev_dev = 0;
        HIP_TRY(hipGetDevice(&prev_dev));
        HIP_TRY(hipSetDevice(devs[0]));
        rc = run_host_batch(&shards[0].b, dst_len_is_result, run, slice_hint);
        (void)hipSetDevice(prev_dev);
        if (rc) return rc;
    } else {
        std::vector<DeviceWorker*> workers((size_t)nd);
        for (int k = 0; k < nd; k++) workers[(size_t)k] = device_worker(k);
        int posted = 0, post_rc = 0;
        for (int k = 0; k < nd; k++) {                               // ascending order: concurrent callers cannot deadlock
            DeviceWorker* w = workers[(size_t)k];
            w->busy.lock();
            Shard* sh = &shards[(size_t)k];
            const int phys = devs[(size_t)k];
            post_rc = w->post([sh, phys, dst_len_is_result, run, slice_hint] {
                if (sh->b.n_blocks == 0) return;
                if (hipSetDevice(phys) != hipSuccess) { sh->rc = LZ4HIP_E_DEVICE; sh->err = "hipSetDevice failed"; return; }
                // nothing may be thrown across the worker's loop (a detached thread: std::terminate for the whole process)
                try { sh->rc = run_host_batch(&sh->b, dst_len_is_result, run, slice_hint); }
                catch (const std::bad_alloc&) { sh->rc = LZ4HIP_E_MEMORY; g_last_error = "out of host memory in a device worker"; }
                catch (const std::exception& e) { sh->rc = LZ4HIP_E_DEVICE; g_last_error = std::string("device worker: ") + e.what(); }
                if (sh->rc) sh->err = g_last_error;                  // thread-local: carry it back to the caller
            });
            if (post_rc) { w->busy.unlock(); break; }
            posted++;
        }
        for (int k = 0; k < posted; k++) { workers[(size_t)k]->wait(); workers[(size_t)k]->busy.unlock(); }
        if (post_rc) return post_rc;
    }
    std::string text;
    if ((rc = hostbatch::merge_shards(hb, shards, devs.data(), text))) return fail(rc, text);
    return 0;
}

// what a host-pointer call runs on each slice's device batch
auto encoder_run(int mode) { return [mode](const lz4hip_batch_t* db, hipStream_t s) { return launch_encode(db, mode, s); }; }
auto decoder_run(int known) { return [known](const lz4hip_batch_t* db, hipStream_t s) { return launch_decode(db, known, s); }; }

int single(const char* src, int src_len, char* dst, int dst_cap, int kind /*0 fast,1 hc,2 dec known,3 dec unknown*/)
{
    if (!src || !dst) return fail(LZ4HIP_E_ARGUMENT, "NULL buffer");
    if (src_len < 0) return fail(LZ4HIP_E_ARGUMENT, "negative length");
    int32_t result = 0;
    lz4hip_batch_t b;
    b.src = src; b.src_off = nullptr; b.src_stride = 0; b.src_len = nullptr; b.src_len_all = src_len;
    b.dst = dst; b.dst_off = nullptr; b.dst_stride = 0; b.dst_cap = nullptr; b.dst_cap_all = dst_cap < 0 ? 0 : dst_cap;
    b.result = &result; b.n_blocks = 1;
    int rc = kind <= 1 ? lz4hip_encode_batch_host(&b, kind) : lz4hip_decode_batch_host(&b, kind == 2);
    return rc ? rc : result;
}

// Number of source bytes a known-size decode of `osize` output bytes will look at.  This only walks
// the token / length bytes (no byte of payload is decoded on the host): LZ4_uncompress() is not
// told its input size (original/lz4.c:812-814), so the extent of the H2D copy has to come from the
// stream itself.  Mirrors the control flow of lz4hip::decode_block<true>.
int known_size_extent(const uint8_t* src, int osize)
{
    int64_t ip = 0, op = 0;
    for (;;) {
        unsigned token = src[ip++];
        int64_t ll = token >> 4;
        if (ll == 15) { unsigned b; do { b = src[ip++]; ll += b; } while (b == 255 && ll < (1 << 30)); }
        if (op + ll > (int64_t)osize - 8) return (int)(op + ll == osize ? ip + ll : ip);
        ip += ll; op += ll;
        ip += 2;
        int64_t ml = token & 15;
        if (ml == 15) { while (src[ip] == 255 && ml < (1 << 30)) { ml += 255; ip++; } ml += src[ip++]; }
        op += ml + 4;
        if (op > (int64_t)osize - 5) return (int)ip;
    }
}


// ---- the framing paths (lz4hip_framing.hpp): LZ4Stream buffers, wrapped messages, batches of LZ4Stream buffers ----------------
// The layouts and the kernel sequences live in that header, shared with the CPU emulator's tests; this is the device they run on here.
struct HipBackend {
    hipStream_t stream;
    HostContext* host = nullptr;                                       // the host pair alone: whose scratch holds the staging image
    template <class... P, class... A>
    void launch(void (*kernel)(P...), Grid grid, unsigned threads, A&&... a) { hipLaunchKernelGGL(kernel, dim3(grid.groups), dim3(threads), 0, stream, P(a)...); }
    int fill(void* p, int byte, size_t bytes) { HIP_TRY(hipMemsetAsync(p, byte, bytes, stream)); return 0; }
    int encode(const lz4hip_batch_t* b, int mode) { return launch_encode(b, mode, stream); }
    int decode(const lz4hip_batch_t* b, int known) { return launch_decode(b, known, stream); }
    // (the dictionary calls of LZ4 frames: `reach` <= 65 535 bytes that end at dict_end)
    int decode_dict(const lz4hip_batch_t* b, const uint8_t* dict_end, int32_t reach, int known) { return launch_decode_dict(b, dict_end - reach, reach, known, stream); }
    int encode_dict_prime(const uint8_t* dict_end, int32_t reach, uint8_t* primed) { return launch_encode_dict_prime(dict_end - reach, reach, primed, stream); }
    int encode_dict(const lz4hip_batch_t* b, const uint8_t* dict_end, int32_t reach, const uint8_t* primed) { return launch_encode_dict(b, dict_end - reach, reach, primed, stream); }
    int dict_upload(const uint8_t* from, int64_t bytes, uint8_t*& dev) { return host->dict_upload(from, bytes, dev); }
    int last_error() { HIP_TRY(hipGetLastError()); return 0; }
    int fail(int code, const std::string& what) { return ::fail(code, what); }
    int reserve(size_t bytes, uint8_t*& base) { int rc = host->scratch.reserve(bytes); base = (uint8_t*)host->scratch.p; return rc; }
    int upload(void* dev, const void* from, size_t bytes) { HIP_TRY(hipMemcpyAsync(dev, from, bytes, hipMemcpyHostToDevice, stream)); return 0; }
    int download(void* to, const void* dev, size_t bytes) { HIP_TRY(hipMemcpyAsync(to, dev, bytes, hipMemcpyDeviceToHost, stream)); return 0; }
    int sync() { HIP_TRY(hipStreamSynchronize(stream)); return 0; }
};

// The host pair stages the whole buffer in the calling thread's device scratch (HostContext: grow-only, freed by
// lz4hip_release_workspaces) and runs the device path on the thread's first kernel stream.
int stream_host_context(HipBackend& be)
{
    int rc = ensure_device(), dev = 0;
    if (rc) return rc;
    HIP_TRY(hipGetDevice(&dev));
    if (!(be.host = host_context(dev))) return fail(LZ4HIP_E_DEVICE, "device index out of range");
    if ((rc = be.host->pipe.init())) return rc;
    be.stream = be.host->pipe.s_k[0];
    return 0;
}

}  // namespace

extern "C" {

const char* lz4hip_last_error(void) { return g_last_error.c_str(); }

int lz4hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* lz4hip_codec_name(void)
{
    static thread_local std::string name;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        name = "HIP gfx950 (no device)";
    } else {
        name = std::string("HIP ") + prop.gcnArchName + " (" + prop.name + ")";
    }
    return name.c_str();
}

int lz4hip_compressBound(int isize) { return isize + isize / 255 + 16; }

// Which sources this binary was built from: lz4net_amd/build.py hashes csrc/ (the hash bench.py and the committed counter files are keyed on) and
// passes it in; the marker string is also how build.py recognises a stale prebuilt library without loading it.
#ifndef LZ4HIP_CSRC_SHA
#define LZ4HIP_CSRC_SHA "unknown"
#endif
#ifdef LZ4HIP_TUNING_BUILD
#define LZ4HIP_BUILD_KIND "+tuning"
#else
#define LZ4HIP_BUILD_KIND ""
#endif
const char* lz4hip_build_id(void)
{
    static const char marker[] = "LZ4HIP_BUILD_ID=" LZ4HIP_CSRC_SHA LZ4HIP_BUILD_KIND;
    return marker + 16;
}

int lz4hip_dispatch_counts(uint64_t* counts, int n)
{
    for (int k = 0; counts && k < n && k < LZ4HIP_K_COUNT; k++) counts[k] = g_dispatch[k].load(std::memory_order_relaxed);
    return LZ4HIP_K_COUNT;
}

int lz4hip_release_workspaces(void)
{
    DeviceState* ds = nullptr;
    int dev = 0, rc = current_device(ds, &dev);
    if (rc) return rc;
    // each workspace after its last user, with what hangs off its lease: the LZ4HC sub-chunk pipeline's streams and events, the lane encoder's slab
    for (HcWorkspace* w : { &ds->hc_ws, &ds->fast_ws }) {
        std::lock_guard<std::mutex> lock(w->mu);
        const bool pipe = w == &ds->hc_ws && ds->hc_pipe.ready, slab = w == &ds->fast_ws && ds->fast_slab.ctl;
        if (!(pipe || slab || w->p)) continue;
        if (w->busy && w->last) HIP_TRY(hipEventSynchronize(w->last));
        if (pipe) ds->hc_pipe.release();
        if (slab) ds->fast_slab.release();
        if (w->p) HIP_TRY(hipFree(w->p));
        w->p = nullptr; w->cap = 0; w->busy = false;
    }
    {
        // the persistent lane decoder's counter ring: every slot's last user must be done (slot by slot, under the slot's lock)
        CounterRing& r = ds->counter_ring;
        std::lock_guard<std::mutex> lk(r.mu);
        if (r.mem) {
            for (CounterSlot& cs : r.slot) {
                std::lock_guard<std::mutex> sl(cs.mu);
                if (cs.used && cs.done) HIP_TRY(hipEventSynchronize(cs.done));
                if (cs.done) { (void)hipEventDestroy(cs.done); cs.done = nullptr; }
                cs.used = false;
            }
            HIP_TRY(hipFree(r.mem));
            r.mem = nullptr;
        }
    }
    // ... and the CALLING thread's host-pointer staging for this device (device images + pinned slots; the host-pointer
    // entry points are synchronous, so nothing of this thread's is in flight here)
    release_host_context(dev);
    // ... and that of the multi-device entry points' persistent workers for this device
    for (int k = 0; k < kMaxWorkers; k++) {
        DeviceWorker* w = nullptr;
        { std::lock_guard<std::mutex> lk(g_worker_mu); w = g_worker[k]; }
        if (!w) continue;
        std::lock_guard<std::mutex> own(w->busy);
        // (a worker is indexed by its slot, not by a device: it may hold a context for every device it ever served)
        if (w->post([] {
                int nd = 0;
                if (hipGetDeviceCount(&nd) != hipSuccess) return;
                for (int d = 0; d < nd && d < kMaxDevices; d++)
                    if (host_context(d, false) && hipSetDevice(d) == hipSuccess) release_host_context(d);
            })) continue;
        w->wait();
    }
    return 0;
}

int lz4hip_tuning_set(const char* name, int value)
{
    knobs_init();
    for (int k = 0; name && k < kKnobCount; k++)
        if (strcmp(name, kKnobInfo[k].name) == 0) {
            if (value < 0 || (kKnobInfo[k].mapping && value > 2)) return fail(LZ4HIP_E_ARGUMENT, std::string("bad value for knob ") + name);
            return g_knob[k].exchange(value, std::memory_order_relaxed);
        }
    return fail(LZ4HIP_E_ARGUMENT, std::string("unknown knob ") + (name ? name : "(null)"));
}

int lz4hip_tuning_get(const char* name)
{
    knobs_init();
    // read-only: what the placement of the current device's lane-encoder slab measured, in M steps per second (0: no slab yet or not measured),
    // and how many candidate placements were built
    if (name && (strcmp(name, "encoder_slab_rate") == 0 || strcmp(name, "encoder_slab_tried") == 0 || strcmp(name, "encoder_slab_chunks") == 0)) {
        DeviceState* ds = nullptr;
        if (current_device(ds)) return 0;
        std::lock_guard<std::mutex> lk(ds->fast_ws.mu);
        return name[13] == 'r' ? (int)(ds->fast_slab.probe * 1000.0) : (name[13] == 't' ? ds->fast_slab.tries : (int)ds->fast_slab.chunks.size());
    }
    // read-only: 1 if lane-mapped decodes on the current device store their ring rows twice (the device's probe confirmed that out-of-range LDS
    // stores are dropped, and the knob decoder_wrapped_stores is 0), 0 if they run the wrapped-row instantiation.  Runs the probe if it has not run yet.
    if (name && strcmp(name, "decoder_dual_store") == 0) {
        DeviceState* ds = nullptr;
        if (ensure_device() || current_device(ds)) return 0;
        return (lds_drop_confirmed(*ds) && knob(kKnobDecoderWrappedStores) == 0) ? 1 : 0;
    }
    for (int k = 0; name && k < kKnobCount; k++)
        if (strcmp(name, kKnobInfo[k].name) == 0) return g_knob[k].load(std::memory_order_relaxed);
    return fail(LZ4HIP_E_ARGUMENT, std::string("unknown knob ") + (name ? name : "(null)"));
}

int lz4hip_encode_batch_device(const lz4hip_batch_t* b, int mode, void* stream)
{
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    return launch_encode(b, mode, (hipStream_t)stream);
}

int lz4hip_decode_batch_device(const lz4hip_batch_t* b, int known_output_size, void* stream)
{
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    return launch_decode(b, known_output_size, (hipStream_t)stream);
}

// How many staging pipelines a single-device call runs as and the slices of an encode: lz4hip_hostbatch.hpp (host_workers_for,
// encode_host_slice_blocks); here the knob and the device's CU count are fetched for them.
int host_workers_for(const lz4hip_batch_t* b, int mode_is_hc) { return hostbatch::host_workers_for(b ? b->n_blocks : 0, mode_is_hc != 0, knob(kKnobHostWorkers)); }

int64_t encode_host_slice_blocks(const lz4hip_batch_t* b, int mode)
{
    int cus = 0;
    DeviceState* ds = nullptr;
    if (mode != LZ4HIP_MODE_HC && b && b->n_blocks >= 4096) {
        if (current_device(ds)) (void)hipGetLastError();
        else cus = ds->cus;
    }
    return hostbatch::encode_host_slice_blocks(b ? b->n_blocks : 0, mode, cus);
}

int lz4hip_encode_batch_host(const lz4hip_batch_t* b, int mode)
{
    // (two pipelines only where the knob asks for them: see host_workers_for)
    const int workers = mode == LZ4HIP_MODE_HC || knob(kKnobHostWorkers) <= 0 ? 1 : host_workers_for(b, 0);
    const int64_t slice = encode_host_slice_blocks(b, mode);
    int dev = 0;
    if (workers > 1 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices)
        return run_host_batch_multi(b, true, 1ull << dev, encoder_run(mode), slice, workers);
    return run_host_batch(b, true, encoder_run(mode), slice);
}

int lz4hip_decode_batch_host(const lz4hip_batch_t* b, int known_output_size)
{
    const int workers = host_workers_for(b, 0);
    int dev = 0;
    if (workers > 1 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices)
        return run_host_batch_multi(b, !known_output_size, 1ull << dev, decoder_run(known_output_size), 0, workers);
    return run_host_batch(b, !known_output_size, decoder_run(known_output_size));
}

int lz4hip_decode_batch_dict_device(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, int known_output_size, void* stream)
{
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = check_dict(dict, dict_len))) return rc;
    if ((rc = ensure_device())) return rc;
    return launch_decode_dict(b, dict, dict_len, known_output_size, (hipStream_t)stream);
}

// The dictionary goes up once, on the calling thread's context, and has landed before a slice is staged; the slices then travel as those of
// lz4hip_decode_batch_host do -- as two pipelines from host_workers_for's size on, whose kernels read the one copy.
int lz4hip_decode_batch_dict_host(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, int known_output_size)
{
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = check_dict(dict, dict_len))) return rc;
    if (b->n_blocks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HostContext* hc = host_context(dev);
    if (!hc) return fail(LZ4HIP_E_DEVICE, "device index out of range");
    const int known = known_output_size;
    auto make_run = [known](const uint8_t* d_dict, int64_t reach) {
        return [=](const lz4hip_batch_t* db, hipStream_t s) { return launch_decode_dict(db, d_dict, reach, known, s); };
    };
    const int workers = host_workers_for(b, 0);
    if (workers > 1) {
        const uint8_t* d_dict = nullptr;
        int64_t reach = 0;
        if ((rc = hostbatch::upload_dictionary(*hc, dict, dict_len, d_dict, reach))) return rc;
        return run_host_batch_multi(b, !known, 1ull << dev, make_run(d_dict, reach), 0, workers);
    }
    return hostbatch::run_host_batch_dict(*hc, b, dict, dict_len, !known, make_run, knob(kKnobHostSlices), knob(kKnobHostThreads));
}

int64_t lz4hip_encode_dict_scratch_bytes(int64_t dict_len) { return dict_len > 0 ? kFastTableBytes : 0; }

int lz4hip_encode_batch_dict_device(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, void* scratch, int64_t scratch_bytes, void* stream)
{
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = check_dict(dict, dict_len))) return rc;
    if (dict_len > 0 && !scratch) return fail(LZ4HIP_E_ARGUMENT, "encode with dictionary: scratch is NULL");
    if (dict_len > 0 && scratch_bytes < kFastTableBytes) return fail(LZ4HIP_E_ARGUMENT, "encode with dictionary: scratch_bytes is less than lz4hip_encode_dict_scratch_bytes gives");
    if (dict_len > 0 && (uintptr_t)scratch % 16) return fail(LZ4HIP_E_ARGUMENT, "encode with dictionary: scratch is not 16-byte aligned");
    if ((rc = ensure_device())) return rc;
    if (dict_len == 0) return launch_encode(b, LZ4HIP_MODE_FAST, (hipStream_t)stream);   // IS the plain call
    if (b->n_blocks == 0) return 0;
    if ((rc = launch_encode_dict_prime(dict, dict_len, scratch, (hipStream_t)stream))) return rc;
    return launch_encode_dict(b, dict, dict_len, scratch, (hipStream_t)stream);
}

// The dictionary goes up once and its table is primed once, on the calling thread's context, and both have landed before a slice is
// staged; the slices are those of lz4hip_encode_batch_host's one pipeline.
int lz4hip_encode_batch_dict_host(const lz4hip_batch_t* b, const void* dict, int64_t dict_len)
{
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = check_dict(dict, dict_len))) return rc;
    if (dict_len == 0) return lz4hip_encode_batch_host(b, LZ4HIP_MODE_FAST);              // IS the plain call
    if (b->n_blocks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HostContext* hc = host_context(dev);
    if (!hc) return fail(LZ4HIP_E_DEVICE, "device index out of range");
    return hostbatch::run_host_batch_encode_dict(*hc, b, dict, dict_len, [](const uint8_t* d_dict, int64_t reach, const uint8_t* table) {
        return [=](const lz4hip_batch_t* db, hipStream_t s) { return launch_encode_dict(db, d_dict, reach, table, s); };
    }, encode_host_slice_blocks(b, LZ4HIP_MODE_FAST), knob(kKnobHostSlices), knob(kKnobHostThreads));
}

int lz4hip_encode_batch_host_multi(const lz4hip_batch_t* b, int mode, uint64_t device_mask)
{
    return run_host_batch_multi(b, true, device_mask, encoder_run(mode), mode == LZ4HIP_MODE_HC ? kHcHostSliceBlocks : 0);
}

int lz4hip_decode_batch_host_multi(const lz4hip_batch_t* b, int known_output_size, uint64_t device_mask)
{
    return run_host_batch_multi(b, !known_output_size, device_mask, decoder_run(known_output_size));
}

int lz4hip_compress_limitedOutput(const char* source, char* dest, int isize, int maxOutputSize)
{
    return single(source, isize, dest, maxOutputSize, 0);
}
int lz4hip_compress(const char* source, char* dest, int isize)
{
    return single(source, isize, dest, lz4hip_compressBound(isize), 0);
}
int lz4hip_compressHC_limitedOutput(const char* source, char* dest, int isize, int maxOutputSize)
{
    return single(source, isize, dest, maxOutputSize, 1);
}
int lz4hip_compressHC(const char* source, char* dest, int isize)
{
    return single(source, isize, dest, lz4hip_compressBound(isize) + 1, 1);   /* original/lz4hc.c:762 */
}
int lz4hip_uncompress_bounded(const char* source, int isize, char* dest, int osize)
{
    return single(source, isize, dest, osize, 2);
}
int lz4hip_uncompress(const char* source, char* dest, int osize)
{
    if (!source || !dest) return fail(LZ4HIP_E_ARGUMENT, "NULL buffer");
    if (osize < 0) return fail(LZ4HIP_E_ARGUMENT, "negative length");
    return single(source, known_size_extent((const uint8_t*)source, osize), dest, osize, 2);
}
int lz4hip_uncompress_unknownOutputSize(const char* source, char* dest, int isize, int maxOutputSize)
{
    return single(source, isize, dest, maxOutputSize, 3);
}

int lz4hip_synth_device(int dist, uint64_t seed, uint64_t first_block, uint64_t block_step, int64_t n_blocks, void* out,
                        int64_t stride, int32_t len, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    if (n_blocks <= 0 || len <= 0) return 0;
    if (!out || dist < 0 || dist > 3) return fail(LZ4HIP_E_ARGUMENT, "bad synth arguments");
    SynthArgs a = { (uint8_t*)out, stride, n_blocks, seed, first_block, block_step, len, dist };
    const unsigned grid = dist <= 1 ? 16384u : (unsigned)((n_blocks + 63) / 64);
    hipLaunchKernelGGL(synth_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lz4hip_checksum_device(const void* data, const int64_t* off, int64_t stride, const int32_t* len,
                           int32_t len_all, uint64_t* sums, int64_t n_blocks, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    if (n_blocks <= 0) return 0;
    ChecksumArgs a = { (const uint8_t*)data, off, stride, len, len_all, sums, n_blocks };
    hipLaunchKernelGGL(checksum_kernel, dim3((unsigned)((n_blocks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lz4hip_compare_device(const void* a, int64_t a_stride, const void* b, int64_t b_stride,
                          const int32_t* len, int32_t len_all, int64_t n_blocks, uint64_t* mismatches,
                          void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    if (n_blocks <= 0) return 0;
    CompareArgs c = { (const uint8_t*)a, a_stride, (const uint8_t*)b, b_stride, len, len_all, n_blocks,
                      (unsigned long long*)mismatches };
    hipLaunchKernelGGL(compare_kernel, dim3((unsigned)((n_blocks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, c);
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t lz4hip_stream_bound(int64_t src_len, int32_t block_size) { return stream_bound(src_len, block_size); }

int64_t lz4hip_stream_encode_scratch_bytes(int64_t src_len, int32_t block_size)
{
    return src_len <= 0 ? 0 : stream_encode_scratch(nullptr, src_len, stream_block(block_size)).bytes;
}

int64_t lz4hip_stream_decode_scratch_bytes(int64_t max_chunks) { return stream_decode_scratch_bytes(max_chunks < 0 ? 0 : max_chunks); }

int lz4hip_stream_encode_device(const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len,
                                void* scratch, int64_t scratch_bytes, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return stream_encode(be, src, src_len, block_size, mode, dst, dst_cap, dst_len, scratch, scratch_bytes);
}

int lz4hip_stream_index_device(const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                               lz4hip_stream_info_t* info, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return stream_index(be, src, src_len, max_chunks, scratch, scratch_bytes, info);
}

int lz4hip_stream_decode_device(const void* src, const lz4hip_stream_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                                void* dst, int64_t dst_cap, lz4hip_stream_info_t* info, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return stream_decode(be, src, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, info);
}

int64_t lz4hip_stream_decode_into_scratch_bytes(int64_t max_chunks) { return stream_decode_into_scratch_bytes(max_chunks < 0 ? 0 : max_chunks); }

int lz4hip_stream_decode_into_device(const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst,
                                     int64_t dst_cap, lz4hip_stream_info_t* info, int64_t* written_bytes, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    StreamIntoPlan p;
    if (int rc = stream_decode_into_plan(be, src, src_len, max_chunks, scratch, scratch_bytes, dst, dst_cap, info, written_bytes, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return stream_decode_into_run(be, p);
}

int lz4hip_stream_directory_device(const void* src, int64_t src_len, int64_t max_chunks, int64_t* hdr_off, int64_t* out_off,
                                   lz4hip_stream_info_t* info, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    if (int rc = stream_directory_check(be, src, src_len, max_chunks, hdr_off, out_off, info)) return rc;
    if (int rc = ensure_device()) return rc;
    return stream_directory_run(be, src, src_len, max_chunks, hdr_off, out_off, info);
}

int lz4hip_stream_encode_host(const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return stream_encode_host(be, src, src_len, block_size, mode, dst, dst_cap, dst_len);
}

int lz4hip_stream_decode_host(const void* src, int64_t src_len, void* dst, int64_t dst_cap, lz4hip_stream_info_t* info)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return stream_decode_host(be, src, src_len, dst, dst_cap, info);
}

int64_t lz4hip_wrap_bound(int64_t n, int64_t src_len) { return wrap_bound(n, src_len); }

int64_t lz4hip_wrap_scratch_bytes(int64_t n, int64_t src_len) { return n <= 0 ? 0 : wrap_scratch(nullptr, n, src_len < 0 ? 0 : src_len).bytes; }

int64_t lz4hip_unwrap_scratch_bytes(int64_t n) { return unwrap_scratch_bytes(n < 0 ? 0 : n); }

int lz4hip_wrap_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode, void* dst, int64_t dst_cap,
                       int64_t* dst_off, int32_t* result, void* scratch, int64_t scratch_bytes, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return wrap_encode(be, src, src_len, src_off, n, mode, dst, dst_cap, dst_off, result, scratch, scratch_bytes);
}

int lz4hip_unwrap_index_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t* dst_off, int32_t* status,
                               void* scratch, int64_t scratch_bytes, lz4hip_unwrap_info_t* info, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return unwrap_index(be, src, src_len, src_off, n, dst_off, status, scratch, scratch_bytes, info);
}

int lz4hip_unwrap_decode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const lz4hip_unwrap_info_t* info_host,
                                void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, const int64_t* dst_off, int32_t* status,
                                lz4hip_unwrap_info_t* info, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return unwrap_decode(be, src, src_len, src_off, n, info_host, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info);
}

int64_t lz4hip_unwrap_into_scratch_bytes(int64_t n) { return unwrap_into_scratch_bytes(n < 0 ? 0 : n); }

int lz4hip_unwrap_into_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* scratch, int64_t scratch_bytes, void* dst,
                              int64_t dst_cap, int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info, int64_t* written_messages,
                              void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    UnwrapIntoPlan p;
    if (int rc = unwrap_into_plan(be, src, src_len, src_off, n, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info, written_messages, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return unwrap_into_run(be, p);
}

int lz4hip_unwrap_spans_into_device(const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m, void* scratch,
                                    int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status,
                                    lz4hip_unwrap_info_t* info, int64_t* written_messages, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    UnwrapIntoPlan p;
    if (int rc = unwrap_spans_into_plan(be, src, src_len, src_begin, src_end, m, scratch, scratch_bytes, dst, dst_cap, dst_off, status, info,
                                        written_messages, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return unwrap_into_run(be, p);
}

int lz4hip_spans_select_device(const int64_t* src_off, int64_t n, const int64_t* sel, int64_t m, int64_t* src_begin, int64_t* src_end, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    if (int rc = spans_select_check(be, src_off, n, sel, m, src_begin, src_end)) return rc;
    if (int rc = ensure_device()) return rc;
    return spans_select_run(be, src_off, n, sel, m, src_begin, src_end);
}

int lz4hip_wrap_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode, void* dst, int64_t dst_cap,
                     int64_t* dst_off, int32_t* result)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return wrap_host(be, src, src_len, src_off, n, mode, dst, dst_cap, dst_off, result);
}

int lz4hip_unwrap_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* dst, int64_t dst_cap, int64_t* dst_off,
                       int32_t* status, lz4hip_unwrap_info_t* info)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return unwrap_host(be, src, src_len, src_off, n, dst, dst_cap, dst_off, status, info);
}

int64_t lz4hip_streams_bound(int64_t n, int64_t src_len, int32_t block_size) { return streams_bound(n, src_len, block_size); }

int64_t lz4hip_streams_encode_scratch_bytes(int64_t n, int64_t src_len, int32_t block_size)
{
    return n <= 0 ? 0 : streams_encode_scratch(nullptr, n, src_len < 0 ? 0 : src_len, stream_block(block_size)).bytes;
}

int64_t lz4hip_streams_decode_scratch_bytes(int64_t n, int64_t max_chunks) { return streams_decode_scratch_bytes(n, max_chunks < 0 ? 0 : max_chunks); }

int lz4hip_streams_encode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode,
                                 void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return streams_encode(be, src, src_len, src_off, n, block_size, mode, dst, dst_cap, dst_off, scratch, scratch_bytes);
}

int lz4hip_streams_index_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks, int64_t* dst_off,
                                int32_t* status, int64_t* error_offset, void* scratch, int64_t scratch_bytes, lz4hip_streams_info_t* info,
                                void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return streams_index(be, src, src_len, src_off, n, max_chunks, dst_off, status, error_offset, scratch, scratch_bytes, info);
}

int lz4hip_streams_decode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const lz4hip_streams_info_t* info_host,
                                 int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, const int64_t* dst_off,
                                 int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info, void* stream)
{
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return streams_decode(be, src, src_len, src_off, n, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, dst_off, status, error_offset,
                          info);
}

int64_t lz4hip_streams_decode_into_scratch_bytes(int64_t n, int64_t max_chunks)
{
    return streams_decode_into_scratch_bytes(n, max_chunks < 0 ? 0 : max_chunks);
}

int lz4hip_streams_decode_into_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks, void* scratch,
                                      int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status,
                                      int64_t* error_offset, lz4hip_streams_info_t* info, int64_t* written_items, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    StreamsIntoPlan p;
    if (int rc = streams_decode_into_plan(be, src, src_len, src_off, n, max_chunks, scratch, scratch_bytes, dst, dst_cap, dst_off, status,
                                          error_offset, info, written_items, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return streams_decode_into_run(be, p);
}

int lz4hip_streams_decode_spans_into_device(const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m,
                                            int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                            int64_t* dst_off, int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info,
                                            int64_t* written_items, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    StreamsIntoPlan p;
    if (int rc = streams_decode_spans_into_plan(be, src, src_len, src_begin, src_end, m, max_chunks, scratch, scratch_bytes, dst, dst_cap, dst_off,
                                                status, error_offset, info, written_items, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return streams_decode_into_run(be, p);
}

int lz4hip_streams_encode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode,
                               void* dst, int64_t dst_cap, int64_t* dst_off)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return streams_encode_host(be, src, src_len, src_off, n, block_size, mode, dst, dst_cap, dst_off);
}

int lz4hip_streams_decode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, void* dst, int64_t dst_cap, int64_t* dst_off,
                               int32_t* status, int64_t* error_offset, lz4hip_streams_info_t* info)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return streams_decode_host(be, src, src_len, src_off, n, dst, dst_cap, dst_off, status, error_offset, info);
}

int64_t lz4hip_decoded_sizes_scratch_bytes(int64_t n_blocks) { return sizes_scratch_bytes(n_blocks); }

// (the arguments are checked before the device is looked for: a bad call is LZ4HIP_E_ARGUMENT on any machine)
int lz4hip_decoded_sizes_device(const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap, void* scratch, int64_t scratch_bytes,
                                lz4hip_sizes_info_t* info, void* stream)
{
    if (!b) return fail(LZ4HIP_E_ARGUMENT, "decoded sizes: batch descriptor is NULL");
    if (b->n_blocks < 0) return fail(LZ4HIP_E_ARGUMENT, "decoded sizes: n_blocks < 0");
    if (scratch_bytes < sizes_scratch_bytes(b->n_blocks)) return fail(LZ4HIP_E_ARGUMENT, "decoded sizes: scratch_bytes < lz4hip_decoded_sizes_scratch_bytes");
    if (b->n_blocks == 0 && !dst_off && !info) return 0;                // (nothing to write)
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return decoded_sizes(be, b, dst_off, dst_cap, scratch, scratch_bytes, info, knob(kKnobSizesGroups));
}

int lz4hip_decoded_sizes_host(const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap, lz4hip_sizes_info_t* info)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return hostbatch::decoded_sizes_host(be, b, dst_off, dst_cap, info, knob(kKnobSizesGroups), knob(kKnobHostThreads));
}

// (the walk looks at no byte of the dictionary: its length is all these take)
int lz4hip_decoded_sizes_dict_device(const lz4hip_batch_t* b, int64_t dict_len, int64_t* dst_off, int32_t* dst_cap, void* scratch, int64_t scratch_bytes,
                                     lz4hip_sizes_info_t* info, void* stream)
{
    if (!b) return fail(LZ4HIP_E_ARGUMENT, "decoded sizes: batch descriptor is NULL");
    if (b->n_blocks < 0) return fail(LZ4HIP_E_ARGUMENT, "decoded sizes: n_blocks < 0");
    if (dict_len < 0) return fail(LZ4HIP_E_ARGUMENT, "dictionary: dict_len < 0");
    if (scratch_bytes < sizes_scratch_bytes(b->n_blocks)) return fail(LZ4HIP_E_ARGUMENT, "decoded sizes: scratch_bytes < lz4hip_decoded_sizes_scratch_bytes");
    if (b->n_blocks == 0 && !dst_off && !info) return 0;                // (nothing to write)
    int rc = ensure_device();
    if (rc) return rc;
    HipBackend be = { (hipStream_t)stream };
    return decoded_sizes(be, b, dst_off, dst_cap, scratch, scratch_bytes, info, knob(kKnobSizesGroups), dict_len);
}

int lz4hip_decoded_sizes_dict_host(const lz4hip_batch_t* b, int64_t dict_len, int64_t* dst_off, int32_t* dst_cap, lz4hip_sizes_info_t* info)
{
    if (!b) return fail(LZ4HIP_E_ARGUMENT, "decoded sizes: batch descriptor is NULL");
    if (b->n_blocks < 0) return fail(LZ4HIP_E_ARGUMENT, "decoded sizes: n_blocks < 0");
    if (dict_len < 0) return fail(LZ4HIP_E_ARGUMENT, "dictionary: dict_len < 0");
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return hostbatch::decoded_sizes_host(be, b, dst_off, dst_cap, info, knob(kKnobSizesGroups), knob(kKnobHostThreads), hostbatch::HostLimits(), dict_len);
}

int64_t lz4hip_encode_packed_scratch_bytes(int64_t n_blocks, int32_t slot_bytes, int64_t round_blocks)
{
    return encode_packed_scratch_bytes(n_blocks, slot_bytes, round_blocks);
}

// (the arguments are checked before the device is looked for: a bad call is LZ4HIP_E_ARGUMENT on any machine)
int lz4hip_encode_packed_device(const lz4hip_batch_t* b, int mode, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                                int32_t* packed_len, void* scratch, int64_t scratch_bytes, lz4hip_packed_info_t* info, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    PackedPlan p;
    if (int rc = encode_packed_plan(be, b, mode, round_blocks, dst, dst_cap, dst_off, packed_len, scratch, scratch_bytes, info, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return encode_packed_run(be, p);
}

int lz4hip_encode_packed_host(const lz4hip_batch_t* b, int mode, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                              int32_t* packed_len, lz4hip_packed_info_t* info)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return hostbatch::encode_packed_host(be, b, mode, round_blocks, dst, dst_cap, dst_off, packed_len, info, knob(kKnobHostThreads));
}

int64_t lz4hip_decode_compact_scratch_bytes(int64_t n_blocks, int32_t slot_bytes, int64_t round_blocks)
{
    return decode_compact_scratch_bytes(n_blocks, slot_bytes, round_blocks);
}

// (the arguments are checked before the device is looked for: a bad call is LZ4HIP_E_ARGUMENT on any machine)
int lz4hip_decode_compact_device(const lz4hip_batch_t* b, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                                 int32_t* decoded_len, void* scratch, int64_t scratch_bytes, lz4hip_compact_info_t* info, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    PackedPlan p;
    if (int rc = decode_compact_plan(be, b, round_blocks, dst, dst_cap, dst_off, decoded_len, scratch, scratch_bytes, info, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return decode_compact_run(be, p);
}

int lz4hip_decode_compact_host(const lz4hip_batch_t* b, int64_t round_blocks, void* dst, int64_t dst_cap, int64_t* dst_off,
                               int32_t* decoded_len, lz4hip_compact_info_t* info)
{
    HipBackend be = {};
    if (int rc = decode_compact_check(be, b, round_blocks, dst, dst_cap, dst_off)) return rc;
    if (int rc = stream_host_context(be)) return rc;
    return hostbatch::decode_compact_host(be, b, round_blocks, dst, dst_cap, dst_off, decoded_len, info, knob(kKnobHostThreads));
}

int64_t lz4hip_frame_bound(int64_t src_len, int32_t chunk_size) { return frame_bound(src_len, chunk_size); }

int64_t lz4hip_frame_encode_scratch_bytes(int64_t src_len, int32_t chunk_size)
{
    if (!frame_chunk_valid(chunk_size)) return fail(LZ4HIP_E_ARGUMENT, "frame encode: chunk_size must be 0 (8 MiB) or 1 .. 0x7E000000");
    return frame_encode_scratch(nullptr, src_len < 0 ? 0 : src_len, frame_chunk(chunk_size)).bytes;
}

int64_t lz4hip_frame_decode_scratch_bytes(int64_t max_chunks) { return frame_decode_scratch_bytes(max_chunks < 0 ? 0 : max_chunks); }

// (the arguments are checked before the device is looked for: a bad call is LZ4HIP_E_ARGUMENT on any machine)
int lz4hip_frame_encode_device(const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len,
                               void* scratch, int64_t scratch_bytes, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    FrameEncodePlan p;
    if (int rc = frame_encode_plan(be, src, src_len, chunk_size, mode, dst, dst_cap, dst_len, scratch, scratch_bytes, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return frame_encode_run(be, p);
}

int lz4hip_frame_index_device(const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                              lz4hip_frame_info_t* info, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    FrameIndexPlan p;
    if (int rc = frame_index_plan(be, src, src_len, chunk_size, max_chunks, scratch, scratch_bytes, info, knob(kKnobSizesGroups), p)) return rc;
    if (int rc = ensure_device()) return rc;
    return frame_index_run(be, p);
}

int lz4hip_frame_decode_device(const void* src, const lz4hip_frame_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                               void* dst, int64_t dst_cap, lz4hip_frame_info_t* info, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    FrameDecodePlan p;
    if (int rc = frame_decode_plan(be, src, info_host, max_chunks, scratch, scratch_bytes, dst, dst_cap, info, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return frame_decode_run(be, p);
}

int64_t lz4hip_frame_decode_compact_scratch_bytes(int32_t chunk_size, int64_t max_chunks, int64_t round_chunks)
{
    return frame_decode_compact_scratch_bytes(chunk_size, max_chunks, round_chunks);
}

int lz4hip_frame_decode_compact_device(const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, int64_t round_chunks,
                                       void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_frame_info_t* info, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    FrameCompactPlan p;
    if (int rc = frame_decode_compact_plan(be, src, src_len, chunk_size, max_chunks, round_chunks, scratch, scratch_bytes, dst, dst_cap, info, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return frame_decode_compact_run(be, p);
}

int lz4hip_frame_encode_host(const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return frame_encode_host(be, src, src_len, chunk_size, mode, dst, dst_cap, dst_len);
}

int lz4hip_frame_decode_host(const void* src, int64_t src_len, int32_t chunk_size, void* dst, int64_t dst_cap, lz4hip_frame_info_t* info)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return frame_decode_host(be, src, src_len, chunk_size, dst, dst_cap, info);
}

// (the arguments are checked before the device is looked for: a bad call is LZ4HIP_E_ARGUMENT on any machine)
int lz4hip_xxh32_rows_device(const void* data, const int64_t* off, int64_t stride, const int32_t* len, int64_t len_all, uint32_t seed,
                             uint32_t* sums, int64_t n_rows, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    if (int rc = xxh32_rows_check(be, data, off, stride, len, len_all, sums, n_rows)) return rc;
    if (n_rows == 0) return 0;
    if (int rc = ensure_device()) return rc;
    const XxhRows rows = { (const uint8_t*)data, off, stride, len, nullptr, len_all, seed, sums, n_rows };
    return xxh32_rows_run(be, rows);
}

int64_t lz4hip_lz4f_bound(int64_t src_len, int block_size_id, unsigned flags) { return lz4f_bound(src_len, block_size_id, flags); }

int64_t lz4hip_lz4f_encode_scratch_bytes(int64_t src_len, int block_size_id)
{
    if (!lz4f_id_valid(block_size_id)) return fail(LZ4HIP_E_ARGUMENT, "lz4f encode: block_size_id must be 0 (64 KiB) or 4 .. 7");
    return lz4f_encode_scratch(nullptr, src_len < 0 ? 0 : src_len, lz4f_block_bytes(lz4f_id(block_size_id))).bytes;
}

int64_t lz4hip_lz4f_decode_scratch_bytes(int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    return lz4f_decode_scratch_bytes(slot_bytes, max_blocks, round_blocks);
}

int lz4hip_lz4f_encode_device(const void* src, int64_t src_len, int block_size_id, int mode, unsigned flags, void* dst, int64_t dst_cap,
                              int64_t* dst_len, void* scratch, int64_t scratch_bytes, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    Lz4fEncodePlan p;
    if (int rc = lz4f_encode_plan(be, src, src_len, block_size_id, mode, flags, dst, dst_cap, dst_len, scratch, scratch_bytes, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return lz4f_encode_run(be, p);
}

int lz4hip_lz4f_decode_device(const void* src, int64_t src_len, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags,
                              void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    Lz4fDecodePlan p;
    if (int rc = lz4f_decode_plan(be, src, src_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return lz4f_decode_run(be, p);
}

// The dictionary calls: the plain call's plan behind the dictionary's check, then the sequence with the dictionary handed to the walk,
// the rounds and the linked decode (lz4hip_framing.hpp); with dict_len == 0 the plain sequence.
int lz4hip_lz4f_decode_dict_device(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int32_t slot_bytes,
                                   int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                   lz4hip_lz4f_info_t* info, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    Lz4fDecodePlan p;
    if (int rc = lz4f_decode_dict_plan(be, src, src_len, dict, dict_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap, info, p))
        return rc;
    if (int rc = ensure_device()) return rc;
    return lz4f_decode_dict_run(be, p, dict, dict_len, dict_id);
}

int lz4hip_lz4f_decode_dict_host(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, unsigned flags, void* dst,
                                 int64_t dst_cap, lz4hip_lz4f_info_t* info)
{
    HipBackend be = {};
    if (int rc = check_dict(dict, dict_len)) return rc;
    if (int rc = stream_host_context(be)) return rc;
    return lz4f_decode_dict_host(be, src, src_len, dict, dict_len, dict_id, flags, dst, dst_cap, info);
}

// The dictionary encode: the plain call's plan in fast mode behind the dictionary's check, with the dictionary's bound, scratch and head
// length, then the sequence with the dictionary handed to the block encoder and the head kernel (lz4hip_framing.hpp); with dict_len == 0
// the plain sequence.
int64_t lz4hip_lz4f_dict_bound(int64_t src_len, int block_size_id, unsigned flags, int64_t dict_len, uint32_t dict_id)
{
    return lz4f_dict_bound(src_len, block_size_id, flags, dict_len, dict_id);
}

int64_t lz4hip_lz4f_encode_dict_scratch_bytes(int64_t src_len, int block_size_id, int64_t dict_len)
{
    if (dict_len < 0) return fail(LZ4HIP_E_ARGUMENT, "dictionary: dict_len < 0");
    if (!lz4f_id_valid(block_size_id)) return fail(LZ4HIP_E_ARGUMENT, "lz4f encode: block_size_id must be 0 (64 KiB) or 4 .. 7");
    return lz4f_encode_scratch(nullptr, src_len < 0 ? 0 : src_len, lz4f_block_bytes(lz4f_id(block_size_id)), dict_len).bytes;
}

int lz4hip_lz4f_encode_dict_device(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int block_size_id, unsigned flags,
                                   void* dst, int64_t dst_cap, int64_t* dst_len, void* scratch, int64_t scratch_bytes, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    Lz4fEncodePlan p;
    Lz4fDict d;
    if (int rc = lz4f_encode_dict_plan(be, src, src_len, dict, dict_len, dict_id, block_size_id, flags, dst, dst_cap, dst_len, scratch, scratch_bytes, p, d)) return rc;
    if (int rc = ensure_device()) return rc;
    return lz4f_encode_dict_run(be, p, d);
}

int lz4hip_lz4f_encode_dict_host(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int block_size_id, unsigned flags,
                                 void* dst, int64_t dst_cap, int64_t* dst_len)
{
    HipBackend be = {};
    if (int rc = check_dict(dict, dict_len)) return rc;
    if (src_len < 0 || !dst_len || !dst || (src_len > 0 && !src)) return fail(LZ4HIP_E_ARGUMENT, "lz4f encode: negative size or NULL pointer");
    if (!lz4f_id_valid(block_size_id) || (flags & ~kLz4fEncodeFlags)) return fail(LZ4HIP_E_ARGUMENT, "lz4f encode: block_size_id must be 0 or 4 .. 7, flags known");
    if (dst_cap < lz4f_dict_bound(src_len, block_size_id, flags, dict_len, dict_id)) return fail(LZ4HIP_E_ARGUMENT, "lz4f encode: dst_cap < lz4hip_lz4f_dict_bound");
    if (int rc = stream_host_context(be)) return rc;
    return lz4f_encode_dict_host(be, src, src_len, dict, dict_len, dict_id, block_size_id, flags, dst, dst_cap, dst_len);
}

int lz4hip_lz4f_encode_host(const void* src, int64_t src_len, int block_size_id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return lz4f_encode_host(be, src, src_len, block_size_id, mode, flags, dst, dst_cap, dst_len);
}

int lz4hip_lz4f_decode_host(const void* src, int64_t src_len, unsigned flags, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return lz4f_decode_host(be, src, src_len, flags, dst, dst_cap, info);
}

int64_t lz4hip_lz4f_batch_bound(int64_t n, int64_t src_len, int block_size_id, unsigned flags) { return lz4f_batch_bound(n, src_len, block_size_id, flags); }

int64_t lz4hip_lz4f_batch_encode_scratch_bytes(int64_t n, int64_t src_len, int block_size_id)
{
    if (!lz4f_id_valid(block_size_id)) return fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: block_size_id must be 0 (64 KiB) or 4 .. 7");
    return n <= 0 ? 0 : lz4f_batch_encode_scratch(nullptr, n, src_len < 0 ? 0 : src_len, lz4f_block_bytes(lz4f_id(block_size_id))).bytes;
}

int64_t lz4hip_lz4f_batch_decode_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks)
{
    return lz4f_batch_decode_scratch_bytes(n, slot_bytes, max_blocks, round_blocks);
}

int lz4hip_lz4f_batch_encode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int mode, unsigned flags,
                                    void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    Lz4fBatchEncodePlan p;
    if (int rc = lz4f_batch_encode_plan(be, src, src_len, src_off, n, block_size_id, mode, flags, dst, dst_cap, dst_off, scratch, scratch_bytes, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return lz4f_batch_encode_run(be, p);
}

int lz4hip_lz4f_batch_decode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t slot_bytes, int64_t max_blocks,
                                    int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                    int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, int64_t* written_items,
                                    void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    Lz4fBatchDecodePlan p;
    if (int rc = lz4f_batch_decode_plan(be, src, src_len, src_off, n, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst, dst_cap,
                                        dst_off, item_info, info, written_items, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return lz4f_batch_decode_run(be, p);
}

int lz4hip_lz4f_batch_decode_dict_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len,
                                         uint32_t dict_id, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch,
                                         int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info,
                                         lz4hip_lz4f_batch_info_t* info, int64_t* written_items, void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    Lz4fBatchDecodePlan p;
    if (int rc = lz4f_batch_decode_dict_plan(be, src, src_len, src_off, n, dict, dict_len, slot_bytes, max_blocks, round_blocks, flags, scratch, scratch_bytes, dst,
                                             dst_cap, dst_off, item_info, info, written_items, p)) return rc;
    if (int rc = ensure_device()) return rc;
    return lz4f_batch_decode_dict_run(be, p, dict, dict_len, dict_id);
}

int lz4hip_lz4f_batch_decode_dict_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                       unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info,
                                       lz4hip_lz4f_batch_info_t* info)
{
    HipBackend be = {};
    if (int rc = check_dict(dict, dict_len)) return rc;
    if (int rc = stream_host_context(be)) return rc;
    return lz4f_batch_decode_dict_host(be, src, src_len, src_off, n, dict, dict_len, dict_id, flags, dst, dst_cap, dst_off, item_info, info);
}

int64_t lz4hip_lz4f_batch_dict_bound(int64_t n, int64_t src_len, int block_size_id, unsigned flags, int64_t dict_len, uint32_t dict_id)
{
    return lz4f_batch_dict_bound(n, src_len, block_size_id, flags, dict_len, dict_id);
}

int64_t lz4hip_lz4f_batch_encode_dict_scratch_bytes(int64_t n, int64_t src_len, int block_size_id, int64_t dict_len)
{
    if (dict_len < 0) return fail(LZ4HIP_E_ARGUMENT, "dictionary: dict_len < 0");
    if (!lz4f_id_valid(block_size_id)) return fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: block_size_id must be 0 (64 KiB) or 4 .. 7");
    return n <= 0 ? 0 : lz4f_batch_encode_scratch(nullptr, n, src_len < 0 ? 0 : src_len, lz4f_block_bytes(lz4f_id(block_size_id)), dict_len).bytes;
}

int lz4hip_lz4f_batch_encode_dict_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                         int block_size_id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes,
                                         void* stream)
{
    HipBackend be = { (hipStream_t)stream };
    Lz4fBatchEncodePlan p;
    Lz4fDict d;
    if (int rc = lz4f_batch_encode_dict_plan(be, src, src_len, src_off, n, dict, dict_len, dict_id, block_size_id, flags, dst, dst_cap, dst_off, scratch,
                                             scratch_bytes, p, d)) return rc;
    if (int rc = ensure_device()) return rc;
    return lz4f_batch_encode_dict_run(be, p, d);
}

int lz4hip_lz4f_batch_encode_dict_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                       int block_size_id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off)
{
    HipBackend be = {};
    if (int rc = check_dict(dict, dict_len)) return rc;
    if (src_len < 0 || n < 0 || !dst_off || (n > 0 && (!src_off || !dst)) || (src_len > 0 && n > 0 && !src))
        return fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: negative size or NULL pointer");
    if (!lz4f_id_valid(block_size_id) || (flags & ~kLz4fEncodeFlags)) return fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: block_size_id must be 0 or 4 .. 7, flags known");
    if (n > 0 && dst_cap < lz4f_batch_dict_bound(n, src_len, block_size_id, flags, dict_len, dict_id))
        return fail(LZ4HIP_E_ARGUMENT, "lz4f batch encode: dst_cap < lz4hip_lz4f_batch_dict_bound");
    if (int rc = stream_host_context(be)) return rc;
    return lz4f_batch_encode_dict_host(be, src, src_len, src_off, n, dict, dict_len, dict_id, block_size_id, flags, dst, dst_cap, dst_off);
}

int lz4hip_lz4f_batch_encode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int mode, unsigned flags,
                                  void* dst, int64_t dst_cap, int64_t* dst_off)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return lz4f_batch_encode_host(be, src, src_len, src_off, n, block_size_id, mode, flags, dst, dst_cap, dst_off);
}

int lz4hip_lz4f_batch_decode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, unsigned flags, void* dst, int64_t dst_cap,
                                  int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info)
{
    HipBackend be = {};
    if (int rc = stream_host_context(be)) return rc;
    return lz4f_batch_decode_host(be, src, src_len, src_off, n, flags, dst, dst_cap, dst_off, item_info, info);
}

}  // extern "C"
