// Where does a LONE wavefront of the lane decoder (lz4hip_decode_lane4.hpp, the shipped <true,192,32,128,2,2,2,16>) spend its cycles?  (not part of the product)
// One wavefront decodes 64 blocks.  Every LZ4HIP_SECTION marker of the iteration reads the clock (s_memtime) and adds the ticks since the
// marker before it to a register of its own, separately for the two copies of the loop body (the iteration that flushes, the one that
// requests input).  A marker's register therefore holds the stretch of code that ENDS at it; the table names each row after the marker
// BEFORE it in source order, the section that stretch is (the first marker's row is the end of the previous iteration and the loop).
// The clock read waits for the wavefront's outstanding LDS operations (lgkmcnt(0)), so an LDS latency is charged to the section that
// issued it and the measured iteration is somewhat longer than the product's; plain value operations (the selects) are not held in
// place by a clock read, the compiler moves them across it.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -Ilz4net_amd/csrc tools/dec_lane_sections.hip -o tools/dec_lane_sections && tools/dec_lane_sections [dist]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "lz4hip_wave.hpp"
#include "lz4hip_common.hpp"
constexpr int kSecMax = 24;
__device__ unsigned g_sec[2][kSecMax], g_iters;
enum { kSecBase = __COUNTER__ + 1 };
#define LZ4HIP_SECTION_BEGIN() uint32_t sec_acc[2][kSecMax] = {}; uint32_t sec_iters = 0; uint64_t sec_mark = __builtin_readcyclecounter()
#define LZ4HIP_SEC_AT(c) do { static_assert((c) - kSecBase < kSecMax, "more markers than slots"); const uint64_t now_ = __builtin_readcyclecounter(); \
        sec_acc[FLUSH ? 0 : 1][(c) - kSecBase] += (uint32_t)(now_ - sec_mark); sec_mark = now_; } while (0)
#define LZ4HIP_SECTION(name) LZ4HIP_SEC_AT(__COUNTER__)
#define LZ4HIP_ITERATION_HOOK(lane) (sec_iters++)
#define LZ4HIP_SECTION_END(lane) do { if ((lane) == 0) { for (int c_ = 0; c_ < 2; c_++) for (int k_ = 0; k_ < kSecMax; k_++) g_sec[c_][k_] = sec_acc[c_][k_]; g_iters = sec_iters; } } while (0)
#include "lz4hip_decode_lane4.hpp"
enum { kSecSites = __COUNTER__ - kSecBase };
#include "lz4hip_encode.hpp"
#include "lz4hip_synth.hpp"
using namespace lz4hip;

// the markers of the iteration in source order (the static_assert below keeps this list in step with the header)
static const char* const kMarker[] = { "T2a flush records", "T2b record read", "T1c near-match reads", "T1a window refill", "T1b cursor view",
                                       "T1c near-match source rows", "T3 chunk size", "T2c ring rows", "T4 parse ahead", "T4 parse ahead where it does not trap, else T4x byte-wise parser", "T4 parse ahead (after the trap)",
                                       "T2d flush stores", "T5 far fetch", "T6 input request", "B1 wait", "B3 chunk append", "B4 promote + literal append", "B5 end of block + loop" };
static_assert(sizeof(kMarker) / sizeof(kMarker[0]) == kSecSites, "kMarker lists the LZ4HIP_SECTION markers of lz4hip_decode_lane4.hpp in source order");

__global__ void __launch_bounds__(64) enc(const uint8_t* raw, uint8_t* comp, int* res)
{
    LZ4HIP_DYN_LDS(lds);
    const int r = encode_fast_block64k(raw + (size_t)blockIdx.x * 65536, 65536, comp + (size_t)blockIdx.x * 65824, 65809, lds, false);
    if (threadIdx.x == 0) res[blockIdx.x] = r;
}
__global__ void __launch_bounds__(64) dec(const uint8_t* comp, const int* clen, uint8_t* back, int* res, unsigned long long* total)
{
    LZ4HIP_STATIC_LDS(lds, lane4_lds_bytes(192));
    const int lane = (int)threadIdx.x;
    const unsigned long long t0 = __builtin_readcyclecounter();
    const int r = lane4_decode_block<true, 192, 32, 128, 2, 2, 2, 16>(lds, lane, true, comp + (size_t)lane * 65824, clen[lane], back + (size_t)lane * 65536, 65536);
    res[lane] = r;
    if (lane == 0) *total = __builtin_readcyclecounter() - t0;
}

int main(int argc, char** argv)
{
    const int n = 64, dist = argc > 1 ? atoi(argv[1]) : 2;
    uint8_t *raw, *comp, *back; int *clen, *res; unsigned long long* total;
    hipMalloc(&raw, (size_t)n * 65536); hipMalloc(&back, (size_t)n * 65536); hipMalloc(&comp, (size_t)n * 65824); hipMalloc(&clen, n * 4); hipMalloc(&res, n * 4); hipMalloc(&total, 8);
    SynthArgs a = { raw, 65536, n, 20260925ull, 0, 1, 65536, dist };
    hipLaunchKernelGGL(synth_kernel, dim3(dist <= 1 ? 4096 : (n + 63) / 64), dim3(64), 0, 0, a);
    hipLaunchKernelGGL(enc, dim3(n), dim3(64), kFastTableBytes, 0, raw, comp, clen);
    if (hipDeviceSynchronize() != hipSuccess) { printf("set-up failed\n"); return 1; }
    for (int rep = 0; rep < 2; rep++) {
        hipMemset(back, 0, (size_t)n * 65536);
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        hipEventRecord(e0);
        hipLaunchKernelGGL(dec, dim3(1), dim3(64), 0, 0, comp, clen, back, res, total);
        hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) { printf("decode failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
        float ms; hipEventElapsedTime(&ms, e0, e1);
        if (rep == 0) continue;
        unsigned sec[2][kSecMax], iters; unsigned long long tot;
        hipMemcpyFromSymbol(sec, HIP_SYMBOL(g_sec), sizeof sec); hipMemcpyFromSymbol(&iters, HIP_SYMBOL(g_iters), sizeof iters); hipMemcpy(&tot, total, 8, hipMemcpyDeviceToHost);
        std::vector<int> r(n), c(n); hipMemcpy(r.data(), res, n * 4, hipMemcpyDeviceToHost); hipMemcpy(c.data(), clen, n * 4, hipMemcpyDeviceToHost);
        std::vector<uint8_t> hr((size_t)n * 65536), hb((size_t)n * 65536);
        hipMemcpy(hr.data(), raw, hr.size(), hipMemcpyDeviceToHost); hipMemcpy(hb.data(), back, hb.size(), hipMemcpyDeviceToHost);
        int bad = 0; for (int i = 0; i < n; i++) bad += r[i] != c[i];
        printf("dist %d, one wavefront, 64 blocks: kernel %.3f ms, %u iterations, %llu ticks = %.0f per iteration (%.1f ticks per us); results %s, bytes %s\n", dist, ms, iters, tot,
               (double)tot / iters, (double)tot / (ms * 1e3), bad ? "WRONG" : "ok", hr == hb ? "ok" : "WRONG");
        printf("%-48s %12s %12s %12s\n", "ticks per iteration, by section", "flush iter", "input iter", "mean");
        const double half = iters / 2.0;
        double sum[2] = { 0, 0 };
        for (int k = 0; k < kSecSites; k++) {
            const double f = sec[0][k] / half, i = sec[1][k] / half;
            sum[0] += f; sum[1] += i;
            printf("%-48s %12.1f %12.1f %12.1f\n", kMarker[(k + kSecSites - 1) % kSecSites], f, i, (f + i) / 2);
        }
        printf("%-48s %12.1f %12.1f %12.1f\n", "sum", sum[0], sum[1], (sum[0] + sum[1]) / 2);
    }
    return 0;
}
