// Issue rate of the integer VALU instructions the lane decoder is made of, per SIMD, at 1 / 3 / 4 / 8 wavefronts per SIMD.
// Each wavefront runs ITER x 32 independent instructions of one kind (8 accumulators); reports SIMD-cycles per
// wavefront-instruction assuming 2.4 GHz.
// Kinds 20 .. 26 are the forms of a CONDITIONAL ASSIGNMENT x = m ? a : x that are not a select: v_mov_b32 inside an EXEC region
// (s_and_saveexec_b64 .. s_mov_b64 exec; 1, 4 or 8 moves per region, the per-lane mask differs from region to region) and v_pk_mov_b32
// (two dwords per instruction), alone and inside such a region.  Their ITER x 32 are MOVED DWORDS: the line gives SIMD-cycles per moved
// dword with the two scalar instructions of each region included, next to what v_cndmask_b32_e64 (kind 10) costs per dword.
// Kinds 30 .. 33 are the CALIBRATION OF A COMPARE IN A MIX: a body of 48 independent instructions in the lane decoder's ratio of encodings
// (28 v_perm_b32 : 20 v_add_u32, eight accumulators) with k = 0, 2, 4, 8 v_cmp_lt_u32_e64 to SGPR pairs of their own interleaved; the slope of
// SIMD-cycles per body over k is what ONE compare adds in the middle of other vector work (the stream of compares alone: kind 15).
//   hipcc --offload-arch=gfx950 -O3 tools/microbench_valu_rate.hip -o tools/microbench_valu_rate
//   tools/microbench_valu_rate [mix]        (mix: only the calibration)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>

template <int KIND>
__global__ void __launch_bounds__(64) k(uint32_t* out, int iters, uint32_t s)
{
    uint32_t a[8];
    for (int j = 0; j < 8; j++) a[j] = threadIdx.x * 2654435761u + j;
    uint32_t b = s ^ threadIdx.x, c = s + 77u;
    uint64_t m64 = 0x5555AAAA3333CCCCull ^ s;
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (KIND >= 20) {
                // 8 moved dwords per trip of r, like the 8 instructions of the other kinds; the mask of a region depends on r and on its place
                const uint64_t ma = m64 ^ (0x0123456789ABCDEFull * (uint64_t)(r + 1)), mb = ~ma ^ 0xF0F0F0F00F0F0F0Full;
                uint64_t sv;                                         // (s_and_saveexec_b64 writes SCC: the statements say so, or the compiler keeps the loop's compare live across them)
                uint64_t* const q = (uint64_t*)a;                    // a[0..7] as four register pairs
#define MOV1(J) "v_mov_b32 %" #J ", %[b]\n\t"
#define RGN(M, BODY) "s_and_saveexec_b64 %[sv], %[" M "]\n\t" BODY "s_mov_b64 exec, %[sv]\n\t"
#define A8 "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), [sv] "=&s"(sv)
#define Q4 "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), [sv] "=&s"(sv)
                if (KIND == 20)                                      // one move per region
                    asm volatile(RGN("ma", MOV1(0)) RGN("mb", MOV1(1)) RGN("ma", MOV1(2)) RGN("mb", MOV1(3)) RGN("ma", MOV1(4)) RGN("mb", MOV1(5)) RGN("ma", MOV1(6)) RGN("mb", MOV1(7))
                                 : A8 : [b] "v"(b), [ma] "s"(ma), [mb] "s"(mb) : "scc");
                if (KIND == 21)                                      // four moves per region
                    asm volatile(RGN("ma", MOV1(0) MOV1(1) MOV1(2) MOV1(3)) RGN("mb", MOV1(4) MOV1(5) MOV1(6) MOV1(7)) : A8 : [b] "v"(b), [ma] "s"(ma), [mb] "s"(mb) : "scc");
                if (KIND == 22)                                      // eight moves per region
                    asm volatile(RGN("ma", MOV1(0) MOV1(1) MOV1(2) MOV1(3) MOV1(4) MOV1(5) MOV1(6) MOV1(7)) : A8 : [b] "v"(b), [ma] "s"(ma) : "scc");
#define PK(J) "v_pk_mov_b32 %" #J ", %[p], %[p] op_sel:[0,1]\n\t"      /* d.lo = p.lo, d.hi = p.hi */
#define PKS(J) "v_pk_mov_b32 %" #J ", %[p], %[p2] op_sel:[1,0]\n\t"    /* d.lo = p.hi, d.hi = p2.lo: a window shifted by one dword */
                const uint64_t p = ((uint64_t)c << 32) | b, p2 = ((uint64_t)b << 32) | c;
                if (KIND == 23) asm volatile(PK(0) PK(1) PK(2) PK(3) : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]) : [p] "v"(p));
                if (KIND == 24) asm volatile(RGN("ma", PK(0) PK(1) PK(2) PK(3)) : Q4 : [p] "v"(p), [ma] "s"(ma) : "scc");          // one region of four: 8 dwords
                if (KIND == 25) asm volatile(PKS(0) PKS(1) PKS(2) PKS(3) : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]) : [p] "v"(p), [p2] "v"(p2));
                if (KIND == 26) asm volatile(RGN("ma", PKS(0) PKS(1) PKS(2) PKS(3)) : Q4 : [p] "v"(p), [p2] "v"(p2), [ma] "s"(ma) : "scc");
#undef MOV1
#undef RGN
#undef A8
#undef Q4
#undef PK
#undef PKS
                continue;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (KIND == 0) asm volatile("v_add_u32 %0, %0, %1" : "+v"(a[j]) : "v"(b));
                if (KIND == 1) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(a[j]) : "v"(b), "v"(c));
                if (KIND == 2) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(a[j]) : "v"(b), "v"(c));
                if (KIND == 3) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(a[j]) : "v"(b));
                if (KIND == 4) asm volatile("v_alignbyte_b32 %0, %0, %1, %2" : "+v"(a[j]) : "v"(b), "v"(c));
                if (KIND == 5) asm volatile("v_lshl_add_u32 %0, %0, 2, %1" : "+v"(a[j]) : "v"(b));
                if (KIND == 6) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a[j]) : "v"(b));
                if (KIND == 7) asm volatile("v_cmp_lt_u32 vcc, %0, %1" : : "v"(a[j]), "v"(b) : "vcc");
                if (KIND == 8) asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(*(uint64_t*)&a[j & 6]) : "v"(*(uint64_t*)&a[(j & 6) ^ 2]));
                if (KIND == 9) asm volatile("v_add_u32 %0, %0, %0" : "+v"(a[0]));          // dependent chain
                if (KIND == 10) asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(a[j]) : "v"(b), "s"(m64));
                if (KIND == 11) asm volatile("v_mov_b32 %0, %1" : "+v"(a[j]) : "v"(b));
                if (KIND == 12) asm volatile("v_and_b32 %0, %0, %1" : "+v"(a[j]) : "v"(b));
                if (KIND == 13) asm volatile("v_lshlrev_b32 %0, 3, %0" : "+v"(a[j]));
                if (KIND == 14) asm volatile("v_bfe_u32 %0, %0, 8, 8" : "+v"(a[j]));
                if (KIND == 15) asm volatile("v_cmp_lt_u32_e64 %0, %1, %2" : "=s"(m64) : "v"(a[j]), "v"(b));
                if (KIND == 16) asm volatile("v_cmp_lt_u32 vcc, %1, %2\n\tv_cndmask_b32 %0, %0, %2, vcc" : "+v"(a[j]) : "v"(a[(j + 1) & 7]), "v"(b) : "vcc");
                if (KIND == 17) asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(a[j]) : "v"(b), "v"(c));
                if (KIND == 18) asm volatile("v_sub_u32 %0, %0, %1" : "+v"(a[j]) : "v"(b));
                if (KIND == 19) asm volatile("v_add_u32 %0, %1, %2" : "=v"(a[j]) : "v"(b), "v"(c));       // no read of dst
            }
        }
    }
    uint32_t x = 0;
    for (int j = 0; j < 8; j++) x ^= a[j];
    out[blockIdx.x * 64 + threadIdx.x] = x;
}

// 48 instructions of the mix, as four dozens of 7 v_perm_b32 + 5 v_add_u32 over a[0..7]; C0 / C1 are the places of a dozen that may hold a compare
#define MP(J) "v_perm_b32 %" #J ", %" #J ", %[b], %[c]\n\t"
#define MA(J) "v_add_u32 %" #J ", %" #J ", %[b]\n\t"
#define MC(S, J) "v_cmp_lt_u32_e64 %[" S "], %" #J ", %[b]\n\t"
#define DOZEN_A(C0, C1) MP(0) MA(1) MP(2) C0 MP(3) MA(4) MP(5) MA(6) MP(7) MP(0) C1 MA(1) MP(2) MA(3)
#define DOZEN_B(C0, C1) MP(4) MA(5) MP(6) C0 MP(7) MA(0) MP(1) MA(2) MP(3) MP(4) C1 MA(5) MP(6) MA(7)
template <int K>
__global__ void __launch_bounds__(64) kmix(uint32_t* out, int iters, uint32_t s)
{
    uint32_t a[8];
    for (int j = 0; j < 8; j++) a[j] = threadIdx.x * 2654435761u + j;
    const uint32_t b = s ^ threadIdx.x, c = 0x07020500u + (s & 3u);
    uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0, m6 = 0, m7 = 0, acc = 0;
    for (int i = 0; i < iters; i++) {
#define MIX_OPS "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), \
                [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3), [m4] "=&s"(m4), [m5] "=&s"(m5), [m6] "=&s"(m6), [m7] "=&s"(m7) : [b] "v"(b), [c] "v"(c)
        if (K == 0) asm volatile(DOZEN_A("", "") DOZEN_B("", "") DOZEN_A("", "") DOZEN_B("", "") : MIX_OPS);
        if (K == 2) asm volatile(DOZEN_A(MC("m0", 1), "") DOZEN_B("", "") DOZEN_A(MC("m1", 6), "") DOZEN_B("", "") : MIX_OPS);
        if (K == 4) asm volatile(DOZEN_A(MC("m0", 1), "") DOZEN_B(MC("m1", 5), "") DOZEN_A(MC("m2", 6), "") DOZEN_B(MC("m3", 2), "") : MIX_OPS);
        if (K == 8) asm volatile(DOZEN_A(MC("m0", 1), MC("m4", 4)) DOZEN_B(MC("m1", 5), MC("m5", 0)) DOZEN_A(MC("m2", 6), MC("m6", 7)) DOZEN_B(MC("m3", 2), MC("m7", 3)) : MIX_OPS);
#undef MIX_OPS
        acc ^= m0 ^ m1 ^ m2 ^ m3 ^ m4 ^ m5 ^ m6 ^ m7;                // (scalar: the masks are read, as the kernel's are by its scalar logic)
    }
    uint32_t x = (uint32_t)acc ^ (uint32_t)(acc >> 32);
    for (int j = 0; j < 8; j++) x ^= a[j];
    out[blockIdx.x * 64 + threadIdx.x] = x;
}
#undef MP
#undef MA
#undef MC
#undef DOZEN_A
#undef DOZEN_B

// SIMD-cycles per body of 48 + K instructions at w wavefronts per SIMD
template <int K>
double run_mix(uint32_t* d, int cus, int w)
{
    const int iters = 20000, grid = cus * 4 * w;
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    kmix<K><<<grid, 64>>>(d, 100, 1);
    hipEventRecord(a);
    kmix<K><<<grid, 64>>>(d, iters, 1);
    hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    const double cyc = ms * 1e-3 * 2.4e9 / ((double)iters * w);
    printf("mix 28 v_perm + 20 v_add + %d v_cmp_e64 ->sgpr  waves/SIMD %d: %.3f ms  %.2f SIMD-cycles per body of a wavefront, %.2f per instruction (at 2.4 GHz)\n",
           K, w, ms, cyc, cyc / (48 + K));
    return cyc;
}
void run_mixes(uint32_t* d, int cus)
{
    for (int w : { 1, 3 }) {
        const double k[4] = { 0, 2, 4, 8 };
        const double y[4] = { run_mix<0>(d, cus, w), run_mix<2>(d, cus, w), run_mix<4>(d, cus, w), run_mix<8>(d, cus, w) };
        double sk = 0, sy = 0, skk = 0, sky = 0;
        for (int i = 0; i < 4; i++) { sk += k[i]; sy += y[i]; skk += k[i] * k[i]; sky += k[i] * y[i]; }
        const double slope = (4 * sky - sk * sy) / (4 * skk - sk * sk);
        printf("marginal cost of a compare in the mix, waves/SIMD %d: %.2f SIMD-cycles (least-squares slope over k = 0, 2, 4, 8; k = 0 -> 8: %.2f)\n", w, slope, (y[3] - y[0]) / 8);
    }
}

template <int KIND>
void run(const char* name, uint32_t* d, int cus)
{
    const int iters = 20000;
    for (int w : { 1, 3, 4, 8 }) {
        const int grid = cus * 4 * w;
        hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
        k<KIND><<<grid, 64>>>(d, 100, 1);
        hipEventRecord(a);
        k<KIND><<<grid, 64>>>(d, iters, 1);
        hipEventRecord(b); hipEventSynchronize(b);
        float ms; hipEventElapsedTime(&ms, a, b);
        const double cyc = ms * 1e-3 * 2.4e9 / ((double)iters * 32 * w);
        if (KIND >= 20) printf("%-34s waves/SIMD %d: %.3f ms  %.2f SIMD-cycles per moved dword of a wavefront (at 2.4 GHz)\n", name, w, ms, cyc);
        else printf("%-18s waves/SIMD %d: %.3f ms  %.2f SIMD-cycles per wavefront-instruction (at 2.4 GHz)\n", name, w, ms, cyc);
    }
}

int main(int argc, char** argv)
{
    hipDeviceProp_t p; hipGetDeviceProperties(&p, 0);
    const int cus = p.multiProcessorCount;
    printf("%s, %d CUs, clock %d MHz\n", p.gcnArchName, cus, p.clockRate / 1000);
    uint32_t* d; hipMalloc(&d, (size_t)cus * 4 * 8 * 64 * 4);
    if (argc > 1 && argv[1][0] == 'm') { run_mixes(d, cus); return 0; }
    run<0>("v_add_u32", d, cus); run<1>("v_perm_b32", d, cus); run<2>("v_and_or_b32", d, cus); run<3>("v_cndmask_b32", d, cus);
    run<4>("v_alignbyte_b32", d, cus); run<5>("v_lshl_add_u32", d, cus); run<6>("v_mul_lo_u32", d, cus); run<7>("v_cmp_lt_u32", d, cus);
    run<8>("v_lshl_add_u64", d, cus); run<9>("dependent v_add", d, cus);
    run<10>("v_cndmask_e64 sgpr", d, cus); run<11>("v_mov_b32", d, cus); run<12>("v_and_b32", d, cus); run<13>("v_lshlrev_b32", d, cus);
    run<14>("v_bfe_u32", d, cus); run<15>("v_cmp_e64 ->sgpr", d, cus); run<16>("v_cmp+v_cndmask vcc (x2)", d, cus); run<17>("v_add3_u32", d, cus);
    run<18>("v_sub_u32", d, cus); run<19>("v_add_u32 d=b+c", d, cus);
    run<20>("v_mov under EXEC, 1 per region", d, cus); run<21>("v_mov under EXEC, 4 per region", d, cus); run<22>("v_mov under EXEC, 8 per region", d, cus);
    run<23>("v_pk_mov_b32 [0,1]", d, cus); run<24>("v_pk_mov_b32 [0,1] under EXEC, 4", d, cus);
    run<25>("v_pk_mov_b32 [1,0] (dword shift)", d, cus); run<26>("v_pk_mov_b32 [1,0] under EXEC, 4", d, cus);
    run_mixes(d, cus);
    return 0;
}
