// dict_encode_asan_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over the emulator translation unit of the encode of block
// batches against a shared dictionary (tests/simt/emu_dict_encode.cpp), for a sanitizer run of the two kernels and the host-pointer call's
// upload, priming and slice loop on the CPU:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Itests/simt -Ilz4net_amd/csrc -Itools/ab \
//         tests/cpp/dict_encode_asan_main.cpp -o dict_encode_asan && ./dict_encode_asan
//
// The new thing in this path is an encoder that reads TWO buffers as one, and must read nothing else of either: not the dictionary before
// its reachable bytes or behind its last, not the block before its first byte or behind its last -- and writes nothing at or past dst_cap.
// So the dictionary's reachable bytes, every block, every output of exactly dst_cap bytes and the table are heap allocations of exactly
// their sizes -- both of their ends are the sanitizer's; the pointer a call gets for a dictionary of more than 65 535 bytes is where
// the whole of it would begin, in front of the allocation -- and the blocks are the shapes of tests/dict_encode_cases.py built by hand: a
// candidate inside the dictionary, counts that cross into the block in the first and in a later round with the straddling dword in lane
// 0, 31 and 63, the dictionary's last 5, 8 and 300 bytes repeated, a catch-up back into the dictionary, the tail of a 1- and a 3-byte
// dictionary in front of the block's start, blocks of 0, 1, 12 and 13 bytes, and dst_cap at the result and one below it, with
// dictionaries of 1, 3, 17, 4 097, 65 535 and 70 000 bytes, with 1 and 5 wavefronts per workgroup.  Every output that fits is decoded
// back by a byte-by-byte decoder with a prefix, written here, and compared with its block.
#include "../simt/emu_dict_encode.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {

typedef std::vector<uint8_t> Bytes;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

Bytes noise(size_t n, uint32_t seed, unsigned lo, unsigned span)
{
    Bytes b(n);
    uint32_t x = seed * 2654435761u + 1u;
    for (size_t i = 0; i < n; i++) { x = x * 1664525u + 1013904223u; b[i] = (uint8_t)(lo + (x >> 24) % span); }
    return b;
}
void append(Bytes& b, const Bytes& a, size_t from = 0, size_t n = (size_t)-1)
{
    if (n == (size_t)-1) n = a.size() - from;
    b.insert(b.end(), a.begin() + (ptrdiff_t)from, a.begin() + (ptrdiff_t)(from + n));
}

// the block format, byte by byte, behind `prefix`: the bytes produced, or nothing if the block is not one
bool decode(const uint8_t* in, size_t n, const Bytes& prefix, size_t want, Bytes& out)
{
    Bytes v = prefix;
    size_t ip = 0;
    for (;;) {
        if (ip >= n) return false;
        const unsigned token = in[ip++];
        size_t ll = token >> 4;
        if (ll == 15) { unsigned b; do { if (ip >= n) return false; b = in[ip++]; ll += b; } while (b == 255); }
        if (ip + ll > n) return false;
        v.insert(v.end(), in + ip, in + ip + ll);
        ip += ll;
        if (ip == n) break;
        if (ip + 2 > n) return false;
        const size_t off = in[ip] | (size_t)in[ip + 1] << 8;
        ip += 2;
        size_t ml = token & 15;
        if (ml == 15) { unsigned b; do { if (ip >= n) return false; b = in[ip++]; ml += b; } while (b == 255); }
        ml += 4;
        if (off == 0 || off > v.size()) return false;
        for (size_t i = 0; i < ml; i++) v.push_back(v[v.size() - off]);
    }
    out.assign(v.begin() + (ptrdiff_t)prefix.size(), v.end());
    return out.size() == want;
}

int bound(size_t n) { return (int)(n + n / 255 + 16); }

// the dictionary: only its reachable bytes exist; `ptr` is where the whole of it would begin
struct Dict {
    size_t len, reach;
    std::unique_ptr<uint8_t[]> store;
    Bytes tail;
    const uint8_t* ptr;
    Dict(size_t n, uint32_t seed) : len(n), reach(n < 65535 ? n : 65535), store(new uint8_t[reach ? reach : 1])
    {
        tail = noise(reach, seed, 1, 160);
        memcpy(store.get(), tail.data(), reach);
        ptr = (const uint8_t*)((uintptr_t)store.get() - (len - reach));
    }
};

// one call over the blocks, each in allocations of exactly its size and its dst_cap; the results
std::vector<int> run(const Dict& d, const std::vector<Bytes>& blocks, const std::vector<int>& caps, unsigned wpg, std::vector<Bytes>& outs)
{
    const size_t n = blocks.size();
    std::vector<std::unique_ptr<uint8_t[]>> src(n), dst(n);
    std::vector<int64_t> so(n), dof(n);
    std::vector<int32_t> sl(n), cp(n), res(n, -12345678);
    for (size_t i = 0; i < n; i++) {
        src[i].reset(new uint8_t[blocks[i].size()]);
        if (!blocks[i].empty()) memcpy(src[i].get(), blocks[i].data(), blocks[i].size());
        dst[i].reset(new uint8_t[(size_t)caps[i]]);
        memset(dst[i].get(), 0x5C, (size_t)caps[i]);
        so[i] = (int64_t)((intptr_t)src[i].get() - (intptr_t)src[0].get());
        dof[i] = (int64_t)((intptr_t)dst[i].get() - (intptr_t)dst[0].get());
        sl[i] = (int32_t)blocks[i].size(); cp[i] = caps[i];
    }
    std::unique_ptr<lz4hip::Aligned16[]> table(new lz4hip::Aligned16[lz4hip::kFastTableBytes / 16]);
    emu_encdict_encode(src[0].get(), so.data(), 0, sl.data(), dst[0].get(), dof.data(), 0, cp.data(), res.data(), (int64_t)n, (int)wpg, d.ptr, (int64_t)d.len,
                       (uint8_t*)table.get());
    outs.assign(n, Bytes());
    for (size_t i = 0; i < n; i++) if (res[i] > 0) outs[i].assign(dst[i].get(), dst[i].get() + res[i]);
    return std::vector<int>(res.begin(), res.end());
}

std::vector<Bytes> shapes(const Dict& d)
{
    const Bytes& t = d.tail;
    const size_t T = t.size();
    std::vector<Bytes> b;
    for (size_t n : { 0, 1, 12, 13, 100 }) b.push_back(noise(n, 7 + (uint32_t)n, 0xA6, 90));
    if (T >= 40) { Bytes x = noise(20, 1, 0xA6, 90); append(x, t, T - 30, 12); append(x, noise(20, 2, 0xA6, 90)); b.push_back(x); }      // a candidate in the dictionary
    for (size_t k : { 6, 130, 258, 262, 386, 514 })                                                                              // the count crosses T
        if (k <= T) { Bytes a = noise(24, 3 + (uint32_t)k, 0xA6, 40), x = a; append(x, t, T - k); append(x, a); append(x, noise(20, 4, 0xD0, 40)); b.push_back(x); }
    for (size_t m : { 5, 8, 300 })                                                                                                // the last m bytes repeated
        if (m <= T) { Bytes x; while (x.size() < 2000) append(x, t, T - m); x.resize(2000); b.push_back(x); }
    {   // the catch-up goes back into the dictionary / the tail of a short dictionary in front of the block's start again
        const size_t j = T < 3 ? T : 3;
        Bytes c = noise(12, 5, 0xA6, 40), x = c;
        append(x, noise(10, 6, 0xD0, 20)); append(x, t, T - j); append(x, c); append(x, noise(20, 8, 0xE8, 20));
        b.push_back(x);
    }
    if (T >= 64) {                                                                                                                // phrases of the dictionary
        Bytes x;
        for (uint32_t i = 0; x.size() < 3000; i++) { append(x, t, (i * 7919u) % (T - 40), 6 + i % 30); append(x, noise(i % 9, i, 0xA6, 90)); }
        b.push_back(x);
    }
    return b;
}

}  // namespace

int main()
{
    size_t checked = 0;
    for (size_t dict_len : { 1, 3, 17, 4097, 65535, 70000 }) {
        const Dict d(dict_len, (uint32_t)dict_len);
        const std::vector<Bytes> blocks = shapes(d);
        std::vector<int> caps;
        for (const Bytes& b : blocks) caps.push_back(bound(b.size()));
        for (unsigned wpg : { 1u, 5u }) {
            std::vector<Bytes> outs, tight, short_outs;
            const std::vector<int> res = run(d, blocks, caps, wpg, outs);
            for (size_t i = 0; i < blocks.size(); i++) {
                Bytes back;
                CHECK(res[i] > 0 && decode(outs[i].data(), outs[i].size(), d.tail, blocks[i].size(), back) && back == blocks[i]);
                checked++;
            }
            // dst_cap at exactly the result, and one below it: the same bytes, and 0 with nothing written at or past dst_cap
            std::vector<int> below(res);
            for (int& c : below) c -= 1;
            CHECK(run(d, blocks, res, wpg, tight) == res && tight == outs);
            const std::vector<int> r0 = run(d, blocks, below, wpg, short_outs);
            for (int r : r0) CHECK(r == 0);
        }
        // the host-pointer call over EmuStage: rows at a stride, two slices
        size_t widest = 0;
        for (const Bytes& b : blocks) widest = b.size() > widest ? b.size() : widest;
        const size_t n = blocks.size(), ss = widest + 16, ds = (size_t)bound(widest) + 16;
        std::unique_ptr<uint8_t[]> src(new uint8_t[n * ss]()), dst(new uint8_t[n * ds]());
        std::vector<int32_t> sl(n), res(n, -1);
        for (size_t i = 0; i < n; i++) { if (!blocks[i].empty()) memcpy(src.get() + i * ss, blocks[i].data(), blocks[i].size()); sl[i] = (int32_t)blocks[i].size(); }
        lz4hip_batch_t hb = {};
        hb.src = src.get(); hb.src_stride = (int64_t)ss; hb.src_len = sl.data(); hb.dst = dst.get(); hb.dst_stride = (int64_t)ds; hb.dst_cap = caps.data();
        hb.result = res.data(); hb.n_blocks = (int64_t)n;
        EmuHostBatch r = {};
        r.fail_at = -1; r.slices_knob = 2; r.dst_len_is_result = 1; r.slice_floor = 0; r.slice_ceiling = r.hinted_ceiling = r.pool_floor = -1;
        EmuEncDictHost h = {};
        std::unique_ptr<uint8_t[]> whole(new uint8_t[dict_len]);
        memset(whole.get(), 0xEE, dict_len);
        memcpy(whole.get() + (dict_len - d.reach), d.tail.data(), d.reach);
        CHECK(emu_encdict_host(&hb, whole.get(), (int64_t)dict_len, 5, &r, &h) == 0);
        CHECK(r.violations == 0 && r.intact == 1 && h.intact == 1 && h.table_unchanged == 1 && h.uploads == 1 && h.primes == 1 && h.bytes == (int64_t)d.reach);
        for (size_t i = 0; i < n; i++) {
            Bytes back;
            CHECK(res[i] > 0 && decode(dst.get() + i * ds, (size_t)res[i], d.tail, blocks[i].size(), back) && back == blocks[i]);
        }
    }
    printf("dict_encode_asan: %zu blocks round-tripped, tight and short capacities and the host call checked\n", checked);
    return 0;
}
