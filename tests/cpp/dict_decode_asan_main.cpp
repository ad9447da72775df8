// dict_decode_asan_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over the emulator translation unit of the decode of block
// batches against a shared dictionary (tests/simt/emu_dict.cpp), for a sanitizer run of the kernels, the sizes walk and the host-pointer
// call's upload and slice loop on the CPU:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Itests/simt -Ilz4net_amd/csrc -Itools/ab \
//         tests/cpp/dict_decode_asan_main.cpp -o dict_decode_asan && ./dict_decode_asan
//
// The new thing in this path is a decoder that reads ANOTHER buffer for the bytes before a block, and must read nothing else there: not
// dst below its first byte, not the dictionary before its first byte or behind its last.  So the dictionary, every source row and every
// output row is a heap allocation of exactly its size -- both of its ends are the sanitizer's -- and the blocks are the shapes of
// tests/dict_cases.py built by hand: the furthest reach and one byte more (refused, not read), matches that begin in the dictionary and
// end in the block with overlapping periods, sources on both sides of the mirror's edges, a run of short sequences out of the dictionary,
// long copies, a dictionary source after a long copy, with dictionaries of 1, 17, 4 095, 4 096, 4 097 and 70 000 bytes, with 1 and 4
// wavefronts per workgroup, known and unknown size.  Expected bytes come from a byte-by-byte decoder with a prefix, written here.
#include "../simt/emu_dict.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {

typedef std::vector<uint8_t> Bytes;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

Bytes noise(size_t n, uint32_t seed)
{
    Bytes b(n);
    uint32_t x = seed * 2654435761u + 1u;
    for (size_t i = 0; i < n; i++) { x = x * 1664525u + 1013904223u; b[i] = (uint8_t)(1 + (x >> 24) % 160); }
    return b;
}

void append(Bytes& b, const Bytes& a) { b.insert(b.end(), a.begin(), a.end()); }
void put_length(Bytes& b, size_t n) { for (; n >= 255; n -= 255) b.push_back(255); b.push_back((uint8_t)n); }

// token, literal length bytes, literals [, offset, match length bytes]; match == 0: a block's last sequence
void sequence(Bytes& b, const Bytes& literals, unsigned offset, size_t match)
{
    const size_t ll = literals.size(), ml = match ? match - 4 : 0;
    b.push_back((uint8_t)((ll < 15 ? ll : 15) << 4 | (ml < 15 ? ml : 15)));
    if (ll >= 15) put_length(b, ll - 15);
    append(b, literals);
    if (match) {
        b.push_back((uint8_t)offset); b.push_back((uint8_t)(offset >> 8));
        if (ml >= 15) put_length(b, ml - 15);
    }
}

struct Part { Bytes literals; unsigned offset; size_t match; };

// a block of the parts and the last literals, what it decodes to behind `dict` (valid == false: a source lies before the dictionary)
struct Block {
    Bytes data, out;
    bool valid = true;
    size_t dict_len = 0;
    Block(const std::vector<Part>& parts, const Bytes& tail, const Bytes& dict) : dict_len(dict.size())
    {
        Bytes all(dict.size() > 65535 ? dict.end() - 65535 : dict.begin(), dict.end());
        const size_t before = all.size();
        for (const Part& p : parts) sequence(data, p.literals, p.offset, p.match);
        for (const Part& p : parts) {
            append(all, p.literals);
            if (p.offset > all.size()) { valid = false; break; }
            for (size_t k = 0; k < p.match; k++) all.push_back(all[all.size() - p.offset]);
        }
        sequence(data, tail, 0, 0);
        append(all, tail);
        out.assign(all.begin() + before, all.end());
        cap = 0;
        for (const Part& p : parts) cap += p.literals.size() + p.match;
        cap += tail.size();
    }
    size_t cap;
};

// an allocation of exactly n bytes (at least 1 for malloc's sake, then the row starts at its last byte's successor minus n)
struct Exact {
    uint8_t* p; size_t n;
    explicit Exact(size_t bytes, int fill = 0xA5) : p((uint8_t*)malloc(bytes ? bytes : 1)), n(bytes) { CHECK(p); memset(p, fill, bytes ? bytes : 1); }
    Exact(const Bytes& b) : Exact(b.size()) { if (!b.empty()) memcpy(p, b.data(), b.size()); }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

void run_group(const Bytes& dict, const std::vector<Block>& blocks)
{
    const int64_t n = (int64_t)blocks.size();
    Exact d(dict);
    for (int known = 0; known < 2; known++)
        for (int wpg = 1; wpg <= 4; wpg += 3) {
            std::vector<std::unique_ptr<Exact>> src, dst;
            std::vector<int64_t> so, dof;
            std::vector<int32_t> sl, cp, res((size_t)n, -12345678);
            for (const Block& b : blocks) {
                src.emplace_back(new Exact(b.data));
                dst.emplace_back(new Exact(b.cap + (known ? 0 : 5)));
                so.push_back(src.back()->p - src[0]->p); dof.push_back(dst.back()->p - dst[0]->p);
                sl.push_back((int32_t)b.data.size()); cp.push_back((int32_t)dst.back()->n);
            }
            emu_dict_decode_at(known, src[0]->p, so.data(), sl.data(), dst[0]->p, dof.data(), cp.data(), res.data(), n, wpg, dict.empty() ? nullptr : d.p, (int64_t)dict.size());
            for (int64_t i = 0; i < n; i++) {
                const Block& b = blocks[(size_t)i];
                if (!b.valid) { CHECK(res[(size_t)i] < 0); continue; }
                CHECK(res[(size_t)i] == (known ? (int32_t)b.data.size() : (int32_t)b.cap));
                CHECK(memcmp(dst[(size_t)i]->p, b.out.data(), b.cap) == 0);
                for (size_t k = b.cap; k < dst[(size_t)i]->n; k++) CHECK(dst[(size_t)i]->p[k] == 0xA5);
            }
        }
    // the sizes walk with the dictionary's length
    {
        std::vector<int64_t> so;
        std::vector<int32_t> sl, res((size_t)n, -7), caps((size_t)n, -7);
        std::vector<int64_t> offs((size_t)n + 1, -7);
        Bytes packed;
        for (const Block& b : blocks) { so.push_back((int64_t)packed.size()); sl.push_back((int32_t)b.data.size()); append(packed, b.data); }
        Exact rows(packed);
        lz4hip_batch_t hb = {};
        hb.src = rows.p; hb.src_off = so.data(); hb.src_len = sl.data(); hb.result = res.data(); hb.n_blocks = n;
        const int64_t need = emu_dict_sizes_scratch_bytes(n);
        Exact scratch((size_t)need, 0);
        lz4hip_sizes_info_t info;
        char error[160];
        CHECK(emu_dict_sizes(&hb, (int64_t)dict.size(), offs.data(), caps.data(), scratch.p, need, &info, 0, error) == 0);
        for (int64_t i = 0; i < n; i++) {
            if (blocks[(size_t)i].valid) CHECK(res[(size_t)i] == (int32_t)blocks[(size_t)i].cap);
            else CHECK(res[(size_t)i] < 0);
        }
        CHECK(info.blocks == n);
    }
    // the host-pointer call: strided rows in exactly sized buffers, two slices
    for (int known = 0; known < 2; known++) {
        size_t max_src = 1, max_dst = 1;
        for (const Block& b : blocks) { max_src = std::max(max_src, b.data.size()); max_dst = std::max(max_dst, b.cap + 5); }
        Exact src(max_src * (size_t)n, 0), dst(max_dst * (size_t)n);
        std::vector<int32_t> sl, cp, res((size_t)n, -12345678);
        for (int64_t i = 0; i < n; i++) {
            const Block& b = blocks[(size_t)i];
            memcpy(src.p + max_src * (size_t)i, b.data.data(), b.data.size());
            sl.push_back((int32_t)b.data.size()); cp.push_back((int32_t)(b.cap + (known ? 0 : 5)));
        }
        lz4hip_batch_t hb = {};
        hb.src = src.p; hb.src_stride = (int64_t)max_src; hb.src_len = sl.data(); hb.dst = dst.p; hb.dst_stride = (int64_t)max_dst; hb.dst_cap = cp.data();
        hb.result = res.data(); hb.n_blocks = n;
        EmuHostBatch r = {};
        r.fail_at = -1; r.slices_knob = 2; r.slice_floor = 0; r.slice_ceiling = r.hinted_ceiling = r.pool_floor = -1;
        EmuDictHost dh;
        CHECK(emu_dict_host(&hb, dict.empty() ? nullptr : d.p, (int64_t)dict.size(), known, 4, &r, &dh) == 0);
        CHECK(r.violations == 0 && r.intact == 1 && dh.intact == 1 && dh.uploads == (dict.empty() ? 0 : 1));
        CHECK(dh.bytes == (int64_t)std::min<size_t>(dict.size(), 65535) && dh.log_at_upload == 0 && dh.kernels_at_upload == 0);
        for (int64_t i = 0; i < n; i++) {
            const Block& b = blocks[(size_t)i];
            if (!b.valid) { CHECK(res[(size_t)i] < 0); continue; }
            CHECK(res[(size_t)i] == (known ? (int32_t)b.data.size() : (int32_t)b.cap));
            CHECK(memcmp(dst.p + max_dst * (size_t)i, b.out.data(), b.cap) == 0);
        }
    }
}

}  // namespace

int main()
{
    const Bytes tail = noise(12, 99), tail40 = noise(40, 98), tail120 = noise(120, 97);
    const size_t lens[] = { 0, 1, 17, 4095, 4096, 4097, 70000 };
    int groups = 0, total = 0;
    for (size_t L : lens) {
        const Bytes dict = noise(L, 7 + (uint32_t)L);
        const unsigned r = (unsigned)std::min<size_t>(L, 65535);
        std::vector<Block> blocks;
        blocks.emplace_back(std::vector<Part>{ { noise(20, 1), 7, 30 }, { {}, 1, 100 } }, tail, dict);                            // the block's own bytes only
        if (r > 0) blocks.emplace_back(std::vector<Part>{ { {}, r, 8 } }, tail, dict);                                            // the furthest reach
        if (r < 65535) blocks.emplace_back(std::vector<Part>{ { {}, r + 1, 8 } }, tail, dict);                                    // one byte more: refused
        if (r + 18u <= 65535u) blocks.emplace_back(std::vector<Part>{ { noise(9, 2), 4, 6 }, { noise(2, 3), 17 + r + 1, 5 } }, tail, dict);
        for (unsigned off = 1; off <= 17 && off <= r; off += 4) {                                                                // periods through dictionary, literals, match
            blocks.emplace_back(std::vector<Part>{ { {}, off, 40 } }, tail, dict);
            blocks.emplace_back(std::vector<Part>{ { {}, off, 300 } }, tail, dict);
            if (off + 3 <= r) blocks.emplace_back(std::vector<Part>{ { noise(3, 4), off + 3, 300 } }, tail, dict);
        }
        if (r >= 30) for (size_t t : { 63, 64, 65 }) blocks.emplace_back(std::vector<Part>{ { noise(10, 5), 30, t - 10 } }, tail, dict);
        if (r >= 2000) {
            blocks.emplace_back(std::vector<Part>{ { noise(5, 6), 2005, 3000 } }, tail, dict);                                   // the long path, 2 000 bytes in the dictionary
            std::vector<Part> run;                                                                                              // a run of short sequences out of the dictionary
            for (unsigned j = 0; j < 24; j++) run.push_back({ noise(2, 10 + j), 8 * j + 2 + 100 + 7 * j, 6 });
            blocks.emplace_back(run, tail120, dict);
            blocks.emplace_back(std::vector<Part>{ { noise(4, 8), 4, 200 }, { {}, 204 + 200, 8 } }, tail40, dict);               // after a long copy: from memory
        }
        for (unsigned dlt : { 4095u, 4096u, 4097u })
            for (unsigned op : { 0u, 1u, 20u, 64u })
                if (dlt <= r) {
                    blocks.emplace_back(std::vector<Part>{ { noise(op, 9), op + dlt, 8 } }, tail, dict);
                    blocks.emplace_back(std::vector<Part>{ { noise(op, 9), op + dlt, 8 } }, tail40, dict);
                }
        if (r >= 4077) for (unsigned off : { 4076u, 4077u }) blocks.emplace_back(std::vector<Part>{ { {}, off, 8 } }, tail40, dict);
        if (r >= 60000) blocks.emplace_back(std::vector<Part>{ { noise(70, 11), 70 + 60000, 70 } }, tail, dict);
        run_group(dict, blocks);
        groups++; total += (int)blocks.size();
    }
    printf("dict_decode_asan: %d dictionaries, %d blocks, known and unknown size, 1 and 4 wavefronts, sizes walk, host call: ok\n", groups, total);
    return 0;
}
