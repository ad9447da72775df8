// lz4f_dict_encode_asan_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over the emulator unit of the frame encode with a
// dictionary (tests/simt/emu_lz4f_dict_encode.cpp): a sanitizer run of the kernels, the launch sequences and the fronts on the CPU:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Itests/simt -Ilz4net_amd/csrc \
//         tests/cpp/lz4f_dict_encode_asan_main.cpp -o lz4f_dict_encode_asan && ./lz4f_dict_encode_asan
//
// (tests/test_lz4f_dict_encode_asan.py builds and runs it).  What is new in this path: an encoder that reads a dictionary which ends
// somewhere else than the block begins, a primed table and a descriptor of three words in the caller's scratch, and a pack that copies
// 11 or 19 descriptor bytes.  So every buffer is a heap block of EXACTLY the size the queries give -- the source, the frame at its
// bound, the scratch -- and the dictionary lies at an odd address in a block of exactly its size + 1: dictionaries of 13 and 65 535
// bytes, sources of 0, 13 and 65 537 bytes, the one-frame and the batch sequence, device and host form, one and five blocks a
// workgroup.  Every frame is read back by the serial reader below, which knows nothing of the kernels.
#include "../simt/emu_lz4f_dict_encode.cpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

namespace {

typedef std::vector<uint8_t> Bytes;

Bytes text(size_t n, uint32_t seed)
{
    Bytes b(n);
    uint32_t x = seed * 2654435761u + 1u;
    for (size_t i = 0; i < n; i++) { x = x * 1664525u + 1013904223u; b[i] = (uint8_t)('a' + (x >> 24) % 6); }
    return b;
}

// pieces of the dictionary's end, and short runs of other bytes
Bytes source(size_t n, const Bytes& dict, uint32_t seed)
{
    Bytes b;
    uint32_t x = seed;
    while (b.size() < n) {
        x = x * 1664525u + 1013904223u;
        const size_t k = 4 + (x >> 8) % 120, at = (x >> 16) % dict.size();
        if ((x >> 28) < 12) for (size_t i = 0; i < k && at + i < dict.size(); i++) b.push_back(dict[at + i]);
        else for (size_t i = 0; i < k % 9 + 1; i++) b.push_back((uint8_t)(x >> (i % 4 * 8)));
    }
    b.resize(n);
    return b;
}

uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// one block against `history` (the dictionary: independent blocks), appended to out
void decode_block(const uint8_t* p, size_t n, const Bytes& history, Bytes& out)
{
    Bytes w = history;
    const size_t base = w.size();
    size_t i = 0;
    while (true) {
        CHECK(i < n);
        const unsigned token = p[i++];
        size_t ll = token >> 4;
        if (ll == 15) { unsigned b; do { CHECK(i < n); b = p[i++]; ll += b; } while (b == 255); }
        CHECK(i + ll <= n);
        w.insert(w.end(), p + i, p + i + ll);
        i += ll;
        if (i == n) break;
        CHECK(i + 2 <= n);
        const size_t offset = p[i] | (size_t)p[i + 1] << 8;
        i += 2;
        size_t ml = token & 15;
        if (ml == 15) { unsigned b; do { CHECK(i < n); b = p[i++]; ml += b; } while (b == 255); }
        ml += 4;
        CHECK(offset >= 1 && offset <= w.size() && offset <= 65535);
        for (size_t k = 0; k < ml; k++) w.push_back(w[w.size() - offset]);
    }
    out.insert(out.end(), w.begin() + (long)base, w.end());
}

// the frame at f[0, n): its descriptor as asked for, every block against the dictionary's reachable tail -> the content
Bytes read_frame(const uint8_t* f, size_t n, const Bytes& dict, uint32_t dict_id, unsigned flags, size_t content)
{
    CHECK(n >= 7 && le32(f) == kLz4fMagic);
    const unsigned flg = f[4];
    const bool sized = (flags & kLz4fContentSize) && content > 0;
    CHECK(flg == (0x60u | (dict_id ? 1u : 0u) | (sized ? 8u : 0u) | ((flags & kLz4fBlockChecksum) ? 0x10u : 0u) | ((flags & kLz4fContentChecksum) ? 4u : 0u)));
    CHECK(f[5] == 0x40);
    size_t at = 6;
    if (sized) { CHECK(le32(f + at) == (uint32_t)content && le32(f + at + 4) == 0); at += 8; }
    if (dict_id) { CHECK(le32(f + at) == dict_id); at += 4; }
    CHECK(f[at] == ((xxh32_serial(f + 4, (int64_t)at - 4, 0) >> 8) & 0xFF));
    at++;
    const Bytes tail(dict.end() - (long)(dict.size() < 65535 ? dict.size() : 65535), dict.end());
    Bytes out;
    while (true) {
        CHECK(at + 4 <= n);
        const uint32_t field = le32(f + at);
        at += 4;
        if (field == 0) break;
        const size_t size = field & ~kLz4fRawBit;
        CHECK(size <= 65536 && at + size <= n);
        if (field & kLz4fRawBit) out.insert(out.end(), f + at, f + at + size);
        else decode_block(f + at, size, tail, out);
        if (flags & kLz4fBlockChecksum) { CHECK(le32(f + at + size) == xxh32_serial(f + at, (int64_t)size, 0)); at += 4; }
        at += size;
    }
    if (flags & kLz4fContentChecksum) { CHECK(at + 4 <= n && le32(f + at) == xxh32_serial(out.data(), (int64_t)out.size(), 0)); at += 4; }
    CHECK(at == n);
    return out;
}

struct Placed {
    Bytes store;
    explicit Placed(const Bytes& d) : store(1, 0xEE) { store.insert(store.end(), d.begin(), d.end()); }
    const uint8_t* ptr() const { return store.data() + 1; }
};

void one_frame(const Bytes& src, const Bytes& dict, uint32_t dict_id, unsigned flags, bool host, int wpg)
{
    const Placed pd(dict);
    const int64_t bound = emu_lz4f_dict_bound((int64_t)src.size(), 4, flags, (int64_t)dict.size(), dict_id);
    CHECK(bound > 0);
    Bytes dst((size_t)bound, 0xA7);
    int64_t* len = new int64_t(-1);
    Lz4fDictEncEmuRun run = {};
    run.waves_per_group = wpg;
    // (a source of no bytes: a heap block of no bytes)
    uint8_t* s = new uint8_t[src.size()];
    if (!src.empty()) memcpy(s, src.data(), src.size());
    if (host) {
        CHECK(emu_lz4f_encode_dict_host(s, (int64_t)src.size(), pd.ptr(), (int64_t)dict.size(), dict_id, 4, flags, dst.data(), bound, len, &run) == 0);
        CHECK(run.dict_uploads == 1 && run.dict_bytes == (int64_t)dict.size() && run.dict_intact == 1 && run.counters.intact == 1);
    } else {
        const int64_t need = emu_lz4f_encode_dict_scratch_bytes((int64_t)src.size(), 4, (int64_t)dict.size());
        CHECK(need > 0);
        uint8_t* scratch = (uint8_t*)aligned_alloc(256, (size_t)need);           // (need is a multiple of 256: exactly the queried bytes)
        CHECK(need % 256 == 0 && scratch);
        CHECK(emu_lz4f_encode_dict(s, (int64_t)src.size(), pd.ptr(), (int64_t)dict.size(), dict_id, 4, flags, dst.data(), bound, len, scratch, need, &run) == 0);
        free(scratch);
    }
    CHECK(run.primes == (src.empty() ? 0 : 1) && run.dict_calls == run.primes && run.plain_calls == 0);
    CHECK(*len > 0 && *len <= bound);
    for (int64_t k = *len; k < bound; k++) CHECK(dst[(size_t)k] == 0xA7);
    CHECK(read_frame(dst.data(), (size_t)*len, dict, dict_id, flags, src.size()) == src);
    delete[] s;
    delete len;
}

void batch(const std::vector<Bytes>& items, const Bytes& dict, uint32_t dict_id, unsigned flags, bool host, int wpg)
{
    const Placed pd(dict);
    Bytes src;
    std::vector<int64_t> off(1, 0);
    for (const Bytes& i : items) { src.insert(src.end(), i.begin(), i.end()); off.push_back((int64_t)src.size()); }
    const int64_t n = (int64_t)items.size();
    const int64_t bound = emu_lz4f_batch_dict_bound(n, (int64_t)src.size(), 4, flags, (int64_t)dict.size(), dict_id);
    CHECK(bound > 0);
    Bytes dst((size_t)bound, 0xA7);
    std::vector<int64_t> dst_off((size_t)n + 1, -1);
    Lz4fDictEncEmuRun run = {};
    run.waves_per_group = wpg;
    if (host) {
        CHECK(emu_lz4f_batch_encode_dict_host(src.data(), (int64_t)src.size(), off.data(), n, pd.ptr(), (int64_t)dict.size(), dict_id, 4, flags, dst.data(), bound,
                                              dst_off.data(), &run) == 0);
        CHECK(run.dict_uploads == 1 && run.dict_bytes == (int64_t)dict.size() && run.dict_intact == 1 && run.counters.intact == 1);
    } else {
        const int64_t need = emu_lz4f_batch_encode_dict_scratch_bytes(n, (int64_t)src.size(), 4, (int64_t)dict.size());
        CHECK(need > 0 && need % 256 == 0);
        uint8_t* scratch = (uint8_t*)aligned_alloc(256, (size_t)need);
        CHECK(scratch);
        CHECK(emu_lz4f_batch_encode_dict(src.data(), (int64_t)src.size(), off.data(), n, pd.ptr(), (int64_t)dict.size(), dict_id, 4, flags, dst.data(), bound,
                                         dst_off.data(), scratch, need, &run) == 0);
        free(scratch);
    }
    CHECK(run.primes == 1 && run.dict_calls == 1 && run.plain_calls == 0 && dst_off[0] == 0 && dst_off[(size_t)n] <= bound);
    for (int64_t k = dst_off[(size_t)n]; k < bound; k++) CHECK(dst[(size_t)k] == 0xA7);
    for (size_t i = 0; i < items.size(); i++)
        CHECK(read_frame(dst.data() + dst_off[i], (size_t)(dst_off[i + 1] - dst_off[i]), dict, dict_id, flags, items[i].size()) == items[i]);
}

}  // namespace

int main()
{
    int cases = 0;
    for (size_t dict_len : { (size_t)13, (size_t)65535 }) {
        const Bytes dict = text(dict_len, (uint32_t)dict_len);
        std::vector<Bytes> items;
        for (size_t n : { (size_t)0, (size_t)13, (size_t)65537 }) {
            const Bytes src = source(n, dict, (uint32_t)(n + dict_len));
            items.push_back(src);
            for (int host = 0; host < 2; host++) {
                one_frame(src, dict, host ? 7u : 0xFFFFFFFFu, host ? 7u : 4u, host != 0, host ? 5 : 1);
                cases++;
            }
            if (n > 13) continue;
            one_frame(src, dict, 0, 0, false, 5);
            cases++;
        }
        for (int host = 0; host < 2; host++) {
            batch(items, dict, 7, host ? 3u : 7u, host != 0, host ? 1 : 5);
            cases++;
        }
    }
    printf("lz4f dict encode asan: %d cases ok\n", cases);
    return 0;
}
