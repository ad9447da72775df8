// built_frames.hpp -- TEST INFRASTRUCTURE ONLY: what the stand-alone sanitizer programs over the framing emulator unit share
// (lz4f_batch_asan_main.cpp, lz4f_linked_asan_main.cpp, lz4f_dict_asan_main.cpp): LZ4 blocks and frames built by hand, sequence by
// sequence, as tests/lz4f_built.py builds them, and the record of a decoded batch.  Included behind
// ../simt/emu_framing.cpp, whose names (the frame format's constants, xxh32_serial, the C interface's records) it uses.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

namespace built_frames {

typedef std::vector<uint8_t> Bytes;

inline Bytes noise(size_t n, uint32_t seed)
{
    Bytes b(n);
    uint32_t x = seed * 2654435761u + 1u;
    for (size_t i = 0; i < n; i++) { x = x * 1664525u + 1013904223u; b[i] = (uint8_t)(x >> 24); }
    return b;
}

inline void put32(Bytes& b, uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); }
inline void append(Bytes& b, const Bytes& a) { b.insert(b.end(), a.begin(), a.end()); }
inline void put_length(Bytes& b, size_t n) { for (; n >= 255; n -= 255) b.push_back(255); b.push_back((uint8_t)n); }

// token, literal length bytes, literals [, offset, match length bytes]; match == 0: a block's last sequence
inline void sequence(Bytes& b, const Bytes& literals, unsigned offset, size_t match)
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

struct Block { Bytes data; bool raw; };
struct Part { Bytes literals; unsigned offset; size_t match; };

const Bytes kTail = { 100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111 };

// the frame under construction and the bytes it decodes to: a block may copy from the dictionary and, in a linked frame, from the
// frame's bytes so far
struct Content {
    Bytes dict, out;
    bool linked;
    Block raw(const Bytes& data) { append(out, data); return { data, true }; }
    Block block(const std::vector<Part>& parts, const Bytes& tail)
    {
        Block b = { Bytes(), false };
        Bytes window = dict;
        if (linked) append(window, out);
        const size_t base = window.size();
        for (const Part& p : parts) {
            sequence(b.data, p.literals, p.offset, p.match);
            append(window, p.literals);
            CHECK(p.offset >= 1 && p.offset <= window.size() && p.offset <= 65535);
            for (size_t k = 0; k < p.match; k++) window.push_back(window[window.size() - p.offset]);
        }
        CHECK(tail.size() >= 12);
        sequence(b.data, tail, 0, 0);
        append(window, tail);
        out.insert(out.end(), window.begin() + (long)base, window.end());
        return b;
    }
};

// dict_id == 0: a frame without a dictionary ID
inline Bytes frame_of(const std::vector<Block>& blocks, bool linked, uint32_t dict_id = 0)
{
    Bytes f;
    put32(f, kLz4fMagic);
    f.push_back((uint8_t)(0x40 | (linked ? 0 : 0x20) | (dict_id ? 0x01 : 0)));
    f.push_back(0x40);
    if (dict_id) put32(f, dict_id);
    f.push_back((uint8_t)(xxh32_serial(f.data() + 4, (int64_t)f.size() - 4, 0) >> 8));
    for (const Block& b : blocks) { put32(f, (uint32_t)b.data.size() | (b.raw ? kLz4fRawBit : 0u)); append(f, b.data); }
    put32(f, 0);
    return f;
}

// what a batch decode left behind
struct Decoded { std::vector<lz4hip_lz4f_info_t> recs; lz4hip_lz4f_batch_info_t info; std::vector<int64_t> off; Bytes out; int64_t written; };

}  // namespace built_frames
