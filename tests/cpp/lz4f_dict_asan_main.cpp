// lz4f_dict_asan_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over the framing emulator's translation unit, for the
// decode of LZ4 frames with a dictionary (tests/simt/emu_framing.cpp, its part emu_lz4f_dict.inc): a sanitizer run of the kernels, the
// launch sequences and the fronts on the CPU:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Itests/simt -Ilz4net_amd/csrc \
//         tests/cpp/lz4f_dict_asan_main.cpp -o lz4f_dict_asan && ./lz4f_dict_asan
//
// The new thing in this path is a decoder that reads BOTH below dst + dst_off[row] (the item's bytes so far) and a dictionary that ends
// somewhere else.  So every case places its item 0 at the very start of an allocation of exactly the decoded size, and the dictionary
// in an allocation of exactly its size, at an even and at an odd address inside it: a match that starts at the dictionary's first
// byte, from a first block (independent) and from behind a raw block (linked); the same one byte further back, which must be refused,
// not read; a source that starts in the dictionary, crosses a raw block and overlaps itself; the run fill of the dictionary's last
// byte; 40 short sequences out of the dictionary and a long copy (the mirror's preload and the long path's two copies) -- with
// dictionaries of 1, 13, 4 095, 4 097, 65 535 and 70 000 bytes, of which only the last 65 535 may be touched: the program hands the
// kernels the WHOLE allocation but poisons nothing, so for 70 000 the check is the result.  Also the host calls, whose staging holds
// exactly the reachable bytes.  The frames are built by hand (built_frames.hpp) as tests/lz4f_built.py builds them.
#include "../simt/emu_framing.cpp"
#include "built_frames.hpp"

namespace {

using namespace built_frames;

// every buffer a heap block of exactly its size; the dictionary at offset `odd` of a block of exactly its size + odd
Decoded decode(const std::vector<Bytes>& frames, const Bytes& dict, uint32_t dict_id, int odd, int64_t rows, int64_t out_bytes, int64_t round_blocks, int grid,
               bool host = false)
{
    Bytes src;
    std::vector<int64_t> off(1, 0);
    for (const Bytes& f : frames) { append(src, f); off.push_back((int64_t)src.size()); }
    const int64_t n = (int64_t)frames.size();
    Bytes placed((size_t)odd, 0xEE);
    append(placed, dict);
    Lz4fDictEmuRun run = {};
    run.grid = grid;
    Decoded d;
    d.recs.resize((size_t)n); d.off.resize((size_t)n + 1); d.out.assign((size_t)out_bytes, 0x5A); d.written = -1;
    if (host) {
        const int rc = emu_lz4f_dict_batch_decode_host(src.data(), (int64_t)src.size(), off.data(), n, placed.data() + odd, (int64_t)dict.size(), dict_id,
                                                       3 | kLz4fAcceptLinked, d.out.data(), out_bytes, d.off.data(), d.recs.data(), &d.info, &run);
        CHECK(rc == d.info.error);
        CHECK(run.dict_uploads == 1 && run.dict_bytes == (int64_t)(dict.size() < 65535 ? dict.size() : 65535) && run.dict_intact == 1 && run.counters.intact == 1);
        return d;
    }
    const int64_t need = emu_lz4f_dict_batch_decode_scratch_bytes(n, 65536, rows, round_blocks);
    CHECK(need > 0);
    Bytes scratch((size_t)need);
    CHECK(emu_lz4f_dict_batch_decode(src.data(), (int64_t)src.size(), off.data(), n, placed.data() + odd, (int64_t)dict.size(), dict_id, 65536, rows, round_blocks,
                                     3 | kLz4fAcceptLinked, scratch.data(), need, d.out.data(), out_bytes, d.off.data(), d.recs.data(), &d.info, &d.written,
                                     &run) == 0);
    CHECK(run.plain_calls == 0 && run.dict_calls > 0);
    return d;
}

struct Case { Bytes frame, content; int64_t blocks; int64_t refused_good; };           // refused_good >= 0: block 1 is refused behind that many bytes

unsigned reach_of(const Bytes& dict) { return (unsigned)(dict.size() < 65535 ? dict.size() : 65535); }

void patch_offset(Block& b, unsigned offset) { b.data[1] = (uint8_t)offset; b.data[2] = (uint8_t)(offset >> 8); }

Case independent_first_byte(const Bytes& dict, bool before)
{
    Content c = { dict, Bytes(), false };
    std::vector<Block> blocks = { c.block({}, noise(100, 1)), c.block({ { Bytes(), reach_of(dict), 20 } }, kTail) };
    if (before) patch_offset(blocks[1], reach_of(dict) + 1);
    return { frame_of(blocks, false, 7), c.out, 2, before ? 100 : -1 };
}
Case linked_behind_a_raw_block(const Bytes& dict, bool before)
{
    Content c = { dict, Bytes(), true };
    const unsigned far = 1000 + dict.size() < 65535 ? 1000 + (unsigned)dict.size() : 65535;
    std::vector<Block> blocks = { c.raw(noise(1000, 4)), c.block({ { Bytes(), far, 20 } }, kTail) };
    if (before) patch_offset(blocks[1], far + 1);
    return { frame_of(blocks, true, 0), c.out, 2, before ? 1000 : -1 };
}
Case linked_across_a_raw_block(const Bytes& dict)
{
    Content c = { dict, Bytes(), true };
    const unsigned k = reach_of(dict) < 3 ? reach_of(dict) : 3;
    const std::vector<Block> blocks = { c.raw(noise(10, 5)), c.block({ { Bytes{ 'x', 'y' }, 12 + k, 40 } }, kTail), c.block({ { Bytes(), 64 + k, 80 } }, kTail) };
    return { frame_of(blocks, true, 7), c.out, 3, -1 };
}
Case linked_run_fill(const Bytes& dict)
{
    Content c = { dict, Bytes(), true };
    const std::vector<Block> blocks = { c.block({ { Bytes(), 1, 1000 } }, kTail) };
    return { frame_of(blocks, true, 7), c.out, 1, -1 };
}
Case linked_short_sequences(const Bytes& dict)
{
    Content c = { dict, Bytes(), true };
    std::vector<Part> parts;
    unsigned at = 0;
    const unsigned span = dict.size() < 3000 ? (unsigned)dict.size() : 3000;
    for (unsigned j = 0; j < 40; j++) {
        const Bytes literals(j % 3, (uint8_t)(65 + j % 26));
        at += (unsigned)literals.size();
        parts.push_back({ literals, at + 1 + 13 * j % span, 4 + j % 15 });
        at += 4 + j % 15;
    }
    parts.push_back({ Bytes(), at + span, 200 });
    const std::vector<Block> blocks = { c.block(parts, noise(150, 8)) };
    return { frame_of(blocks, true, 0), c.out, 1, -1 };
}

void one_item_at_the_start_of_its_allocation(const Bytes& dict, int grid)
{
    std::vector<Case> cases = { independent_first_byte(dict, false), linked_behind_a_raw_block(dict, false), linked_across_a_raw_block(dict),
                                linked_run_fill(dict), linked_short_sequences(dict) };
    if (dict.size() < 65535) cases.push_back(independent_first_byte(dict, true));
    if (1000 + dict.size() < 65535) cases.push_back(linked_behind_a_raw_block(dict, true));
    for (const Case& k : cases)
        for (int odd : { 0, 1 })
            for (int64_t round_blocks : { (int64_t)0, (int64_t)2 }) {
                // (a refused independent block takes no bytes, a refused linked one keeps its place)
                const bool linked = !(k.frame[4] & 0x20);
                const int64_t bytes = k.refused_good >= 0 && !linked ? k.refused_good : (int64_t)k.content.size();
                const Decoded d = decode({ k.frame }, dict, 7, odd, k.blocks, bytes, round_blocks, grid);
                CHECK(d.recs[0].blocks == k.blocks && d.info.decoded_bytes == bytes);
                if (k.refused_good < 0) {
                    CHECK(d.recs[0].error == kLz4fOk && d.out == k.content && d.written == 1 && d.info.first_error == -1);
                } else {
                    CHECK(d.recs[0].error == kLz4fCorruptBlock && d.recs[0].good_bytes == k.refused_good);
                    CHECK(memcmp(d.out.data(), k.content.data(), (size_t)k.refused_good) == 0);
                }
            }
}

void batches(const Bytes& dict, int grid)
{
    const Case a = independent_first_byte(dict, false), b = linked_across_a_raw_block(dict), c = linked_run_fill(dict);
    const Bytes other = frame_of({ { Bytes{ '0', '1', '2' }, true } }, false, 8);
    Bytes skippable;
    put32(skippable, kLz4fSkippableMagic + 3); put32(skippable, 5); append(skippable, Bytes{ 1, 2, 3, 4, 5 });
    const std::vector<Bytes> frames = { a.frame, b.frame, skippable, c.frame, other };
    Bytes want;
    std::vector<int64_t> ends(1, 0);
    for (const Bytes& x : { a.content, b.content, Bytes(), c.content, Bytes() }) { append(want, x); ends.push_back((int64_t)want.size()); }
    const int64_t rows = a.blocks + b.blocks + c.blocks;
    for (int64_t round_blocks : { (int64_t)0, (int64_t)2 }) {
        const Decoded d = decode(frames, dict, 7, 1, rows, (int64_t)want.size(), round_blocks, grid);
        CHECK(d.off == ends && d.out == want && d.written == 5 && d.info.blocks == rows && d.info.first_error == 4 && d.info.error == kLz4fDictIdMismatch);
        const Decoded q = decode(frames, dict, 7, 0, rows, 0, round_blocks, grid);
        CHECK(q.off == ends && q.written == 0 && q.info.decoded_bytes == (int64_t)want.size());
        const int64_t cap = ends[1] + 10 + 30;                         // inside the second block of the linked three-block item
        const Decoded clip = decode(frames, dict, 7, 1, rows, cap, round_blocks, grid);
        CHECK(clip.off == ends && clip.written == 1 && memcmp(clip.out.data(), want.data(), (size_t)ends[1] + 10) == 0);
        for (int64_t x = ends[1] + 10; x < cap; x++) CHECK(clip.out[(size_t)x] == 0x5A);
    }
    const Decoded h = decode(frames, dict, 7, 1, rows, (int64_t)want.size(), 0, grid, true);
    CHECK(h.off == ends && h.out == want && h.info.error == kLz4fDictIdMismatch);
}

}  // namespace

int main()
{
    for (size_t n : { (size_t)1, (size_t)13, (size_t)4095, (size_t)4097, (size_t)65535, (size_t)70000 }) {
        Bytes dict = noise(n, 77);
        if (n >= 2 && dict[n - 1] == dict[n - 2]) dict[n - 1] ^= 0x55;
        for (int grid : { 0, 1, 3 }) {
            one_item_at_the_start_of_its_allocation(dict, grid);
            batches(dict, grid);
        }
    }
    printf("lz4f dict: the hand-built frames at the start of their allocations, dictionaries of 1 .. 70 000 bytes at even and odd addresses, the mixed batch "
           "and the host call ran clean at grids 0, 1, 3\n");
    return 0;
}
