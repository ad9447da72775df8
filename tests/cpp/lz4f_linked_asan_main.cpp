// lz4f_linked_asan_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over the framing emulator's translation unit, for the
// decode of LZ4 frames with linked blocks (tests/simt/emu_framing.cpp, the linked entry points of its part emu_lz4f_batch.inc): a
// sanitizer run of the kernels, the launch sequences and the fronts on the CPU:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Itests/simt -Ilz4net_amd/csrc \
//         tests/cpp/lz4f_linked_asan_main.cpp -o lz4f_linked_asan && ./lz4f_linked_asan
//
// The new thing in this path is a decoder that READS BELOW dst + dst_off[row]: the bytes of the blocks before.  So every case places
// its item 0 at the very start of an allocation of exactly the decoded size: a match that starts at the frame's first byte (a), one
// byte before it (a': it must be refused, not read), a source that crosses a raw block and overlaps itself (c), the run fill out of the
// history (d), and the mixed batch of tests/test_simt_lz4f_linked.py with its clips, at the library's grids and at grids forced to 1
// and 3.  The frames are built by hand (built_frames.hpp) as tests/lz4f_built.py builds them; the independent items hold raw blocks
// only, so the stand-in block codec is handed nothing but empty rows.
#include "../simt/emu_framing.cpp"
#include "built_frames.hpp"

namespace {

using namespace built_frames;

// every buffer a heap block of exactly its size; the table holds `rows` rows, all of them empty rows to the stand-in codec
Decoded decode(const std::vector<Bytes>& frames, int64_t rows, int64_t out_bytes, int64_t round_blocks, int grid, unsigned flags = 3 | kLz4fAcceptLinked)
{
    Bytes src;
    std::vector<int64_t> off(1, 0);
    for (const Bytes& f : frames) { append(src, f); off.push_back((int64_t)src.size()); }
    const int64_t n = (int64_t)frames.size();
    std::vector<int32_t> zeros32((size_t)rows + 1, 0);
    std::vector<int64_t> zeros64((size_t)rows + 1, 0);
    Bytes blob(1, 0);
    Lz4fBatchEmuRun run = {};
    run.dec_results = zeros32.data(); run.dec_len = zeros32.data(); run.dec_at = zeros64.data(); run.dec_bytes = blob.data(); run.dec_rows = rows; run.grid = grid;
    const int64_t need = emu_lz4f_batch_decode_scratch_bytes(n, 65536, rows, round_blocks);
    CHECK(need > 0);
    Bytes scratch((size_t)need);
    Decoded d;
    d.recs.resize((size_t)n); d.off.resize((size_t)n + 1); d.out.assign((size_t)out_bytes, 0x5A); d.written = -1;
    CHECK(emu_lz4f_linked_batch_decode(src.data(), (int64_t)src.size(), off.data(), n, 65536, rows, round_blocks, flags, scratch.data(), need, d.out.data(),
                                       out_bytes, d.off.data(), d.recs.data(), &d.info, &d.written, &run) == 0);
    CHECK(run.shape_errors == 0);
    return d;
}

Block full_block(Content& c, uint32_t seed) { return c.block({ { noise(32762, seed), 32762, 32762 } }, kTail); }

struct Case { Bytes frame, content; int64_t blocks; };

Case case_a(unsigned offset)
{
    Content c = { Bytes(), Bytes(), true };
    std::vector<Block> blocks = { c.raw(noise(1000, 1)), c.block({ { Bytes(), 1000, 20 } }, kTail) };
    blocks[1].data[1] = (uint8_t)offset; blocks[1].data[2] = (uint8_t)(offset >> 8);
    return { frame_of(blocks, true), c.out, 2 };
}
Case case_c()
{
    Content c = { Bytes(), Bytes(), true };
    const std::vector<Block> blocks = { full_block(c, 3), c.raw(noise(10, 4)), c.block({ { Bytes(), 20, 40 }, { Bytes{ 'x', 'y' }, 65535, 5 } }, kTail) };
    return { frame_of(blocks, true), c.out, 3 };
}
Case case_d()
{
    Content c = { Bytes(), Bytes(), true };
    const std::vector<Block> blocks = { c.block({}, noise(50, 5)), c.block({ { Bytes(), 1, 1000 } }, kTail) };
    return { frame_of(blocks, true), c.out, 2 };
}

void one_item_at_the_start_of_its_allocation(int grid)
{
    for (const Case& k : { case_a(1000), case_c(), case_d() })
        for (int64_t round_blocks : { (int64_t)0, (int64_t)2 }) {
            const Decoded d = decode({ k.frame }, k.blocks, (int64_t)k.content.size(), round_blocks, grid);
            CHECK(d.recs[0].error == kLz4fOk && d.recs[0].blocks == k.blocks && d.out == k.content && d.written == 1 && d.info.first_error == -1);
            const Decoded refused = decode({ k.frame }, k.blocks, (int64_t)k.content.size(), round_blocks, grid, 3);
            CHECK(refused.recs[0].error == kLz4fUnsupportedLinked && refused.info.decoded_bytes == 0 && refused.out == Bytes(k.content.size(), 0x5A));
        }
    // (a'): the match starts one byte before the frame, which is one byte before the allocation
    const Case bad = case_a(1001);
    const Decoded d = decode({ bad.frame }, 2, (int64_t)bad.content.size(), 0, grid);
    CHECK(d.recs[0].error == kLz4fCorruptBlock && d.recs[0].good_bytes == 1000 && d.recs[0].decoded_bytes == 1032 && d.recs[0].error_offset == 7 + 4 + 1000);
    CHECK(memcmp(d.out.data(), bad.content.data(), 1000) == 0);
}

void mixed_batch(int grid)
{
    const Case two = case_d(), three = case_c();
    const Bytes one_src = noise(3000, 11), two_src = noise(65536 + 100, 12);
    Bytes skippable;
    put32(skippable, kLz4fSkippableMagic + 3); put32(skippable, 5); append(skippable, Bytes{ 1, 2, 3, 4, 5 });
    const std::vector<Bytes> frames = {
        frame_of({ { one_src, true } }, false), two.frame, skippable, three.frame,
        frame_of({ { Bytes(two_src.begin(), two_src.begin() + 65536), true }, { Bytes(two_src.begin() + 65536, two_src.end()), true } }, false),
        frame_of({}, false), frame_of({ { Bytes{ '0', '1', '2' }, true } }, true, 7),
    };
    const std::vector<Bytes> contents = { one_src, two.content, Bytes(), three.content, two_src, Bytes(), Bytes() };
    Bytes want;
    std::vector<int64_t> ends(1, 0);
    for (const Bytes& c : contents) { append(want, c); ends.push_back((int64_t)want.size()); }
    const int64_t rows = 1 + 2 + 3 + 2;
    for (int64_t round_blocks : { (int64_t)0, (int64_t)2 }) {
        const Decoded d = decode(frames, rows, (int64_t)want.size(), round_blocks, grid);
        CHECK(d.off == ends && d.out == want && d.written == 7 && d.info.blocks == rows && d.info.first_error == 6 && d.info.error == kLz4fUnsupportedDict);
        for (size_t i = 0; i < 6; i++) CHECK(d.recs[i].error == kLz4fOk);
        // a size query, and a cap inside the second block of the linked two-block item: that block is not written at all
        const Decoded q = decode(frames, rows, 0, round_blocks, grid);
        CHECK(q.off == ends && q.written == 0 && q.info.decoded_bytes == (int64_t)want.size());
        const int64_t cap = ends[1] + 50 + 500;
        const Decoded c = decode(frames, rows, cap, round_blocks, grid);
        CHECK(c.off == ends && c.written == 1 && memcmp(c.out.data(), want.data(), (size_t)ends[1] + 50) == 0);
        for (int64_t x = ends[1] + 50; x < cap; x++) CHECK(c.out[(size_t)x] == 0x5A);
    }
    const Decoded f = decode(frames, rows - 1, 4096, 0, grid);
    CHECK(f.info.error == kLz4fTableFull && f.info.blocks == rows && f.out == Bytes(4096, 0x5A));
}

}  // namespace

int main()
{
    for (int grid : { 0, 1, 3 }) {
        one_item_at_the_start_of_its_allocation(grid);
        mixed_batch(grid);
    }
    printf("lz4f linked: (a), (a'), (c), (d) at the start of their allocations and the mixed batch ran clean at grids 0, 1, 3\n");
    return 0;
}
