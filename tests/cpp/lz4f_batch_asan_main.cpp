// lz4f_batch_asan_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over the framing emulator's translation unit, for the batch
// of LZ4 frames (tests/simt/emu_framing.cpp, its part emu_lz4f_batch.inc): a sanitizer run of the kernels, the launch sequences and the
// fronts on the CPU:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Itests/simt -Ilz4net_amd/csrc \
//         tests/cpp/lz4f_batch_asan_main.cpp -o lz4f_batch_asan && ./lz4f_batch_asan
//
// It runs every outcome once in ONE batch (each fault as an item between good items) and 4 100 one-block items of 1 .. 40 bytes, every
// buffer a heap block of exactly its size, at the library's grids and at grids forced to 1 and 3.  There is no block codec here: a
// "compressed" block is len / 2 opaque bytes that the stand-in decoder answers with the source's bytes, which is all the framing sees of one.
#include "../simt/emu_framing.cpp"
#include "built_frames.hpp"

namespace {

using namespace built_frames;

struct Batch { Bytes bytes; std::vector<int64_t> off; };

Batch join(const std::vector<Bytes>& items)
{
    Batch b;
    b.off.push_back(0);
    for (const Bytes& it : items) { b.bytes.insert(b.bytes.end(), it.begin(), it.end()); b.off.push_back((int64_t)b.bytes.size()); }
    return b;
}

Bytes item_of(int64_t n, unsigned seed)
{
    Bytes b((size_t)n);
    for (int64_t i = 0; i < n; i++) b[(size_t)i] = (uint8_t)((i * 2654435761u + seed * 40503u) >> 11);
    return b;
}

// block j of the batch is "compressed" (to half its length) when `pick(j, len)` says so
template <class Pick>
std::vector<Bytes> encode(const std::vector<Bytes>& items, unsigned flags, int grid, Pick pick, std::vector<int>* compressed = nullptr)
{
    const Batch in = join(items);
    const int64_t n = (int64_t)items.size(), src_len = (int64_t)in.bytes.size();
    std::vector<int32_t> results, lens;
    std::vector<int64_t> at, where;
    Bytes blob;
    for (int64_t i = 0; i < n; i++)
        for (int64_t done = 0; done < (int64_t)items[(size_t)i].size(); done += 65536) {
            const int32_t len = (int32_t)std::min<int64_t>(65536, (int64_t)items[(size_t)i].size() - done);
            const int32_t res = pick((int64_t)results.size(), len) ? len / 2 : 0;
            results.push_back(res); lens.push_back(len); at.push_back((int64_t)blob.size()); where.push_back(in.off[(size_t)i] + done);
            for (int32_t k = 0; k < res; k++) blob.push_back((uint8_t)(0xC0 + results.size() + k));
            if (compressed) compressed->push_back(res > 0);
        }
    const int64_t rows = (int64_t)results.size();
    results.push_back(0); lens.push_back(0); at.push_back(0); where.push_back(0); blob.push_back(0);
    Lz4fBatchEmuRun run = {};
    run.enc_results = results.data(); run.enc_bytes = blob.data(); run.enc_at = at.data(); run.enc_len = lens.data(); run.enc_src = where.data();
    run.enc_rows = rows; run.grid = grid;
    const int64_t bound = emu_lz4f_batch_bound(n, src_len, 4, flags), need = emu_lz4f_batch_encode_scratch_bytes(n, src_len, 4);
    Bytes dst((size_t)bound), scratch((size_t)need);
    std::vector<int64_t> dst_off((size_t)n + 1);
    CHECK(emu_lz4f_batch_encode(in.bytes.data(), src_len, in.off.data(), n, 4, 0, flags, dst.data(), bound, dst_off.data(), scratch.data(), need, &run) == 0);
    CHECK(run.shape_errors == 0 && dst_off[0] == 0 && dst_off[(size_t)n] <= bound);
    std::vector<Bytes> frames;
    for (int64_t i = 0; i < n; i++) frames.emplace_back(dst.begin() + dst_off[(size_t)i], dst.begin() + dst_off[(size_t)i + 1]);
    return frames;
}

struct Row { int32_t result, len; Bytes bytes; };                          // what the stand-in decoder holds for one table row

Decoded decode(const std::vector<Bytes>& frames, const std::vector<Row>& rows, int64_t out_bytes, int64_t round_blocks, int grid)
{
    const Batch in = join(frames);
    const int64_t n = (int64_t)frames.size(), m = (int64_t)rows.size() > 0 ? (int64_t)rows.size() : 1;
    std::vector<int32_t> results((size_t)m + 1), lens((size_t)m + 1);
    std::vector<int64_t> at((size_t)m + 1);
    Bytes blob;
    for (size_t k = 0; k < rows.size(); k++) {
        results[k] = rows[k].result; lens[k] = rows[k].len; at[k] = (int64_t)blob.size();
        blob.insert(blob.end(), rows[k].bytes.begin(), rows[k].bytes.end());
    }
    blob.push_back(0);
    Lz4fBatchEmuRun run = {};
    run.dec_results = results.data(); run.dec_len = lens.data(); run.dec_at = at.data(); run.dec_bytes = blob.data(); run.dec_rows = m; run.grid = grid;
    const int64_t need = emu_lz4f_batch_decode_scratch_bytes(n, 65536, m, round_blocks);
    CHECK(need > 0);
    Bytes scratch((size_t)need);
    Decoded d;
    d.recs.resize((size_t)n); d.off.resize((size_t)n + 1); d.out.assign((size_t)out_bytes, 0x5A); d.written = -1;
    CHECK(emu_lz4f_batch_decode(in.bytes.data(), (int64_t)in.bytes.size(), in.off.data(), n, 65536, m, round_blocks, 3, scratch.data(), need, d.out.data(),
                                out_bytes, d.off.data(), d.recs.data(), &d.info, &d.written, &run) == 0);
    CHECK(run.shape_errors == 0);
    return d;
}

Bytes flipped(Bytes b, size_t at, uint8_t x = 1) { b[at] ^= x; return b; }
Bytes cut(const Bytes& b, size_t n) { return Bytes(b.begin(), b.begin() + n); }

void every_outcome_in_one_batch(int grid)
{
    // good items of several blocks, every other block "compressed"; the faults are made of a frame of one raw block
    const std::vector<Bytes> good_src = { item_of(3 * 65536 + 5, 1), item_of(65537, 2), item_of(13, 3), item_of(0, 4), item_of(65536, 5) };
    std::vector<int> compressed;
    const std::vector<Bytes> good = encode(good_src, 7, grid, [](int64_t j, int32_t len) { return j % 2 == 0 && len >= 4; }, &compressed);
    const Bytes one_src = item_of(1000, 9);
    const Bytes one = encode({ one_src }, 7, grid, [](int64_t, int32_t) { return false; })[0];
    CHECK(one.size() == 15 + 4 + 1000 + 4 + 4 + 4);
    Bytes wrong_size = flipped(one, 6);
    wrong_size[14] = (uint8_t)(xxh32_serial(wrong_size.data() + 4, 10, 0) >> 8);
    Bytes big_field = one;
    big_field[15] = 0x01; big_field[16] = 0x00; big_field[17] = 0x01; big_field[18] = 0x00;            // 65537
    Bytes linked = one;
    linked[4] &= (uint8_t)~0x20;
    linked[14] = (uint8_t)(xxh32_serial(linked.data() + 4, 10, 0) >> 8);
    struct Fault { Bytes frame; int error; int64_t blocks; };
    const std::vector<Fault> faults = {
        { Bytes{ 'a', 'b', 'c' }, kLz4fBadMagic, 0 }, { flipped(one, 1), kLz4fBadMagic, 0 }, { flipped(one, 4, 0x80), kLz4fBadHeader, 0 },
        { flipped(one, 14), kLz4fHeaderChecksum, 0 }, { linked, kLz4fUnsupportedLinked, 0 }, { cut(one, 17), kLz4fTruncated, 0 },
        { cut(one, 15 + 4 + 100), kLz4fTruncated, 0 }, { cut(one, one.size() - 2), kLz4fTruncated, 1 }, { big_field, kLz4fBadBlockSize, 0 },
        { flipped(one, 15 + 4 + 13, 0xFF), kLz4fBlockChecksumError, 1 }, { wrong_size, kLz4fContentSizeError, 1 },
        { flipped(one, one.size() - 1), kLz4fContentChecksumError, 1 },
        { flipped(flipped(one, 15 + 4 + 13, 0xFF), one.size() - 1), kLz4fBlockChecksumError, 1 },         // two faults: the lowest bad block wins
        { cut(flipped(one, 15 + 4 + 13, 0xFF), one.size() - 2), kLz4fBlockChecksumError, 1 },
    };
    // the batch: good items in turn, a fault between every two; the stand-in's rows follow the walked blocks
    std::vector<Bytes> frames;
    std::vector<Row> rows;
    std::vector<int> want_error;
    std::vector<Bytes> want_out;
    auto add_good = [&](size_t g) {
        frames.push_back(good[g]); want_error.push_back(0); want_out.push_back(good_src[g]);
        size_t first = 0;
        for (size_t h = 0; h < g; h++) first += (good_src[h].size() + 65535) / 65536;
        for (size_t done = 0, k = first; done < good_src[g].size(); done += 65536, k++) {
            const int32_t len = (int32_t)std::min<size_t>(65536, good_src[g].size() - done);
            if (compressed[k]) rows.push_back({ len, len / 2, Bytes(good_src[g].begin() + done, good_src[g].begin() + done + len) });
            else rows.push_back({ 0, 0, Bytes() });
        }
    };
    for (size_t k = 0; k < faults.size(); k++) {
        add_good(k % good.size());
        frames.push_back(faults[k].frame); want_error.push_back(faults[k].error);
        const bool keeps = faults[k].blocks == 1 && faults[k].error != kLz4fBlockChecksumError;
        want_out.push_back(keeps ? one_src : Bytes());
        for (int64_t b = 0; b < faults[k].blocks; b++) rows.push_back({ 0, 0, Bytes() });                  // (a raw block: the decoder sees an empty row)
    }
    add_good(4);
    const Batch want = join(want_out);
    for (int64_t round_blocks : { (int64_t)0, (int64_t)3 }) {
        const Decoded d = decode(frames, rows, (int64_t)want.bytes.size(), round_blocks, grid);
        for (size_t i = 0; i < frames.size(); i++) {
            CHECK(d.recs[i].error == want_error[i]);
            CHECK(d.off[i] == want.off[i]);
        }
        CHECK(d.off.back() == want.off.back() && d.out == want.bytes && d.written == (int64_t)frames.size());
        CHECK(d.info.first_error == 1 && d.info.error == kLz4fBadMagic && d.info.items == (int64_t)frames.size() && d.info.blocks == (int64_t)rows.size());
    }
    // clipped in the middle of an item, and a table one row short
    const Decoded c = decode(frames, rows, 70000, 2, grid);
    CHECK(c.written == 0 && c.info.decoded_bytes == (int64_t)want.bytes.size() && memcmp(c.out.data(), want.bytes.data(), 70000) == 0);
    std::vector<Row> fewer(rows.begin(), rows.end() - 1);
    const Decoded f = decode(frames, fewer, 4096, 0, grid);
    CHECK(f.info.error == kLz4fTableFull && f.info.blocks == (int64_t)rows.size() && f.out == Bytes(4096, 0x5A));
}

void tiny_items(int grid)
{
    std::vector<Bytes> src;
    for (int i = 0; i < 4100; i++) src.push_back(item_of(1 + (i * 7919) % 40, (unsigned)i));
    std::vector<int> compressed;
    const std::vector<Bytes> frames = encode(src, 7, grid, [](int64_t j, int32_t len) { return j % 3 == 0 && len >= 4; }, &compressed);
    std::vector<Row> rows;
    for (size_t i = 0; i < src.size(); i++) {
        const int32_t len = (int32_t)src[i].size();
        if (compressed[i]) rows.push_back({ len, len / 2, src[i] });
        else rows.push_back({ 0, 0, Bytes() });
    }
    const Batch want = join(src);
    const Decoded d = decode(frames, rows, (int64_t)want.bytes.size(), 4099, grid);
    CHECK(d.info.error == 0 && d.info.first_error == -1 && d.info.blocks == 4100 && d.out == want.bytes && d.off == want.off && d.written == 4100);
    for (const lz4hip_lz4f_info_t& r : d.recs) CHECK(r.error == 0 && r.checks == 5 && r.blocks == 1);
}

}  // namespace

int main()
{
    for (int grid : { 0, 1, 3 }) {
        every_outcome_in_one_batch(grid);
        tiny_items(grid);
    }
    printf("lz4f batch: every outcome in one batch and 4100 tiny items ran clean at grids 0, 1, 3\n");
    return 0;
}
