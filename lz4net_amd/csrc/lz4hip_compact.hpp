// lz4hip_compact.hpp -- the compact decode of a plain block batch: n independent blocks of UNKNOWN decoded size, each with an upper
// bound (the slot width), decoded into ONE buffer of exactly the bytes they produced, block i at dst[dst_off[i], dst_off[i + 1]) -- no
// size walk before the decode and no slot per block in the output.  It is the packed encode (lz4hip_packed.hpp) run the other way, and
// nearly all of it IS the packed encode: the batch goes in rounds of at most K blocks through one ring of K slots, and per round
//
//   packed_caps_kernel (the round's limits and its lengths with every negative one as 0: the decoders are handed a sanitised copy) ->
//   [launch_decode, unknown size, on the round's rows into the ring, row k at k * slot] -> compact_sizes_kernel (below) ->
//   stream_scan_* -> packed_rebase_kernel -> packed_pack_kernel
//
// and after the last round packed_info_kernel: lz4hip_compact_info_t has lz4hip_packed_info_t's layout (lz4hip_framing.hpp checks it).
// The one kernel of its own is the sizes step, because a decoder's failure is result < 0 where an encoder's is result <= 0: an empty
// block decodes to 0 bytes and that is a success.
//
// The legacy frame's one-call decode sits on top (lz4hip_framing.hpp: frame_decode_compact_run): frame_walk_kernel, the compact decode
// over every row of the table with slot and limit chunk_size, and frame_compact_info_kernel below.
//
// What a round costs in memory and in time: the ring of round_blocks = 0 is n slots, for a frame max_chunks * chunk_size bytes, which
// is large at 8 MiB chunks.  Rounds shrink the ring to K slots, but rounds do not overlap -- a round's pack has to read the ring before
// the next round's decoders write it -- and a round that does not fill the chip runs at the pace of its slowest wavefront however
// many rounds follow: 262 144 blocks of 64 KiB took 25 ms in one round, 41 ms in rounds of 65 536 and 138 ms in rounds of 16 384; a
// 1 GiB frame of 8 MiB chunks 230 ms in one round and 1.8 s in rounds of 16 chunks, sixteen wavefronts at a time (DESIGN.md 7,
// profiles/decode_compact/).  Rounds bound memory; they are not a way to go faster.
//
// Every kernel here is launch-only work on the caller's stream over caller scratch.
#pragma once
#include "lz4hip_packed.hpp"
#include "lz4hip_frame.hpp"

namespace lz4hip {

// packed_sizes_kernel with the decoders' failure rule: a block whose length was negative gets LZ4HIP_E_ARGUMENT as its result (the
// decoder saw an empty block in its place); max(result, 0) into the round's stretch of dst_off and of decoded_len; the lowest index
// with a NEGATIVE result.  A decoder returns at most its limit; packed_block_len holds anything else inside the slot all the same.
__global__ void __launch_bounds__(kStreamThreads) compact_sizes_kernel(PackedRound a)
{
    for (int64_t k = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; k < a.cnt; k += (int64_t)gridDim.x * kStreamThreads) {
        int32_t r = a.result[k];
        if (a.len_in && a.len_in[k] < 0) a.result[k] = r = kPackedBadLength;
        const int32_t len = packed_block_len(r, a.limit);
        a.offs[k] = len;
        if (a.lens) a.lens[k] = len;
        if (r < 0) atomicMin((unsigned long long*)(a.state + kPackedBad), (unsigned long long)(a.first + k));
    }
}

// The frame's record after the compact decode of its table: frame_info_kernel's, with the lowest bad chunk taken from the compact
// decode's state block (`bad`: a device pointer to it) -- the lowest row with a negative decoder result.
__global__ void __launch_bounds__(64) frame_compact_info_kernel(FrameTables t, const int64_t* bad, FrameInfo* info)
{
    if (threadIdx.x != 0) return;
    *info = frame_info_of(t, (unsigned long long)*bad);
}

}  // namespace lz4hip
