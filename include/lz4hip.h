/*
 * lz4hip.h -- C ABI of liblz4hip.so: the MI355X (gfx950) batched LZ4 block codec that stands in for
 * lz4net's back-end ladder (LZ4mm / LZ4cc / LZ4pn / LZ4ps) behind LZ4.LZ4Codec.Encode/Decode/EncodeHC.
 *
 * Plain C, plain pointers and sizes: P/Invoke-able from C# (bindings/csharp/HipLZ4Service.cs), callable
 * through ctypes (lz4net_amd/_lib.py) and from C/C++ (include/lz4net/LZ4Codec.hpp).  All paths below
 * citing the reference are relative to the lz4net repository.
 *
 * Conventions (identical to the reference's core functions):
 *   encode           : bytes written, or 0 when the output limit would be exceeded
 *   decode, known    : bytes CONSUMED from the source, or -(error position in the source)
 *   decode, unknown  : bytes PRODUCED, or -(error position in the source)
 * Library-level failures (no device, HIP error, bad argument) are reported as LZ4HIP_E_* values,
 * which are far outside the range of any codec result, plus lz4hip_last_error().
 * There is no CPU fallback: without a usable gfx950 device every call fails with LZ4HIP_E_DEVICE.
 *
 * Thread safety: all entry points are re-entrant.  Host-pointer calls use per-thread device scratch
 * and the per-thread default stream; device-pointer calls are asynchronous on the stream given.
 */
#ifndef LZ4HIP_H
#define LZ4HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZ4HIP_E_DEVICE   (-2000000001)   /* no usable HIP device / HIP runtime error */
#define LZ4HIP_E_ARGUMENT (-2000000002)   /* null pointer, negative size, ... */
#define LZ4HIP_E_MEMORY   (-2000000003)   /* device allocation failed */

#define LZ4HIP_MODE_FAST 0
#define LZ4HIP_MODE_HC   1

/* ---- information ------------------------------------------------------------------------------ */
/* lz4hip_uncompress is not told its source length (neither is LZ4_uncompress, original/lz4.c:812-814): like the
 * reference it trusts the stream and reads on until `osize` bytes are produced -- on a corrupt stream that walk is
 * unbounded on the host side exactly as the reference's is.  Use lz4hip_uncompress_bounded for untrusted input. */
/* Counterpart of LZ4Codec.CodecName (src/LZ4/LZ4Codec.cs:298-308), e.g. "HIP gfx950 (AMD Instinct MI355X)". */
const char* lz4hip_codec_name(void);
int         lz4hip_device_count(void);
const char* lz4hip_last_error(void);
/* The kernel sources this binary was compiled from: the first 16 hex digits of the SHA-256 over lz4net_amd/csrc/ (file names + contents, sorted;
 * lz4net_amd/build.py csrc_sha()), "+tuning" appended for -DLZ4HIP_TUNING_BUILD libraries, "unknown" for a build that bypassed build.py.
 * bench.py prints it next to the hash of the tree it runs from and refuses to measure when the two differ. */
const char* lz4hip_build_id(void);

/* LZ4_compressBound (original/lz4.h:85-86) == LZ4Codec.MaximumOutputLength (src/LZ4ps/LZ4Codec.cs:142-145). */
int lz4hip_compressBound(int isize);

/* ---- single block, host memory, lz4.h-shaped ----------------------------------------------------
 * Drop-in for the functions lz4net's native back-end binds (src/LZ4cc/LZ4Codec.64.cpp:31-36,81-100,
 * 139-144 call I64_LZ4_compress_limitedOutput / I64_LZ4_uncompress / I64_LZ4_uncompress_unknownOutputSize /
 * I64_LZ4_compressHC_limitedOutput; declarations original/lz4.h:59-60,101,116 and original/lz4hc.h:47,57). */
int lz4hip_compress_limitedOutput(const char* source, char* dest, int isize, int maxOutputSize);
int lz4hip_compress(const char* source, char* dest, int isize);
int lz4hip_compressHC_limitedOutput(const char* source, char* dest, int isize, int maxOutputSize);
int lz4hip_compressHC(const char* source, char* dest, int isize);
int lz4hip_uncompress(const char* source, char* dest, int osize);
int lz4hip_uncompress_unknownOutputSize(const char* source, char* dest, int isize, int maxOutputSize);
/* Known-size decode that is also told the source length and never reads past it -- what
 * ILZ4Service.Decode(..., knownOutputLength: true) needs (src/LZ4/ILZ4Service.cs:30-36: the service
 * always has inputLength; the wrapper compares the result with it, src/LZ4pn/LZ4Codec.Unsafe.cs:373-378). */
int lz4hip_uncompress_bounded(const char* source, int isize, char* dest, int osize);

/* ---- batches -------------------------------------------------------------------------------------
 * The reference has no batch API; lz4net users loop over LZ4Codec.Encode/Decode per block (e.g.
 * LZ4Stream.FlushCurrentChunk / AcquireNextChunk, src/LZ4/LZ4Stream.cs:239-312).  One descriptor
 * describes n independent blocks; block i starts at base + (off ? off[i] : i * stride). */
typedef struct lz4hip_batch {
    const void*    src;
    const int64_t* src_off;      /* optional byte offsets (packed layouts), else NULL */
    int64_t        src_stride;
    const int32_t* src_len;      /* per-block input bytes, or NULL to use src_len_all */
    void*          dst;
    const int64_t* dst_off;
    int64_t        dst_stride;
    const int32_t* dst_cap;      /* per-block capacity (encode, unknown-size decode) or exact size (known-size decode); NULL => dst_cap_all */
    int32_t        dst_cap_all;
    int32_t        src_len_all;  /* length of every block when src_len == NULL; otherwise a HINT: 0 = unknown, else it MUST be an upper
                                    bound on every src_len[i] (LZ4HC picks its 16-bit-head kernels from "<= 65536"; a too-small
                                    value with longer blocks is a caller error and yields LZ4HIP_E_ARGUMENT results for those blocks) */
    int32_t*       result;       /* per-block codec result, conventions above */
    int64_t        n_blocks;
} lz4hip_batch_t;

/* Device-resident batches: every pointer in *b is device memory of the CURRENT device; the call only
 * enqueues kernels on `stream` (a hipStream_t, NULL = default stream) and returns 0 or LZ4HIP_E_*.
 * One exception, once per device and size: the FIRST fast-encode batch of >= 49152 blocks on a device (and a later one that needs
 * more resident wavefronts than any before) builds the lane encoder's table slab inside the call -- device allocations, for
 * slabs >= 2 GiB a few timed probe launches (hipEventSynchronize) on a stream of the library's own, and, when a smaller slab is
 * replaced, one hipDeviceSynchronize before that one is freed (it stays in place if the larger one cannot be had): 0.1 - 3.5 s
 * during which the calling thread blocks and holds the device's encoder workspace.  LZ4HC batches likewise
 * allocate their tables on first use; GROWING them for a later, larger batch waits for the device (hipDeviceSynchronize) before the old tables
 * are freed.  The first lane-mapped decode on a device runs a ~1 ms probe launch and waits for it (knob decoder_wrapped_stores).  Every later call is launch-only. */
int lz4hip_encode_batch_device(const lz4hip_batch_t* b, int mode, void* stream);
int lz4hip_decode_batch_device(const lz4hip_batch_t* b, int known_output_size, void* stream);

/* Host-resident batches: stages through device memory (H2D, kernels, D2H) in slices whose copies and kernels overlap, and synchronises.  DECODE
 * batches of >= 8192 blocks are cut round-robin over two staging pipelines on the current device, each on a persistent worker thread of the
 * library (knob host_workers); fast-ENCODE batches run as one pipeline whose slices are equal and at most one residency round of the
 * wavefront-mapped encoder each (ten blocks per CU): its kernels are the bottleneck. */
int lz4hip_encode_batch_host(const lz4hip_batch_t* b, int mode);
int lz4hip_decode_batch_host(const lz4hip_batch_t* b, int known_output_size);

/* ---- block batches decoded against a shared dictionary -------------------------------------------------------------------------------
 * LZ4_decompress_safe_usingDict in a loop (K4os.Compression.LZ4: LZ4Codec.Decode(source, target, dictionary)): every block of the batch
 * shares ONE dictionary dict[0, dict_len).  Block i's result and bytes are what lz4hip_decode_batch_device gives for it, known_output_size
 * 0 or 1, when the dictionary's bytes lie immediately in front of its dst: the return values and the rules are that call's.
 *   - A match source at index s of the block's output with -dict_len <= s < 0 reads dict[dict_len + s].
 *   - A source before that is the error a plain block gets for a source before the block, with the same return value.
 *   - Only the last 65 535 bytes of the dictionary can ever be reached (an offset has 16 bits); the others are never read.
 *   - Nothing outside [dict, dict + dict_len) is read, and nothing is written that the plain call would not write.
 *   - dict_len == 0 (dict may then be NULL) is the plain call, result for result and byte for byte.
 *   - The dictionary may have any alignment.  It is not copied: it must stay valid until the kernels have run.
 * The device call carries the contract of lz4hip_decode_batch_device: device pointers of the current device -- dict included -- launch-only
 * on `stream`, 0 or LZ4HIP_E_*; dict_len < 0, and dict == NULL with dict_len > 0, are LZ4HIP_E_ARGUMENT, checked before a device is looked
 * for.  THE COST: these calls run the wavefront mapping (one wavefront per block) at every batch size -- lz4hip_dispatch_counts moves
 * LZ4HIP_K_DECODE_WAVE only -- so a large dictionary batch decodes at that mapping's rate, not at the lane mapping's.  Each wavefront
 * first copies the dictionary's last 4 096 bytes into its LDS mirror, so that runs of short sequences that copy out of the dictionary
 * stay on the decoder's fast paths.
 * The host call stages the blocks as lz4hip_decode_batch_host does; the dictionary's reachable bytes are uploaded once per call into
 * per-thread grow-only device memory (freed by lz4hip_release_workspaces) and have landed before any slice's kernels start.
 * The sizes calls are lz4hip_decoded_sizes_device / _host for such blocks: a match may start up to min(dict_len, 65 535) bytes before its
 * block.  They need no byte of the dictionary; the scratch query is lz4hip_decoded_sizes_scratch_bytes.
 * Out of scope: LZ4 frames with a dictionary (below: lz4hip_lz4f_*_dict_*); a dictionary per block; the lane mapping; a _multi host
 * form; the compact and packed decode forms.  (Encoding against a dictionary: lz4hip_encode_batch_dict_*, next.) */
int lz4hip_decode_batch_dict_device(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, int known_output_size, void* stream);
int lz4hip_decode_batch_dict_host(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, int known_output_size);

/* ---- block batches encoded against a shared dictionary -------------------------------------------------------------------------------
 * K4os.Compression.LZ4's LZ4Codec.Encode(source, target, dictionary) in a loop: every block of the batch shares ONE dictionary
 * dict[0, dict_len).  FAST MODE ONLY.  result[i], dst_cap and the returned 0 when a block does not fit are those of
 * lz4hip_encode_batch_device; nothing is written at or past a block's dst_cap.  A block's bytes are legal input for
 * lz4hip_decode_batch_dict_device and for LZ4_decompress_safe_usingDict with the same dictionary.
 * The reference has no such parse to be bit-exact to, so the bytes are DEFINED here: they are what the reference's generic
 * encoder (LZ4_compressCtx: U32[4096] table, hash shift 20) writes when it runs over the dictionary's last T = min(dict_len, 65 535) bytes
 * followed by the block, starts at the block's first byte -- anchor and first table insert there, first probe one byte later -- and finds
 * its table primed: bucket h holds the highest position p <= T - 4 of the dictionary's tail whose four bytes hash to h, and position 0
 * where there is none.  Matches may start in the dictionary and run on into the block; literals are the block's; offsets are <= 65 535.
 * A block of fewer than 13 bytes is literals only.  They are not the bytes liblz4's LZ4_compress_fast_continue writes, but of the
 * same kind and, on 4 KiB text records against a 64 KiB dictionary, the same size.
 *   - Only the last 65 535 bytes of the dictionary are read, and nothing outside [dict, dict + dict_len).
 *   - dict_len == 0 (dict and scratch may then be NULL) IS lz4hip_encode_batch_device(b, LZ4HIP_MODE_FAST, stream), result for result
 *     and byte for byte -- that call's choice of the 64k variant for blocks below 65 547 bytes and its two mappings included.
 *   - The dictionary may have any alignment.  It is not copied: it must stay valid until the kernels have run.
 *   - A block of more than 0x7E000000 bytes (LZ4_MAX_INPUT_SIZE) gets the result 0.
 * The device call carries the contract of lz4hip_decode_batch_dict_device: device pointers of the current device -- dict and scratch
 * included -- launch-only on `stream`, nothing allocated, 0 or LZ4HIP_E_*; dict_len < 0, and dict == NULL with dict_len > 0, are
 * LZ4HIP_E_ARGUMENT, checked before a device is looked for, and so are, with dict_len > 0, a NULL scratch, one that is not 16-byte
 * aligned and scratch_bytes below lz4hip_encode_dict_scratch_bytes(dict_len).  The scratch holds the primed table (16 KiB), which a
 * one-workgroup kernel builds from the dictionary at the start of every call; the blocks only read it.
 * THE COST: these calls run the wavefront mapping (one wavefront per block, the table in 16 KiB of LDS, workgroups of one or five blocks
 * as lz4hip_encode_batch_device picks them) at every batch size -- lz4hip_dispatch_counts moves LZ4HIP_K_ENCODE_WAVE only.  There is no
 * lane mapping and no hand-over to it, so a large batch of sequence-dense blocks encodes at the wavefront mapping's rate.  Each wavefront
 * first copies the primed table into its LDS, in place of the plain encoder's zero fill.
 * The host call stages the blocks as lz4hip_encode_batch_host does (one pipeline, that call's slices); the dictionary's reachable bytes
 * are uploaded once per call and its table is primed once per call, both into per-thread grow-only device memory (freed by
 * lz4hip_release_workspaces), and both have landed before any slice's kernels start.
 * Out of scope: LZ4HC against a dictionary; a dictionary per block; the lane mapping; a _multi host form; the packed encode form.
 * (LZ4 frames with a dictionary on the encode side -- LZ4F_compressFrame_usingCDict -- are this call under the frame rounds:
 * lz4hip_lz4f_encode_dict_* and lz4hip_lz4f_batch_encode_dict_*, "LZ4 frames encoded with a dictionary" below.) */
int64_t lz4hip_encode_dict_scratch_bytes(int64_t dict_len);
int lz4hip_encode_batch_dict_device(const lz4hip_batch_t* b, const void* dict, int64_t dict_len, void* scratch, int64_t scratch_bytes, void* stream);
int lz4hip_encode_batch_dict_host(const lz4hip_batch_t* b, const void* dict, int64_t dict_len);

/* Host-resident batches sharded over several GPUs of the node: block i is processed by the (i mod N)-th device
 * selected by device_mask (bit d = HIP device d; 0 = every visible device) -- the round-robin partition of
 * SURVEY.md 8e.  One PERSISTENT worker thread and one staging pipeline per device (started on first use, reused by every
 * later call; lz4hip_release_workspaces gives their memory back), no inter-device traffic; per-block results
 * and payloads land in the caller's arrays in global block order.  This is what a C# caller (HipLZ4Batch,
 * bindings/csharp) uses to spread LZ4Codec work over the 8 GPUs of a node without any launcher. */
int lz4hip_encode_batch_host_multi(const lz4hip_batch_t* b, int mode, uint64_t device_mask);
int lz4hip_decode_batch_host_multi(const lz4hip_batch_t* b, int known_output_size, uint64_t device_mask);

/* ---- LZ4Stream buffers ---------------------------------------------------------------------------
 * The wire format of lz4net's LZ4Stream (src/LZ4/LZ4Stream.cs:239-312): a run of chunks
 *     varint(flags) varint(originalLength) [varint(compressedLength) if flags & 1] payload
 * flags: 1 Compressed, 2 HighCompression.  A source of src_len bytes is cut into ceil(src_len / block_size) chunks (block_size is
 * clamped to >= 16, like LZ4Stream); a chunk is stored raw when the encoder does not shrink it; an LZ4HC stream carries flag 2 on
 * EVERY chunk, raw ones included, as the reference writes it.  Decoding skips empty chunks (original length 0) and stops at the
 * first bad header.  Stream-level outcomes (lz4hip_stream_info_t.error): */
#define LZ4HIP_STREAM_OK            0
#define LZ4HIP_STREAM_END_OF_STREAM 1   /* truncated / corrupt header or payload  (EndOfStreamException) */
#define LZ4HIP_STREAM_PASSES        2   /* compressed chunk with passes != 0      (NotSupportedException) */
#define LZ4HIP_STREAM_CORRUPT_BLOCK 3   /* a chunk's LZ4 block failed to decode   (ArgumentException)     */
#define LZ4HIP_STREAM_TABLE_FULL    4   /* more chunks than max_chunks; .chunks = the count needed        */
typedef struct lz4hip_stream_info {
    int64_t chunks, compressed_chunks;  /* non-empty chunks before the first header error (all of them, also when the table is full) */
    int64_t decoded_bytes;              /* sum of their original lengths */
    int64_t error_offset;               /* stream offset of the failing chunk's header (TABLE_FULL: of the first chunk that did not fit), -1 if none */
    int32_t error, reserved;
} lz4hip_stream_info_t;

/* Bytes an encoded stream can take: len + n * (1 + 2 * varint_len(block_size)), n = ceil(len / block_size). */
int64_t lz4hip_stream_bound(int64_t src_len, int32_t block_size);
/* Device scratch (bytes) of the two device calls below; 0 for an empty source. */
int64_t lz4hip_stream_encode_scratch_bytes(int64_t src_len, int32_t block_size);
int64_t lz4hip_stream_decode_scratch_bytes(int64_t max_chunks);

/* Device-resident streams: every pointer is device memory of the CURRENT device, the calls only enqueue kernels on `stream` (a
 * hipStream_t, NULL = default stream), read no device value on the host and allocate nothing: scratch comes from the caller.  They
 * return 0 or LZ4HIP_E_*.  The exceptions are those of lz4hip_encode_batch_device / lz4hip_decode_batch_device, which these calls
 * run on the chunks: a stream encode whose chunk count reaches 49152 (fast) may build the lane encoder's table slab, an LZ4HC encode
 * may allocate or grow its tables, and a decode of 16384 compressed chunks or more may run the lane decoder's probe and allocate its
 * counters -- each once per device.
 *
 * Encode: writes the stream to dst (dst_cap >= lz4hip_stream_bound, else LZ4HIP_E_ARGUMENT) and its length to *dst_len (device).
 * scratch_bytes must be >= lz4hip_stream_encode_scratch_bytes(src_len, block_size). */
int lz4hip_stream_encode_device(const void* src, int64_t src_len, int32_t block_size, int mode,
                                void* dst, int64_t dst_cap, int64_t* dst_len,
                                void* scratch, int64_t scratch_bytes, void* stream);
/* Decode is two calls; the caller reads *info back between them (one synchronisation) to learn the chunk counts and the output size.
 * Index: walks the headers of src[0, src_len) into a table of max_chunks entries in scratch and writes *info (device).  When the
 * stream has more non-empty chunks than max_chunks, info.error = LZ4HIP_STREAM_TABLE_FULL and info.chunks is the count needed.
 * Decode: decodes what the index found, given the info it reported (host copy) and the same scratch and max_chunks: every chunk
 * before the first header error is written to dst[0, decoded_bytes), and *info (device) is the index's, except that a corrupt
 * block -- which always comes before the header error -- turns it into LZ4HIP_STREAM_CORRUPT_BLOCK at the FIRST such chunk's header.
 * LZ4HIP_E_ARGUMENT for an info_host whose error is not OK / END_OF_STREAM / PASSES, or whose decoded_bytes exceed dst_cap. */
int lz4hip_stream_index_device(const void* src, int64_t src_len, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                               lz4hip_stream_info_t* info, void* stream);
int lz4hip_stream_decode_device(const void* src, const lz4hip_stream_info_t* info_host, int64_t max_chunks,
                                void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                lz4hip_stream_info_t* info, void* stream);

/* Decode in ONE call, with no value read on the host, into a buffer the caller already owns (a tensor of known shape, a cache page,
 * an arena): the contract of lz4hip_frame_decode_compact_device.  The arguments are checked first, whatever the device --
 * LZ4HIP_E_ARGUMENT for a negative size, NULL src with src_len > 0, NULL dst with dst_cap > 0, NULL info or scratch, too little
 * scratch, more than 2^31 - 1 table rows -- and after that the call is launch-only on `stream`: nothing is read back and nothing is
 * allocated, with the first-use exceptions of lz4hip_decode_batch_device.  written_bytes may be NULL; dst_cap is any value >= 0, and
 * the call's cost follows the device-side end of the output, not dst_cap.
 *
 * The headers carry every chunk's decoded size, so the index already lays the output out: the index runs as above, the block decoder
 * (known size) runs ONCE over all max_chunks rows of the table -- the rows past the stream's count are empty blocks -- and writes
 * straight to dst.  With dst_cap >= the decoded size every output is what the two calls above write with the same max_chunks, byte
 * for byte: dst[0, decoded_bytes) and *info, and *written_bytes (device) = decoded_bytes.  Otherwise the output is clipped at a chunk
 * boundary: a chunk is written iff its end offset is <= dst_cap, *written_bytes is the end of the last such chunk (0 if none), no byte
 * at or past it is written and the chunks that do not fit are not decoded; info.chunks, compressed_chunks and decoded_bytes are
 * complete all the same, so dst_cap = 0 is a size query in one call.  A corrupt block is found only in a chunk that was written:
 * *info is the index's, turned into LZ4HIP_STREAM_CORRUPT_BLOCK by the first corrupt block among the written chunks.  On
 * LZ4HIP_STREAM_TABLE_FULL *info is the index's (chunks = the count needed), nothing is written to dst and *written_bytes = 0.
 *
 * max_chunks: size the table to the stream.  The decoder's choice between its wavefront and lane mappings goes by the table size, not
 * by the stream's real chunk count: a table of 16 384 rows or more around 1 024 chunks of 1 MiB takes the lane mapping for them.
 * scratch_bytes must be >= lz4hip_stream_decode_into_scratch_bytes(max_chunks). */
int64_t lz4hip_stream_decode_into_scratch_bytes(int64_t max_chunks);
int lz4hip_stream_decode_into_device(const void* src, int64_t src_len, int64_t max_chunks,
                                     void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                     lz4hip_stream_info_t* info, int64_t* written_bytes, void* stream);

/* The chunk directory of ONE stream, for a stream that is decoded more than once or in parts: the index's header walk (one wavefront,
 * one dependent round trip per chunk -- latency-bound by design, and the point is that it runs once per stream) with its result
 * kept.  The arguments are checked first, whatever the device; then the call is launch-only on `stream` and takes no scratch: it writes
 * straight to the caller's device arrays hdr_off and out_off of max_chunks + 1 entries each.  For every non-empty chunk k before the
 * first header error hdr_off[k] is the offset of its header and out_off[k] its decoded offset; the closing entry hdr_off[chunks] is
 * the offset at which the walk ended (src_len for a clean stream, else error_offset) and out_off[chunks] = decoded_bytes.  *info
 * (device) is what lz4hip_stream_index_device reports, with its stop rules and error codes.  With more chunks than max_chunks
 * info.error = LZ4HIP_STREAM_TABLE_FULL and info.chunks is the count needed: entries [0, max_chunks) are valid and the closing entry is
 * not written.
 * A stream is the concatenation of its chunks and each chunk a valid one-chunk stream: src[hdr_off[k], hdr_off[k + 1]) is chunk k plus
 * the empty chunks' headers behind it, an item of lz4hip_streams_decode_spans_into_device, in which every chunk's header is read by a
 * wavefront of its own.  Chunks k0 .. k1 as such spans decode to bytes [out_off[k0], out_off[k1 + 1]) of the stream. */
int lz4hip_stream_directory_device(const void* src, int64_t src_len, int64_t max_chunks,
                                   int64_t* hdr_off, int64_t* out_off, lz4hip_stream_info_t* info, void* stream);

/* Host-resident streams: stage the whole buffer through device memory (per-thread, grow-only, freed by lz4hip_release_workspaces),
 * run the device calls above and synchronise.  Encode returns 0 or LZ4HIP_E_* (dst_cap >= lz4hip_stream_bound); *dst_len on the host.
 * Decode returns info->error (0 or a positive LZ4HIP_STREAM_* code; the chunks before the error are in dst) or LZ4HIP_E_*; with
 * dst_cap below the decoded size it returns LZ4HIP_E_ARGUMENT with info->decoded_bytes filled in (a size query: dst_cap = 0). */
int lz4hip_stream_encode_host(const void* src, int64_t src_len, int32_t block_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len);
int lz4hip_stream_decode_host(const void* src, int64_t src_len, void* dst, int64_t dst_cap, lz4hip_stream_info_t* info);

/* ---- wrapped messages ----------------------------------------------------------------------------
 * The self-describing format of lz4net's LZ4Codec.Wrap / WrapHC / Unwrap (src/LZ4/LZ4Codec.cs:471-599), for many independent
 * messages at once:  int32 originalLength, int32 payloadLength (both little-endian), payload.
 * A batch of n messages is one buffer src of src_len bytes plus int64 offsets src_off[n + 1]: message i is
 * src[src_off[i], src_off[i + 1]).  Wrap writes exactly this layout and Unwrap reads it: one call's output is the other's input.
 *
 * Wrap (as the reference): an empty message becomes 8 zero bytes; the encoder runs with outputLength = inputLength (fast or HC)
 * and its output is used when 0 < r < inputLength; otherwise the message is stored raw with both fields = inputLength.
 * result[i]: the payload size of a compressed message, 0 for one stored raw, LZ4HIP_E_ARGUMENT for offsets that decrease, fall
 * outside [0, src_len] or give a length above INT32_MAX -- such a message takes 0 bytes of dst.  When offsets decrease, messages
 * may overlap: their output is then unspecified, dst_off[n] may exceed dst_cap, and nothing past dst_cap is written.
 *
 * Unwrap (as the reference, with signed fields), per message, in this order:
 *   fewer than 8 bytes                             LZ4HIP_WRAP_SIZE_INVALID   ("inputBuffer size is invalid")
 *   payloadLength < 0 or > available - 8          LZ4HIP_WRAP_CORRUPT_HEADER ("inputBuffer size is invalid or has been corrupted";
 *                                                  for a negative payloadLength the reference throws no ArgumentException but
 *                                                  fails later, in the decoder's argument checks or the allocation)
 *   payloadLength >= originalLength                the payload as it is (payloadLength bytes; also for a negative originalLength)
 *   otherwise                                      a known-size decode of originalLength bytes; consumed != payloadLength is
 *                                                  LZ4HIP_WRAP_CORRUPT_BLOCK ("LZ4 block is corrupted, or invalid length has been
 *                                                  given.", Decode64, src/LZ4pn/LZ4Codec.Unsafe.cs:373-378)
 * Bad offsets (as for Wrap) give the status LZ4HIP_E_ARGUMENT.  Every message with a valid header is decoded, not only those before
 * the first failure.  A failed message's output range is unspecified (0 bytes for a header failure, originalLength for a corrupt
 * block); no byte outside it is written.  info.first_error is the lowest failing index, header errors and corrupt blocks alike --
 * what a sequential [Unwrap(w) for w in ...] raises first -- and info.error that message's status. */
#define LZ4HIP_WRAP_OK             0
#define LZ4HIP_WRAP_SIZE_INVALID   1   /* < 8 bytes                          */
#define LZ4HIP_WRAP_CORRUPT_HEADER 2   /* payloadLength < 0 or past the end  */
#define LZ4HIP_WRAP_CORRUPT_BLOCK  3   /* block did not decode exactly       */
typedef struct lz4hip_unwrap_info {
    int64_t messages, compressed;       /* n, and the messages that go through the block decoder */
    int64_t decoded_bytes;              /* dst_off[n] */
    int64_t first_error;                /* lowest failing message index, -1 if none */
    int32_t error, reserved;            /* that message's status */
} lz4hip_unwrap_info_t;

/* src_len + 8 n: the exact worst case of a wrapped batch (every message stored raw). */
int64_t lz4hip_wrap_bound(int64_t n, int64_t src_len);
/* Device scratch (bytes) of the device calls below; the index and the decode of one batch share theirs. */
int64_t lz4hip_wrap_scratch_bytes(int64_t n, int64_t src_len);
int64_t lz4hip_unwrap_scratch_bytes(int64_t n);

/* Device-resident batches: the contract of the lz4hip_stream_*_device calls -- device pointers of the CURRENT device, launch-only
 * on `stream`, no device value read on the host, scratch from the caller, 0 or LZ4HIP_E_* returned -- with the first-use exceptions
 * of lz4hip_encode_batch_device / lz4hip_decode_batch_device, which these calls run on the messages.
 *
 * Wrap: dst_cap >= lz4hip_wrap_bound(n, src_len), scratch_bytes >= lz4hip_wrap_scratch_bytes(n, src_len); writes dst_off[n + 1]
 * (dst_off[n] = the total) and, if result is not NULL, result[n]. */
int lz4hip_wrap_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode,
                       void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* result,
                       void* scratch, int64_t scratch_bytes, void* stream);
/* Unwrap is two calls; the caller reads *info back between them (one synchronisation) to size dst.
 * Index: reads every header, writes dst_off[n + 1] (dst_off[n] = decoded_bytes), the header statuses status[n] and *info (device).
 * Decode: given the index's info (host copy) and the same src, offsets, scratch, dst_off and status, decodes every message with a valid
 * header into dst[dst_off[i], dst_off[i + 1]), adds LZ4HIP_WRAP_CORRUPT_BLOCK statuses and writes the final *info (device).
 * LZ4HIP_E_ARGUMENT for an info_host whose decoded_bytes exceed dst_cap or that does not describe n messages. */
int lz4hip_unwrap_index_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n,
                               int64_t* dst_off, int32_t* status,
                               void* scratch, int64_t scratch_bytes, lz4hip_unwrap_info_t* info, void* stream);
int lz4hip_unwrap_decode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n,
                                const lz4hip_unwrap_info_t* info_host, void* scratch, int64_t scratch_bytes,
                                void* dst, int64_t dst_cap, const int64_t* dst_off, int32_t* status,
                                lz4hip_unwrap_info_t* info, void* stream);

/* Unwrap in ONE call, with no value read on the host, into a buffer the caller already owns: lz4hip_stream_decode_into_device for
 * wrapped messages, with its contract and argument checks (n > 0 also needs src_off and status).  The index runs as above, the block
 * decoder (known size) runs once over all n rows of the table and writes straight to dst.  With dst_cap >= the decoded size dst,
 * dst_off, status and *info are what the two calls above write, byte for byte, and *written_messages (device, may be NULL) = n.
 * Otherwise message i is written iff dst_off[i + 1] <= dst_cap: *written_messages is the length of that prefix, no byte at or past
 * dst_off[*written_messages] is written and the other messages are not decoded; dst_off, the header statuses and
 * info.decoded_bytes are complete all the same (dst_cap = 0: a size query in one call), and a corrupt block is found only in a
 * message that was written.  scratch_bytes must be >= lz4hip_unwrap_into_scratch_bytes(n). */
int64_t lz4hip_unwrap_into_scratch_bytes(int64_t n);
int lz4hip_unwrap_into_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n,
                              void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                              int64_t* dst_off, int32_t* status,
                              lz4hip_unwrap_info_t* info, int64_t* written_messages, void* stream);

/* Unwrap CHOSEN messages of an arena in one call: lz4hip_unwrap_into_device with m spans in the place of n consecutive messages.
 * Message j of the call is src[src_begin[j], src_end[j]) (device arrays of m entries); the spans may come in any order, repeat,
 * overlap and leave holes -- the source is only read -- so the cost follows m, not the arena.  Everything else is the contract of
 * lz4hip_unwrap_into_device with m for n: the argument checks (m > 0 also needs src_begin, src_end and status), launch-only, scratch
 * of lz4hip_unwrap_into_scratch_bytes(m); dst_off[m + 1] and status[m] are indexed by CALL position, info.first_error is the lowest
 * failing call position, and dst_cap clips a prefix in call order (message j is written iff dst_off[j + 1] <= dst_cap; dst_cap = 0
 * is the size query).  A span with begin < 0, end < begin, end > src_len or longer than INT32_MAX gets LZ4HIP_E_ARGUMENT and 0 bytes,
 * as bad offsets do.  With src_begin = src_off and src_end = src_off + 1 every output is what lz4hip_unwrap_into_device writes, byte
 * for byte.  With repeats the decoded size has no bound in src_len: size dst from the size query. */
int lz4hip_unwrap_spans_into_device(const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m,
                                    void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                    int64_t* dst_off, int32_t* status,
                                    lz4hip_unwrap_info_t* info, int64_t* written_messages, void* stream);
/* The spans of chosen entries, for callers with nothing to index a device array with: begin[j] = src_off[sel[j]], end[j] =
 * src_off[sel[j] + 1]; a sel[j] outside [0, n) gives begin[j] = end[j] = -1, which the span calls (this one and
 * lz4hip_streams_decode_spans_into_device) answer with LZ4HIP_E_ARGUMENT for that item.  The arguments are checked first (n, m >= 0;
 * m > 0 needs sel, src_begin and src_end, and src_off unless n = 0); then one launch on `stream`, no scratch. */
int lz4hip_spans_select_device(const int64_t* src_off, int64_t n, const int64_t* sel, int64_t m,
                               int64_t* src_begin, int64_t* src_end, void* stream);

/* Host-resident batches (what a C# byte[][] caller binds): stage everything through device memory (per-thread, grow-only, freed by
 * lz4hip_release_workspaces), run the device calls above and synchronise; every pointer is host memory.
 * Wrap returns 0 or LZ4HIP_E_* (dst_cap >= lz4hip_wrap_bound).  Unwrap returns 0 when every message unwrapped, else info->error (a
 * positive LZ4HIP_WRAP_* code, or LZ4HIP_E_ARGUMENT for bad offsets; dst, dst_off and status are filled in all the same) or
 * LZ4HIP_E_*; with dst_cap below the decoded size it returns LZ4HIP_E_ARGUMENT with info->decoded_bytes, dst_off and status filled in
 * (a size query: dst_cap = 0). */
int lz4hip_wrap_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int mode,
                     void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* result);
int lz4hip_unwrap_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n,
                       void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status, lz4hip_unwrap_info_t* info);

/* ---- batches of LZ4Stream buffers ----------------------------------------------------------------
 * Many independent LZ4Stream buffers per call -- what a service holds: serialized objects, cache entries, log segments of one to a
 * handful of chunks each -- in the layout of the wrapped-message calls: one buffer src of src_len bytes plus int64 offsets
 * src_off[n + 1], item i is src[src_off[i], src_off[i + 1]).  Encode turns every item into the stream lz4hip_stream_encode_device
 * writes for that item alone, byte for byte, and lays the streams back to back in dst with dst_off[n + 1]; decode reads exactly that
 * layout: one call's output is the other's input.  Items may be longer than 2 GiB (chunks cannot).  The chunks of ALL items go
 * through the block codecs as one batch, and on the way back every item's headers are walked by a wavefront of its own.
 *
 * Per item, decoding is what the one-stream calls do: every chunk before the item's first header error is decoded into
 * dst[dst_off[i], dst_off[i + 1]); status[i] is an LZ4HIP_STREAM_* code and error_offset[i] the failing header's offset RELATIVE TO
 * THE ITEM'S START (-1 if none); a corrupt block, which always comes before the header error, wins.  A failing item never disturbs
 * another item's bytes or status, and no byte outside an item's range is written.  Offsets that decrease or fall outside
 * [0, src_len] give that item the status LZ4HIP_E_ARGUMENT and 0 bytes; on encode such an item takes 0 bytes of dst (when offsets
 * decrease, items may overlap: their output is then unspecified, dst_off[n] may exceed dst_cap, and nothing past dst_cap is written). */
typedef struct lz4hip_streams_info {
    int64_t items;                      /* n */
    int64_t chunks, compressed_chunks;  /* non-empty chunks of all items before their header errors (TABLE_FULL: chunks = the count needed) */
    int64_t decoded_bytes;              /* dst_off[n] */
    int64_t first_error;                /* lowest failing item index, -1 if none: what a sequential loop over the items raises first */
    int64_t error_offset;               /* that item's error_offset, -1 if none */
    int32_t error, reserved;            /* that item's status, or LZ4HIP_STREAM_TABLE_FULL for the whole batch */
} lz4hip_streams_info_t;

/* src_len + (src_len / block_size + n) * (1 + 2 * varint_len(block_size)): covers every partition of src_len bytes into n items
 * (sum of ceil(len_i / block_size) <= src_len / block_size + n).  block_size is clamped to >= 16. */
int64_t lz4hip_streams_bound(int64_t n, int64_t src_len, int32_t block_size);
/* Device scratch (bytes) of the device calls below; the index and the decode of one batch share theirs.  0 for an empty batch. */
int64_t lz4hip_streams_encode_scratch_bytes(int64_t n, int64_t src_len, int32_t block_size);
int64_t lz4hip_streams_decode_scratch_bytes(int64_t n, int64_t max_chunks);

/* Device-resident batches: the contract of the lz4hip_stream_*_device and lz4hip_wrap_device calls -- device pointers of the CURRENT
 * device, launch-only on `stream`, no device value read on the host, no allocation, scratch from the caller, 0 or LZ4HIP_E_*
 * returned -- with the first-use exceptions of lz4hip_encode_batch_device / lz4hip_decode_batch_device, which these calls run on the
 * chunks.  The offsets are device values, so the host sizes the chunk table by the bound src_len / block_size + n; entries past the
 * real count are empty blocks.
 *
 * Encode: dst_cap >= lz4hip_streams_bound, scratch_bytes >= lz4hip_streams_encode_scratch_bytes; writes dst and dst_off[n + 1]
 * (dst_off[n] = the total). */
int lz4hip_streams_encode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode,
                                 void* dst, int64_t dst_cap, int64_t* dst_off,
                                 void* scratch, int64_t scratch_bytes, void* stream);
/* Decode is two calls; the caller reads *info back between them (one synchronisation) to size dst.
 * Index: walks every item's headers (twice: to count, and to fill the tables), writes dst_off[n + 1] (dst_off[n] = decoded_bytes), the
 * header statuses status[n], error_offset[n] and *info (device).  max_chunks is the table size for the WHOLE batch; when the items
 * hold more non-empty chunks, info.error = LZ4HIP_STREAM_TABLE_FULL and info.chunks is the count needed.
 * Decode: given the index's info (host copy) and the same src, offsets, max_chunks, scratch, dst_off, status and error_offset, decodes
 * what the index found, turns the items with a corrupt block into LZ4HIP_STREAM_CORRUPT_BLOCK at the first such chunk's header and
 * writes the final *info (device).  LZ4HIP_E_ARGUMENT for an info_host that reports TABLE_FULL, does not describe n items or whose
 * decoded_bytes exceed dst_cap. */
int lz4hip_streams_index_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks,
                                int64_t* dst_off, int32_t* status, int64_t* error_offset,
                                void* scratch, int64_t scratch_bytes, lz4hip_streams_info_t* info, void* stream);
int lz4hip_streams_decode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n,
                                 const lz4hip_streams_info_t* info_host, int64_t max_chunks, void* scratch, int64_t scratch_bytes,
                                 void* dst, int64_t dst_cap, const int64_t* dst_off, int32_t* status, int64_t* error_offset,
                                 lz4hip_streams_info_t* info, void* stream);

/* Decode in ONE call, with no value read on the host, into a buffer the caller already owns: lz4hip_stream_decode_into_device for a
 * batch of streams, with its contract and argument checks (n > 0 also needs src_off, status, error_offset and scratch; more than
 * 2^31 - 1 items or table rows are refused).  The index runs as above, the block decoder (known size) runs once over all max_chunks
 * rows of the table -- size it to the batch: the decoder's choice of mapping goes by the table size -- and writes straight to dst.
 * With dst_cap >= the decoded size dst, dst_off, status, error_offset and *info are what the two calls above write with the same
 * max_chunks, byte for byte, and *written_items (device, may be NULL) = n.  Otherwise item i is written iff dst_off[i + 1] <= dst_cap:
 * *written_items is the length of that prefix, no byte at or past dst_off[*written_items] is written and the other items' chunks are
 * not decoded; dst_off, the header statuses, error_offset and info.decoded_bytes are complete all the same (dst_cap = 0: a size
 * query in one call), and a corrupt block is found only in an item that was written.  On LZ4HIP_STREAM_TABLE_FULL *info, dst_off,
 * status and error_offset are the index's, nothing is written to dst and *written_items = 0.
 * scratch_bytes must be >= lz4hip_streams_decode_into_scratch_bytes(n, max_chunks), which is 0 for an empty batch. */
int64_t lz4hip_streams_decode_into_scratch_bytes(int64_t n, int64_t max_chunks);
int lz4hip_streams_decode_into_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int64_t max_chunks,
                                      void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                      int64_t* dst_off, int32_t* status, int64_t* error_offset,
                                      lz4hip_streams_info_t* info, int64_t* written_items, void* stream);

/* Decode CHOSEN items of an arena in one call: lz4hip_streams_decode_into_device with m spans in the place of n consecutive items.
 * Item j of the call is src[src_begin[j], src_end[j]) (device arrays of m entries; lz4hip_spans_select_device makes them from
 * offsets and indices, lz4hip_stream_directory_device from one stream's chunks); the spans may come in any order, repeat, overlap and
 * leave holes.  Everything else is the contract of lz4hip_streams_decode_into_device with m for n: the argument checks (m > 0 also
 * needs src_begin, src_end, status, error_offset and scratch), launch-only, scratch of lz4hip_streams_decode_into_scratch_bytes(m,
 * max_chunks); dst_off[m + 1], status[m] and error_offset[m] are indexed by CALL position, error_offset is relative to src_begin[j],
 * info.first_error is the lowest failing call position, and dst_cap clips a prefix in call order.  max_chunks counts the chunks of
 * the chosen items with multiplicity; LZ4HIP_STREAM_TABLE_FULL works as above.  A span with begin < 0, end < begin or end > src_len
 * gets LZ4HIP_E_ARGUMENT and 0 bytes.  With src_begin = src_off and src_end = src_off + 1 every output is what
 * lz4hip_streams_decode_into_device writes, byte for byte. */
int lz4hip_streams_decode_spans_into_device(const void* src, int64_t src_len, const int64_t* src_begin, const int64_t* src_end, int64_t m,
                                            int64_t max_chunks, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                            int64_t* dst_off, int32_t* status, int64_t* error_offset,
                                            lz4hip_streams_info_t* info, int64_t* written_items, void* stream);

/* Host-resident batches (what a C# byte[][] caller binds): stage everything through device memory (per-thread, grow-only, freed by
 * lz4hip_release_workspaces), run the device calls above and synchronise; every pointer is host memory.
 * Encode returns 0 or LZ4HIP_E_* (dst_cap >= lz4hip_streams_bound; bad offsets, which the host can see here, are LZ4HIP_E_ARGUMENT).
 * Decode returns 0 when every item decoded, else info->error (a positive LZ4HIP_STREAM_* code, or LZ4HIP_E_ARGUMENT for bad offsets;
 * dst, dst_off, status and error_offset are filled in all the same) or LZ4HIP_E_*; with dst_cap below the decoded size it returns
 * LZ4HIP_E_ARGUMENT with info->decoded_bytes, dst_off, status and error_offset filled in (a size query: dst_cap = 0). */
int lz4hip_streams_encode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t block_size, int mode,
                               void* dst, int64_t dst_cap, int64_t* dst_off);
int lz4hip_streams_decode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n,
                               void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* status, int64_t* error_offset,
                               lz4hip_streams_info_t* info);

/* ---- the decoded sizes of a batch, before decoding it ---------------------------------------------
 * What a caller holding nothing but compressed blocks needs before an unknown-size decode: for block i, result[i] is what
 * LZ4_uncompress_unknownOutputSize (original/lz4.c:916-1044) returns for it when maxOutputSize is too large ever to bind -- the bytes
 * produced, or -(error position in the source) -- found by walking the block's tokens without writing a byte of output.  An empty
 * block gives 0; a count above INT32_MAX, where the reference's int would have wrapped, and a negative length give LZ4HIP_E_ARGUMENT.
 *
 * For a block that obeys the format's end rules -- the last match starts at least 12 bytes before the end and the last 5 bytes are
 * literals; every block an LZ4 encoder wrote does -- a following unknown-size decode with dst_cap = result[i] returns result[i].  A
 * malformed block that walks to a size but breaks those rules then fails in the decoder with the reference's error, exactly as the
 * reference would at that capacity.
 *
 * The call reads b->src, src_off / src_stride, src_len / src_len_all, result and n_blocks; the dst fields are ignored and may be NULL
 * or 0.  It writes, each only where the pointer is not NULL: b->result[n]; dst_cap[n] = max(result[i], 0); dst_off[n + 1], the
 * exclusive scan of dst_cap (a packed layout without padding, dst_off[n] = the total); *info.  The two arrays are laid out so that the
 * second step is the existing call, unchanged:
 *     lz4hip_batch_t d = *b;  d.dst = out;  d.dst_off = dst_off;  d.dst_cap = dst_cap;  lz4hip_decode_batch_device(&d, 0, stream);
 * A block whose walk failed has capacity 0 there and fails again without writing a byte. */
typedef struct lz4hip_sizes_info {
    int64_t blocks;                     /* n */
    int64_t decoded_bytes;              /* dst_off[n]: the sum of the non-negative results */
    int64_t first_error;                /* lowest index with a negative result, -1 if none */
    int32_t error, reserved;            /* that block's result, 0 if none */
} lz4hip_sizes_info_t;

/* Device scratch (bytes) of the device call; 0 for an empty batch, non-decreasing in n_blocks. */
int64_t lz4hip_decoded_sizes_scratch_bytes(int64_t n_blocks);
/* Device-resident batch: the contract of the other device calls -- device pointers of the CURRENT device, launch-only on `stream`, no
 * device value read on the host, no allocation, scratch from the caller, 0 or LZ4HIP_E_* returned (arguments are checked first: a NULL
 * batch, a negative n_blocks or too little scratch is LZ4HIP_E_ARGUMENT whatever the device). */
int lz4hip_decoded_sizes_device(const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap,
                                void* scratch, int64_t scratch_bytes, lz4hip_sizes_info_t* info, void* stream);
/* Host-resident batch: stages the blocks and their lengths through device memory (per-thread, grow-only, freed by
 * lz4hip_release_workspaces), runs the device call and synchronises; only result, dst_off, dst_cap and info travel back.  Returns 0
 * (block failures are in result and info) or LZ4HIP_E_*. */
int lz4hip_decoded_sizes_host(const lz4hip_batch_t* b, int64_t* dst_off, int32_t* dst_cap, lz4hip_sizes_info_t* info);
/* The same two calls for blocks that are decoded against a dictionary of dict_len >= 0 bytes (lz4hip_decode_batch_dict_*, above). */
int lz4hip_decoded_sizes_dict_device(const lz4hip_batch_t* b, int64_t dict_len, int64_t* dst_off, int32_t* dst_cap,
                                     void* scratch, int64_t scratch_bytes, lz4hip_sizes_info_t* info, void* stream);
int lz4hip_decoded_sizes_dict_host(const lz4hip_batch_t* b, int64_t dict_len, int64_t* dst_off, int32_t* dst_cap, lz4hip_sizes_info_t* info);

/* ---- a block batch encoded into one packed buffer ---------------------------------------------------
 * The pack step the framed encoders end in, for the plain block batch: n blocks are compressed as lz4hip_encode_batch_device compresses
 * them, but land back to back in ONE buffer -- block i at dst[dst_off[i], dst_off[i + 1]), no padding -- instead of one compressBound
 * slot each.  The offsets and lengths written are exactly the src_off / src_len of the size query above and of an offsets-form decode
 * batch: one call's output is the other's input.
 *
 * The source side of *b is read as the batch encoder reads it: src, src_off / src_stride, src_len / src_len_all (with its hint
 * meaning) and n_blocks.  b->dst, dst_off and dst_stride are ignored and may be NULL or 0.  b->dst_cap_all must be > 0: it is the slot
 * width, slot_bytes below, and the per-block output limit where b->dst_cap is NULL; with b->dst_cap given, block i's limit is
 * min(dst_cap[i], dst_cap_all) -- LZ4_compress_limitedOutput semantics per block.  b->result[n], if not NULL, receives the raw
 * per-block encoder results.
 *
 * The call writes dst_off[n + 1] (required): the exclusive scan of max(result[i], 0), dst_off[n] the total; packed_len[n] (optional):
 * max(result[i], 0); the bytes; and *info.  A block that failed its limit (result 0) or its arguments (LZ4HIP_E_ARGUMENT: a negative
 * length -- the call itself gives that result: such a length never reaches the block encoders, which do not check it) takes 0 bytes
 * and its neighbours pack around it.
 *
 * dst_cap may be any value >= 0: it need not reach a bound.  The offsets are monotone, so block i is written iff
 * dst_off[i + 1] <= dst_cap; info.written_blocks is the length of that prefix, the bytes of dst from dst_off[written_blocks] up to
 * dst_cap are unspecified, and no byte at or past dst_cap is ever written.  dst_off, packed_len, result and info.packed_bytes are
 * complete in either case: the encoders are deterministic, so a second call with dst_cap = packed_bytes fits, and dst_cap = 0 is a
 * size query (dst may then be NULL).
 *
 * Rounds: round_blocks = 0 runs the batch as one round; round_blocks = K > 0 runs ceil(n / K) rounds of at most K blocks through ONE
 * ring of min(K, n) slots, so the scratch -- the ring, a round's tables and a few hundred bytes -- does not grow with n once n > K.
 * Each round is a normal batch encode of its rows: the wavefront / lane dispatch rules and the first-use exceptions of the batch
 * encoder above (the lane encoder's table slab from 49152 blocks, the LZ4HC tables) apply to the ROUND's size, not to n. */
typedef struct lz4hip_packed_info {
    int64_t blocks;          /* n */
    int64_t packed_bytes;    /* dst_off[n]: the bytes the whole batch needs, whatever dst_cap was */
    int64_t written_blocks;  /* leading blocks that lie wholly inside dst_cap (n when all do) */
    int64_t first_failed;    /* lowest index whose encoder result is <= 0, -1 if none */
    int32_t error, reserved; /* that block's result (0 = did not fit its per-block limit, or LZ4HIP_E_ARGUMENT), 0 if none */
} lz4hip_packed_info_t;

/* Device scratch (bytes) of the device call; 0 for an empty batch, non-decreasing in n_blocks and the same for every
 * n_blocks >= round_blocks > 0.  LZ4HIP_E_ARGUMENT for slot_bytes <= 0 or round_blocks < 0. */
int64_t lz4hip_encode_packed_scratch_bytes(int64_t n_blocks, int32_t slot_bytes, int64_t round_blocks);
/* Device-resident batch: the contract of the other device calls -- device pointers of the CURRENT device, launch-only on `stream`, no
 * device value read on the host, no allocation beyond what the block encoder itself does on first use, scratch from the caller, 0 or
 * LZ4HIP_E_* returned.  Arguments are checked first: a NULL batch or dst_off, a negative n_blocks, dst_cap or round_blocks,
 * dst_cap_all <= 0, a bad mode, too little scratch or more than 2^31 - 1 blocks in a round is LZ4HIP_E_ARGUMENT whatever the device.
 * An empty batch writes dst_off[0] = 0 and an info with first_failed = -1.  info may be NULL. */
int lz4hip_encode_packed_device(const lz4hip_batch_t* b, int mode, int64_t round_blocks,
                                void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* packed_len,
                                void* scratch, int64_t scratch_bytes, lz4hip_packed_info_t* info, void* stream);
/* Host-resident batch: every pointer is host memory.  Gathers the rows, stages them with their lengths and limits through device
 * memory (per-thread, grow-only, freed by lz4hip_release_workspaces), runs the device call, reads info and the per-block arrays back
 * and copies only min(packed_bytes, dst_cap) bytes of output.  The arguments are checked as the device call checks them; info may
 * be NULL.  Returns 0 (block failures are in result and info) or LZ4HIP_E_*. */
int lz4hip_encode_packed_host(const lz4hip_batch_t* b, int mode, int64_t round_blocks,
                              void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* packed_len,
                              lz4hip_packed_info_t* info);

/* ---- a block batch decoded into one packed buffer, without a size walk ---------------------------------
 * The packed encode the other way, for blocks whose decoded sizes the caller does not know but for which it knows an UPPER BOUND per
 * block: a frame's chunk size, a stream's block size, the row width the data was cut to.  The decoders then answer the size question
 * themselves: a round of blocks is decoded into a ring of bound-sized slots, the produced sizes are scanned and the round is packed
 * back to back into dst -- block i at dst[dst_off[i], dst_off[i + 1]).  No size query (lz4hip_decoded_sizes_device walks every
 * block's tokens, which costs more than decoding it), no read-back between two calls, and no n * slot bytes of output.
 *
 * The source side of *b is read as the batch decoder reads it: src, src_off / src_stride, src_len / src_len_all and n_blocks.  b->dst,
 * dst_off and dst_stride are ignored and may be NULL or 0.  b->dst_cap_all must be > 0: it is the slot width, slot_bytes below, and the
 * per-block output limit where b->dst_cap is NULL; with b->dst_cap given, block i's limit is min(max(dst_cap[i], 0), dst_cap_all).
 * b->result[n], if not NULL, receives the raw per-block results: result[i] is what lz4hip_decode_batch_device (known_output_size = 0)
 * gives block i at that limit -- the bytes produced, or -(error position), the latter also for a block that would produce more than
 * its limit: LZ4_uncompress_unknownOutputSize(src_i, slot, len_i, limit_i).  An empty block succeeds with 0.  A negative length gives
 * LZ4HIP_E_ARGUMENT: the call itself produces that result, the decoders only ever see a sanitised copy of the lengths.
 *
 * The call writes dst_off[n + 1] (required): the exclusive scan of max(result[i], 0), dst_off[n] the total; decoded_len[n] (optional):
 * max(result[i], 0); the bytes; and *info (optional).  A failed block -- result < 0; the packed encode's rule is <= 0, the one place
 * the two differ -- takes 0 bytes and its neighbours pack around it.
 *
 * dst_cap may be any value >= 0.  Block i is written iff dst_off[i + 1] <= dst_cap; info.written_blocks is the length of that prefix,
 * the bytes of dst from dst_off[written_blocks] up to dst_cap are unspecified, and no byte at or past dst_cap is ever written.
 * dst_off, decoded_len, result and info.decoded_bytes are complete in either case: dst_cap = 0 is a size query at decode speed (dst may
 * then be NULL), and a second call with dst_cap = decoded_bytes fits -- it decodes again.
 *
 * Rounds: round_blocks = 0 runs the batch as one round; round_blocks = K > 0 runs ceil(n / K) rounds of at most K blocks through ONE
 * ring of min(K, n) slots of the slot width rounded up to 16 bytes, so the scratch does not grow with n once n > K.  Each round is a
 * normal unknown-size batch decode of its rows into the ring (dst_stride = the slot): the wavefront / lane dispatch rules and the lane
 * decoder's first-use probe apply to the ROUND's size, not to n.  Rounds do not overlap, so they bound memory and cost time (262 144
 * blocks of 64 KiB: 25 ms in one round, 138 ms in rounds of 16 384), and a round of few large blocks leaves most of the
 * device idle: see the frame call below. */
typedef struct lz4hip_compact_info {
    int64_t blocks;          /* n */
    int64_t decoded_bytes;   /* dst_off[n]: the bytes the whole batch decodes to, whatever dst_cap was */
    int64_t written_blocks;  /* leading blocks that lie wholly inside dst_cap (n when all do) */
    int64_t first_failed;    /* lowest index with a NEGATIVE result, -1 if none */
    int32_t error, reserved; /* that block's result, 0 if none */
} lz4hip_compact_info_t;

/* Device scratch (bytes) of the device call; 0 for an empty batch, non-decreasing in n_blocks and the same for every
 * n_blocks >= round_blocks > 0.  LZ4HIP_E_ARGUMENT for slot_bytes <= 0 or round_blocks < 0. */
int64_t lz4hip_decode_compact_scratch_bytes(int64_t n_blocks, int32_t slot_bytes, int64_t round_blocks);
/* Device-resident batch: the contract of the other device calls -- device pointers of the CURRENT device, launch-only on `stream`, no
 * device value read on the host, no allocation beyond what the block decoder itself does on first use, scratch from the caller, 0 or
 * LZ4HIP_E_* returned.  Arguments are checked first: a NULL batch or dst_off, a negative n_blocks, dst_cap or round_blocks,
 * dst_cap_all <= 0, too little scratch or more than 2^31 - 1 blocks in a round is LZ4HIP_E_ARGUMENT whatever the device.  An empty
 * batch writes dst_off[0] = 0 and an info with first_failed = -1. */
int lz4hip_decode_compact_device(const lz4hip_batch_t* b, int64_t round_blocks,
                                 void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* decoded_len,
                                 void* scratch, int64_t scratch_bytes, lz4hip_compact_info_t* info, void* stream);
/* Host-resident batch: every pointer is host memory.  Gathers the rows, stages them with their lengths and limits through device
 * memory (per-thread, grow-only, freed by lz4hip_release_workspaces), runs the device call, reads info and the per-block arrays back
 * and copies only min(decoded_bytes, dst_cap) bytes of output.  The arguments are checked as the device call checks them, before the
 * device is looked for.  Returns 0 (block failures are in result and info) or LZ4HIP_E_*. */
int lz4hip_decode_compact_host(const lz4hip_batch_t* b, int64_t round_blocks,
                               void* dst, int64_t dst_cap, int64_t* dst_off, int32_t* decoded_len,
                               lz4hip_compact_info_t* info);

/* ---- legacy frames ---------------------------------------------------------------------------------
 * The frame of the demo command-line tool that ships with the reference (original/lz4demo.c:84-87, 167-317): the format files
 * written by that tool (and by lz4 before r120) arrive in; files from current tools use the LZ4 frame further down:
 *     LE32 magic 0x184C2102   { LE32 compressedSize  payload }*
 * The writer cuts a source of src_len bytes into ceil(src_len / chunk_size) chunks (8 MiB in the tool) and compresses each with
 * LZ4_compress / LZ4_compressHC into an LZ4_compressBound buffer; an empty source is the 4 magic bytes alone.  The reader checks the
 * magic, skips a size field that equals the magic (the header of an appended frame) and decodes every payload with
 * LZ4_uncompress_unknownOutputSize(in, out, size, chunk_size); a negative result ends the read.  An empty chunk (size field 0) decodes
 * to 0 bytes, as it does there.  chunk_size: 0 means 8 MiB, 1 .. 0x7E000000 (LZ4_MAX_INPUT_SIZE) is taken as given, anything else is
 * LZ4HIP_E_ARGUMENT.  Frame-level outcomes (lz4hip_frame_info_t.error): */
#define LZ4HIP_FRAME_OK            0
#define LZ4HIP_FRAME_BAD_MAGIC     1   /* fewer than 4 bytes, or the first 4 are not the magic ("Unrecognized header") */
#define LZ4HIP_FRAME_TRUNCATED     2   /* 1-3 bytes where a size field should be, or a payload that runs past the end   */
#define LZ4HIP_FRAME_BAD_SIZE      3   /* a size field above the compressBound of chunk_size: more than the writer can produce
                                          and than the reference reader's buffer holds; tested BEFORE the truncation rule */
#define LZ4HIP_FRAME_CORRUPT_BLOCK 4   /* a chunk did not decode into <= chunk_size bytes ("Decoding Failed ! Corrupted input !") */
#define LZ4HIP_FRAME_TABLE_FULL    5   /* more chunks than max_chunks; .chunks = the count needed */
typedef struct lz4hip_frame_info {
    int64_t chunks;         /* chunks before the first header error (all of them, also when the table is full) */
    int64_t decoded_bytes;  /* dst_off[chunks]: the sum of the caps; the output buffer's size */
    int64_t good_bytes;     /* what a sequential reader has written when it stops: dst_off[first bad chunk], decoded_bytes if none */
    int64_t error_offset;   /* frame offset of the failing size field (BAD_MAGIC: 0; TABLE_FULL: of the first chunk that did not fit), -1 if none */
    int32_t error, reserved;
} lz4hip_frame_info_t;

/* Bytes a frame can take: 4 + sum over the chunks of (4 + compressBound(len_k)); 4 for an empty source. */
int64_t lz4hip_frame_bound(int64_t src_len, int32_t chunk_size);
/* Device scratch (bytes) of the device calls below.  The encoder's includes one compressBound slot per chunk; an empty source still
 * needs its few hundred bytes. */
int64_t lz4hip_frame_encode_scratch_bytes(int64_t src_len, int32_t chunk_size);
int64_t lz4hip_frame_decode_scratch_bytes(int64_t max_chunks);

/* Device-resident frames: the contract of the LZ4Stream device calls -- device pointers of the CURRENT device, launch-only on `stream`
 * (a hipStream_t, NULL = default stream), no device value read on the host, no allocation, scratch from the caller, 0 or LZ4HIP_E_*
 * returned.  Arguments are checked first: LZ4HIP_E_ARGUMENT for them holds whatever the device.  The first-use exceptions of
 * lz4hip_encode_batch_device / lz4hip_decode_batch_device, which these calls run on the chunks, apply.
 *
 * Encode: writes the frame to dst (dst_cap >= lz4hip_frame_bound, else LZ4HIP_E_ARGUMENT) and its length to *dst_len (device).  With
 * a compressBound capacity the block encoder cannot fail, so there is no per-chunk failure. */
int lz4hip_frame_encode_device(const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap,
                               int64_t* dst_len, void* scratch, int64_t scratch_bytes, void* stream);
/* Decode is two calls; the caller reads *info back between them (one synchronisation) to learn the chunk count and the output size.
 * Index: walks the size fields of src[0, src_len) into a table of max_chunks rows in scratch, finds every chunk's decoded size without
 * decoding it (as lz4hip_decoded_sizes_device does) and writes *info (device).  A chunk whose size walk fails or exceeds chunk_size
 * -- the chunk the reference's reader fails on -- is a bad chunk: it takes 0 bytes of the output, so its neighbours pack around it,
 * and turns the outcome into LZ4HIP_FRAME_CORRUPT_BLOCK at the LOWEST such chunk's size field; that always wins over the header
 * error, which lies after every chunk in the table.  With more chunks than max_chunks, info.error = LZ4HIP_FRAME_TABLE_FULL and
 * info.chunks is the count needed.
 * Decode: given the info the index reported (host copy) and the same scratch and max_chunks, decodes every chunk before the first header
 * error, bad ones excepted, into dst[0, decoded_bytes) -- exactly the decoded size, no slot per chunk -- and writes *info (device)
 * again: a chunk that walked to a size but breaks the format's end rules fails in the decoder and is a bad chunk too.  A bad chunk
 * never disturbs another chunk's bytes and no byte outside [0, decoded_bytes) is written.  LZ4HIP_E_ARGUMENT for an info_host with
 * TABLE_FULL, counts that do not fit max_chunks, or decoded_bytes > dst_cap. */
int lz4hip_frame_index_device(const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks,
                              void* scratch, int64_t scratch_bytes, lz4hip_frame_info_t* info, void* stream);
int lz4hip_frame_decode_device(const void* src, const lz4hip_frame_info_t* info_host, int64_t max_chunks,
                               void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                               lz4hip_frame_info_t* info, void* stream);

/* Decode in ONE call, with no value read on the host: the size field walk into a table of max_chunks rows, then
 * lz4hip_decode_compact_device over all max_chunks rows -- slot and limit chunk_size; the rows past the frame's count are empty
 * blocks -- straight into dst, then *info (device): chunks; decoded_bytes, the total; good_bytes, dst_off of the lowest chunk with a
 * negative decoder result; and the error in the index's precedence: LZ4HIP_FRAME_TABLE_FULL, then LZ4HIP_FRAME_CORRUPT_BLOCK at the
 * lowest bad chunk's size field, then the walk's header error.  A bad chunk takes 0 bytes and its neighbours pack around it.  dst_cap is
 * any value >= 0 and clips as it does there: chunk k is written iff the offset after it is <= dst_cap, nothing at or past dst_cap is
 * written, and decoded_bytes is complete either way (dst_cap = 0: a size query at decode speed).  On TABLE_FULL the contents of dst are
 * unspecified: the caller grows the table to info.chunks and calls again.
 *
 * Every chunk gets chunk_size bytes of room, which is exactly the reference's reader (original/lz4demo.c:276-300:
 * LZ4_uncompress_unknownOutputSize(in, out, size, chunk_size)).  The two-call path above decodes a chunk at the capacity its size walk
 * found and is therefore STRICTER than that reader: a chunk that breaks the format's end rules without being cut short -- one whose
 * last sequence is only legal because the output limit lies further on -- is a bad chunk there and decodes here as it does in the
 * reference.
 *
 * round_chunks is lz4hip_decode_compact_device's round_blocks.  The ring of round_chunks = 0 is max_chunks slots of chunk_size bytes
 * (rounded up to 16), which is large at 8 MiB chunks; rounds shrink it to round_chunks slots, but rounds do not overlap and a round
 * of few large chunks leaves most of the device idle (one wavefront decodes one 8 MiB chunk): a 1 GiB frame of 8 MiB chunks took
 * 230 ms in one round and 1.8 s in rounds of 16 on an MI355X.
 * Scratch: lz4hip_frame_decode_compact_scratch_bytes, LZ4HIP_E_ARGUMENT for arguments the call refuses.  The arguments are checked
 * first, whatever the device: negative sizes, a bad chunk_size, NULL src (with src_len > 0), scratch, info or dst (with dst_cap > 0),
 * too little scratch. */
int64_t lz4hip_frame_decode_compact_scratch_bytes(int32_t chunk_size, int64_t max_chunks, int64_t round_chunks);
int lz4hip_frame_decode_compact_device(const void* src, int64_t src_len, int32_t chunk_size, int64_t max_chunks, int64_t round_chunks,
                                       void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                       lz4hip_frame_info_t* info, void* stream);

/* Host-resident frames: stage the whole buffer through device memory (per-thread, grow-only, freed by lz4hip_release_workspaces), run
 * the device calls above and synchronise.  Encode returns 0 or LZ4HIP_E_* (dst_cap >= lz4hip_frame_bound); *dst_len on the host.
 * Decode returns info->error (0 or a positive LZ4HIP_FRAME_* code, with dst[0, decoded_bytes) filled) or LZ4HIP_E_*; with dst_cap below
 * the decoded size it returns LZ4HIP_E_ARGUMENT with *info filled in (a size query: dst_cap = 0). */
int lz4hip_frame_encode_host(const void* src, int64_t src_len, int32_t chunk_size, int mode, void* dst, int64_t dst_cap, int64_t* dst_len);
int lz4hip_frame_decode_host(const void* src, int64_t src_len, int32_t chunk_size, void* dst, int64_t dst_cap, lz4hip_frame_info_t* info);

/* ---- xxHash32 of rows, and LZ4 frames (magic 0x184D2204) on the device ---------------------------------------------------------------
 * lz4hip_xxh32_rows_device: XXH32 with `seed` of n_rows rows of device bytes, row i at data + (off ? off[i] : i * stride) with length
 * len ? len[i] : len_all (a negative length counts as 0), one uint32 per row into sums (device).  Four lanes per row, sixteen rows
 * per wavefront; a single long row runs at the latency of its four chains, whatever the device.  Launch-only on `stream`; no byte
 * outside a row is read.  0 or LZ4HIP_E_*; the arguments are checked before the device is looked for. */
int lz4hip_xxh32_rows_device(const void* data, const int64_t* off, int64_t stride, const int32_t* len, int64_t len_all, uint32_t seed,
                             uint32_t* sums, int64_t n_rows, void* stream);

/* The LZ4 frame format (LZ4 Frame format v1.6.x): what `lz4`, LZ4F_compressFrame, K4os.Compression.LZ4.Streams and python-lz4 write.
 *     LE32 0x184D2204  FLG  BD  [LE64 contentSize]  HC   { LE32 blockSize  data  [LE32 xxh32(data)] }*   LE32 0   [LE32 xxh32(content)]
 * The contract is that of the lz4hip_frame_*_device calls: device pointers of the current device, launch-only on the caller's stream,
 * no device value read on the host, no allocation, scratch from the caller (the *_scratch_bytes queries), arguments checked before the
 * device is looked for, 0 or LZ4HIP_E_* returned.
 *
 * Encode flags: */
#define LZ4HIP_LZ4F_BLOCK_CHECKSUM   1u   /* FLG.4: xxh32 of every block's stored bytes                                      */
#define LZ4HIP_LZ4F_CONTENT_CHECKSUM 2u   /* FLG.2: xxh32 of the whole source -- ONE row of the checksum kernel, serial work */
#define LZ4HIP_LZ4F_CONTENT_SIZE     4u   /* FLG.3: the source's length in the descriptor (omitted for an empty source)      */
/* Decode flags: which of the checksums the frame carries are verified */
#define LZ4HIP_LZ4F_VERIFY_BLOCKS    1u
#define LZ4HIP_LZ4F_VERIFY_CONTENT   2u   /* one serial row over dst[0, decoded_bytes): only when all of it was written and no block is bad */
/* ... and an opt-in of the four decode calls (lz4hip_lz4f_decode_* and lz4hip_lz4f_batch_decode_*): frames whose blocks are LINKED
 * (FLG.5 clear -- the default of LZ4F_compressFrame, python-lz4 and Arrow's LZ4_FRAME codec for content above one block) are decoded
 * instead of refused with UNSUPPORTED_LINKED.  Without the flag every call is what it was; these four calls refuse frames with a dictionary ID either way (lz4hip_lz4f_*_dict_* take them).
 * COST: a linked frame is ONE serial chain and runs on ONE wavefront, so one large linked frame decodes far slower than on a host core
 * (INTEGRATION.md 4 has a lone wavefront's figures).  The flag pays only in batches of many items, one wavefront each.  With it:
 *  - an independent frame or item takes the path it always took: the same bytes, the same record;
 *  - a linked one yields what a sequential reader (LZ4F_decompress) yields.  A match may start anywhere in the bytes of the SAME frame
 *    already produced, earlier blocks (stored-raw ones included) up to 65 535 back, never before the frame's first output byte
 *    whatever dst holds there: that is a corrupt block;
 *  - the first bad block ends a linked item, as it ends a sequential read.  A block known bad before the layout -- a checksum mismatch
 *    under VERIFY_BLOCKS, a size walk that fails, a size above the frame's block maximum -- takes 0 bytes and so does every block of
 *    the item behind it: BLOCK_CHECKSUM_ERROR or CORRUPT_BLOCK at that block's size field, good_bytes what lay before it.  A block
 *    that walks to a size but that the decoder then refuses (a match that starts before the frame; the end rules broken at its own
 *    size, the caveat of the two-call legacy frame path above) KEEPS its place: CORRUPT_BLOCK at its size field, good_bytes the
 *    item's bytes before it, the item's blocks behind it not touched, the item's bytes from good_bytes on unspecified.  No other item's
 *    bytes or record are disturbed.  Such a block is only found when it is reached: not behind the dst_cap clip, so not in a size query;
 *  - dst_cap clips a linked item at a BLOCK boundary: its blocks that lie wholly inside dst_cap are written, the first one that does
 *    not and those behind it are not (an independent item keeps the byte-exact clip).  Nothing at or past dst_cap is written; offsets,
 *    sizes and decoded_bytes are complete either way, dst_cap = 0 is the size query, written_items and "present but not checked" are
 *    as ever; VERIFY_CONTENT covers linked items;
 *  - the *_decode_scratch_bytes values include one more int32 per table row, flag or no flag. */
#define LZ4HIP_LZ4F_ACCEPT_LINKED    8u   /* (4u is not a decode flag and stays refused as an unknown one, as callers have pinned it) */
/* Outcomes (lz4hip_lz4f_info_t.error).  Precedence, as a sequential reader meets them: TABLE_FULL; a descriptor error (no block is
 * walked then); the lowest bad block (BLOCK_CHECKSUM_ERROR / CORRUPT_BLOCK, at its size field); the walk's error (TRUNCATED /
 * BAD_BLOCK_SIZE: it lies after every tabled block); CONTENT_SIZE_ERROR; CONTENT_CHECKSUM_ERROR. */
#define LZ4HIP_LZ4F_OK                     0
#define LZ4HIP_LZ4F_BAD_MAGIC              1   /* fewer than 4 bytes, or neither the frame magic nor a skippable one */
#define LZ4HIP_LZ4F_BAD_HEADER             2   /* version, a reserved bit, or a block size id below 4 */
#define LZ4HIP_LZ4F_HEADER_CHECKSUM        3
#define LZ4HIP_LZ4F_UNSUPPORTED_LINKED     4   /* FLG.5 clear: linked blocks decode only in order, each against the 64 KiB before it (LZ4HIP_LZ4F_ACCEPT_LINKED takes them) */
#define LZ4HIP_LZ4F_UNSUPPORTED_DICT       5   /* FLG.0 set, in a call without a dictionary: lz4hip_lz4f_decode_dict_* and lz4hip_lz4f_batch_decode_dict_* take such frames */
#define LZ4HIP_LZ4F_SLOT_TOO_SMALL         6   /* the frame's block maximum exceeds slot_bytes: call again with .block_max */
#define LZ4HIP_LZ4F_TRUNCATED              7   /* the frame ends inside the descriptor, a size field, data, a checksum, or before its EndMark */
#define LZ4HIP_LZ4F_BAD_BLOCK_SIZE         8   /* a size field above the frame's block maximum (tested before the truncation rule) */
#define LZ4HIP_LZ4F_CORRUPT_BLOCK          9   /* a block did not decode into <= the frame's block maximum */
#define LZ4HIP_LZ4F_BLOCK_CHECKSUM_ERROR   10
#define LZ4HIP_LZ4F_CONTENT_SIZE_ERROR     11
#define LZ4HIP_LZ4F_CONTENT_CHECKSUM_ERROR 12
#define LZ4HIP_LZ4F_TABLE_FULL             13  /* more blocks than max_blocks; .blocks = the count needed */
#define LZ4HIP_LZ4F_DICT_ID_MISMATCH       14  /* the dictionary calls: the descriptor's dictionary ID is not the non-zero dict_id of the call (a descriptor error, at the ID field) */
#define LZ4HIP_LZ4F_KIND_FRAME     0
#define LZ4HIP_LZ4F_KIND_SKIPPABLE 1           /* magic 0x184D2A50 .. 0x184D2A5F: frame_bytes = 8 + its size, no output */
typedef struct lz4hip_lz4f_info {
    int64_t blocks;          /* data blocks in the frame */
    int64_t decoded_bytes;   /* bytes of all good blocks: the size dst needs (a bad block takes 0 bytes, its neighbours pack around it) */
    int64_t good_bytes;      /* what a sequential reader had written when it stopped */
    int64_t error_offset;    /* where in the frame the outcome was met, -1 for none */
    int64_t content_size;    /* the descriptor's, -1 if absent */
    int64_t frame_bytes;     /* everything up to and including the content checksum: an appended frame starts there (meaningful without a walk error) */
    int32_t error;           /* LZ4HIP_LZ4F_* */
    int32_t kind;            /* LZ4HIP_LZ4F_KIND_* */
    int32_t block_max;       /* the frame's block maximum in bytes (0: the descriptor did not parse) */
    int32_t flg, bd;         /* the descriptor's bytes */
    int32_t checks;          /* bits 0-1: block checksums, bits 2-3: content checksum; 0 absent, 1 verified, 2 present but not checked */
} lz4hip_lz4f_info_t;

/* Upper bound of a frame of src_len bytes (every block stored raw); LZ4HIP_E_ARGUMENT for a block_size_id other than 0, 4 .. 7 or an
 * unknown flag.  block_size_id: 4 = 64 KiB, 5 = 256 KiB, 6 = 1 MiB, 7 = 4 MiB; 0 means 4, the format library's default. */
int64_t lz4hip_lz4f_bound(int64_t src_len, int block_size_id, unsigned flags);
int64_t lz4hip_lz4f_encode_scratch_bytes(int64_t src_len, int block_size_id);
/* slot_bytes: the caller's bound on the frame's block maximum (it sizes the ring): 65536, 262144, 1048576, 4194304, or 0 = 4194304;
 * max_blocks >= 1 table rows; round_blocks as in lz4hip_decode_compact_device (0: one round) */
int64_t lz4hip_lz4f_decode_scratch_bytes(int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks);

/* Encode one frame: independent blocks, no dictionary, a block that does not shrink stored raw (the format library's rule: the block
 * encoder gets length - 1 bytes of room).  mode: LZ4HIP_MODE_FAST or LZ4HIP_MODE_HC, the same format either way.  dst_cap >=
 * lz4hip_lz4f_bound; the frame's length goes to *dst_len (device).  The bytes differ from liblz4's (another parse), the descriptor's
 * do not; every conforming reader reads them. */
int lz4hip_lz4f_encode_device(const void* src, int64_t src_len, int block_size_id, int mode, unsigned flags, void* dst, int64_t dst_cap,
                              int64_t* dst_len, void* scratch, int64_t scratch_bytes, void* stream);
/* Decode ONE frame (or skip one skippable frame) at src in one call: the walk over the size fields (one wavefront, one dependent load
 * per block), the block checksums, the compact decode of every block through a ring of slot_bytes slots -- a raw block is copied from
 * the source -- packed back to back into dst and clipped at dst_cap (any value >= 0; 0 is a size query), the content size and the
 * content checksum.  *info (device) receives the record.  Appended frames are the caller's loop over info.frame_bytes.  One wavefront
 * decodes one block: a frame of 4 MiB blocks decodes like the legacy frame's 8 MiB chunks. */
int lz4hip_lz4f_decode_device(const void* src, int64_t src_len, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags,
                              void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info, void* stream);
/* Host-pointer forms, staged like lz4hip_frame_*_host.  Encode returns 0 or LZ4HIP_E_*; *dst_len on the host.  Decode returns
 * info->error (0 or a positive LZ4HIP_LZ4F_* code, with dst[0, decoded_bytes) filled) or LZ4HIP_E_*; with dst_cap below the decoded
 * size only *info is filled and LZ4HIP_E_ARGUMENT returned (dst_cap = 0: a size query). */
int lz4hip_lz4f_encode_host(const void* src, int64_t src_len, int block_size_id, int mode, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_len);
int lz4hip_lz4f_decode_host(const void* src, int64_t src_len, unsigned flags, void* dst, int64_t dst_cap, lz4hip_lz4f_info_t* info);

/* ---- LZ4 frames decoded with a dictionary ------------------------------------------------------------
 * LZ4F_decompress_usingDict (frames of LZ4F_compressFrame_usingCDict, K4os streams with a dictionary): the four decode calls, argument
 * for argument, with ONE dictionary dict[0, dict_len) per call and the ID the caller expects behind the source arguments.  The one-frame
 * forms are here, the batch forms behind lz4hip_lz4f_batch_decode_host below.
 *   - The dictionary's bytes count as lying immediately in front of the first output byte of EVERY frame of the call, whether or not
 *     the frame's descriptor carries a dictionary ID (FLG.0).
 *   - An INDEPENDENT frame (FLG.5 set): every block sees the dictionary and only the dictionary, never the block before it.  Block k's
 *     result and bytes are what lz4hip_decode_batch_dict_device gives that block.
 *   - A LINKED frame (it needs LZ4HIP_LZ4F_ACCEPT_LINKED, as ever): a match at item offset p with offset o > p reads
 *     dict[dict_len - (o - p)], legal if and only if o - p <= dict_len.  A source before the dictionary's first byte is what a source
 *     before the frame is in the plain calls: the decoder refuses that block, which keeps its planned place -- CORRUPT_BLOCK at its size
 *     field, good_bytes the bytes before it.  Once 65 535 bytes of the item lie in front of a block the dictionary is out of reach.
 *   - Only the dictionary's last 65 535 bytes are ever read, and nothing outside [dict, dict + dict_len).  Any alignment.  The device
 *     calls do not copy it: it must stay valid until the kernels have run.  The host calls upload those last min(dict_len, 65 535)
 *     bytes once per call, into staging apart from the call's image.
 *   - dict_id == 0: no check.  Otherwise a frame whose descriptor carries a DIFFERENT ID gets LZ4HIP_LZ4F_DICT_ID_MISMATCH in the place
 *     of UNSUPPORTED_DICT -- after the header checksum, before the linked check and the slot check; no block is walked; error_offset is
 *     the ID field's (6, or 14 behind a content size).  A frame without an ID is accepted whatever dict_id is.
 *   - dict_len == 0: dict may be NULL, dict_id is ignored and the call IS the plain call, record for record and byte for byte,
 *     UNSUPPORTED_DICT for frames with an ID included.  dict_len < 0, or dict == NULL with dict_len > 0: LZ4HIP_E_ARGUMENT, checked
 *     before a device is looked for.
 *   - Scratch (the plain calls' *_decode_scratch_bytes queries), flags, the clipping, the size query, written_items, the checksum
 *     verdicts and the precedence of outcomes are the plain calls'.
 * COST: the rounds of a dictionary call decode EVERY compressed independent block with one wavefront per block at every batch size, as
 * lz4hip_decode_batch_dict_device does (the lane mapping has no dictionary mode): lz4hip_dispatch_counts moves LZ4HIP_K_DECODE_WAVE only,
 * and a large batch decodes at that mapping's rate.  Linked items run one wavefront each, as in the plain calls.
 * Out of scope: a dictionary per item; the lane mapping for dictionary rows; span forms.  (Encoding frames with a dictionary:
 * lz4hip_lz4f_encode_dict_* and lz4hip_lz4f_batch_encode_dict_*, below.) */
int lz4hip_lz4f_decode_dict_device(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int32_t slot_bytes,
                                   int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                   lz4hip_lz4f_info_t* info, void* stream);
int lz4hip_lz4f_decode_dict_host(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, unsigned flags, void* dst,
                                 int64_t dst_cap, lz4hip_lz4f_info_t* info);

/* ---- batches of LZ4 frames ---------------------------------------------------------------------------
 * Many independent frames per call, in the layout of the lz4hip_streams_* and lz4hip_wrap_* calls: one buffer src of src_len bytes plus
 * device offsets src_off[n + 1]; item i is src[src_off[i], src_off[i + 1]); outputs lie back to back in dst with dst_off[n + 1] (device),
 * so one call's output is the other's input.  The contract is that of lz4hip_lz4f_*_device: device pointers of the current device,
 * launch-only on the caller's stream, no device value read on the host, no allocation, scratch from the caller (the *_scratch_bytes
 * queries), arguments checked before the device is looked for, 0 or LZ4HIP_E_* returned.
 *
 * Out of scope: a dictionary per item (one per call: lz4hip_lz4f_batch_decode_dict_*; without one a frame with a dictionary ID is refused,
 * the item's outcome says so; frames with linked blocks are the caller's choice: LZ4HIP_LZ4F_ACCEPT_LINKED); following appended frames inside one item (an
 * item is ONE frame, what lies behind it is left alone and shows only in frame_bytes); span forms (chosen items of an arena); a block
 * decoder for large blocks -- one wavefront still decodes one block.
 *
 * Encode: every item becomes the frame lz4hip_lz4f_encode_device writes for that item alone with the same block_size_id, mode and
 * flags, byte for byte (an empty item's frame carries no content size).  The offsets are device values, so the block table is sized by
 * the bound src_len / block + n; ONE block encoder call runs over the blocks of all items, the block checksums are rows of one
 * checksum launch and the n content checksums n rows of another.  dst_cap >= lz4hip_lz4f_batch_bound.  An item whose offsets decrease
 * or leave [0, src_len] takes 0 bytes, as in lz4hip_streams_encode_device. */
int64_t lz4hip_lz4f_batch_bound(int64_t n, int64_t src_len, int block_size_id, unsigned flags);
int64_t lz4hip_lz4f_batch_encode_scratch_bytes(int64_t n, int64_t src_len, int block_size_id);
int lz4hip_lz4f_batch_encode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int mode, unsigned flags,
                                    void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes, void* stream);

/* Decode: ONE frame per item.  item_info[n] (device) receives one lz4hip_lz4f_info_t per item, and dst[dst_off[i], dst_off[i + 1]) its
 * bytes: what lz4hip_lz4f_decode_device gives for that item alone with a table and a dst_cap that hold it, every field, offsets relative
 * to the item's start -- a skippable item (kind, 0 bytes), UNSUPPORTED_LINKED (without LZ4HIP_LZ4F_ACCEPT_LINKED), UNSUPPORTED_DICT and SLOT_TOO_SMALL as the ITEM's outcome,
 * trailing bytes behind frame_bytes left alone.  A failing item never disturbs another item's bytes or record; an item whose offsets
 * decrease or leave [0, src_len] gets error = LZ4HIP_E_ARGUMENT and 0 bytes.  The walks run one wavefront per item, the content
 * checksums as n rows of one checksum launch.
 * max_blocks sizes the table for the WHOLE batch and slot_bytes bounds every item's block maximum; the block decoder picks its mapping
 * by the rows it is handed, so size max_blocks to the batch (a table many times too large decodes a small batch with the mapping of a
 * large one).  With more blocks than max_blocks: info.error = LZ4HIP_LZ4F_TABLE_FULL, info.blocks = the count needed, every item's
 * error is TABLE_FULL and nothing is written to dst.
 * dst_cap clips by position, as in the one-frame call (0 is a size query): nothing at or past dst_cap is written, *written_items
 * (device) = the prefix of items that lie wholly inside dst_cap, the content checksum of an item not wholly written is "present but not
 * checked", dst_off and decoded_bytes are complete all the same. */
typedef struct lz4hip_lz4f_batch_info {
    int64_t items;
    int64_t blocks;          /* data blocks of all items: the rows the table needs */
    int64_t decoded_bytes;   /* dst_off[n]: the size dst needs */
    int64_t first_error;     /* the lowest failing item (what a sequential loop over the items raises first), -1 if none */
    int64_t error_offset;    /* that item's error_offset, relative to the item's start; -1 if none */
    int32_t error;           /* that item's error, LZ4HIP_LZ4F_TABLE_FULL for a table that is too small, 0 if no item failed */
    int32_t reserved;
} lz4hip_lz4f_batch_info_t;
int64_t lz4hip_lz4f_batch_decode_scratch_bytes(int64_t n, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks);
int lz4hip_lz4f_batch_decode_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int32_t slot_bytes, int64_t max_blocks,
                                    int64_t round_blocks, unsigned flags, void* scratch, int64_t scratch_bytes, void* dst, int64_t dst_cap,
                                    int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info, int64_t* written_items,
                                    void* stream);
/* Host-pointer forms, staged like lz4hip_streams_*_host: one device image, results out; offsets that decrease or leave [0, src_len] are
 * refused.  Encode returns 0 or LZ4HIP_E_*.  Decode sizes its slots by the largest block maximum among the items' descriptors and
 * returns 0, the first failing item's code (dst, dst_off, item_info and info filled), or LZ4HIP_E_*; with dst_cap below the decoded size
 * it returns LZ4HIP_E_ARGUMENT with dst_off, item_info and info filled in (dst_cap = 0: a size query). */
int lz4hip_lz4f_batch_encode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, int block_size_id, int mode, unsigned flags,
                                  void* dst, int64_t dst_cap, int64_t* dst_off);
int lz4hip_lz4f_batch_decode_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, unsigned flags, void* dst, int64_t dst_cap,
                                  int64_t* dst_off, lz4hip_lz4f_info_t* item_info, lz4hip_lz4f_batch_info_t* info);
/* The batch decode with ONE dictionary for all items ("LZ4 frames decoded with a dictionary", above: the contract is there).  A
 * DICT_ID_MISMATCH is the ITEM's outcome, as UNSUPPORTED_LINKED is. */
int lz4hip_lz4f_batch_decode_dict_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len,
                                         uint32_t dict_id, int32_t slot_bytes, int64_t max_blocks, int64_t round_blocks, unsigned flags, void* scratch,
                                         int64_t scratch_bytes, void* dst, int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info,
                                         lz4hip_lz4f_batch_info_t* info, int64_t* written_items, void* stream);
int lz4hip_lz4f_batch_decode_dict_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                       unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, lz4hip_lz4f_info_t* item_info,
                                       lz4hip_lz4f_batch_info_t* info);

/* ---- LZ4 frames encoded with a dictionary -----------------------------------------------------------------
 * LZ4F_compressFrame_usingCDict with independent blocks, and K4os' streams with a dictionary: lz4hip_encode_batch_dict_device under the
 * frame rounds.  The argument order mirrors the decode side: dict, dict_len, dict_id go behind the source arguments.
 *   MODE: fast mode only -- there is no `mode` argument.  LZ4HC against a dictionary is out of scope.
 *   BLOCKS: independent (FLG.5 is set).  Every block is encoded against the SAME dictionary and never sees the block before it, which is
 * what LZ4F_compressFrame_usingCDict does with independent blocks.  The raw-store rule is the plain frame encoder's: the block encoder
 * gets length - 1 bytes of room, and a result of 0 stores the block raw.
 *   BLOCK BYTES: block k's bytes are exactly what lz4hip_encode_batch_dict_device writes for that block with dst_cap = len - 1 and the
 * same dictionary -- the parse that call's section defines.  The frame therefore decodes with lz4hip_lz4f_decode_dict_* and with
 * LZ4F_decompress_usingDict.
 *   dict_id != 0: FLG.0 is set and the 4-byte little-endian ID sits behind the content size (behind BD when there is no size); the HC
 * byte is computed over it; the descriptor is 4 bytes longer, 11 or 19 bytes.  dict_id == 0: no ID is written, as liblz4 does for
 * dictID = 0; the dictionary is still used.
 *   DICTIONARY: only its last 65 535 bytes are read, and nothing outside [dict, dict + dict_len); any alignment; the device calls do not
 * copy it.  dict_len == 0: dict may be NULL, dict_id is ignored, and the call IS lz4hip_lz4f_encode_device /
 * lz4hip_lz4f_batch_encode_device with LZ4HIP_MODE_FAST, byte for byte; the two bounds and the two scratch queries return the plain
 * queries' values.
 *   ARGUMENTS: dict_len < 0, dict == NULL with dict_len > 0, an unknown flag, a bad block_size_id, dst_cap below the bound and scratch
 * below the query return LZ4HIP_E_ARGUMENT, checked before a device is looked for.
 *   DEVICE CALLS: launch-only on `stream`; they read no device value on the host and allocate nothing.  The 16 KiB primed table lives in
 * the caller's scratch (the query includes it when dict_len > 0) and is built once per call by encode_dict_prime_kernel, before the block
 * encoder runs (a one-frame call with an empty source has no block and primes nothing).
 *   BATCH: item i's frame is byte for byte what the one-frame dictionary call writes for that item alone; an empty item carries no
 * content size; an item with bad offsets takes 0 bytes; one dictionary and one ID serve the whole call; ONE block encoder launch runs over
 * the blocks of all items.
 *   HOST FORMS: the dictionary's reachable tail goes up once per call, into staging apart from the image; the table is primed once; the
 * device sequence runs over one image.  Offsets that decrease or leave [0, src_len] are refused, as in lz4hip_lz4f_batch_encode_host.
 *   COST: as lz4hip_encode_batch_dict_device -- the wavefront mapping at every batch size, in workgroups of one or five blocks;
 * lz4hip_dispatch_counts moves LZ4HIP_K_ENCODE_WAVE only; there is no lane mapping.
 * Out of scope: LZ4HC with a dictionary; linked-block frames on the encode side; a dictionary per item; a _multi host form; the packed
 * encode form with a dictionary; the lane mapping for dictionary rows. */
int64_t lz4hip_lz4f_dict_bound(int64_t src_len, int block_size_id, unsigned flags, int64_t dict_len, uint32_t dict_id);
int64_t lz4hip_lz4f_encode_dict_scratch_bytes(int64_t src_len, int block_size_id, int64_t dict_len);
int lz4hip_lz4f_encode_dict_device(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int block_size_id, unsigned flags,
                                   void* dst, int64_t dst_cap, int64_t* dst_len, void* scratch, int64_t scratch_bytes, void* stream);
int lz4hip_lz4f_encode_dict_host(const void* src, int64_t src_len, const void* dict, int64_t dict_len, uint32_t dict_id, int block_size_id, unsigned flags,
                                 void* dst, int64_t dst_cap, int64_t* dst_len);
int64_t lz4hip_lz4f_batch_dict_bound(int64_t n, int64_t src_len, int block_size_id, unsigned flags, int64_t dict_len, uint32_t dict_id);
int64_t lz4hip_lz4f_batch_encode_dict_scratch_bytes(int64_t n, int64_t src_len, int block_size_id, int64_t dict_len);
int lz4hip_lz4f_batch_encode_dict_device(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                         int block_size_id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off, void* scratch, int64_t scratch_bytes,
                                         void* stream);
int lz4hip_lz4f_batch_encode_dict_host(const void* src, int64_t src_len, const int64_t* src_off, int64_t n, const void* dict, int64_t dict_len, uint32_t dict_id,
                                       int block_size_id, unsigned flags, void* dst, int64_t dst_cap, int64_t* dst_off);

/* ---- diagnostics ---------------------------------------------------------------------------------
 * Launch counters per kernel family since the library was loaded: which block->hardware mapping a call
 * actually used (the GPU tests assert these).  Copies min(n, LZ4HIP_K_COUNT) counters, returns LZ4HIP_K_COUNT. */
#define LZ4HIP_K_DECODE_WAVE 0   /* lz4hip_decode.hpp:         one wavefront per block */
#define LZ4HIP_K_DECODE_LANE 1   /* lz4hip_decode_lane4.hpp:   one lane per block      */
#define LZ4HIP_K_ENCODE_WAVE 2
#define LZ4HIP_K_ENCODE_LANE 3
#define LZ4HIP_K_HC_WAVE     4
#define LZ4HIP_K_HC_LANE     5
#define LZ4HIP_K_COUNT       6
int lz4hip_dispatch_counts(uint64_t* counts, int n);

/* Named integer knobs for tests, A/B runs and deployment tuning.  Every knob takes its initial value from the
 * environment variable in brackets ONCE, when the library first looks at a knob; the launch paths never call getenv().
 *   "decoder", "encoder", "hc"   [LZ4HIP_DECODER / _ENCODER / _HC = wave | lane]  0 automatic, 1 one wavefront per block,
 *                                 2 one lane per block -- forces that mapping for EVERY block, whatever the batch size
 *   "encoder_waves_per_cu", "hc_waves_per_cu"  [LZ4HIP_ENCODER_WAVES_PER_CU, LZ4HIP_HC_WAVES_PER_CU]  residency of the
 *                                 persistent lane-per-block encoder grids (0 = built-in default)
 *   "hc_groups"                  [LZ4HIP_HC_GROUPS]  wavefronts of the LZ4HC lane grid (0 = from the residency)
 *   "host_threads", "host_slices" [LZ4HIP_HOST_THREADS, LZ4HIP_HOST_SLICES]  host-pointer batches: threads of the process-wide row pool that gathers /
 *                                 scatters rows (0 = a quarter of the hardware threads, at least 8 and at most 64, never more than the host has; read when the pool starts a thread), slices per batch
 *   "decoder_gen", "decoder_ring" [LZ4HIP_DECODER_GEN, LZ4HIP_DECODER_RING]  lane decoder generation (0 default = 4, lz4hip_decode_lane4.hpp;
 *                                 2 and 3 exist only in libraries built with -DLZ4HIP_TUNING_BUILD) and, for generation 4, its
 *                                 configuration: bytes of output ring per lane + 1000 x variant (bit 0: 128-byte flush units,
 *                                 bit 1: 32-byte input pieces, bit 2: one flush store instruction instead of two, bit 3: the flush runs in every second
 *                                 iteration only, bit 4: input pieces are requested in the other iterations only, bit 5: the pieces come out of whole
 *                                 64-byte sectors fetched once; 0 = default 59192; other configurations exist only in tuning builds)
 *   "hc_gen"                     [LZ4HIP_HC_GEN]  LZ4HC lane mapping: 0 default (4 for blocks <= 64 KiB, else 2); 4 the state machine over
 *                                 precomputed chains that carry shared lengths (lz4hip_hc_lcp.hpp), 2 the state machine with the
 *                                 insert loop (lz4hip_hc_conv.hpp: blocks > 64 KiB; smaller ones only in tuning builds); 1 and 3 (one
 *                                 loop nest per lane; precomputed chains without lengths) exist only in -DLZ4HIP_TUNING_BUILD libraries
 *   "hc_ctrl_every", "hc_ctrl_lanes" [LZ4HIP_HC_CTRL_EVERY, LZ4HIP_HC_CTRL_LANES]  generation 4: the parse's control flow runs for all
 *                                 waiting lanes every N-th iteration (a power of two) or as soon as M lanes wait (0 = defaults 8 / 32)
 *   "decoder_persist"            [LZ4HIP_DECODER_PERSIST]  lane decoder: 0 = automatic (one block per lane under hardware dispatch for large batches whose
 *                                 blocks nearly all take the lane mapping; a persistent grid whose lanes pull blocks from a counter for batches of fewer
 *                                 than three residency rounds and for batches with many blocks routed to the wavefront mapping -- counted on the device),
 *                                 1 = always the persistent grid, 2 = never;  "decoder_groups" [LZ4HIP_DECODER_GROUPS]: wavefronts of that grid
 *                                 (0 = the residency; tests use 1 so that every lane restarts hundreds of times)
 *   "hc_sub_chunks"              [LZ4HIP_HC_SUB_CHUNKS]  LZ4HC lane mapping, blocks <= 64 KiB: a chunk of blocks is cut into this many sub-chunks whose
 *                                 table builders and lane kernels overlap on separate streams (0 = default 2, 1 = one after the other, at most 8)
 *   "encoder_slab_tries"         [LZ4HIP_ENCODER_SLAB_TRIES]  fast encoder, lane mapping: its hash tables live in a slab of separately allocated chunks;
 *                                 when the slab is built (first large batch on a device) the library times a probe kernel on it and, if the placement
 *                                 is slower than a well spread one, builds up to this many candidates and keeps the fastest (0 = default 4;
 *                                 1 = the first candidate, unmeasured).  Read-only through lz4hip_tuning_get: "encoder_slab_rate" (what the
 *                                 current device's slab measured, 1000 x G probe steps per second; 0 = none / unmeasured), "encoder_slab_tried" (candidates built),
 *                                 "encoder_slab_chunks" (separate allocations the slab in use consists of)
 *   "host_workers"               [LZ4HIP_HOST_WORKERS]  host-pointer batches of >= 8192 blocks on ONE device (lz4hip_*_batch_host; not LZ4HC) run as this many staging
 *                                 pipelines that share the device -- the persistent workers of the *_multi entry points, block i -> worker i mod k -- so that one pipeline's
 *                                 kernels and copies fill the other's gaps (0 = default: 2 for decode, 1 for fast encode, whose kernels are the bottleneck either way;
 *                                 1 = the calling thread's own pipeline alone; at most 8)
 *   "encoder_wave_version"       [LZ4HIP_ENCODER_WAVE_VERSION]  wavefront-mapped fast encoder, blocks below LZ4_64KLIMIT: 0 = default 2 (encode_fast_block64k, round 6);
 *                                 1 = the first version (exists in -DLZ4HIP_TUNING_BUILD libraries only: A/B runs)
 *   "encoder_wg5"                [LZ4HIP_ENCODER_WG5]  wavefront-mapped fast encoder: 0 = default, workgroups of FIVE blocks (five wavefronts, 80 KiB of LDS; two per CU = ten
 *                                 blocks) wherever that saves the batch a residency round (2 305 - 2 560 blocks, 16 384, everything from 23 040 blocks up on 256 CUs) -- gfx950 hands out LDS in granules of 1 280 bytes, a 16 KiB table takes thirteen of a
 *                                 CU's 128, so only nine one-block workgroups fit; 1 = always one block per workgroup (rounds 1-5); 2 = five per workgroup whatever the size
 *   "decoder_wg4"                [LZ4HIP_DECODER_WG4]  lane decoder, batches of at most one residency round: 0 = default, workgroups of FOUR wavefronts (they go to the four SIMDs of
 *                                 one CU, whatever ran on the device before) while the batch has more than one wavefront per CU and at most one residency round; 1 = always workgroups of one
 *                                 wavefront; 2 = the four-wavefront form from four wavefronts on (tests); 3 = whatever the batch size (A/B runs)
 *   "decoder_wrapped_stores"     [LZ4HIP_DECODER_WRAPPED_STORES]  lane decoder: its default instantiation stores every ring row at `row` and at `row - ring size`
 *                                 and relies on gfx950 dropping the LDS store that falls outside the workgroup's allocation; the library CHECKS that rule once per
 *                                 device before the first lane-mapped decode (a ~1 ms probe launch) and uses the instantiation that wraps its rows instead (same bytes,
 *                                 a few per cent slower) where the probe does not confirm it.  1 = always the wrapped-row instantiation (debuggers, trap-on-violation
 *                                 modes).  Read-only through lz4hip_tuning_get: "decoder_dual_store" = 1 if lane-mapped decodes on the current device store twice, else 0
 *   "sizes_groups"               [LZ4HIP_SIZES_GROUPS]  lz4hip_decoded_sizes_*: wavefronts of the walk's grid (0 = one lane per block, one wavefront per
 *                                 64 blocks; tests use a few so that every lane walks many blocks)
 *   "logical_devices"            [LZ4HIP_LOGICAL_DEVICES]  the *_multi entry points run this many device workers over the
 *                                 selected devices, wrapping around (0 = one per device): exercises the threaded path on one GPU
 * lz4hip_tuning_set returns the previous value (>= 0) or LZ4HIP_E_ARGUMENT; lz4hip_tuning_get the current value. */
int lz4hip_tuning_set(const char* name, int value);
int lz4hip_tuning_get(const char* name);

/* Frees the grow-only kernel workspaces (encoder hash-table / LZ4HC slabs) of the CURRENT device after
 * waiting for their last user, the calling thread's host-pointer staging (device images, pinned slots) for it, and that of the *_multi entry
 * points' persistent device workers.  The reference frees its tables before every return (original/lz4.c:780-786);
 * the library caches them between calls, this is how a caller gets the memory back. */
int lz4hip_release_workspaces(void);

/* ---- device-side synthetic data + verification (bench / tests) ---------------------
 * dist: 0 zeros, 1 incompressible, 2 reference fuzzer generator (original/fuzzer.c:149-168), 3 record-like.
 * Row i of `out` is synthetic block number first_block + i * block_step (block_step = world size gives a
 * rank its round-robin share of a global batch).  Bit-identical to the CPU twins in oracle/synth.c. */
int lz4hip_synth_device(int dist, uint64_t seed, uint64_t first_block, uint64_t block_step, int64_t n_blocks,
                        void* out, int64_t stride, int32_t len, void* stream);
int lz4hip_checksum_device(const void* data, const int64_t* off, int64_t stride, const int32_t* len,
                           int32_t len_all, uint64_t* sums, int64_t n_blocks, void* stream);
/* *mismatches (device, unsigned 64-bit, caller zeroes it) += number of differing bytes */
int lz4hip_compare_device(const void* a, int64_t a_stride, const void* b, int64_t b_stride,
                          const int32_t* len, int32_t len_all, int64_t n_blocks, uint64_t* mismatches,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LZ4HIP_H */
