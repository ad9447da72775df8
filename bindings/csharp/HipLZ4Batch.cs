// HipLZ4Batch.cs -- batch entry points of liblz4hip.so for C# callers (source only: no .NET toolchain in
// the build environment; the same calls are exercised through ctypes by lz4net_amd/stream.py,
// lz4net_amd/legacy_frame.py and LZ4Codec.WrapMany/UnwrapMany in lz4net_amd/codec.py; the lz4hip_streams_*_host
// declarations below have never been compiled either, tests/test_streams_device.py calls the same symbols through ctypes).
//
// lz4net itself has no batch API: callers loop over LZ4Codec.Encode/Decode (LZ4Stream.FlushCurrentChunk /
// AcquireNextChunk, src/LZ4/LZ4Stream.cs:239-312).  A GPU pays off per batch, so this is the call a
// maintainer would route LZ4Stream's chunks or arrays of Wrap()ped messages through: all blocks of one call
// go to the device in one lz4hip_encode_batch_host / lz4hip_decode_batch_host (include/lz4hip.h).
using System;
using System.Runtime.InteropServices;

namespace LZ4hip
{
    public static class HipLZ4Batch
    {
        private const string Lib = "lz4hip";
        private const int ModeFast = 0, ModeHC = 1;                 // LZ4HIP_MODE_FAST / LZ4HIP_MODE_HC
        private const int ErrFirst = -2000000003, ErrLast = -2000000001;

        // struct lz4hip_batch (include/lz4hip.h), field for field
        [StructLayout(LayoutKind.Sequential)]
        private unsafe struct Batch
        {
            public byte* src; public long* src_off; public long src_stride; public int* src_len;
            public byte* dst; public long* dst_off; public long dst_stride; public int* dst_cap;
            public int dst_cap_all; public int src_len_all;
            public int* result; public long n_blocks;
        }

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_encode_batch_host(Batch* b, int mode);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_decode_batch_host(Batch* b, int knownOutputSize);

        // Sharded over the GPUs of the node: block i -> the (i mod N)-th device of deviceMask (bit d = device d,
        // 0 = all visible devices); include/lz4hip.h, SURVEY.md 8e.  No launcher, no collective.
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_encode_batch_host_multi(Batch* b, int mode, ulong deviceMask);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_decode_batch_host_multi(Batch* b, int knownOutputSize, ulong deviceMask);

        // The decoded size of every block before an unknown-size decode (include/lz4hip.h, "the decoded sizes of a batch"): result,
        // dstCap = max(result, 0) and dstOff[n + 1], their exclusive scan, are what lz4hip_decode_batch_host(b, 0) then takes.
        // (Declaration only: not compiled or run by this repository's tests.)
        // struct lz4hip_sizes_info, field for field
        [StructLayout(LayoutKind.Sequential)]
        public struct SizesInfo
        {
            public long blocks, decoded_bytes, first_error;
            public int error, reserved;
        }

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_decoded_sizes_host(Batch* b, long* dstOff, int* dstCap, SizesInfo* info);

        // Block batches decoded against ONE shared dictionary (include/lz4hip.h, "block batches decoded against a shared dictionary"):
        // K4os.Compression.LZ4's LZ4Codec.Decode(source, target, dictionary) for many blocks in one call.  Only the dictionary's last
        // 65 535 bytes can be reached; dictLen = 0 (dict may be null) is the plain call.  One device, no _multi form.
        // (Declarations only: not compiled or run by this repository's tests, tests/test_gpu_dict_decode.py calls the same symbols
        // through ctypes.)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_decode_batch_dict_host(Batch* b, byte* dict, long dictLen, int knownOutputSize);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_encode_batch_dict_host(Batch* b, byte* dict, long dictLen);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_decoded_sizes_dict_host(Batch* b, long dictLen, long* dstOff, int* dstCap, SizesInfo* info);

        // A batch encoded into ONE buffer of exactly the bytes produced (include/lz4hip.h, "a block batch encoded into one packed buffer"):
        // b's dst fields are ignored, b.dst_cap_all is the slot width (MaximumOutputLength of the longest block); dstOff[n + 1] and
        // packedLen[n] come back in the layout lz4hip_decoded_sizes_host and an offsets-form decode batch read.  dstCap may be anything
        // >= 0: info.written_blocks leading blocks fit, info.packed_bytes is what all of them need (dstCap = 0: a size query).
        // roundBlocks = 0: one round; K > 0: rounds of K blocks through a ring of K slots of device scratch.
        // (Declarations only: not compiled or run by this repository's tests, tests/test_gpu_encode_packed.py calls the same symbol
        // through ctypes.)
        // struct lz4hip_packed_info, field for field
        [StructLayout(LayoutKind.Sequential)]
        public struct PackedInfo
        {
            public long blocks, packed_bytes, written_blocks, first_failed;
            public int error, reserved;
        }

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern long lz4hip_encode_packed_scratch_bytes(long nBlocks, int slotBytes, long roundBlocks);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_encode_packed_host(Batch* b, int mode, long roundBlocks, byte* dst, long dstCap, long* dstOff,
                                                                   int* packedLen, PackedInfo* info);

        // Many LZ4Stream buffers per call (include/lz4hip.h, "batches of LZ4Stream buffers"): one buffer plus offsets[n + 1] in, the
        // same layout out; every item becomes / is read as the stream LZ4Stream writes for it, the chunks of all items in one batch.
        // struct lz4hip_streams_info, field for field
        [StructLayout(LayoutKind.Sequential)]
        public struct StreamsInfo
        {
            public long items, chunks, compressed_chunks, decoded_bytes, first_error, error_offset;
            public int error, reserved;
        }

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern long lz4hip_streams_bound(long n, long srcLen, int blockSize);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_streams_encode_host(byte* src, long srcLen, long* srcOff, long n, int blockSize, int mode,
                                                                    byte* dst, long dstCap, long* dstOff);

        // dstCap = 0 is a size query: LZ4HIP_E_ARGUMENT with info->decoded_bytes, dstOff, status and errorOffset filled in
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_streams_decode_host(byte* src, long srcLen, long* srcOff, long n, byte* dst, long dstCap,
                                                                    long* dstOff, int* status, long* errorOffset, StreamsInfo* info);

        // Whole legacy frames of the reference's command-line tool per call (include/lz4hip.h, "legacy frames"): magic, then a size field
        // and an LZ4 block per chunk; chunkSize 0 = the tool's 8 MiB.  (Declarations only: not compiled or run by this repository's tests,
        // tests/test_gpu_frame_device.py calls the same symbols through ctypes.)
        // struct lz4hip_frame_info, field for field
        [StructLayout(LayoutKind.Sequential)]
        public struct FrameInfo
        {
            public long chunks, decoded_bytes, good_bytes, error_offset;
            public int error, reserved;
        }

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern long lz4hip_frame_bound(long srcLen, int chunkSize);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_frame_encode_host(byte* src, long srcLen, int chunkSize, int mode, byte* dst, long dstCap, long* dstLen);

        // returns info->error (LZ4HIP_FRAME_*); dstCap = 0 is a size query: LZ4HIP_E_ARGUMENT with *info filled in
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_frame_decode_host(byte* src, long srcLen, int chunkSize, byte* dst, long dstCap, FrameInfo* info);

        // Many LZ4 frames (magic 0x184D2204) per call (include/lz4hip.h, "batches of LZ4 frames"): one buffer plus offsets[n + 1], one
        // frame per item.  (Declarations only: not compiled or run by this repository's tests, tests/test_gpu_lz4f_batch.py calls the
        // same symbols through ctypes.)
        // struct lz4hip_lz4f_info and struct lz4hip_lz4f_batch_info, field for field
        [StructLayout(LayoutKind.Sequential)]
        public struct Lz4fInfo
        {
            public long blocks, decoded_bytes, good_bytes, error_offset, content_size, frame_bytes;
            public int error, kind, block_max, flg, bd, checks;
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct Lz4fBatchInfo
        {
            public long items, blocks, decoded_bytes, first_error, error_offset;
            public int error, reserved;
        }

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern long lz4hip_lz4f_batch_bound(long n, long srcLen, int blockSizeId, uint flags);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_lz4f_batch_encode_host(byte* src, long srcLen, long* srcOff, long n, int blockSizeId, int mode, uint flags,
                                                                       byte* dst, long dstCap, long* dstOff);

        /// <summary>Decode flags of lz4hip_lz4f_batch_decode_host (LZ4HIP_LZ4F_VERIFY_BLOCKS, _VERIFY_CONTENT, _ACCEPT_LINKED).
        /// Lz4fAcceptLinked decodes items whose blocks are linked (LZ4F_compressFrame's default above one block) instead of failing
        /// them with UNSUPPORTED_LINKED; each such item is one serial chain on ONE wavefront, so it pays only in batches of many items.</summary>
        public const uint Lz4fVerifyBlocks = 1, Lz4fVerifyContent = 2, Lz4fAcceptLinked = 8;

        // returns 0, the first failing item's LZ4HIP_LZ4F_* code, or LZ4HIP_E_*; dstCap = 0 is a size query: LZ4HIP_E_ARGUMENT with dstOff,
        // itemInfo and *info filled in
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern unsafe int lz4hip_lz4f_batch_decode_host(byte* src, long srcLen, long* srcOff, long n, uint flags, byte* dst, long dstCap,
                                                                       long* dstOff, Lz4fInfo* itemInfo, Lz4fBatchInfo* info);

        /// <summary>Devices the batch calls shard over (bit d = HIP device d; 0 = every visible device).</summary>
        public static ulong DeviceMask = 0;

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        private static extern int lz4hip_compressBound(int isize);

        private static void Check(int rc)
        {
            if (rc >= ErrFirst && rc <= ErrLast) throw new InvalidOperationException("liblz4hip failed: " + rc);
        }

        /// <summary>Compresses every block (LZ4Codec.Encode / EncodeHC semantics per block, outputLength =
        /// MaximumOutputLength).  results[i] is what Encode would have returned for block i.</summary>
        public static unsafe byte[][] Encode(byte[][] blocks, bool highCompression, out int[] results)
        {
            int n = blocks.Length;
            long total = 0, capTotal = 0;
            var srcOff = new long[n]; var dstOff = new long[n]; var lens = new int[n]; var caps = new int[n];
            for (int i = 0; i < n; i++)
            {
                srcOff[i] = total; lens[i] = blocks[i].Length; total += lens[i];
                dstOff[i] = capTotal; caps[i] = lz4hip_compressBound(lens[i]); capTotal += caps[i];
            }
            var src = new byte[Math.Max(total, 1)]; var dst = new byte[Math.Max(capTotal, 1)];
            for (int i = 0; i < n; i++) Buffer.BlockCopy(blocks[i], 0, src, (int)srcOff[i], lens[i]);
            results = new int[n];
            fixed (byte* ps = src, pd = dst)
            fixed (long* so = srcOff, dof = dstOff)
            fixed (int* sl = lens, dc = caps, res = results)
            {
                var b = new Batch { src = ps, src_off = so, src_len = sl, dst = pd, dst_off = dof, dst_cap = dc, result = res, n_blocks = n };
                Check(lz4hip_encode_batch_host_multi(&b, highCompression ? ModeHC : ModeFast, DeviceMask));
            }
            var output = new byte[n][];
            for (int i = 0; i < n; i++)
            {
                int len = results[i];
                if (highCompression && len <= 0) len = results[i] = -1;       // src/LZ4pn/LZ4Codec.Unsafe.cs:576-578
                output[i] = new byte[Math.Max(len, 0)];
                if (len > 0) Buffer.BlockCopy(dst, (int)dstOff[i], output[i], 0, len);
            }
            return output;
        }

        /// <summary>Decompresses every block into a buffer of outputLengths[i] bytes
        /// (LZ4Codec.Decode(..., knownOutputLength: true) semantics per block).</summary>
        public static unsafe byte[][] Decode(byte[][] blocks, int[] outputLengths)
        {
            int n = blocks.Length;
            long total = 0, outTotal = 0;
            var srcOff = new long[n]; var dstOff = new long[n]; var lens = new int[n];
            for (int i = 0; i < n; i++)
            {
                srcOff[i] = total; lens[i] = blocks[i].Length; total += lens[i];
                dstOff[i] = outTotal; outTotal += outputLengths[i];
            }
            var src = new byte[Math.Max(total, 1)]; var dst = new byte[Math.Max(outTotal, 1)];
            for (int i = 0; i < n; i++) Buffer.BlockCopy(blocks[i], 0, src, (int)srcOff[i], lens[i]);
            var results = new int[n];
            fixed (byte* ps = src, pd = dst)
            fixed (long* so = srcOff, dof = dstOff)
            fixed (int* sl = lens, dc = outputLengths, res = results)
            {
                var b = new Batch { src = ps, src_off = so, src_len = sl, dst = pd, dst_off = dof, dst_cap = dc, result = res, n_blocks = n };
                Check(lz4hip_decode_batch_host_multi(&b, 1, DeviceMask));
            }
            var output = new byte[n][];
            for (int i = 0; i < n; i++)
            {
                if (results[i] != lens[i])                                    // src/LZ4pn/LZ4Codec.Unsafe.cs:373-378
                    throw new ArgumentException("LZ4 block is corrupted, or invalid length has been given.");
                output[i] = new byte[outputLengths[i]];
                Buffer.BlockCopy(dst, (int)dstOff[i], output[i], 0, outputLengths[i]);
            }
            return output;
        }

        /// <summary>Decompresses every block against one shared dictionary into a buffer of outputLengths[i] bytes
        /// (LZ4_decompress_safe_usingDict per block, knownOutputLength: true semantics).</summary>
        public static unsafe byte[][] DecodeWithDictionary(byte[][] blocks, int[] outputLengths, byte[] dictionary)
        {
            int n = blocks.Length;
            long total = 0, outTotal = 0;
            var srcOff = new long[n]; var dstOff = new long[n]; var lens = new int[n];
            for (int i = 0; i < n; i++)
            {
                srcOff[i] = total; lens[i] = blocks[i].Length; total += lens[i];
                dstOff[i] = outTotal; outTotal += outputLengths[i];
            }
            var src = new byte[Math.Max(total, 1)]; var dst = new byte[Math.Max(outTotal, 1)];
            for (int i = 0; i < n; i++) Buffer.BlockCopy(blocks[i], 0, src, (int)srcOff[i], lens[i]);
            var results = new int[n];
            var dict = dictionary.Length > 0 ? dictionary : new byte[1];
            fixed (byte* ps = src, pd = dst, pdict = dict)
            fixed (long* so = srcOff, dof = dstOff)
            fixed (int* sl = lens, dc = outputLengths, res = results)
            {
                var b = new Batch { src = ps, src_off = so, src_len = sl, dst = pd, dst_off = dof, dst_cap = dc, result = res, n_blocks = n };
                Check(lz4hip_decode_batch_dict_host(&b, pdict, dictionary.Length, 1));
            }
            var output = new byte[n][];
            for (int i = 0; i < n; i++)
            {
                if (results[i] != lens[i])
                    throw new ArgumentException("LZ4 block is corrupted, or invalid length has been given.");
                output[i] = new byte[outputLengths[i]];
                Buffer.BlockCopy(dst, (int)dstOff[i], output[i], 0, outputLengths[i]);
            }
            return output;
        }

        /// <summary>Compresses every block against one shared dictionary (fast mode; K4os's LZ4Codec.Encode(source, target, dictionary)
        /// per block, the parse of include/lz4hip.h).  Each result decodes with DecodeWithDictionary and the same dictionary.</summary>
        public static unsafe byte[][] EncodeWithDictionary(byte[][] blocks, byte[] dictionary)
        {
            int n = blocks.Length;
            long total = 0, outTotal = 0;
            var srcOff = new long[n]; var dstOff = new long[n]; var lens = new int[n]; var caps = new int[n];
            for (int i = 0; i < n; i++)
            {
                srcOff[i] = total; lens[i] = blocks[i].Length; total += lens[i];
                caps[i] = lens[i] + lens[i] / 255 + 16;
                dstOff[i] = outTotal; outTotal += caps[i];
            }
            var src = new byte[Math.Max(total, 1)]; var dst = new byte[Math.Max(outTotal, 1)];
            for (int i = 0; i < n; i++) Buffer.BlockCopy(blocks[i], 0, src, (int)srcOff[i], lens[i]);
            var results = new int[n];
            var dict = dictionary.Length > 0 ? dictionary : new byte[1];
            fixed (byte* ps = src, pd = dst, pdict = dict)
            fixed (long* so = srcOff, dof = dstOff)
            fixed (int* sl = lens, dc = caps, res = results)
            {
                var b = new Batch { src = ps, src_off = so, src_len = sl, dst = pd, dst_off = dof, dst_cap = dc, result = res, n_blocks = n };
                Check(lz4hip_encode_batch_dict_host(&b, pdict, dictionary.Length));
            }
            var output = new byte[n][];
            for (int i = 0; i < n; i++)
            {
                if (results[i] <= 0)
                    throw new InvalidOperationException("Compression has been corrupted");
                output[i] = new byte[results[i]];
                Buffer.BlockCopy(dst, (int)dstOff[i], output[i], 0, results[i]);
            }
            return output;
        }
    }
}
