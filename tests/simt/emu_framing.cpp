// emu_framing.cpp -- TEST INFRASTRUCTURE ONLY.
// libsimt_framing.so: the framing side of the library (lz4net_amd/csrc/lz4hip_framing.hpp and lz4hip_hostbatch.hpp's calls on top of it,
// with every kernel they launch) compiled against the SIMT emulator, once, over the one emulated device of emu_framing.hpp.  Each part
// below holds the C entry points of one path and, where the path has promises of its own to verify, its stand-in block codec.  The
// emulator defines __global__ as nothing, so the kernels are ordinary functions: the parts share this one translation unit, and a new
// path is a new part and a line here.  Built with g++ by build_emu.py, never shipped.
#include "simt_wave.hpp"

#include "lz4hip_common.hpp"

using namespace lz4hip;

#include "emu_framing.hpp"
#include "lz4hip_hostbatch.hpp"

using emu_framing::EmuBackend;
using emu_framing::backend;
using emu_framing::finish;
using emu_framing::kJunk;
using emu_framing::kWaveDecodeLdsBytes;
using emu_framing::device_batch;
using emu_framing::same_kernel;

#include "emu_stream.inc"    // LZ4Stream, Wrap and batches of streams: single kernels, sequences, fronts, host-pointer calls
#include "emu_frame.inc"     // the legacy frame
#include "emu_into.inc"      // the one-call decodes, with the stand-in decoder that verifies its table ...
#include "emu_spans.inc"     // ... and their span forms over the same stand-in
#include "emu_sizes.inc"     // the size query of a block batch
#include "emu_packed.inc"    // the packed encode of a block batch
#include "emu_compact.inc"   // the compact decode of a block batch and of a legacy frame
#include "emu_lz4f.inc"      // xxHash32 rows and the LZ4 frame, with the stand-in decoder keyed by global table row ...
#include "emu_lz4f_batch.inc"  // ... the batch of LZ4 frames over the same stand-in, and frames with linked blocks
#include "emu_lz4f_dict.inc"   // LZ4 frames with a dictionary, every block through the real decoder
