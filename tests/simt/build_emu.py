"""Builds the emulator libraries (TEST INFRASTRUCTURE): the real kernel sources and the library's own host code compiled with g++
against the SIMT emulator.  libsimt_kernels.so holds the block codec kernels and the host-pointer block batch calls
(emu_kernels.cpp; also built 'starved', and as libsimt_dict.so inside emu_dict.cpp with the dictionary mode's counters),
libsimt_framing.so everything on the framing side (emu_framing.cpp and its parts, emu_*.inc).  Each is rebuilt when a kernel header
or an emulator file is newer."""
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "lz4net_amd", "csrc")
AB = os.path.join(ROOT, "tools", "ab")


def _files(*patterns):
    return [f for p in patterns for f in glob.glob(p)]


def _build(so, source, deps, flags):
    deps = deps + [os.path.join(HERE, source)]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = "%s.%d.tmp" % (so, os.getpid())                               # (test processes that start together never load a half-written file)
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused", "-Wno-parentheses", "-Wno-unknown-pragmas",
                        "-I" + HERE, "-I" + CSRC, *flags, "-o", tmp, os.path.join(HERE, source)], check=True)
        os.replace(tmp, so)
    return so


def _build_kernels(name, source, flags):
    """a build of emu_kernels.cpp, alone or inside `source`, with the tuning tree's headers where the high-compression encoder is there"""
    flags = ["-I" + AB] + (["-DLZ4HIP_HAVE_HC", "-DLZ4HIP_TUNING_BUILD"] if os.path.exists(os.path.join(CSRC, "lz4hip_hc.hpp")) else []) + flags
    deps = _files(os.path.join(AB, "*.hpp"), os.path.join(CSRC, "*.hpp"), os.path.join(CSRC, "*.inc"), os.path.join(HERE, "*.hpp"),
                  os.path.join(HERE, "emu_kernels.cpp"))
    return _build(os.path.join(HERE, name), source, deps, flags)


def build(starved: bool = False) -> str:
    """starved=True: the same kernels with the lane decoder's cooperative flush cut down to 4 lines per round, so that
    lanes miss flush rounds again and again and run their rings full (and its cooperative staging
    load to 2 pieces per round, so that lanes run out of input) -- the rare states of the lane decoder (a lane that
    cannot append, a far-match chunk fetched but not consumed) become the common ones."""
    starve = ["-DLZ4HIP_DEC_FLUSH_RECS=4", "-DLZ4HIP_DEC_LOAD_PIECES=2", "-DLZ4HIP_DEC3_FLUSH_RECS=4", "-DLZ4HIP_DEC3_LOAD_PIECES=2", "-DLZ4HIP_DEC4_FLUSH_RECS=2"]
    return _build_kernels("libsimt_kernels_starved.so" if starved else "libsimt_kernels.so", "emu_kernels.cpp", starve if starved else [])


def build_dict(defines=(), name: str = "libsimt_dict.so") -> str:
    """libsimt_dict.so (emu_dict.cpp): emu_kernels.cpp once more, with the counters of the decoder's dictionary mode.  `defines` are
    further -D flags of a variant, which then needs a `name` of its own."""
    return _build_kernels(name, "emu_dict.cpp", ["-pthread", *defines])


def build_framing() -> str:
    deps = _files(os.path.join(CSRC, "*.hpp"), os.path.join(CSRC, "*.inc"), os.path.join(HERE, "*.hpp"), os.path.join(HERE, "*.inc"))
    return _build(os.path.join(HERE, "libsimt_framing.so"), "emu_framing.cpp", deps, ["-pthread"])
