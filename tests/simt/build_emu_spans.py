"""Builds tests/simt/libsimt_spans.so (TEST INFRASTRUCTURE): the span forms of the one-call decodes, the selection kernel and the chunk directory
(kernels of lz4hip_stream.hpp, lz4hip_streams.hpp and lz4hip_wrap.hpp, host code of lz4hip_framing.hpp) compiled with g++ against the SIMT emulator,
together with emu_into.cpp's decoder stand-in and consecutive forms.  Rebuilt when a kernel header or an emulator file is newer."""
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "lz4net_amd", "csrc")
SO = os.path.join(HERE, "libsimt_spans.so")


def build() -> str:
    deps = glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(HERE, "*.hpp")) + [os.path.join(HERE, f) for f in ("emu_spans.cpp", "emu_into.cpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-Wno-unused", "-Wno-parentheses", "-Wno-unknown-pragmas",
                        "-I" + HERE, "-I" + CSRC, "-o", SO, os.path.join(HERE, "emu_spans.cpp")], check=True)
    return SO
