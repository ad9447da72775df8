"""Builds tests/simt/libsimt_lz4f.so (TEST INFRASTRUCTURE): the xxHash32 row kernel, the LZ4 frame's kernels and their host code
(lz4hip_lz4f.hpp, lz4hip_framing.hpp) compiled with g++ against the SIMT emulator.  Rebuilt when a kernel header or an emulator file is newer."""
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "lz4net_amd", "csrc")
SO = os.path.join(HERE, "libsimt_lz4f.so")


def build() -> str:
    deps = glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(HERE, "*.hpp")) + [os.path.join(HERE, "emu_lz4f.cpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-Wno-unused", "-Wno-parentheses", "-Wno-unknown-pragmas",
                        "-I" + HERE, "-I" + CSRC, "-o", SO, os.path.join(HERE, "emu_lz4f.cpp")], check=True)
    return SO
