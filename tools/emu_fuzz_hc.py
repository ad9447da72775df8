"""Fuzz of the LZ4HC kernels under the SIMT emulator against the oracle (tests/encoder_fuzz.py: the rows; tests/encoder_cases.py:
the forms): the precomputed-table kernels (lz4hip_hc_nat.hpp / lz4hip_hc_lcp.hpp) on the rows up to 64 KiB, the large-block kernel
(lz4hip_hc_conv.hpp) and the wavefront mapping on the others; 192 rows per round.  A mismatch names seed, round and block and saves the row to
the working directory.
usage: python tools/emu_fuzz_hc.py <seed> <rounds> [nat|lcp|conv|wave]     (TEST INFRASTRUCTURE: needs tests/simt and oracle/)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import encoder_fuzz
from oracle.oracle import Oracle

seed = int(sys.argv[1]); rounds = int(sys.argv[2]); kind = sys.argv[3] if len(sys.argv) > 3 else "lcp"
names = {"nat": ("hc-lane-natural-chains",), "lcp": ("hc-lane-chains-with-shared-lengths",), "conv": ("hc-lane-large-blocks",),
         "wave": ("hc-wave-heads16", "hc-wave-heads32")}[kind]
forms = [f for f in encoder_fuzz.emu_forms() if f.name in names]
o = Oracle()
total = bad = 0
for r in range(rounds):
    t, b = encoder_fuzz.run_round(o, forms, seed, r, 192, save_dir=os.getcwd())
    total += t; bad += b
    print("seed", seed, "round", r, "total", total, "bad", bad, flush=True)
sys.exit(1 if bad else 0)
