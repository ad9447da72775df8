"""Differential fuzz of every encoder form on the GPU against the CPU oracle (tests/encoder_fuzz.py: the rows; tests/encoder_cases.py:
the forms -- fast and LZ4HC, each mapping forced in turn and the default dispatch), with full and with too-small output limits (return value,
bytes, guard bytes).  Through the host-pointer C ABI.  A mismatch names seed, round and block and saves the row to the working directory.
usage: python tools/fuzz_gpu_encoders.py [rounds] [seed]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401
import encoder_fuzz
from oracle.oracle import Oracle

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 606
o = Oracle()
total = bad = 0
t0 = time.time()
for r in range(rounds):
    t, b = encoder_fuzz.run_round(o, encoder_fuzz.gpu_forms(), seed, r, 192, save_dir=os.getcwd())
    total += t; bad += b
    print("round %d done: %d comparisons so far, %d mismatches, %.0f s" % (r, total, bad, time.time() - t0), flush=True)
print("TOTAL %d comparisons, %d mismatches" % (total, bad))
sys.exit(1 if bad else 0)
