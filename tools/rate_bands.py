"""Holds one library's rate files against another's two runs of the same tools in the same session (order: yardstick, new, yardstick).
For every timing (a key ending in `_ms`) of every row the band is what the yardstick's two runs span, widened on either side by its own
width -- the session's run-to-run noise as the yardstick itself shows it; a new figure above the band is slower than that noise allows,
one below it faster.  Wall-time figures (`loop_*`) and differences of timings are held to the same rule and marked.

    python tools/rate_bands.py DIR            DIR/{parent1,new,parent2}/*.json -> DIR/bands.json, and the rows outside their band
"""
import glob
import json
import os
import sys

root = sys.argv[1]
bands, outside = {}, []
for path in sorted(glob.glob(os.path.join(root, "new", "*.json"))):
    name = os.path.basename(path)
    runs = {p: json.load(open(os.path.join(root, p, name))) for p in ("parent1", "new", "parent2")}
    for row, fields in runs["new"].items():
        if not isinstance(fields, dict):
            continue
        for key, new in fields.items():
            if not key.endswith("_ms") and not key.endswith("_ms_per_item"):
                continue
            a, b = runs["parent1"][row][key], runs["parent2"][row][key]
            lo, hi = min(a, b), max(a, b)
            low, high = lo - (hi - lo), hi + (hi - lo)
            verdict = "inside" if low <= new <= high else ("above" if new > high else "below")
            kind = "wall" if key.startswith("loop_") else ("difference" if "difference" in key else "event")
            bands[f"{name}:{row}:{key}"] = {"parent1": a, "new": new, "parent2": b, "band": [low, high], "verdict": verdict, "kind": kind,
                                            "new_over_parent_mean": new / ((a + b) / 2)}
            if verdict != "inside":
                outside.append((f"{name}:{row}:{key}", a, new, b, verdict))
with open(os.path.join(root, "bands.json"), "w") as f:
    json.dump(bands, f, indent=1)
print(f"{len(bands)} timings, {len(outside)} outside their band")
for name, a, new, b, verdict in outside:
    print(f"  {verdict:6s} {name}: parent {a:.4f} / {b:.4f}, new {new:.4f} ({100 * (new / ((a + b) / 2) - 1):+.2f} %)")
