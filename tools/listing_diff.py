"""Kernel-by-kernel comparison of two gfx950 assembly listings (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S of lz4hip_api.hip,
parent and new): for every kernel named, the instruction counts and the lines that differ after comments, directives and label numbers
are removed; for kernels only the new listing has, their instruction count and what the listing says of their registers and scratch.

    python tools/listing_diff.py parent.s new.s decode_kernel lz4f_linked_decode_kernel sizes_walk_kernelE --new decode_dict_kernel

A name selects every kernel whose mangled name contains it."""
import argparse
import difflib
import re


def kernels(path):
    """mangled name -> (instruction lines, {metadata key: value})"""
    out, name, body = {}, None, []
    meta = {}
    for line in open(path, errors="replace"):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            meta_name = m.group(1)
            meta[meta_name] = {}
        m = re.match(r"^\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size|group_segment_fixed_size|accum_offset)\s+(\S+)", line)
        if m and meta:
            meta[meta_name][m.group(1)] = m.group(2)
            continue
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            s = line.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            if not s or s.startswith(".") and not s.startswith(".LBB") or s.endswith(":"):
                continue
            body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", s))
    return out, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("names", nargs="+")
    ap.add_argument("--new-only", nargs="*", default=[], dest="new_only")
    a = ap.parse_args()
    old, _ = kernels(a.parent)
    new, meta = kernels(a.new)
    for want in a.names:
        for k in sorted(k for k in new if want in k and k in old):
            d = [x for x in difflib.unified_diff(old[k], new[k], lineterm="", n=0) if x[0] in "+-" and not x.startswith(("+++", "---"))]
            print(k, len(old[k]), len(new[k]), "differing lines", len(d))
            for x in d:
                print("    " + x)
    for want in a.new_only:
        for k in sorted(k for k in new if want in k and k not in old):
            m = meta.get(k, {})
            print(k, "new:", len(new[k]), "instructions,", "VGPRs", m.get("next_free_vgpr"), "SGPRs", m.get("next_free_sgpr"),
                  "scratch bytes per lane", m.get("private_segment_fixed_size"), "LDS bytes per workgroup", m.get("group_segment_fixed_size"))


if __name__ == "__main__":
    main()
