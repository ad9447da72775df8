"""Per-section instruction table of the SHIPPED lane decoder kernel (lz4hip::decode_lane4_kernel<true,192,32,128,2,2,2,16>).

Builds lz4hip_api.hip with -DLZ4HIP_SECTION_MARKERS (every LZ4HIP_SECTION("...") of lz4hip_decode_lane4.hpp becomes a comment line in
the listing), walks the kernel's listing in layout order and attributes every instruction to the marker before it.  The loop body exists
twice (the flushing iteration and the one that requests input), so every section appears twice; rare paths (the byte-wise parser, the end of
a block, the exact tail) are sections of their own and are left out of the per-iteration sum.  Instructions are classified as
  VOP3  vector-ALU, 64-bit encoding (v_cndmask_b32_e64, v_perm_b32, v_alignbyte_b32, v_lshl_add_u32, v_and_or_b32, v_add3_u32, v_bfe_u32, *_e64, v_pk_* ...)
  VOP2  vector-ALU, 32-bit encoding (v_add_u32, v_and_b32, v_mov_b32, v_cmp_*_e32 ...)
  SALU / LDS / VMEM / WAIT
The column "cycles" PRICES the vector-ALU instructions of a section in SIMD-cycles per wavefront at three wavefronts per SIMD, each v_* mnemonic
by its class in profiles/lane_encodings/microbench_valu_rate.txt (PRICE below); nothing else in the listing is priced.  A run of v_mov_b32 /
v_pk_mov_b32 between s_and_saveexec_b64 and the s_mov_b64 that restores EXEC is an EXEC region: its two scalar instructions are charged to
it, by region size.  "cmp" is the section's full count of vector compares.
usage: python tools/isa_lane4_table.py [out.txt] [--root DIR]     (CPU only: hipcc cross-compiles; DIR: another checkout of the sources)"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN6lz4hip19decode_lane4_kernelILb1ELi192ELi32ELi128ELi2ELi2ELi2ELi16EEEvNS_5BatchEiPKjij"
VOP3_ONLY = ("v_perm_b32", "v_alignbyte_b32", "v_alignbit_b32", "v_lshl_add_u32", "v_add_lshl_u32", "v_and_or_b32", "v_or3_b32", "v_add3_u32", "v_bfe_u32", "v_bfe_i32",
             "v_bfi_b32", "v_lshl_or_b32", "v_mad_u32_u24", "v_mad_u64_u32", "v_mul_lo_u32", "v_mul_hi_u32", "v_lshlrev_b64", "v_lshrrev_b64", "v_ashrrev_i64",
             "v_lshl_add_u64", "v_mbcnt_lo_u32_b32", "v_mbcnt_hi_u32_b32", "v_readlane_b32", "v_writelane_b32", "v_min3_u32", "v_max3_u32", "v_med3_u32", "v_xad_u32",
             "v_cmp_class", "v_sad_u32", "v_msad_u8", "v_pk_")


def classify(op, text):
    if op.startswith("v_"):
        if op.endswith("_e64") or op.startswith(VOP3_ONLY) or op.endswith("_sdwa") or op.endswith("_dpp"):
            return "VOP3"
        if op.startswith("v_cmp") and not op.endswith("_e32"):
            # v_cmp_xx vcc, ... is VOPC (32-bit); with an SGPR destination the listing says _e64
            return "VOP2"
        if op.startswith(("v_add_co", "v_sub_co", "v_addc_co", "v_subb_co")) and "vcc" not in text:
            return "VOP3"
        return "VOP2"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"):
        return "WAIT"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "OTHER"


# SIMD-cycles per wavefront-instruction at three wavefronts per SIMD (profiles/lane_encodings/microbench_valu_rate.txt)
PRICE = collections.OrderedDict([
    ("compare", 5.55),        # v_cmp_* in either encoding: 5.53 (VCC), 5.57 (SGPR pair)
    ("64-bit encoding", 4.55),  # v_cndmask_b32_e64 4.55, v_perm_b32 4.56, v_bfe_u32 4.44, v_and_or_b32 4.46, v_add3_u32 4.57, v_alignbyte_b32 4.65
    ("64-bit add", 5.66),     # v_lshl_add_u64
    ("shift", 4.26),          # v_lshlrev_b32 and its kin, even as 32-bit encodings
    ("32-bit, reads dst", 3.83),  # v_add_u32 d, d, x
    ("32-bit", 3.45),         # v_and_b32 3.40, v_sub_u32 3.51 (v_or, v_xor, v_min, v_max priced alike)
    ("32-bit add, three addresses", 2.93),
    ("move", 2.80),           # v_mov_b32
    ("packed move", 4.84),    # v_pk_mov_b32: 2.42 per dword
    ("move under EXEC", None),  # by region size, see region_price
])
COMPARE_IN_MIX = 4.21     # slope of a body of 28 v_perm_b32 + 20 v_add_u32 over the compares interleaved in it, three wavefronts per SIMD (tools/microbench_valu_rate.hip mix)
SHIFTS = ("v_lshlrev_b32", "v_lshrrev_b32", "v_ashrrev_i32")


def region_price(moves, packed):
    """An EXEC region of `moves` v_mov_b32 and `packed` v_pk_mov_b32, its two scalar instructions included: 9.51 for one move, 3.34 per dword in
    a region of four, 3.09 in one of eight (2.0 for the region + 2.84 per move fits both); packed 2.56 - 2.64 per dword in a region of four."""
    if moves + packed == 0:
        return 0.0
    if moves == 1 and packed == 0:
        return 9.51
    return 2.0 + 2.84 * moves + 4.8 * packed


def price_class(op, text):
    """class of a v_* instruction OUTSIDE an EXEC region of moves"""
    base = re.sub(r"_(e32|e64|sdwa|dpp)$", "", op)
    if base.startswith("v_cmp"):
        return "compare"
    if base == "v_pk_mov_b32":
        return "packed move"
    if base == "v_mov_b32":
        return "move"
    if base in ("v_lshl_add_u64", "v_lshlrev_b64", "v_lshrrev_b64", "v_ashrrev_i64", "v_mad_u64_u32"):
        return "64-bit add"
    if base in SHIFTS:
        return "shift"
    if classify(op, text) == "VOP3":
        return "64-bit encoding"
    if base in ("v_add_u32", "v_add_co_u32"):
        regs = [r.strip() for r in text.split(None, 1)[1].split(",")] if " " in text else []
        regs = [r for r in regs if r != "vcc"]
        return "32-bit, reads dst" if len(regs) >= 3 and regs[0] in regs[1:] else "32-bit add, three addresses"
    return "32-bit"


def main():
    args = [a for a in sys.argv[1:]]
    global ROOT
    if "--root" in args:
        i = args.index("--root")
        ROOT = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else None
    with tempfile.TemporaryDirectory() as td:
        s_file = os.path.join(td, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "lz4net_amd", "csrc"), "-DLZ4HIP_SECTION_MARKERS",
               "-S", "--cuda-device-only", os.path.join(ROOT, "lz4net_amd", "csrc", "lz4hip_api.hip"), "-o", s_file]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        lines = open(s_file, errors="replace").read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    seen = collections.Counter()
    sec = "prologue (one block per lane: set-up)"
    table = collections.OrderedDict()
    mnem = collections.defaultdict(collections.Counter)
    cyc = collections.Counter()                                      # section -> priced SIMD-cycles of its vector-ALU instructions
    pcls = collections.defaultdict(collections.Counter)              # section -> price class -> instructions
    pcyc = collections.defaultdict(collections.Counter)              # section -> price class -> SIMD-cycles
    region = None                                                    # [section, v_mov_b32, v_pk_mov_b32] behind an s_and_saveexec_b64, while only moves follow
    meta = {}

    def close_region(as_region):
        nonlocal region
        if region is None:
            return
        rsec, mv, pk = region
        region = None
        if as_region and mv + pk:
            c_ = region_price(mv, pk)
            cyc[rsec] += c_
            pcls[rsec]["move under EXEC"] += mv + pk
            pcyc[rsec]["move under EXEC"] += c_
        else:                                                        # (a real branch: the moves are ordinary instructions)
            for k_, n_ in (("move", mv), ("packed move", pk)):
                cyc[rsec] += n_ * PRICE[k_]
                pcls[rsec][k_] += n_
                pcyc[rsec][k_] += n_ * PRICE[k_]
    for l in lines[start:end]:
        t = l.strip()
        m = re.match(r";\s*@@SECTION (.*)", t)
        if m:
            name = m.group(1).strip()
            seen[name] += 1
            copy = (seen[name] + (1 if name.startswith("T4 parse") else 0)) // (2 if name.startswith("T4 parse") else 1)
            sec = "%s [copy %d]" % (name, copy)
            continue
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
            continue
        op = t.split()[0]
        c = classify(op, t)
        table.setdefault(sec, collections.Counter())[c] += 1
        mnem[sec][op] += 1
        if op == "s_and_saveexec_b64":
            close_region(False)
            region = [sec, 0, 0]
        elif region is not None and op == "s_mov_b64" and re.match(r"s_mov_b64\s+exec\b", t):
            close_region(True)
        elif region is not None and op in ("v_mov_b32", "v_mov_b32_e32"):
            region[1] += 1
        elif region is not None and op == "v_pk_mov_b32":
            region[2] += 1
        else:
            close_region(False)
            if op.startswith("v_"):
                k_ = price_class(op, t)
                cyc[sec] += PRICE[k_]
                pcls[sec][k_] += 1
                pcyc[sec][k_] += PRICE[k_]
    close_region(False)
    for l in lines[end:end + 400]:
        m = re.search(r"\.(num_vgpr|numbered_sgpr|private_seg_size), (\d+)", l)
        if m and KERNEL in l:
            meta[m.group(1)] = int(m.group(2))
    rows = []
    rows.append("# lz4hip::decode_lane4_kernel<true,192,32,128,2,2,2,16> -- static instruction counts of the compiled kernel by source section")
    rows.append("# (tools/isa_lane4_table.py: hipcc -O3 -DLZ4HIP_SECTION_MARKERS; the loop body exists twice: copy 1 = the iteration that flushes, copy 2 = the one that requests input)")
    rows.append("# registers: %s" % meta)
    rows.append("%-52s %5s %5s %5s %4s %5s %5s %5s %8s" % ("section", "VOP3", "VOP2", "SALU", "LDS", "VMEM", "WAIT", "cmp", "cycles"))
    hot = [collections.Counter(), collections.Counter()]
    hot_cyc, hot_cmp = [0.0, 0.0], [0, 0]
    RARE = ("T4x", "B5 ", "prologue")
    for name, c in table.items():
        rows.append("%-52s %5d %5d %5d %4d %5d %5d %5d %8.1f" % (name, c["VOP3"], c["VOP2"], c["SALU"], c["LDS"], c["VMEM"], c["WAIT"], pcls[name]["compare"], cyc[name]))
        if not name.startswith(RARE):
            k = 0 if "[copy 1]" in name else 1
            hot[k].update(c)
            hot_cyc[k] += cyc[name]
            hot_cmp[k] += pcls[name]["compare"]
    for k in (0, 1):
        c = hot[k]
        rows.append("%-52s %5d %5d %5d %4d %5d %5d %5d %8.1f   <- always-executed sections, VALU %d" % ("SUM copy %d (without T4x trap, B5 end of block)" % (k + 1), c["VOP3"], c["VOP2"], c["SALU"], c["LDS"], c["VMEM"], c["WAIT"], hot_cmp[k], hot_cyc[k], c["VOP3"] + c["VOP2"]))
    both = hot[0] + hot[1]
    rows.append("per iteration (mean of the two copies): VALU %.0f (VOP3 %.0f, VOP2 %.0f), SALU %.0f, LDS %.1f, VMEM %.1f" % (
        (both["VOP3"] + both["VOP2"]) / 2, both["VOP3"] / 2, both["VOP2"] / 2, both["SALU"] / 2, both["LDS"] / 2, both["VMEM"] / 2))
    rows.append("priced per iteration (mean of the two copies): %.1f SIMD-cycles of vector ALU per wavefront at three wavefronts per SIMD, %.1f vector compares" % (
        (hot_cyc[0] + hot_cyc[1]) / 2, (hot_cmp[0] + hot_cmp[1]) / 2))
    n_cmp = (hot_cmp[0] + hot_cmp[1]) / 2
    rows.append("... with a compare at what it adds in the middle of other vector work (%.2f, profiles/lane_compares/microbench_compare_in_mix.txt): %.1f SIMD-cycles" % (
        COMPARE_IN_MIX, (hot_cyc[0] + hot_cyc[1]) / 2 - n_cmp * (PRICE["compare"] - COMPARE_IN_MIX)))
    rows.append("")
    rows.append("# priced classes per iteration (mean of the two copies, hot sections): instructions, SIMD-cycles")
    tot_n, tot_c = collections.Counter(), collections.Counter()
    for name in table:
        if not name.startswith(RARE):
            tot_n.update(pcls[name]); tot_c.update(pcyc[name])
    for k_ in PRICE:
        if tot_n[k_]:
            rows.append("%-32s %6.1f %8.1f" % (k_, tot_n[k_] / 2, tot_c[k_] / 2))
    rows.append("")
    rows.append("# vector compares per hot section (both copies summed), every mnemonic")
    cagg = collections.defaultdict(collections.Counter)
    for name, c in mnem.items():
        if not name.startswith(RARE):
            cagg[re.sub(r" \[copy \d\]", "", name)].update({o: n_ for o, n_ in c.items() if o.startswith("v_cmp")})
    for name, c in cagg.items():
        if c:
            rows.append("%-44s %3d  %s" % (name, sum(c.values()), ", ".join("%s x%d" % kv for kv in c.most_common())))
    rows.append("")
    rows.append("# most frequent mnemonics per hot section (both copies summed)")
    agg = collections.defaultdict(collections.Counter)
    for name, c in mnem.items():
        if not name.startswith(RARE):
            agg[re.sub(r" \[copy \d\]", "", name)].update(c)
    for name, c in agg.items():
        rows.append("%-44s %s" % (name, ", ".join("%s x%d" % kv for kv in c.most_common(14))))
    text = "\n".join(rows)
    print(text)
    if out:
        open(out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
