"""Instruction table of the forward kernel (k_wsplit_accum, lag sums, no outer radix) at R0 = 18, 20:
compiles transport_analysis_amd/csrc/wfft.hip to gfx950 assembly four times -- the run-time pass
(-DWF_PASS_SPLIT=0: the code before the split), each pass's body alone (-DWF_FIX_PASS=0 / 1) and the
shipped kernel (both bodies behind one branch) -- and counts, per instantiation, the static
v_fma_f64 / v_fmac_f64 / v_mul_f64 / v_add_f64, the other VALU instructions, ds_read_b128 / ds_write_b128 and
buffer_load_*; VGPRs and scratch from the kernel's own footer.  Under each table, where the 16-byte row requests of the
shipped kernel stand between the barriers of S2: each run of buffer_load_dwordx4 with the FP64 instructions between it and
the memory instruction, barrier or branch in front of it and behind it.

usage: python tools/wfft/isa_table.py [-o profiles/r08_headline_isa.txt] [extra hipcc flags]
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(ROOT, "transport_analysis_amd", "csrc", "wfft.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BUILDS = (("run-time pass", ["-DWF_PASS_SPLIT=0"]), ("pass 0 body", ["-DWF_FIX_PASS=0"]),
          ("pass 1 body", ["-DWF_FIX_PASS=1"]), ("shipped (both)", []))
KERNEL = re.compile(r"^_ZN2ta14k_wsplit_accumINS_5WPlanILi(18|20)EEELb0ELb0ELb0ELb([01])EEE\w*:")
COLS = ("v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64", "other VALU", "ds_read_b128", "ds_write_b128", "buffer_load", "VGPRs",
        "scratch")


def assemble(flags, extra):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "wfft.s")
        subprocess.check_call([HIPCC, "-O3", "-std=c++20", "--offload-arch=gfx950", "-ffp-contract=fast",
                               "--cuda-device-only", "-S", "-w", *flags, *extra, SRC, "-o", out])
        with open(out) as f:
            return f.read().splitlines()


def count(lines):
    """{(R0, slab): {column: n}} over the kernels KERNEL matches"""
    res, cur = {}, None
    for l in lines:
        m = KERNEL.match(l)
        if m:
            cur = res.setdefault((int(m.group(1)), "float32" if m.group(2) == "1" else "float64"), dict.fromkeys(COLS, 0))
            cur["rows"], seg, armed, fp, inloop = [], None, False, 0, False
            continue
        if cur is None:
            continue
        for key, pat in (("VGPRs", r";\s*NumVgprs:\s*(\d+)"), ("scratch", r";\s*ScratchSize:\s*(\d+)")):
            f = re.match(pat, l.strip())
            if f:
                cur[key] = int(f.group(1))
        if re.match(r";\s*Occupancy:", l.strip()):  # last line of the kernel's footer
            cur = None
            continue
        if l.startswith(".LBB"):  # the block's comment says whether it belongs to a loop
            inloop = "Loop" in l
        op = l.split()[0] if l.startswith("\t") and l.split() else ""
        op = op[:-4] if op.endswith(("_e32", "_e64")) else op
        # S2: from a barrier that LDS reads follow to the next barrier, the blocks of the unit loop only.  A run of 16-byte requests:
        # [requests, FP64 instructions in front of it, behind it, still counting], counted from / up to the nearest
        # LDS or buffer instruction, branch, barrier or other run
        if op == "s_barrier" or (seg is not None and op == "s_endpgm"):
            if seg:
                cur["rows"].append(seg)
            seg, armed, fp = None, True, 0
        elif op.startswith("ds_read") and armed and seg is None:
            seg, fp = [], 0
        elif seg is not None:
            if op == "buffer_load_dwordx4" and not inloop:
                pass
            elif op == "buffer_load_dwordx4":
                if seg and seg[-1][3] and seg[-1][2] == 0:
                    seg[-1][0] += 1
                else:
                    if seg:
                        seg[-1][3] = False
                    seg.append([1, fp, 0, True])
                fp = 0
            elif op.endswith("_f64"):
                fp += 1
                if seg and seg[-1][3]:
                    seg[-1][2] += 1
            elif op.startswith(("ds_", "buffer_", "s_cbranch", "s_branch")):
                if seg:
                    seg[-1][3] = False
                fp = 0
        if op in ("v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64", "ds_read_b128", "ds_write_b128"):
            cur[op] += 1
        elif op.startswith("buffer_load_"):
            cur["buffer_load"] += 1
        elif op.startswith("v_"):
            cur["other VALU"] += 1
    return res


def main():
    args = sys.argv[1:]
    dest = None
    if args[:1] == ["-o"]:
        dest, args = args[1], args[2:]
    with concurrent.futures.ThreadPoolExecutor(len(BUILDS)) as ex:
        tabs = list(ex.map(lambda b: count(assemble(b[1], args)), BUILDS))
    rows = ["# tools/wfft/isa_table.py: static instruction counts, k_wsplit_accum<WPlan<R0>, false, false, false, SRC32>, gfx950",
            "# (a body alone = -DWF_FIX_PASS: counts only; the shipped kernel holds both bodies, its registers and scratch are what runs)"]
    for key in sorted(tabs[0]):
        rows.append("")
        rows.append("R0 = %d, %s slab" % key)
        rows.append("%-16s" % "" + "".join("%15s" % c for c in COLS))
        for (name, _), tab in zip(BUILDS, tabs):
            rows.append("%-16s" % name + "".join("%15d" % tab[key][c] for c in COLS))
        for seg in tabs[-1][key]["rows"]:
            rows.append("S2 of the shipped kernel [FP64 in front | buffer_load_dwordx4 | FP64 behind]: " +
                        " ".join("[%d | %d | %d]" % (f, n, b) for n, f, b, _ in seg))
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if dest:
        with open(dest, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
