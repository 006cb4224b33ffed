"""Instruction table of the forward kernel (k_wsplit_accum, lag sums, no outer radix) at R0 = 18, 20:
compiles transport_analysis_amd/csrc/wfft.hip to gfx950 assembly four times -- the run-time pass
(-DWF_PASS_SPLIT=0: the code before the split), each pass's body alone (-DWF_FIX_PASS=0 / 1) and the
shipped kernel (both bodies behind one branch) -- and counts, per instantiation, the static
v_fma_f64 / v_mul_f64 / v_add_f64, the other VALU instructions, ds_read_b128 / ds_write_b128 and
buffer_load_*; VGPRs and scratch from the kernel's own footer.

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
COLS = ("v_fma_f64", "v_mul_f64", "v_add_f64", "other VALU", "ds_read_b128", "ds_write_b128", "buffer_load", "VGPRs",
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
        op = l.split()[0] if l.startswith("\t") and l.split() else ""
        if op in ("v_fma_f64", "v_mul_f64", "v_add_f64", "ds_read_b128", "ds_write_b128"):
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
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if dest:
        with open(dest, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
