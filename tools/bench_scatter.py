#!/usr/bin/env python3
"""Intermediate scattering functions (ta_scatter_staged) on float64 and float32 device slabs against the streaming, lag-sum
and species-sum comparators, one JSON line.

Values ta_stage_synth'd straight into two device slabs of the same values (default 10000 frames x 100000 atoms x 3: 24 GB
as float64, 12 GB as float32).  In ONE run:
  sort       : k_species_sort of the float64 slab with one species (ta_species_self_staged: 24 GB read, 24 GB written) --
               the streaming yardstick of the phase pass, on the same staged slab;
  vacf2      : the VACF lag sum (ta_vacf_fft_staged) of a float64 slab of n_atoms x 2 columns: what one wavevector's block of
               the phase slab costs the self part, timed alone;
  sum2       : the one-species current pass (ta_current_staged without cross term) of that slab: what it costs the density;
  scatter    : per slab type, K in --kvectors (default 1 4 16) and with / without the collective part:
               ta_scatter_staged(fft=1) -- k_phase per chunk, then per wavevector a lag sum and a species-sum pass.
Per case: `steps` timed calls after `warmup` warm-ups; `call_ms` = median / min / max of the whole call's device-event
interval (ta_timing_history), `kernel_ms` = the same of the named kernel's own interval in `steps` MORE calls with the
kernel timeline on (ta_kernel_timeline; k_phase: all its launches of a call together), `kernels` = the per-kernel split of
the last of them.
  phase_tb_per_s = (launches x slab bytes + K x n_atoms x pitch x 16) / k_phase median;
  sort_tb_per_s  = (slab bytes + float64 bytes) / k_species_sort median;  phase_over_sort = their ratio (expected >= 0.8);
  parts_ms       = k_phase median + K x (vacf2 call median + sum2 pass median);  overhead_ms = call median - parts_ms.
No ratio is gated: the figures are the result.

    python tools/bench_scatter.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--kvectors 1 4 16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SEED = 20240917


def stats(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def timed(torch, ctx, call, steps, warmup, kernel=None):
    ctx.set_option("timeline", 0)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    out = {"call_ms": stats(t for t, _ in ctx.timing_history(steps)), "steps": steps}
    ctx.set_option("timeline", 1)
    own, kernels = [], {}
    for _ in range(steps):
        call()
        torch.cuda.synchronize()
        kernels = {name: round(t, 3) for name, t in ctx.kernel_timeline(64)}
        if kernel:
            own.append(kernels[kernel])
    if kernel:
        out["kernel_ms"] = stats(own)
        out["launches"] = ctx.kernel_launches(kernel)
    ctx.set_option("timeline", 0)
    out["kernels"] = kernels
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kvectors", type=int, nargs="+", default=[1, 4, 16])
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, A, D = args.frames, args.atoms, 3
    pitch = (T + 7) // 8 * 8
    dev = torch.device("cuda", 0)
    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = _lib.Context(0)
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 1)
        ctx.stage_synth(0, SEED, 0, A * D)
        slabs[name] = ctx
    nbytes = {"64": T * A * D * 8, "32": T * A * D * 4}
    z_bytes = A * pitch * 16  # one wavevector's block of the phase slab
    c64 = slabs["64"]
    cases = []

    # the streaming yardstick on the same staged slab
    lab = np.zeros(A, dtype=np.int32)
    out1 = torch.zeros((1, T), dtype=torch.float64, device=dev)
    sort = timed(torch, c64, lambda: c64.species_self_staged(1, 1, 1, lab, out1.data_ptr()), args.steps, args.warmup,
                 kernel="k_species_sort")
    sort["case"] = "sort"
    sort["sort_tb_per_s"] = round((nbytes["64"] + T * A * D * 8) / (sort["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
    cases.append(sort)
    c64.trim()

    # one wavevector's block alone: a float64 slab of A x 2 columns
    two = _lib.Context(0)
    two.stage_alloc_device(T, A, 2, 1)
    two.stage_synth(0, SEED + 1, 0, A * 2)
    lagsum = torch.zeros(T, dtype=torch.float64, device=dev)
    vacf2 = timed(torch, two, lambda: two.vacf_fft_staged(lagsum.data_ptr()), args.steps, args.warmup)
    vacf2["case"] = "vacf2"
    d_lab = torch.zeros(A, dtype=torch.int32, device=dev)
    cur = torch.zeros((1, T, 2), dtype=torch.float64, device=dev)
    sum2 = timed(torch, two, lambda: two.current_staged(1, 1, d_lab.data_ptr(), cur.data_ptr()), args.steps, args.warmup,
                 kernel="k_species_current")
    sum2["case"] = "sum2"
    cases += [vacf2, sum2]
    two.stage_free()
    two.close()

    report = []
    rng = np.random.default_rng(3)
    for K in args.kvectors:
        k = rng.uniform(-2.0, 2.0, size=(K, D))
        fs = torch.zeros((K, T), dtype=torch.float64, device=dev)
        rho = torch.zeros((K, T, 2), dtype=torch.float64, device=dev)
        coll = torch.zeros((K, T), dtype=torch.float64, device=dev)
        for with_coll in (False, True):
            got = {}
            for slab, ctx in slabs.items():
                def call(ctx=ctx):
                    ctx.scatter_staged(1, k, fs.data_ptr(), rho.data_ptr() if with_coll else 0, coll.data_ptr() if with_coll else 0)
                t = timed(torch, ctx, call, args.steps, args.warmup, kernel="k_phase")
                t.update({"case": "scatter", "slab": "float" + slab, "n_k": K, "collective": with_coll})
                moved = t["launches"] * nbytes[slab] + K * z_bytes
                t["phase_tb_per_s"] = round(moved / (t["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
                got[slab] = t
                cases.append(t)
            s64, s32 = got["64"], got["32"]
            parts = s64["kernel_ms"]["median"] + K * (vacf2["call_ms"]["median"] + (sum2["kernel_ms"]["median"] if with_coll else 0.0))
            report.append({
                "n_k": K, "collective": with_coll, "launches": s64["launches"],
                "phase64_tb_per_s": s64["phase_tb_per_s"], "phase32_tb_per_s": s32["phase_tb_per_s"],
                "phase_over_sort": round(s64["phase_tb_per_s"] / sort["sort_tb_per_s"], 4),
                "call64_ms": s64["call_ms"]["median"], "call32_ms": s32["call_ms"]["median"],
                "parts_ms": round(parts, 3), "overhead_ms": round(s64["call_ms"]["median"] - parts, 3)})
    result = {"metric": "scatter_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A, "dim": D,
              "fft": True, "slab_bytes": nbytes, "block_bytes": z_bytes, "sort_tb_per_s": sort["sort_tb_per_s"],
              "vacf2_ms": vacf2["call_ms"]["median"], "sum2_ms": sum2["kernel_ms"]["median"], "report": report, "cases": cases}
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
