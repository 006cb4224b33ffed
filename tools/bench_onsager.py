#!/usr/bin/env python3
"""Species-resolved Onsager moments (ta_onsager_staged) against the conductivity's moment pass, one JSON line.

Positions ta_stage_synth'd straight into the device slab (default 10000 frames x 100000 atoms x 3 float64: 24 GB).
In ONE run, on the same slab:
  baseline          : ta_conductivity_staged, the moment alone -- k_cond_moment, the single pass whose S repetitions
                      (one per species, the other species' charges masked to zero) the new call replaces;
  per S in --species (default 1 2 4 8) and label order (interleaved: atom n is species n % S; sorted: contiguous
  blocks of equal size):
      moments       : ta_onsager_staged without the cross term -- k_species_moment + its partial sums;
      whole         : moments + the cross MSD C (T, S, S) (fft=True).
Per case: ms per call from ta_timing_history (K timed calls after W warm-ups: median and min) and the per-kernel split of
one extra call (ta_kernel_timeline); for the pass its ratio to k_cond_moment, its fraction of the 8 TB/s HBM roof, and
`gate` = the pass takes less than S passes of k_cond_moment.

    python tools/bench_onsager.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--species 1 2 4 8]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
SEED = 20240917


def timed(torch, ctx, call, steps, warmup):
    """(sorted ms per call, {kernel: ms} of one more call)"""
    ctx.set_option("timeline", 0)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    ms = sorted(t for t, _ in ctx.timing_history(steps))
    ctx.set_option("timeline", 1)
    call()
    torch.cuda.synchronize()
    kernels = {}
    for name, t in ctx.kernel_timeline(64):
        kernels[name] = round(kernels.get(name, 0.0) + t, 3)
    ctx.set_option("timeline", 0)
    return ms, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--species", type=int, nargs="+", default=[1, 2, 4, 8])
    args = ap.parse_args()
    import torch

    from transport_analysis_amd import _lib

    T, A, D = args.frames, args.atoms, 3
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    ctx.stage_alloc_device(T, A, D, 1)
    ctx.stage_synth(0, SEED, 0, A * D)
    slab = T * A * D * 8

    q = torch.ones(A, dtype=torch.float64, device=dev)
    q[1::2] = -1.0
    mom = torch.zeros((T, D), dtype=torch.float64, device=dev)
    ms, kernels = timed(torch, ctx, lambda: ctx.conductivity_staged(True, q.data_ptr(), mom.data_ptr()), args.steps, args.warmup)
    cond_ms = kernels["k_cond_moment"]
    baseline = {"case": "k_cond_moment", "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3),
                "pass_ms": cond_ms, "hbm_roof_frac": round(slab / (cond_ms * 1e-3) / HBM_BYTES_PER_S, 4), "kernels": kernels}

    cases = []
    w = torch.ones(A, dtype=torch.float64, device=dev)
    for S in args.species:
        moments = torch.zeros((S, T, D), dtype=torch.float64, device=dev)
        cross = torch.zeros((T, S, S), dtype=torch.float64, device=dev)
        for order in ("interleaved", "sorted"):
            n = torch.arange(A, device=dev)
            lab = (n % S if order == "interleaved" else (n * S) // A).to(torch.int32)
            for what, d_cross in (("moments", 0), ("whole", cross.data_ptr())):
                ms, kernels = timed(torch, ctx, lambda: ctx.onsager_staged(True, S, lab.data_ptr(), moments.data_ptr(),
                                                                           w.data_ptr(), d_cross), args.steps, args.warmup)
                k_ms = kernels["k_species_moment"]
                cases.append({"n_species": S, "labels": order, "case": what, "ms_median": round(ms[len(ms) // 2], 3),
                              "ms_min": round(ms[0], 3), "steps": len(ms), "pass_ms": k_ms,
                              "pass_over_cond_moment": round(k_ms / cond_ms, 3), "gate": bool(S == 1 or k_ms < S * cond_ms),
                              "hbm_roof_frac": round(slab / (k_ms * 1e-3) / HBM_BYTES_PER_S, 4), "kernels": kernels})
    out = {"metric": "onsager_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A, "dim": D,
           "fft": True, "slab_bytes": slab, "baseline": baseline, "cases": cases}
    ctx.stage_free()
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
