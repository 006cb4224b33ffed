#!/usr/bin/env python3
"""Einstein-Helfand conductivity throughput (ta_conductivity_staged), one JSON line.

Positions ta_stage_synth'd straight into the device slab (default 10000 frames x 100000 atoms x 3 float64: 24 GB),
charges +1 / -1 alternating, fft=True.  Cases:
  moment            : the moment alone (no collective, no self term): the k_cond_moment pass + its partial sums;
  collective        : the class default, moment + Phi of the moment;
  nernst_einstein   : moment + Phi + the self term (the weighted slab written by the same pass, then the Einstein MSD's
                      lag sums of it).
Per case: ms per step from ta_timing_history (K timed calls after W warm-ups: median and min) and the per-kernel split
of one extra call (ta_kernel_timeline); for the moment pass its bytes (slab read once, plus the weighted slab written
under nernst_einstein) and their fraction of the 8 TB/s HBM roof.  `cpu_baseline`: the library's CPU backend
(C++/OpenMP, all host cores) on an atom block of the same tensor, extrapolated linearly to all atoms.

    python tools/bench_conductivity.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--no-cpu-baseline]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
SEED = 20240917


def run_case(torch, ctx, T, A, D, coll, self_term, steps, warmup):
    dev = torch.device("cuda", 0)
    q = torch.ones(A, dtype=torch.float64, device=dev)
    q[1::2] = -1.0
    mom = torch.zeros((T, D), dtype=torch.float64, device=dev)
    phi = torch.zeros(T, dtype=torch.float64, device=dev) if coll else None
    slf = torch.zeros(T, dtype=torch.float64, device=dev) if self_term else None
    args = (True, q.data_ptr(), mom.data_ptr(), phi.data_ptr() if coll else 0, slf.data_ptr() if self_term else 0)
    torch.cuda.synchronize()
    ctx.set_option("timeline", 0)
    for _ in range(warmup):
        ctx.conductivity_staged(*args)
    torch.cuda.synchronize()
    for _ in range(steps):
        ctx.conductivity_staged(*args)
    torch.cuda.synchronize()
    ms = sorted(t for t, _ in ctx.timing_history(steps))
    ctx.set_option("timeline", 1)
    ctx.conductivity_staged(*args)
    torch.cuda.synchronize()
    kernels = {}
    for name, t in ctx.kernel_timeline():
        kernels[name] = round(kernels.get(name, 0.0) + t, 3)
    ctx.set_option("timeline", 0)
    slab = T * A * D * 8
    moment_bytes = slab * (2 if self_term else 1)
    k_ms = kernels.get("k_cond_moment", float("nan"))
    return {
        "case": "nernst_einstein" if self_term else ("collective" if coll else "moment"),
        "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "steps": len(ms),
        "moment_pass_ms": k_ms, "moment_pass_bytes": moment_bytes,
        "moment_pass_hbm_roof_frac": round(moment_bytes / (k_ms * 1e-3) / HBM_BYTES_PER_S, 4),
        "kernels": kernels,
    }


def cpu_baseline(T, A_total, D, atoms):
    import numpy as np

    from transport_analysis_amd import _lib

    c = _lib.Context("cpu")
    c.stage_alloc(T, atoms, D)
    c.stage_synth(0, SEED, 0, A_total * D)  # the first atoms' columns of the same tensor
    q = np.where(np.arange(atoms) % 2 == 0, 1.0, -1.0)
    out = {"what": "CPU backend (C++/OpenMP) ta_conductivity fft=1", "n_frames": T, "atoms_timed": atoms,
           "threads": os.cpu_count(), "n_atoms": A_total}
    for name, self_term in (("collective", False), ("nernst_einstein", True)):
        c.conductivity(True, q, self_term=self_term)  # warm-up (plans, first touch)
        t0 = time.perf_counter()
        c.conductivity(True, q, self_term=self_term)
        dt = time.perf_counter() - t0
        out[name] = {"seconds_timed": round(dt, 4), "ms_extrapolated_to_n_atoms": round(dt * 1e3 * A_total / atoms, 1)}
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-atoms", type=int, default=2000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    import torch

    from transport_analysis_amd import _lib

    T, A, D = args.frames, args.atoms, 3
    ctx = _lib.Context(0)
    ctx.stage_alloc_device(T, A, D, 1)
    ctx.stage_synth(0, SEED, 0, A * D)
    cases = [run_case(torch, ctx, T, A, D, coll, slf, args.steps, args.warmup)
             for coll, slf in ((False, False), (True, False), (True, True))]
    out = {"metric": "conductivity_ms_per_step", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A,
           "dim": D, "fft": True, "slab_bytes": T * A * D * 8, "cases": cases}
    ctx.stage_free()
    ctx.close()
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(T, A, D, min(args.cpu_atoms, A))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
