#!/usr/bin/env python3
"""Periodic unwrapping throughput (ta_unwrap), one JSON line.

Positions ta_stage_synth'd straight into the device slab, 10000 frames x 100000 atoms x 3 float64 (24 GB), unwrapped in
place with three box tables: a constant orthorhombic box (k_unwrap_ortho, the box row at frame 0 for every frame), a
per-frame orthorhombic box (+-3 %, NPT) and a per-frame triclinic box (k_unwrap_tric).  The synthetic values are
zero-mean noise inside a box of ~10: the cost does not depend on them, and repeated calls stay valid input.

Per case: ms per call from ta_timing_history (device time of each call, box-table copy included, K timed calls after W
warm-ups: median and min), algorithmic bytes (the slab read once and written once: 48 GB) and their fraction of the
8 TB/s HBM roof, and the per-kernel split of one extra call (ta_kernel_timeline).  `einstein_msd`: the staged
EinsteinMSD evaluation (ta_msd_staged, fft=1, by-particle array) alone and after an unwrap of the same slab.
`cpu_baseline`: the library's CPU backend (C++/OpenMP, all host cores) on an atom block of the same tensor,
extrapolated linearly to 100000 atoms.

    python tools/bench_unwrap.py [--steps K] [--warmup W] [--no-cpu-baseline]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
SEED = 20240917


def boxes(kind, T):
    d = np.tile(np.array([10.0, 11.0, 12.0, 90.0, 90.0, 90.0]), (T, 1))
    if kind != "const":
        d[:, :3] *= 1.0 + 0.03 * np.sin(np.arange(T)[:, None] * 0.05 + np.array([0.0, 1.0, 2.0]))
    if kind == "triclinic":
        d[:, 3:] = [80.0, 85.0, 75.0]
    return d


def timed(ctx, torch, fn, steps, warmup, per_step):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    hist = ctx.timing_history(steps * per_step)
    return [sum(t for t, _ in hist[i:i + per_step]) for i in range(0, len(hist), per_step)]


def run_case(torch, ctx, T, A, D, kind, steps, warmup):
    dims = boxes(kind, T)
    ms = sorted(timed(ctx, torch, lambda: ctx.unwrap(0, dims, [0, 1, 2]), steps, warmup, 1))
    ctx.set_option("timeline", 1)
    ctx.unwrap(0, dims, [0, 1, 2])
    kernels = {}
    for name, t in ctx.kernel_timeline():
        kernels[name] = round(kernels.get(name, 0.0) + t, 3)
    ctx.set_option("timeline", 0)
    nbytes = 2 * T * A * D * 8
    med = ms[len(ms) // 2]
    return {
        "box": kind, "n_frames": T, "n_atoms": A, "dim": D, "ms_median": round(med, 3), "ms_min": round(ms[0], 3),
        "steps": len(ms), "algorithmic_bytes": nbytes, "hbm_roof_frac": round(nbytes / (med * 1e-3) / HBM_BYTES_PER_S, 4),
        "kernels": kernels,
    }


def msd_case(torch, ctx, T, A, steps, warmup):
    dev = torch.device("cuda", 0)
    lag = torch.zeros(T, dtype=torch.float64, device=dev)
    bp = torch.empty((T, A), dtype=torch.float64, device=dev)
    dims = boxes("npt", T)

    def msd():
        ctx.msd_staged(True, lag.data_ptr(), bp.data_ptr(), A)

    def both():
        ctx.unwrap(0, dims, [0, 1, 2])
        msd()

    plain = sorted(timed(ctx, torch, msd, steps, warmup, 1))
    with_unwrap = sorted(timed(ctx, torch, both, steps, warmup, 2))
    del lag, bp
    return {"what": "ta_msd_staged fft=1 with the by-particle array, alone and after ta_unwrap (per-frame box)",
            "ms_median": round(plain[len(plain) // 2], 3),
            "ms_median_with_unwrap": round(with_unwrap[len(with_unwrap) // 2], 3)}


def cpu_baseline(T, A_total, D, atoms=1536):
    from transport_analysis_amd import _lib

    c = _lib.Context("cpu")
    c.stage_alloc(T, atoms, D)
    c.stage_synth(0, SEED, 0, A_total * D)  # the first atoms' columns of the same tensor
    out = {}
    for kind in ("const", "triclinic"):
        dims = boxes(kind, T)
        c.unwrap(0, dims, [0, 1, 2])  # warm-up (first touch)
        t0 = time.perf_counter()
        c.unwrap(0, dims, [0, 1, 2])
        dt = time.perf_counter() - t0
        out[kind] = round(dt * 1e3 * A_total / atoms, 1)
    c.close()
    return {"what": "CPU backend (C++/OpenMP) ta_unwrap", "n_frames": T, "atoms_timed": atoms,
            "threads": os.cpu_count(), "ms_extrapolated_to_n_atoms": out, "n_atoms": A_total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    import torch

    from transport_analysis_amd import _lib

    ctx = _lib.Context(0)
    T, A, D = 10000, 100000, 3
    ctx.stage_alloc_device(T, A, D, 1)
    ctx.stage_synth(0, SEED, 0, A * D)
    torch.cuda.synchronize()
    cases = [run_case(torch, ctx, T, A, D, kind, args.steps, args.warmup) for kind in ("const", "npt", "triclinic")]
    out = {"metric": "unwrap_ms_per_call", "device": torch.cuda.get_device_name(0),
           "headline_ms": cases[0]["ms_median"], "cases": cases,
           "einstein_msd": msd_case(torch, ctx, T, A, args.steps, args.warmup)}
    ctx.stage_free()
    ctx.close()
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(T, A, D)
        out["speedup_vs_cpu_baseline"] = round(out["cpu_baseline"]["ms_extrapolated_to_n_atoms"]["const"]
                                               / cases[0]["ms_median"], 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
