#!/usr/bin/env python3
"""Partial scattering functions (ta_partial_density_staged) on float64 and float32 device slabs against the one-group
density of ta_scatter_staged and a streaming read, one JSON line (also written to --out).

Positions ta_stage_synth'd straight into one device slab per element type (default 10000 frames x 100000 atoms x 3: 24 GB as
float64, 12 GB as float32).  In ONE run, on the same staged slabs:
  stream   : k_species_current of slab 0 with one species (ta_current_staged without cross term): a pure streaming read of
             the same layout, per slab type -- the floor of any pass over the slab;
  scatter  : per slab type and K in --kvectors (default 1 4 16): ta_scatter_staged asked for the density only -- k_phase and
             the species-sum pass that reads its phase slab back: the route to the S = 1 density before this kernel;
  partial  : per slab type, S in --species (default 1 2 4 8, interleaved labels n mod S) and K: ta_partial_density_staged
             (fft = 1) with the cross term -- k_species_density once per KC wavevectors (KC from ta_partial_density_tile),
             k_sum_partials, then the polarisation of all wavevectors in one by-particle evaluation.
Per case: `steps` timed calls after `warmup` warm-ups; `call_ms` = median / min / max of the whole call's device-event
interval (ta_timing_history), `kernel_ms` = the same of the named kernel's own interval (all its launches of a call
together) in `steps` MORE calls with the kernel timeline on (ta_kernel_timeline).  The report rows hold, per (slab, K), the
medians and the two ratios the design asks about: partial(S = 1) / scatter, and partial(S) / partial(S = 1) next to the
launch counts.  No ratio is gated: the figures are the result.

    python tools/bench_partial_scattering.py [--frames T] [--atoms A] [--steps N] [--warmup W] [--kvectors 1 4 16] [--species 1 2 4 8]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SEED = 20241019


def stats(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def timed(torch, ctx, call, steps, warmup, kernel):
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
        kernels = {}
        for name, t in ctx.kernel_timeline(256):
            kernels[name] = round(kernels.get(name, 0.0) + t, 3)
        own.append(kernels[kernel])
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
    ap.add_argument("--species", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--out", default=None, help="default: profiles/partial_scattering_bench_<T>x<A>.json")
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, A, D = args.frames, args.atoms, 3
    out_path = args.out or os.path.join(ROOT, "profiles", f"partial_scattering_bench_{T}x{A}.json")
    dev = torch.device("cuda", 0)
    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = _lib.Context(0)
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 1)
        ctx.stage_synth(0, SEED, 0, A * D)
        slabs[name] = ctx
    nbytes = {"64": T * A * D * 8, "32": T * A * D * 4}
    rng = np.random.default_rng(3)
    cases, report = [], []
    zero_lab = torch.zeros(A, dtype=torch.int32, device=dev)
    one = torch.zeros((1, T, D), dtype=torch.float64, device=dev)
    stream = {}
    for slab, ctx in slabs.items():
        t = timed(torch, ctx, lambda ctx=ctx: ctx.current_staged(1, 1, zero_lab.data_ptr(), one.data_ptr()), args.steps, args.warmup,
                  "k_species_current")
        t.update({"case": "stream", "slab": "float" + slab})
        t["stream_tb_per_s"] = round(nbytes[slab] / (t["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
        stream[slab] = t
        cases.append(t)
    labels = {S: (torch.arange(A, dtype=torch.int32, device=dev) % S).contiguous() for S in args.species}
    for K in args.kvectors:
        k = rng.uniform(-2.0, 2.0, size=(K, D))
        for slab, ctx in slabs.items():
            row = {"n_k": K, "slab": "float" + slab, "stream_ms": stream[slab]["kernel_ms"]["median"]}
            rho1 = torch.zeros((K, T, 2), dtype=torch.float64, device=dev)
            s = timed(torch, ctx, lambda ctx=ctx: ctx.scatter_staged(1, k, 0, rho1.data_ptr(), 0), args.steps, args.warmup, "k_phase")
            s.update({"case": "scatter", "slab": "float" + slab, "n_k": K})
            cases.append(s)
            ctx.trim()
            row["scatter_density_call_ms"] = s["call_ms"]["median"]
            for S in args.species:
                tile = _lib.partial_density_tile(S)
                rho = torch.zeros((K, S, T, 2), dtype=torch.float64, device=dev)
                cr = torch.zeros((K, T, S, S), dtype=torch.float64, device=dev)
                t = timed(torch, ctx,
                          lambda ctx=ctx: ctx.partial_density_staged(1, k, S, labels[S].data_ptr(), rho.data_ptr(), cr.data_ptr()),
                          args.steps, args.warmup, "k_species_density")
                t.update({"case": "partial", "slab": "float" + slab, "n_k": K, "n_species": S, "tile": tile})
                t["pass_tb_per_s"] = round(t["launches"] * nbytes[slab] / (t["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
                cases.append(t)
                row[f"S{S}_pass_ms"] = t["kernel_ms"]["median"]
                row[f"S{S}_call_ms"] = t["call_ms"]["median"]
                row[f"S{S}_launches"] = t["launches"]
                del rho, cr
                ctx.trim()
            first = args.species[0]
            row[f"S{first}_pass_over_scatter"] = round(row[f"S{first}_pass_ms"] / row["scatter_density_call_ms"], 3)
            for S in args.species[1:]:
                row[f"S{S}_pass_over_S{first}"] = round(row[f"S{S}_pass_ms"] / row[f"S{first}_pass_ms"], 3)
            report.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    result = {"metric": "partial_scattering_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A,
              "dim": D, "fft": True, "slab_bytes": nbytes, "report": report, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
