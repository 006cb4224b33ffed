#!/usr/bin/env python3
"""The overlap-density pass (ta_overlap_density_staged, k_overlap_density) on float64 and float32 device slabs against
k_overlap at the same lags and cutoffs and k_species_density (one species) at the same wavevectors, one JSON line.

Two device slabs of the same values (default 10000 frames x 100000 atoms x 3: 24 GB as float64, 12 GB as float32) of
ta_stage_synth's unit-variance white noise (|dr| ~ 2.3 at every lag).  In ONE run, on the same staged slabs:
  sort    : k_species_sort of the float64 slab with one species (one streaming read of the slab, one write of as many
            bytes): half of it stands for the streaming share of a single pass;
  overlap : per slab type and C in --cutoffs (default 1 4; the cutoffs 2 for C = 1, else 1, 2, ... C), L = --lags (8;
            log-spaced from 1 to n_frames / 2) with "overlap_chunk" set to k_overlap_density's lags per launch, so that
            the launches compare one to one;
  density : per slab type and K in --kvectors (default 1 4 16; random within +-6 rad per length unit), k_species_density
            with one species and "partial_chunk" set to k_overlap_density's wavevectors per launch;
  overlap_density : per slab type, C and K: `steps` timed calls after `warmup` warm-ups; `call_ms` = median / min / max of
            the whole call's device-event interval (ta_timing_history), `kernel_ms` = the same of k_overlap_density's own
            interval (all its launches of a call together) in `steps` MORE calls with the kernel timeline on.
  per launch: k_overlap_density median / launches against `expected` = k_overlap per launch + max(0, k_species_density per
  launch - sort / 2), the design's expectation; over_expected is their ratio.
No time is gated: the figures are the result.

    python tools/bench_overlap_density.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--lags 8] [--cutoffs 1 4]
                                          [--kvectors 1 4 16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_vanhove import SEED, log_spaced, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lags", type=int, default=8)
    ap.add_argument("--cutoffs", type=int, nargs="+", default=[1, 4], choices=[1, 2, 3, 4])
    ap.add_argument("--kvectors", type=int, nargs="+", default=[1, 4, 16])
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, A, D = args.frames, args.atoms, 3
    dev = torch.device("cuda", 0)
    tile = _lib.overlap_density_tile()
    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = _lib.Context(0)
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 1)
        ctx.stage_synth(0, SEED, 0, A * D)
        slabs[name] = ctx
    torch.cuda.synchronize()
    c64 = slabs["64"]
    lab = np.zeros(A, dtype=np.int32)
    out1 = torch.zeros((1, T), dtype=torch.float64, device=dev)
    cases, report = [], []
    sort = timed(torch, c64, lambda: c64.species_self_staged(1, 1, 1, lab, out1.data_ptr()), args.steps, args.warmup, "k_species_sort")
    sort["case"] = "sort"
    sort_ms = sort["kernel_ms"]["median"]
    cases.append(sort)
    c64.trim()
    lags = log_spaced(np, T, args.lags)
    pairs = float(A) * float((T - lags).sum())
    kall = np.random.default_rng(SEED).uniform(-6.0, 6.0, size=(max(args.kvectors), D))
    d_lab = torch.zeros(A, dtype=torch.int32, device=dev)
    # k_species_density, one species, the same wavevectors per launch
    den = {}
    for K in args.kvectors:
        rho = torch.zeros((K, 1, T, 2), dtype=torch.float64, device=dev)
        for slab, ctx in slabs.items():
            ctx.set_option("partial_chunk", tile["KC"])
            t = timed(torch, ctx, lambda ctx=ctx: ctx.partial_density_staged(0, kall[:K], 1, d_lab.data_ptr(), rho.data_ptr()),
                      args.steps, args.warmup, "k_species_density")
            ctx.set_option("partial_chunk", 0)
            t.update({"case": "density", "slab": "float" + slab, "n_k": K})
            cases.append(t)
            den[(K, slab)] = t["kernel_ms"]["median"] / t["launches"]
    for C in args.cutoffs:
        cutoffs = [2.0] if C == 1 else [float(i + 1) for i in range(C)]
        Lc = min(len(lags), max(1, tile["SL"] // C))
        q = torch.zeros((C, len(lags), T), dtype=torch.int64, device=dev)
        ov = {}
        for slab, ctx in slabs.items():
            ctx.set_option("overlap_chunk", Lc)
            t = timed(torch, ctx, lambda ctx=ctx: ctx.overlap_staged(lags, cutoffs, q.data_ptr()), args.steps, args.warmup, "k_overlap")
            ctx.set_option("overlap_chunk", 0)
            t.update({"case": "overlap", "slab": "float" + slab, "n_lags": int(len(lags)), "n_cutoffs": C, "lags_per_launch": Lc})
            cases.append(t)
            ov[slab] = t["kernel_ms"]["median"] / t["launches"]
        Q = q.cpu().numpy()
        for K in args.kvectors:
            w = torch.zeros((K, C, len(lags), T, 2), dtype=torch.float64, device=dev)
            row = {"n_k": K, "n_lags": int(len(lags)), "lag_max": int(lags[-1]), "n_cutoffs": C, "cutoffs": cutoffs,
                   "lags_per_launch": Lc, "pairs": pairs}
            for slab, ctx in slabs.items():
                t = timed(torch, ctx, lambda ctx=ctx: ctx.overlap_density_staged(kall[:K], lags, cutoffs, w.data_ptr()),
                          args.steps, args.warmup, "k_overlap_density")
                t.update({"case": "overlap_density", "slab": "float" + slab, "n_k": K, "n_lags": int(len(lags)), "n_cutoffs": C})
                cases.append(t)
                ms, n = t["kernel_ms"]["median"], t["launches"]
                expected = ov[slab] + max(0.0, den[(K, slab)] - 0.5 * sort_ms)
                row[f"k_overlap_density{slab}_ms"] = ms
                row[f"call{slab}_ms"] = t["call_ms"]["median"]
                row[f"launches{slab}"] = n
                row[f"per_launch{slab}_ms"] = round(ms / n, 3)
                row[f"k_overlap_per_launch{slab}_ms"] = round(ov[slab], 3)
                row[f"k_species_density_per_launch{slab}_ms"] = round(den[(K, slab)], 3)
                row[f"expected{slab}_ms"] = round(expected, 3)
                row[f"over_expected{slab}"] = round(ms / n / expected, 3)
                row[f"sum_ms{slab}"] = t["kernels"].get("k_overlap_density_sum")
            Wh = w.cpu().numpy()
            # (white noise: the sums are O(sqrt N); what is checked is that the counts behind them are k_overlap's)
            assert float(np.abs(Wh).max()) <= float(Q.max()) + 1e-6 and float(np.abs(Wh).max()) > 0.0
            report.append(row)
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    result = {"metric": "overlap_density_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A,
              "dim": D, "tile": tile, "slab_bytes": {"64": T * A * D * 8, "32": T * A * D * 4}, "k_species_sort_ms": sort_ms,
              "report": report, "cases": cases}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
