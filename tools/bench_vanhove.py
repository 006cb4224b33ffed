#!/usr/bin/env python3
"""The self van Hove pass (ta_vanhove_staged, k_vanhove) on float64 and float32 device slabs against one streaming pass over
the same slab, one JSON line.

Two device slabs of the same values (default 10000 frames x 100000 atoms x 3: 24 GB as float64, 12 GB as float32), per
`--data`:
  noise : ta_stage_synth's unit-variance white noise -- every lag has the same broad displacement distribution (|dr| ~ 2.3),
          the bins of a lag are hit evenly;
  walk  : a random walk built on the device (steps of `--step` per frame and component, frame pieces through
          ta_stage_commit_dev) -- small lags concentrate in the first few bins: what same-address LDS atomics cost shows as
          the difference to `noise` at equal lags.
In ONE run:
  sort    : k_species_sort of the float64 slab with one species (ta_species_self_staged: one streaming read of the slab, one
            write of as many bytes) -- the floor for any single pass, on the same staged slab;
  vanhove : per data kind, slab type and L in --lags (default 8 32; log-spaced from 1 to n_frames / 2), B = --bins (200),
            r_max = --rmax (8): `steps` timed calls after `warmup` warm-ups; `call_ms` = median / min / max of the whole call's
            device-event interval (ta_timing_history), `kernel_ms` = the same of k_vanhove's own interval (all its launches of
            a call together) in `steps` MORE calls with the kernel timeline on (ta_kernel_timeline).
  pairs_per_ns  = sum_l A (T - tau_l) / k_vanhove median;   over_sort = k_vanhove median / k_species_sort median.
No time is gated: the figures are the result.  `--profile`: ONE sort call and ONE vanhove call per slab type (L = the first of
--lags) and nothing else -- the run to put under a counters-only profiler (the sort pass's known bytes calibrate the
counter).

    python tools/bench_vanhove.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--lags 8 32] [--data noise walk]
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
        kernels = {name: round(t, 3) for name, t in ctx.kernel_timeline(64)}
        own.append(kernels[kernel])
    out["kernel_ms"] = stats(own)
    out["launches"] = ctx.kernel_launches(kernel)
    ctx.set_option("timeline", 0)
    out["kernels"] = kernels
    return out


def log_spaced(np, T, L):
    """L strictly increasing integer lags from 1 to about T / 2, logarithmically spaced where integers allow"""
    lags = np.rint(np.geomspace(1, max(T // 2, L), L)).astype(np.int64)
    for i in range(1, L):
        lags[i] = max(lags[i], lags[i - 1] + 1)
    return lags[lags < T]


def fill_walk(torch, np, slabs, T, A, D, step, piece=250):
    """the same random walk into both slabs, frame piece by frame piece (float32: the float64 values rounded once)"""
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    carry = torch.zeros((1, A * D), dtype=torch.float64, device="cuda")
    for lo in range(0, T, piece):
        hi = min(T, lo + piece)
        x = carry + torch.cumsum(torch.randn((hi - lo, A * D), dtype=torch.float64, device="cuda", generator=gen) * step, dim=0)
        carry = x[-1:].clone()
        x32 = x.float()
        slabs["64"].stage_commit_dev(0, x.data_ptr(), A * D, lo, hi, dtype=np.float64)
        slabs["32"].stage_commit_dev(0, x32.data_ptr(), A * D, lo, hi, dtype=np.float32)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lags", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--rmax", type=float, default=8.0)
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--data", nargs="+", default=["noise"], choices=["noise", "walk"])
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, A, D, B = args.frames, args.atoms, 3, args.bins
    dr = args.rmax / B
    dev = torch.device("cuda", 0)
    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = _lib.Context(0)
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 1)
        slabs[name] = ctx
    nbytes = {"64": T * A * D * 8, "32": T * A * D * 4}
    c64 = slabs["64"]
    lab = np.zeros(A, dtype=np.int32)
    out1 = torch.zeros((1, T), dtype=torch.float64, device=dev)
    cases, report, sort_ms = [], [], None
    for data in args.data:
        if data == "noise":
            for ctx in slabs.values():
                ctx.stage_synth(0, SEED, 0, A * D)
        else:
            fill_walk(torch, np, slabs, T, A, D, args.step)
        torch.cuda.synchronize()
        if args.profile:
            c64.species_self_staged(1, 1, 1, lab, out1.data_ptr())
            lags = log_spaced(np, T, args.lags[0])
            for ctx in slabs.values():
                cnt = torch.zeros((len(lags), B + 1), dtype=torch.int64, device=dev)
                ctx.vanhove_staged(lags, B, dr, cnt.data_ptr())
            torch.cuda.synchronize()
            continue
        if sort_ms is None:  # the streaming yardstick on the same staged slab (its time does not depend on the values)
            sort = timed(torch, c64, lambda: c64.species_self_staged(1, 1, 1, lab, out1.data_ptr()), args.steps, args.warmup,
                         "k_species_sort")
            sort["case"] = "sort"
            sort_ms = sort["kernel_ms"]["median"]
            cases.append(sort)
            c64.trim()
        for L in args.lags:
            lags = log_spaced(np, T, L)
            pairs = float(A) * float((T - lags).sum())
            cnt = torch.zeros((len(lags), B + 1), dtype=torch.int64, device=dev)
            mom = torch.zeros((len(lags), 2), dtype=torch.float64, device=dev)
            row = {"data": data, "n_lags": int(len(lags)), "lag_max": int(lags[-1]), "pairs": pairs}
            for slab, ctx in slabs.items():
                t = timed(torch, ctx, lambda ctx=ctx: ctx.vanhove_staged(lags, B, dr, cnt.data_ptr(), mom.data_ptr()), args.steps,
                          args.warmup, "k_vanhove")
                t.update({"case": "vanhove", "data": data, "slab": "float" + slab, "n_lags": int(len(lags))})
                cases.append(t)
                ms = t["kernel_ms"]["median"]
                row[f"k_vanhove{slab}_ms"] = ms
                row[f"call{slab}_ms"] = t["call_ms"]["median"]
                row[f"pairs_per_ns{slab}"] = round(pairs / (ms * 1e6), 3)
                row[f"over_sort{slab}"] = round(ms / sort_ms, 3)
                row[f"launches{slab}"] = t["launches"]
            counts = cnt.cpu().numpy()
            row["overflow_share"] = round(float(counts[:, -1].sum()) / pairs, 6)
            row["top_bin_share_first_lag"] = round(float(counts[0].max()) / float(counts[0].sum()), 4)
            assert counts.sum() == int(pairs)
            report.append(row)
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    if args.profile:
        return
    result = {"metric": "vanhove_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A, "dim": D,
              "n_bins": B, "r_max": args.rmax, "slab_bytes": nbytes, "k_species_sort_ms": sort_ms, "report": report, "cases": cases}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
