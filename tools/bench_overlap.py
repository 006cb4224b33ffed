#!/usr/bin/env python3
"""The self-overlap pass (ta_overlap_staged, k_overlap) on float64 and float32 device slabs against k_vanhove at the same
lags and against one streaming pass over the same slab, one JSON line.

Two device slabs of the same values (default 10000 frames x 100000 atoms x 3: 24 GB as float64, 12 GB as float32) of
ta_stage_synth's unit-variance white noise (|dr| ~ 2.3 at every lag).  In ONE run:
  sort    : k_species_sort of the float64 slab with one species (ta_species_self_staged: one streaming read of the slab, one
            write of as many bytes) -- the floor for any single pass, on the same staged slab;
  vanhove : per slab type and L in --lags (default 8 32; log-spaced from 1 to n_frames / 2), B = --bins (200), r_max = 8:
            k_vanhove makes the same reads and is the closest kernel the library had before;
  overlap : per slab type, L and C in --cutoffs (default 1 4; the cutoffs 2 for C = 1, else 1, 2, ... C): `steps` timed calls
            after `warmup` warm-ups; `call_ms` = median / min / max of the whole call's device-event interval
            (ta_timing_history), `kernel_ms` = the same of k_overlap's own interval (all its launches of a call together) in
            `steps` MORE calls with the kernel timeline on (ta_kernel_timeline).
  pairs_per_ns = sum_l A (T - tau_l) / k_overlap median;  over_vanhove = k_overlap median / k_vanhove median at the same
  lags;  over_sort = k_overlap median / k_species_sort median.
No time is gated: the figures are the result.

    python tools/bench_overlap.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--lags 8 32] [--cutoffs 1 4]
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
    ap.add_argument("--lags", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--cutoffs", type=int, nargs="+", default=[1, 4], choices=[1, 2, 3, 4])
    ap.add_argument("--bins", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, A, D, B = args.frames, args.atoms, 3, args.bins
    dr = 8.0 / B
    dev = torch.device("cuda", 0)
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
    for L in args.lags:
        lags = log_spaced(np, T, L)
        pairs = float(A) * float((T - lags).sum())
        cnt = torch.zeros((len(lags), B + 1), dtype=torch.int64, device=dev)
        vh_ms = {}
        for slab, ctx in slabs.items():
            t = timed(torch, ctx, lambda ctx=ctx: ctx.vanhove_staged(lags, B, dr, cnt.data_ptr()), args.steps, args.warmup, "k_vanhove")
            t.update({"case": "vanhove", "slab": "float" + slab, "n_lags": int(len(lags))})
            cases.append(t)
            vh_ms[slab] = t["kernel_ms"]["median"]
        for C in args.cutoffs:
            cutoffs = [2.0] if C == 1 else [float(i + 1) for i in range(C)]
            q = torch.zeros((C, len(lags), T), dtype=torch.int64, device=dev)
            row = {"n_lags": int(len(lags)), "lag_max": int(lags[-1]), "n_cutoffs": C, "cutoffs": cutoffs, "pairs": pairs}
            for slab, ctx in slabs.items():
                t = timed(torch, ctx, lambda ctx=ctx: ctx.overlap_staged(lags, cutoffs, q.data_ptr()), args.steps, args.warmup, "k_overlap")
                t.update({"case": "overlap", "slab": "float" + slab, "n_lags": int(len(lags)), "n_cutoffs": C})
                cases.append(t)
                ms = t["kernel_ms"]["median"]
                row[f"k_overlap{slab}_ms"] = ms
                row[f"k_vanhove{slab}_ms"] = vh_ms[slab]
                row[f"call{slab}_ms"] = t["call_ms"]["median"]
                row[f"pairs_per_ns{slab}"] = round(pairs / (ms * 1e6), 3)
                row[f"over_vanhove{slab}"] = round(ms / vh_ms[slab], 3)
                row[f"over_sort{slab}"] = round(ms / sort_ms, 3)
                row[f"launches{slab}"] = t["launches"]
            Q = q.cpu().numpy()
            row["mean_overlap_share"] = [round(float(Q[c].sum()) / pairs, 6) for c in range(C)]
            assert 0 < Q[-1].sum() <= int(pairs)
            report.append(row)
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    result = {"metric": "overlap_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A, "dim": D,
              "vanhove_bins": B, "slots": _lib.overlap_tile(), "slab_bytes": {"64": T * A * D * 8, "32": T * A * D * 4},
              "k_species_sort_ms": sort_ms, "report": report, "cases": cases}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
