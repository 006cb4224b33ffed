#!/usr/bin/env python3
"""Pair lifetimes (ta_pair_find, ta_pair_lifetime_staged) against the two kernels they were modelled on, one JSON line.

Values ta_stage_synth'd straight into device slabs.  In ONE run:
  find    : default 2000 frames x 20000 atoms x 3 (float64 and float32 slabs), every 10th frame searched, all atoms against
            themselves, no box (the synthetic values are independent unit-variance draws per frame: a pair is within 0.1 in
            about 1e-4 of the frames, within 1.0 in about 9 %, almost always for one frame): ta_pair_find with `r_cut`
            (k_vhd_gather, k_pair_find, k_pair_count, k_pair_list) against ta_vanhove_distinct_staged at lag 0 with B = 200
            bins on the same slab, every 10th frame an origin (k_vhd_gather, k_vhd_pairs).  k_pair_find does strictly less
            per pair (no bin search, no LDS add): find_over_pairs = k_pair_find median / k_vhd_pairs median.
  series  : default 10000 frames x 100000 atoms x 3 (float64 and float32 slabs) with the 10^5 explicit pairs (n, n + 1):
            ta_pair_lifetime_staged asking for the run lengths alone (k_pair_series, k_pair_runs) against ta_orient_staged in
            bond mode, rank 1, on the same slab and the same atom pairs (k_orient): the same gather, one third of the stores.
            series_over_orient = k_pair_series median / k_orient median;  whole: the call with all three outputs, fft = 1.
Per case: `steps` timed calls after `warmup` warm-ups; `kernel_ms` = median / min / max of the named kernel's own interval
with the kernel timeline on (ta_kernel_timeline), `kernels` = the per-kernel split of the last call.  No ratio is gated: the
figures are the result.

    python tools/bench_pair_lifetime.py [--find-frames T] [--find-atoms A] [--frames T] [--atoms A] [--pairs P] [--r-cut R]
                                        [--series-r-cut R]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_scatter import SEED, timed  # noqa: E402  (the same timing loop as the scattering rows)


def staged(_lib, T, A, D, f32):
    ctx = _lib.Context(0)
    ctx.set_option("stage_device_f32", f32)
    ctx.stage_alloc_device(T, A, D, 1)
    ctx.stage_synth(0, SEED, 0, A * D)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--find-frames", type=int, default=2000)
    ap.add_argument("--find-atoms", type=int, default=20000)
    ap.add_argument("--stride", type=int, default=10)
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--r-cut", type=float, default=0.1)
    ap.add_argument("--series-r-cut", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    dev = torch.device("cuda", 0)
    D, cases, report = 3, [], {}

    # ---- the search against the pair histogram
    T, A = args.find_frames, args.find_atoms
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = staged(_lib, T, A, D, f32)
        found = {}

        def search(ctx=ctx, found=found):
            found["n"] = int(ctx.pair_find(args.r_cut, search_stride=args.stride).shape[0])

        t = timed(torch, ctx, search, args.steps, args.warmup, kernel="k_pair_find")
        t.update({"case": "find", "slab": "float" + name, "n_pairs": found["n"]})
        cases.append(t)
        cnt = torch.zeros((1, 201), dtype=torch.int64, device=dev)
        h = timed(torch, ctx, lambda ctx=ctx: ctx.vanhove_distinct_staged([0], 200, 4.0 * args.r_cut / 200, cnt.data_ptr(),
                                                                          origin_stride=args.stride),
                  args.steps, args.warmup, kernel="k_vhd_pairs")
        h.update({"case": "vhd_pairs", "slab": "float" + name})
        cases.append(h)
        report["find%s_ms" % name] = t["kernel_ms"]["median"]
        report["vhd_pairs%s_ms" % name] = h["kernel_ms"]["median"]
        report["find%s_over_pairs" % name] = round(t["kernel_ms"]["median"] / h["kernel_ms"]["median"], 4)
        report["find%s_call_ms" % name] = t["call_ms"]["median"]
        report["n_found"] = found["n"]
        ctx.stage_free()
        ctx.close()

    # ---- the indicator series against the bond vectors
    T, A, P = args.frames, args.atoms, args.pairs
    pairs = np.stack([np.arange(P) % A, (np.arange(P) + 1) % A], axis=1).astype(np.int32)
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = staged(_lib, T, A, D, f32)
        runs = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        ci, nb, c1 = (torch.zeros(T, dtype=torch.float64, device=dev) for _ in range(3))
        s = timed(torch, ctx, lambda ctx=ctx: ctx.pair_lifetime_staged(1, args.series_r_cut, pairs, d_runs=runs.data_ptr()), args.steps,
                  args.warmup, kernel="k_pair_series")
        s.update({"case": "series", "slab": "float" + name, "runs_ms": s["kernels"].get("k_pair_runs")})
        cases.append(s)
        w = timed(torch, ctx, lambda ctx=ctx: ctx.pair_lifetime_staged(1, args.series_r_cut, pairs, d_ci=ci.data_ptr(),
                                                                       d_runs=runs.data_ptr(), d_nb=nb.data_ptr()),
                  args.steps, args.warmup)
        w.update({"case": "whole", "slab": "float" + name})
        cases.append(w)
        ctx.trim()
        o = timed(torch, ctx, lambda ctx=ctx: ctx.orient_staged(1, pairs, "bond", None, None, c1.data_ptr()), args.steps, args.warmup,
                  kernel="k_orient")
        o.update({"case": "orient", "slab": "float" + name})
        cases.append(o)
        report["series%s_ms" % name] = s["kernel_ms"]["median"]
        report["runs%s_ms" % name] = s["runs_ms"]
        report["orient%s_ms" % name] = o["kernel_ms"]["median"]
        report["series%s_over_orient" % name] = round(s["kernel_ms"]["median"] / o["kernel_ms"]["median"], 4)
        report["whole%s_call_ms" % name] = w["call_ms"]["median"]
        ctx.stage_free()
        ctx.close()
    result = {"metric": "pair_lifetime_ms", "device": torch.cuda.get_device_name(0), "find_shape": [args.find_frames, args.find_atoms, D],
              "search_stride": args.stride, "series_shape": [args.frames, args.atoms, D], "n_pairs": P, "r_cut": args.r_cut,
              "series_r_cut": args.series_r_cut, "report": report, "cases": cases}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
