#!/usr/bin/env python3
"""Bond lifetimes (ta_bond_lifetime_staged) against the pair lifetimes they extend, one JSON line.

Values ta_stage_synth'd straight into device slabs (independent unit-variance draws per frame), default 10000 frames x 100000
atoms x 3, float64 and float32 slabs, 10^5 bonds (n, n + 1, n + 2) and the pairs (n, n + 2) of their first and last atoms.
Every comparison is made in ONE run on the same staged slab, for two inputs:
  short : r_cut 1.0, r_break 1.5 -- a pair is within 1.0 in about 9 % of the frames, almost always for one frame;
  long  : r_cut 5.0, r_break 6.0 -- a pair is within 5.0 in about 99.4 % of the frames: runs of some 170 frames, the input on
          which the filters matter and on which k_pair_runs counts its runs by atomics (they are longer than 8 frames).
Per input and slab:
  triplet_over_pair : k_bond_series with triplets (cos_cut -0.5, cos_break -0.25) / k_pair_series with the pairs
  levels_over_pair  : k_bond_series with n_at = 2 / k_pair_series: the cost of the two levels
  filter_over_runs  : k_pair_filter (n_at = 2) / k_pair_runs of the pair call: the same pairs, a block of the same size (the
                      filter reads AND writes the block: up to twice the bytes).  runs_after_filter*_ms is k_pair_runs on
                      the FILTERED block, whose runs are longer
  whole_over_pair   : the whole ta_bond_lifetime_staged (triplets, gap 2, all three outputs, fft = 1) / ta_pair_lifetime_staged
`steps` timed calls after `warmup` warm-ups, medians; the kernels' own intervals from ta_kernel_timeline.  No ratio is gated.

    python tools/bench_bond_lifetime.py [--frames T] [--atoms A] [--bonds P] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_pair_lifetime import staged  # noqa: E402
from bench_scatter import timed  # noqa: E402  (the same timing loop as the scattering rows)

INPUTS = {"short": (1.0, 1.5), "long": (5.0, 6.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--bonds", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    dev = torch.device("cuda", 0)
    T, A, P, D = args.frames, args.atoms, args.bonds, 3
    n = np.arange(P)
    triplets = np.stack([n % A, (n + 1) % A, (n + 2) % A], axis=1).astype(np.int32)
    pairs = np.ascontiguousarray(triplets[:, ::2])
    cases, report = [], {}
    for slab, f32 in (("64", 0), ("32", 1)):
        ctx = staged(_lib, T, A, D, f32)
        runs = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        ci, nb = (torch.zeros(T, dtype=torch.float64, device=dev) for _ in range(2))
        out3 = dict(d_ci=ci.data_ptr(), d_runs=runs.data_ptr(), d_nb=nb.data_ptr())
        for name, (r_cut, r_break) in INPUTS.items():
            key = f"{name}{slab}"

            def run(case, call, kernel=None):
                t = timed(torch, ctx, call, args.steps, args.warmup, kernel=kernel)
                t.update({"case": case, "slab": "float" + slab, "input": name})
                cases.append(t)
                return t

            ps = run("pair_series", lambda: ctx.pair_lifetime_staged(1, r_cut, pairs, d_runs=runs.data_ptr()), "k_pair_series")
            b3 = run("bond_series_triplets", lambda: ctx.bond_lifetime_staged(
                1, triplets, r_cut, r_break=r_break, cos_cut=-0.5, cos_break=-0.25, gap=2, d_runs=runs.data_ptr()), "k_bond_series")
            b2 = run("bond_series_pairs", lambda: ctx.bond_lifetime_staged(1, pairs, r_cut, r_break=r_break, gap=2, d_runs=runs.data_ptr()),
                     "k_bond_series")
            wp = run("whole_pair", lambda: ctx.pair_lifetime_staged(1, r_cut, pairs, **out3))
            wb = run("whole_bond", lambda: ctx.bond_lifetime_staged(1, triplets, r_cut, r_break=r_break, cos_cut=-0.5, cos_break=-0.25,
                                                                    gap=2, **out3))
            series = ps["kernel_ms"]["median"]
            report[key] = {
                "pair_series_ms": series, "pair_runs_ms": ps["kernels"].get("k_pair_runs"),
                "bond_series3_ms": b3["kernel_ms"]["median"], "bond_series2_ms": b2["kernel_ms"]["median"],
                "filter3_ms": b3["kernels"].get("k_pair_filter"), "runs_after_filter3_ms": b3["kernels"].get("k_pair_runs"),
                "filter2_ms": b2["kernels"].get("k_pair_filter"), "runs_after_filter2_ms": b2["kernels"].get("k_pair_runs"),
                "triplet_over_pair": round(b3["kernel_ms"]["median"] / series, 4),
                "levels_over_pair": round(b2["kernel_ms"]["median"] / series, 4),
                "filter_over_runs": round(b2["kernels"]["k_pair_filter"] / ps["kernels"]["k_pair_runs"], 4),
                "whole_pair_call_ms": wp["call_ms"]["median"], "whole_bond_call_ms": wb["call_ms"]["median"],
                "whole_over_pair": round(wb["call_ms"]["median"] / wp["call_ms"]["median"], 4),
                "bonded_fraction_triplets": round(float(nb.sum().item()) / (float(T) * P), 4),
            }
        ctx.stage_free()
        ctx.close()
    print(json.dumps({"metric": "bond_lifetime_ms", "device": torch.cuda.get_device_name(0), "shape": [T, A, D], "n_bonds": P,
                      "inputs": INPUTS, "gap": 2, "report": report, "cases": cases}), flush=True)


if __name__ == "__main__":
    main()
