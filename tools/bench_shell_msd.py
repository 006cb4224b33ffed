#!/usr/bin/env python3
"""The shell-resolved MSD (ta_shell_msd_staged): k_shell_msd against the distance pass of the same call, one JSON line, also
written to profiles/.

Values ta_stage_synth'd straight into device slabs (independent unit-variance draws per frame: white noise).  Default 10000
frames x 100000 atoms x 3, on a float64 and a float32 slab, the first 100 atoms the reference group and the remaining 99900 the
observed items, no box.  Two inputs, both conditions, max_lag 256 and 1024:
  sparse : `r_cut` 0.1, r_break = 1.5 r_cut, gap 2: an item is inside in about 1e-4 of the frames, nearly every chunk of origins
           is left after its words have been read.
  dense  : r_cut 1000 (no box: the stand-in for "half the box"): every observed item is inside in every frame, every term is
           taken.  terms = n_observed sum_{tau <= L} (T - tau) per axis; a gated term of one axis is a subtraction and an fma
           (3 flop): tflops = 3 D terms / kernel time, against the vector pipe's nominal 78.6 TFLOP/s in float64.
Per case: msd_ms = the SUM of the k_shell_msd launches of a call (one per block of observed items), series_ms the same for
k_shell_series IN THE SAME CALL, msd_over_series their ratio; bits_ms, fold_ms the two small kernels around it.  Medians of
`steps` (2) timed calls after `warmup` (1).  No ratio is gated: the figures are the result.

    python tools/bench_shell_msd.py [--frames T] [--atoms A] [--reference N] [--r-cut R] [--lags 256,1024] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_pair_lifetime import staged  # noqa: E402
from bench_shell_residence import timed_sum  # noqa: E402

FP64_VECTOR_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--reference", type=int, default=100)
    ap.add_argument("--r-cut", type=float, default=0.1)
    ap.add_argument("--lags", default="256,1024")
    ap.add_argument("--inputs", default="sparse,dense")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    dev = torch.device("cuda", 0)
    T, A, D, Na = args.frames, args.atoms, 3, args.reference
    idx_a, idx_b = np.arange(Na), np.arange(Na, A)
    lags = [min(int(v), T - 1) for v in args.lags.split(",")]
    cases, report = [], {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = staged(_lib, T, A, D, f32)
        runs = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        nb = torch.zeros(T, dtype=torch.float64, device=dev)
        for kind in args.inputs.split(","):
            cuts = dict(r_cut=args.r_cut, r_break=1.5 * args.r_cut, gap=2) if kind == "sparse" else dict(r_cut=1000.0)
            for L in lags:
                sums = torch.zeros((L + 1, D), dtype=torch.float64, device=dev)
                count = torch.zeros(L + 1, dtype=torch.int64, device=dev)
                for condition in ("continuous", "endpoints"):
                    s = timed_sum(torch, ctx, lambda: ctx.shell_msd_staged(condition, L, idx_a=idx_a, idx_b=idx_b, d_sums=sums.data_ptr(),
                                                                           d_count=count.data_ptr(), d_runs=runs.data_ptr(),
                                                                           d_nb=nb.data_ptr(), **cuts),
                                  args.steps, args.warmup, "k_shell_msd")
                    terms = int(count.sum().item())
                    msd_ms, series_ms = s["kernel_ms"]["median"], s["kernels"]["k_shell_series"]
                    s.update({"case": kind, "slab": "float" + name, "max_lag": L, "condition": condition, "terms_per_axis": terms,
                              "mean_inside": float(nb.mean().item()), "msd_ms": msd_ms, "series_ms": series_ms,
                              "msd_over_series": round(msd_ms / series_ms, 4), "bits_ms": s["kernels"]["k_shell_bits"],
                              "fold_ms": s["kernels"]["k_shell_fold"]})
                    key = "%s%s_L%d_%s" % (kind, name, L, condition)
                    report[key + "_msd_ms"], report[key + "_series_ms"] = msd_ms, series_ms
                    report[key + "_msd_over_series"] = s["msd_over_series"]
                    if kind == "dense":
                        assert terms == (A - Na) * sum(T - k for k in range(L + 1)), "dense: every term must be taken"
                        s["gated_terms_per_s"] = D * terms / (msd_ms * 1e-3)
                        s["tflops"] = round(3 * s["gated_terms_per_s"] / 1e12, 3)
                        s["of_fp64_vector_peak"] = round(s["tflops"] / FP64_VECTOR_PEAK_TFLOPS, 4)
                        report[key + "_gated_terms_per_s"] = s["gated_terms_per_s"]
                        report[key + "_of_fp64_vector_peak"] = s["of_fp64_vector_peak"]
                    cases.append(s)
        ctx.stage_free()
        ctx.close()
    result = {"metric": "shell_msd_ms", "device": torch.cuda.get_device_name(0), "shape": [T, A, D], "n_reference": Na,
              "n_observed": A - Na, "r_cut": args.r_cut, "fp64_vector_peak_tflops": FP64_VECTOR_PEAK_TFLOPS, "report": report,
              "cases": cases}
    line = json.dumps(result)
    print(line, flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "shell_msd_bench_%dx%d.json" % (T, A))
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
