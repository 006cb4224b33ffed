#!/usr/bin/env python3
"""The shell-resolved reorientation (ta_shell_orient_staged): k_shell_orient against three comparison points measured in the same
run, one JSON line, also written to profiles/.

Values ta_stage_synth'd straight into device slabs (independent unit-variance draws per frame: white noise).  Default 10000
frames x 99999 atoms x 3 as 33333 bisector triples (3 n, 3 n + 1, 3 n + 2) anchored on their first atom, on a float64 and a
float32 slab; the reference group is the 100 atoms 3 n + 1, n < 100 (partners of the first triples: disjoint from the anchors);
no box.  Two inputs, both conditions, max_lag 256 and 1024:
  sparse : `r_cut` 0.1, r_break = 1.5 r_cut, gap 2: an anchor is inside in about 1 % of the frames; most chunks of origins are
           left after their words have been read, and u is formed only in the others.
  dense  : r_cut 1000: every anchor is inside in every frame, every term is taken.
Per case: orient_ms = the SUM of the k_shell_orient launches of a call (one per block of observed items), and in the same run
  msd_ms      k_shell_msd on the anchors with the same gate and lags (ta_shell_msd_staged);
  series_ms   k_shell_series of the same call;
  korient_ms  ONE k_orient rank-1 pass over the same vectors (ta_orient_staged, total only): the least the route through a
              block of u would have added in front of any gated walk, with block_bytes = 3 n_vectors pitch 16.
Medians of `steps` (3) timed calls after `warmup` (1).  No ratio is gated: the figures are the result.

    python tools/bench_shell_orientation.py [--frames T] [--vectors N] [--reference N] [--r-cut R] [--lags 256,1024] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_pair_lifetime import staged  # noqa: E402
from bench_shell_residence import timed_sum  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--vectors", type=int, default=33333)
    ap.add_argument("--reference", type=int, default=100)
    ap.add_argument("--r-cut", type=float, default=0.1)
    ap.add_argument("--lags", default="256,1024")
    ap.add_argument("--inputs", default="sparse,dense")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    dev = torch.device("cuda", 0)
    T, N, D, Na = args.frames, args.vectors, 3, args.reference
    A = 3 * N
    rows = (3 * np.arange(N)[:, None] + np.arange(3)[None, :]).astype(np.int32)
    idx_a, idx_b = 3 * np.arange(Na) + 1, rows[:, 0].astype(np.int64)
    lags = [min(int(v), T - 1) for v in args.lags.split(",")]
    pitch = (T + 7) // 8 * 8
    cases, report = [], {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = staged(_lib, T, A, D, f32)
        runs = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        nb = torch.zeros(T, dtype=torch.float64, device=dev)
        total = torch.zeros((T, 3), dtype=torch.float64, device=dev)
        k = timed_sum(torch, ctx, lambda: ctx.orient_staged(0, rows, "bisector", d_total=total.data_ptr()), args.steps, args.warmup, "k_orient")
        korient_ms = k["kernel_ms"]["median"]
        ctx.trim()  # (the block of u goes away again: the shell calls never need it)
        report["korient%s_ms" % name] = korient_ms
        for kind in args.inputs.split(","):
            cuts = dict(r_cut=args.r_cut, r_break=1.5 * args.r_cut, gap=2) if kind == "sparse" else dict(r_cut=1000.0)
            for L in lags:
                sums = torch.zeros((L + 1, 3), dtype=torch.float64, device=dev)
                count = torch.zeros(L + 1, dtype=torch.int64, device=dev)
                for condition in ("continuous", "endpoints"):
                    out = dict(d_count=count.data_ptr(), d_runs=runs.data_ptr(), d_nb=nb.data_ptr())
                    m = timed_sum(torch, ctx, lambda: ctx.shell_msd_staged(condition, L, idx_a=idx_a, idx_b=idx_b, d_sums=sums.data_ptr(),
                                                                           **out, **cuts),
                                  args.steps, args.warmup, "k_shell_msd")
                    n_msd = int(count.sum().item())
                    s = timed_sum(torch, ctx, lambda: ctx.shell_orient_staged(condition, L, rows, "bisector", idx_a=idx_a, idx_b=idx_b,
                                                                              d_sums=sums.data_ptr(), **out, **cuts),
                                  args.steps, args.warmup, "k_shell_orient")
                    terms = int(count.sum().item())
                    assert terms == n_msd, "the two calls must gate the same terms"
                    orient_ms, msd_ms, series_ms = s["kernel_ms"]["median"], m["kernel_ms"]["median"], s["kernels"]["k_shell_series"]
                    s.update({"case": kind, "slab": "float" + name, "max_lag": L, "condition": condition, "terms": terms,
                              "mean_inside": float(nb.mean().item()), "orient_ms": orient_ms, "msd_ms": msd_ms, "series_ms": series_ms,
                              "korient_ms": korient_ms, "orient_over_msd": round(orient_ms / msd_ms, 4),
                              "orient_over_korient": round(orient_ms / korient_ms, 4),
                              "orient_over_series": round(orient_ms / series_ms, 4), "bits_ms": s["kernels"]["k_shell_bits"],
                              "fold_ms": s["kernels"]["k_shell_fold"]})
                    key = "%s%s_L%d_%s" % (kind, name, L, condition)
                    for field in ("orient_ms", "msd_ms", "series_ms", "orient_over_msd", "orient_over_korient"):
                        report[key + "_" + field] = s[field]
                    if kind == "dense":
                        assert terms == N * sum(T - j for j in range(L + 1)), "dense: every term must be taken"
                        s["gated_terms_per_s"] = terms / (orient_ms * 1e-3)
                        report[key + "_gated_terms_per_s"] = s["gated_terms_per_s"]
                    cases.append(s)
        ctx.stage_free()
        ctx.close()
    result = {"metric": "shell_orientation_ms", "device": torch.cuda.get_device_name(0), "shape": [T, A, D], "n_vectors": N,
              "mode": "bisector", "n_reference": Na, "r_cut": args.r_cut, "block_bytes": 3 * N * pitch * 16, "report": report,
              "cases": cases}
    line = json.dumps(result)
    print(line, flush=True)
    # (the file is named after the atom count rounded up to thousands: 99999 atoms -> 10000x100000)
    out = args.out or os.path.join(ROOT, "profiles", "shell_orientation_bench_%dx%d.json" % (T, -(-A // 1000) * 1000))
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
