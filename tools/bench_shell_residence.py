#!/usr/bin/env python3
"""Shell residence times (ta_shell_residence_staged) against the pair search they share their distance pass with, one JSON
line, also written to profiles/.

Values ta_stage_synth'd straight into device slabs (independent unit-variance draws per frame: white noise; an item is within
0.1 of a given other one in about 1e-4 of the frames).  Default 10000 frames x 100000 atoms x 3, on a float64 and a float32
slab, the first 100 atoms the reference group and the remaining 99900 the observed items, no box.  In ONE run, over the SAME
item lists and the same number of frames:
  shell   : ta_shell_residence_staged with `r_cut`, r_break = 1.5 r_cut, gap 2, all three outputs, fft = 1 (k_vhd_gather,
            k_shell_series, k_pair_filter, k_pair_runs, the lag sums, the species sum).  shell_ms = the SUM of the
            k_shell_series launches of a call (one per chunk of 64-frame words).
  find    : ta_pair_find with the same `r_cut` on every frame (k_vhd_gather, k_pair_find, k_pair_count, k_pair_list).
            find_ms = the SUM of the k_pair_find launches of a call.
Both kernels do the same distance arithmetic per (reference item, observed item, frame); k_shell_series adds two compares and
its stores and drops the atomics: shell_over_find = shell_ms / find_ms.  Medians of `steps` (3) timed calls after `warmup`
(1) warm-up.  No ratio is gated: the figures are the result.

    python tools/bench_shell_residence.py [--frames T] [--atoms A] [--reference N] [--r-cut R] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_pair_lifetime import staged  # noqa: E402
from bench_scatter import stats  # noqa: E402


def timed_sum(torch, ctx, call, steps, warmup, kernel):
    """bench_scatter.timed for a kernel launched several times per call: kernel_ms is the sum of its launches"""
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
        for name, t in ctx.kernel_timeline(65536):
            kernels[name] = round(kernels.get(name, 0.0) + t, 3)
        own.append(kernels[kernel])
    out["kernel_ms"] = stats(own)
    out["launches"] = ctx.kernel_launches(kernel)
    out["kernels"] = kernels
    ctx.set_option("timeline", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--reference", type=int, default=100)
    ap.add_argument("--r-cut", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    dev = torch.device("cuda", 0)
    T, A, D, Na = args.frames, args.atoms, 3, args.reference
    idx_a, idx_b = np.arange(Na), np.arange(Na, A)
    cases, report = [], {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = staged(_lib, T, A, D, f32)
        runs = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        ci, nb = (torch.zeros(T, dtype=torch.float64, device=dev) for _ in range(2))
        s = timed_sum(torch, ctx, lambda ctx=ctx: ctx.shell_residence_staged(1, args.r_cut, r_break=1.5 * args.r_cut, gap=2, idx_a=idx_a,
                                                                             idx_b=idx_b, d_ci=ci.data_ptr(), d_runs=runs.data_ptr(),
                                                                             d_nb=nb.data_ptr()),
                      args.steps, args.warmup, "k_shell_series")
        s.update({"case": "shell", "slab": "float" + name, "mean_inside": float(nb.mean().item())})
        cases.append(s)
        ctx.trim()
        found = {}

        def search(ctx=ctx, found=found):
            found["n"] = int(ctx.pair_find(args.r_cut, idx_a=idx_a, idx_b=idx_b).shape[0])

        f = timed_sum(torch, ctx, search, args.steps, args.warmup, "k_pair_find")
        f.update({"case": "find", "slab": "float" + name, "n_pairs": found["n"]})
        cases.append(f)
        report["shell%s_ms" % name] = s["kernel_ms"]["median"]
        report["find%s_ms" % name] = f["kernel_ms"]["median"]
        report["shell%s_over_find" % name] = round(s["kernel_ms"]["median"] / f["kernel_ms"]["median"], 4)
        report["shell%s_call_ms" % name] = s["call_ms"]["median"]
        report["find%s_call_ms" % name] = f["call_ms"]["median"]
        ctx.stage_free()
        ctx.close()
    result = {"metric": "shell_residence_ms", "device": torch.cuda.get_device_name(0), "shape": [T, A, D], "n_reference": Na,
              "n_observed": A - Na, "r_cut": args.r_cut, "report": report, "cases": cases}
    line = json.dumps(result)
    print(line, flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "shell_residence_bench_%dx%d.json" % (T, A))
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
