#!/usr/bin/env python3
"""Orientational correlation functions (ta_orient_staged) on float64 and float32 device slabs against the streaming
yardstick, one JSON line.

Values ta_stage_synth'd straight into two device slabs of the same values (default 10000 frames x 99999 atoms x 3 as 33333
triples (a, b, c): 24 GB as float64, 12 GB as float32).  In ONE run:
  sort    : k_species_sort of the float64 slab with one species (ta_species_self_staged: 24 GB read, 24 GB written) -- the
            streaming yardstick of the other rows, on the same staged slab;
  orient  : per slab type, mode (bond, bisector, normal), rank (1: only c1 asked for, 2: only c2) and box (none, a constant
            triclinic box, a per-frame one): ta_orient_staged(fft=1) -- one k_orient launch, then one lag-sum evaluation;
  whole   : per slab type, the bisector with a constant box and all four outputs: both ranks, the sum and the collective part.
Per case: `steps` timed calls after `warmup` warm-ups; `call_ms` = median / min / max of the whole call's device-event
interval (ta_timing_history), `kernel_ms` = the same of k_orient's own interval in `steps` MORE calls with the kernel
timeline on (ta_kernel_timeline), `kernels` = the per-kernel split of the last of them.
  orient_tb_per_s = (atoms per row x n_vectors x n_frames x 3 x element bytes read + block bytes written) / k_orient median;
  sort_tb_per_s   = (slab bytes + float64 bytes) / k_species_sort median;  orient_over_sort = their ratio.
No ratio is gated: the figures are the result.

    python tools/bench_orient.py [--frames T] [--triples N] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_scatter import SEED, timed  # noqa: E402  (the same timing loop as the scattering rows)

MODES = ("bond", "bisector", "normal")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--triples", type=int, default=33333)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, N, D = args.frames, args.triples, 3
    A = 3 * N
    pitch = (T + 7) // 8 * 8
    dev = torch.device("cuda", 0)
    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = _lib.Context(0)
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 1)
        ctx.stage_synth(0, SEED, 0, A * D)
        slabs[name] = ctx
    nbytes = {"64": T * A * D * 8, "32": T * A * D * 4}
    c64 = slabs["64"]
    cases = []

    # the streaming yardstick on the same staged slab
    lab = np.zeros(A, dtype=np.int32)
    out1 = torch.zeros((1, T), dtype=torch.float64, device=dev)
    sort = timed(torch, c64, lambda: c64.species_self_staged(1, 1, 1, lab, out1.data_ptr()), args.steps, args.warmup,
                 kernel="k_species_sort")
    sort["case"] = "sort"
    sort["sort_tb_per_s"] = round((nbytes["64"] + T * A * D * 8) / (sort["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
    cases.append(sort)
    c64.trim()

    triples = np.arange(A, dtype=np.int32).reshape(N, 3)
    box = np.tile(np.array([11.0, 12.0, 13.0, 75.0, 80.0, 70.0]), (T, 1))
    moving = box.copy()
    moving[:, :3] *= (1.0 + 0.02 * np.sin(0.3 * np.arange(T)))[:, None]
    boxes = {"none": None, "constant": box, "per-frame": moving}
    outs = [torch.zeros(s, dtype=torch.float64, device=dev) for s in ((T,), (T,), (T, 3), (T,))]
    report = []
    for mode in MODES:
        idx = np.ascontiguousarray(triples[:, :2]) if mode == "bond" else triples
        for rank in (1, 2):
            block = (3 * N + 1) // 2 * pitch * 16 if rank == 1 else 3 * N * pitch * 16
            for box_name, dims in boxes.items():
                row = {"mode": mode, "rank": rank, "box": box_name}
                for slab, ctx in slabs.items():
                    def call(ctx=ctx):
                        ctx.orient_staged(1, idx, mode, dims, None, outs[0].data_ptr() if rank == 1 else 0,
                                          outs[1].data_ptr() if rank == 2 else 0)
                    t = timed(torch, ctx, call, args.steps, args.warmup, kernel="k_orient")
                    t.update({"case": "orient", "slab": "float" + slab, **row})
                    moved = idx.shape[1] * N * T * 3 * (8 if slab == "64" else 4) + block
                    t["orient_tb_per_s"] = round(moved / (t["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
                    cases.append(t)
                    row["orient%s_ms" % slab] = t["kernel_ms"]["median"]
                    row["orient%s_tb_per_s" % slab] = t["orient_tb_per_s"]
                    row["call%s_ms" % slab] = t["call_ms"]["median"]
                row["orient_over_sort"] = round(row["orient64_tb_per_s"] / sort["sort_tb_per_s"], 4)
                report.append(row)
    whole = {}
    for slab, ctx in slabs.items():
        t = timed(torch, ctx, lambda ctx=ctx: ctx.orient_staged(1, triples, "bisector", box, None, *[o.data_ptr() for o in outs]),
                  args.steps, args.warmup)
        t.update({"case": "whole", "slab": "float" + slab})
        cases.append(t)
        whole["float" + slab] = t["call_ms"]["median"]
    result = {"metric": "orient_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A, "n_vectors": N,
              "dim": D, "fft": True, "slab_bytes": nbytes, "sort_tb_per_s": sort["sort_tb_per_s"],
              "sort_ms": sort["kernel_ms"]["median"], "whole_call_ms": whole, "report": report, "cases": cases}
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
