#!/usr/bin/env python3
"""Chain normal modes (ta_chain_modes_staged) on float64 and float32 device slabs against two yardsticks on the same staged
values, one JSON line.

Values ta_stage_synth'd straight into two device slabs of the same values (default 10000 frames x 100000 atoms x 3 as 1000
chains of 100 consecutive atoms: 24 GB as float64, 12 GB as float32).  In ONE run:
  chain    : per slab type, Q = 1, 4 and 16 Rouse modes and box (none, a constant triclinic box, a per-frame one):
             ta_chain_modes_staged(fft=1) -- ceil(Q / tile modes) k_chain_modes launches per batch, then one lag-sum evaluation
             per mode;
  compound : (a) per slab type, k_compound with the chains as compounds and no weights (ta_compound: the same read with no
             image step and one output per chain).  ta_compound replaces the slab, so every call runs on a re-synthesised one;
  composed : (b) the route without k_chain_modes: one ta_compound call per mode with that mode's cosine weights, each on a
             re-synthesised slab; only the kernels are timed (the staging again, the unwrap pass and the lag sums that route
             also needs are left out: it is a lower bound of that route).
Per chain case: `steps` timed calls after `warmup` warm-ups; `call_ms` = median / min / max of the whole call's device-event
interval (ta_timing_history), `kernel_ms` = the same of ALL k_chain_modes launches of a call in `steps` MORE calls with the
kernel timeline on (ta_kernel_timeline adds up the launches of one name), `launch_ms` = its median over the `launches`,
`kernels` = the per-kernel split of the last of them.
  slab_tb_per_s     = slab bytes / one k_chain_modes launch;   launch_over_compound = that launch / yardstick (a)'s k_compound
                      (its median; launch_over_fastest_compound: the fastest k_compound of all calls of the run, (b)'s included);
  call_over_composed = the whole call / the sum of route (b)'s Q k_compound kernels.
No ratio is gated: the figures are the result.

    python tools/bench_chain_modes.py [--frames T] [--chains C] [--beads N] [--steps K] [--warmup W] [--boxes ...] [--no-yardsticks]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_scatter import SEED, stats, timed  # noqa: E402  (the same timing loop as the scattering rows)

QS = (1, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--beads", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--boxes", nargs="+", default=["none", "constant", "per-frame"], choices=["none", "constant", "per-frame"])
    ap.add_argument("--no-yardsticks", action="store_true", help="the chain cases alone (comparing builds of the kernel's tile)")
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib
    from transport_analysis_amd.rouse import rouse_coefficients

    T, C, N, D = args.frames, args.chains, args.beads, 3
    A = C * N
    dev = torch.device("cuda", 0)

    def synth(ctx, f32):
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 1)
        ctx.stage_synth(0, SEED, 0, A * D)

    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        slabs[name] = _lib.Context(0)
        synth(slabs[name], f32)
    nbytes = {"64": T * A * D * 8, "32": T * A * D * 4}
    members = np.arange(A, dtype=np.int32).reshape(C, N)
    box = np.tile(np.array([11.0, 12.0, 13.0, 75.0, 80.0, 70.0]), (T, 1))
    moving = box.copy()
    moving[:, :3] *= (1.0 + 0.02 * np.sin(0.3 * np.arange(T)))[:, None]
    boxes = {k: v for k, v in {"none": None, "constant": box, "per-frame": moving}.items() if k in args.boxes}
    tile = _lib.chain_modes_tile()
    out = torch.zeros((max(QS), T), dtype=torch.float64, device=dev)
    cases, report = [], []
    for Q in QS:
        coeff = rouse_coefficients(N, np.arange(1, Q + 1))
        for box_name, dims in boxes.items():
            row = {"modes": Q, "box": box_name}
            for slab, ctx in slabs.items():
                t = timed(torch, ctx, lambda ctx=ctx: ctx.chain_modes_staged(1, members, coeff, dims, out.data_ptr()), args.steps,
                          args.warmup, kernel="k_chain_modes")
                t.update({"case": "chain", "slab": "float" + slab, **row})
                t["launch_ms"] = round(t["kernel_ms"]["median"] / t["launches"], 3)
                t["slab_tb_per_s"] = round(nbytes[slab] / (t["launch_ms"] * 1e-3) / 1e12, 3)
                cases.append(t)
                row["launch%s_ms" % slab] = t["launch_ms"]
                row["launches%s" % slab] = t["launches"]
                row["slab%s_tb_per_s" % slab] = t["slab_tb_per_s"]
                row["call%s_ms" % slab] = t["call_ms"]["median"]
            report.append(row)
    for ctx in slabs.values():
        ctx.trim()

    # the yardsticks: ta_compound replaces the slab, so each call gets a re-synthesised one; its main kernel is k_compound
    offsets = np.arange(C + 1, dtype=np.int64) * N
    flat = members.ravel()

    def compound_ms(ctx, f32, weights):
        synth(ctx, f32)
        ctx.compound(offsets, flat, weights)
        return ctx.last_timing()[1]

    yard, composed, fastest = {}, {}, {}
    for (slab, ctx), f32 in zip(() if args.no_yardsticks else slabs.items(), (0, 1)):
        compound_ms(ctx, f32, None)  # (warm-up)
        plain = [compound_ms(ctx, f32, None) for _ in range(args.steps)]
        yard[slab] = stats(plain)
        per_mode = [compound_ms(ctx, f32, np.tile(rouse_coefficients(N, [p])[0], C)) for p in range(1, max(QS) + 1)]
        composed[slab] = {str(Q): round(sum(per_mode[:Q]), 3) for Q in QS}
        # (k_compound writes a slab that ta_compound has just allocated; the fastest of all its calls is kept beside the median)
        fastest[slab] = round(min(plain + per_mode), 3)
        cases.append({"case": "compound", "slab": "float" + slab, "kernel_ms": yard[slab], "fastest_of_all_calls_ms": fastest[slab],
                      "slab_tb_per_s": round(nbytes[slab] / (yard[slab]["median"] * 1e-3) / 1e12, 3)})
        cases.append({"case": "composed", "slab": "float" + slab, "k_compound_ms_per_mode": [round(v, 3) for v in per_mode],
                      "kernels_ms": composed[slab]})
    for row in report:
        for slab in yard:
            row["launch%s_over_compound" % slab] = round(row["launch%s_ms" % slab] / yard[slab]["median"], 3)
            row["launch%s_over_fastest_compound" % slab] = round(row["launch%s_ms" % slab] / fastest[slab], 3)
            row["call%s_over_composed" % slab] = round(row["call%s_ms" % slab] / composed[slab][str(row["modes"])], 3)
    result = {"metric": "chain_modes_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A,
              "n_chains": C, "chain_len": N, "dim": D, "fft": True, "tile": tile, "slab_bytes": nbytes,
              "compound_ms": {s: yard[s]["median"] for s in yard}, "compound_fastest_ms": fastest, "composed_kernels_ms": composed, "report": report, "cases": cases}
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
