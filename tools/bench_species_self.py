#!/usr/bin/env python3
"""Per-species self terms (ta_species_self_staged) on float64 and float32 device slabs against the streaming and lag-sum
comparators, one JSON line.

Values ta_stage_synth'd straight into two device slabs of the same values (default 10000 frames x 100000 atoms x 3: 24 GB
as float64, 12 GB as float32).  In ONE run:
  relayout   : k_relayout of the float64 slab's frame-major copy back into the slab (ta_stage_commit_dev: 24 GB read,
               24 GB written) -- the streaming comparator of (a);
  whole      : per quantity, the lag sums of the whole float64 slab: ta_msd_staged(fft=1) / ta_vacf_fft_staged;
  self       : per quantity, slab type and S in --species (default 1 2 4 8; labels interleaved, atom n is species n % S):
               ta_species_self_staged(fft=1) -- k_species_sort, then S lag-sum calls on the S blocks.
Per case: K timed calls after W warm-ups; `call_ms` = median / min / max of the whole call's device-event interval
(ta_timing_history; relayout: torch events on the stream), `sort_ms` = the same of k_species_sort's own interval in K MORE
calls with the kernel timeline on (ta_kernel_timeline), `kernels` = the per-kernel split of the last of them,
`sort_tb_per_s` = (slab bytes read + float64 bytes written) / sort median.
Reported per (quantity, S):
  a_sort_over_relayout : sort64 median / relayout median (the same 24 + 24 GB);
  b_excess_ms          : self64 call median - (whole call median + sort64 median): what S small blocks cost over one
                         whole-slab lag sum; b_call_over_sum the ratio;
  c_sort32_over_sort64, c_call32_over_call64 : the float32 slab against the float64 slab.
No ratio is gated: the figures are the result.

    python tools/bench_species_self.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--species 1 2 4 8]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SEED = 20240917
QUANTITIES = (("msd", 0), ("vacf", 1))


def stats(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def timed(torch, ctx, call, steps, warmup, kernel=None):
    """{call_ms: median / min / max over `steps` calls} and, with `kernel`, {sort_ms: the same of that kernel's timeline
    interval over `steps` more calls, kernels: {name: ms} of the last one}"""
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
        for name, t in ctx.kernel_timeline(64):
            kernels[name] = round(kernels.get(name, 0.0) + t, 3)
        if kernel:
            own.append(kernels[kernel])
    ctx.set_option("timeline", 0)
    if kernel:
        out["sort_ms"] = stats(own)
    out["kernels"] = kernels
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--species", type=int, nargs="+", default=[1, 2, 4, 8])
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, A, D = args.frames, args.atoms, 3
    dev = torch.device("cuda", 0)
    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = _lib.Context(0)
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 1)
        ctx.stage_synth(0, SEED, 0, A * D)
        slabs[name] = ctx
    nbytes = {"64": T * A * D * 8, "32": T * A * D * 4}
    out_bytes = T * A * D * 8

    # (a)'s comparator: the float64 slab's frame-major copy transposed back into it (the same values)
    c64 = slabs["64"]
    frame_major = torch.empty((T, A * D), dtype=torch.float64, device=dev)
    c64.stage_read_dev(0, frame_major.data_ptr(), A * D)
    torch.cuda.synchronize()
    ms = []
    for i in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        c64.stage_commit_dev(0, frame_major.data_ptr(), A * D, 0, T)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    del frame_major
    torch.cuda.empty_cache()
    relayout = {"case": "relayout", "call_ms": stats(ms), "steps": args.steps}
    relayout["tb_per_s"] = round((nbytes["64"] + out_bytes) / (relayout["call_ms"]["median"] * 1e-3) / 1e12, 3)
    cases, report = [relayout], []

    w = torch.ones(A, dtype=torch.float64, device=dev)
    w[1::2] = -1.0
    lagsum = torch.zeros(T, dtype=torch.float64, device=dev)
    for qname, quantity in QUANTITIES:
        whole_call = (lambda: c64.msd_staged(1, lagsum.data_ptr())) if qname == "msd" else (lambda: c64.vacf_fft_staged(lagsum.data_ptr()))
        whole = timed(torch, c64, whole_call, args.steps, args.warmup)
        whole.update({"case": "whole", "quantity": qname, "slab": "float64"})
        cases.append(whole)
        for S in args.species:
            lab = (np.arange(A) % S).astype(np.int32)
            out = torch.zeros((S, T), dtype=torch.float64, device=dev)
            got = {}
            for slab, ctx in slabs.items():
                t = timed(torch, ctx, lambda: ctx.species_self_staged(quantity, 1, S, lab, out.data_ptr(), w.data_ptr()),
                          args.steps, args.warmup, kernel="k_species_sort")
                t.update({"case": "self", "quantity": qname, "slab": "float" + slab, "n_species": S})
                t["sort_tb_per_s"] = round((nbytes[slab] + out_bytes) / (t["sort_ms"]["median"] * 1e-3) / 1e12, 3)
                got[slab] = t
                cases.append(t)
            s64, s32 = got["64"], got["32"]
            floor = whole["call_ms"]["median"] + s64["sort_ms"]["median"]
            report.append({
                "quantity": qname, "n_species": S,
                "a_sort_over_relayout": round(s64["sort_ms"]["median"] / relayout["call_ms"]["median"], 4),
                "b_excess_ms": round(s64["call_ms"]["median"] - floor, 3),
                "b_call_over_sum": round(s64["call_ms"]["median"] / floor, 4),
                "c_sort32_over_sort64": round(s32["sort_ms"]["median"] / s64["sort_ms"]["median"], 4),
                "c_call32_over_call64": round(s32["call_ms"]["median"] / s64["call_ms"]["median"], 4)})
    result = {"metric": "species_self_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A,
              "dim": D, "fft": True, "slab_bytes": nbytes, "report": report, "cases": cases}
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
