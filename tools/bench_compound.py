#!/usr/bin/env python3
"""ta_compound (k_compound) on float64 and float32 device slabs against the streaming comparators, one JSON line.

Values ta_stage_synth'd straight into a device slab (default 10000 frames x 100000 atoms x 3: 24 GB as float64, 12 GB as
float32).  ta_compound REPLACES the slab, so every timed call starts from a fresh ta_stage_alloc_device + ta_stage_synth
(not timed).  In ONE run:
  relayout : k_relayout of the float64 slab's frame-major copy back into the slab (ta_stage_commit_dev: 24 GB read, 24 GB
             written);
  sort     : k_species_sort with one species on the same slab (ta_species_self_staged, its timeline interval): it reads
             the same bytes and writes at least as many as any compound plan, so it is the comparator;
  compound : per slab type, plan and with / without the barycentric term (frame weights 1 / n_atoms):
               size1 : every atom its own compound;      size4 : compounds of four atoms;
               mix   : electrolyte-like, groups of 56 atoms = compounds of 1, 15, 10, 10, 10, 10 atoms;
             each "contiguous" (a compound's atoms are neighbours) and "interleaved" (atom n in compound n % C; the mix: atom
             n in group n % G, the group split in that order) -- for size1 the two coincide and run once.
Per case: K timed calls after W warm-ups; `call_ms` = median / min / max of the whole call's device-event interval
(ta_timing_history), `kernel_ms` = the same of k_compound's own timeline interval (ta_kernel_timeline, K more calls),
`kernels` = the per-kernel split of the last of them, `tb_per_s` = (slab bytes + new slab bytes) / kernel median,
`over_sort` = kernel median / the sort pass's median on the slab of the same element type.
No ratio is gated: the figures are the result.

    python tools/bench_compound.py [--frames T] [--atoms A] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SEED = 20240917
MIX = (1, 15, 10, 10, 10, 10)


def stats(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def plans(np, A):
    """{name: (offsets, members)}"""
    out = {"size1": (np.arange(A + 1, dtype=np.int64), np.arange(A, dtype=np.int32))}
    C = A // 4
    off4 = np.arange(C + 1, dtype=np.int64) * 4
    out["size4_contiguous"] = (off4, np.arange(4 * C, dtype=np.int32))
    out["size4_interleaved"] = (off4, (np.arange(4)[None, :] * C + np.arange(C)[:, None]).astype(np.int32).ravel())
    G, g = A // sum(MIX), sum(MIX)
    offm = np.concatenate([[0], np.cumsum(np.tile(MIX, G))]).astype(np.int64)
    out["mix_contiguous"] = (offm, np.arange(g * G, dtype=np.int32))
    out["mix_interleaved"] = (offm, (np.arange(g)[None, :] * G + np.arange(G)[:, None]).astype(np.int32).ravel())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, A, D = args.frames, args.atoms, 3
    dev = torch.device("cuda", 0)
    nbytes = {"64": T * A * D * 8, "32": T * A * D * 4}
    ctx = _lib.Context(0)

    def fresh(f32):
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 1)
        ctx.stage_synth(0, SEED, 0, A * D)

    # the comparators, on the slabs a compound call would start from
    fresh(0)
    frame_major = torch.empty((T, A * D), dtype=torch.float64, device=dev)
    ctx.stage_read_dev(0, frame_major.data_ptr(), A * D)
    torch.cuda.synchronize()
    ms = []
    for i in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.stage_commit_dev(0, frame_major.data_ptr(), A * D, 0, T)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    del frame_major
    torch.cuda.empty_cache()
    relayout = {"case": "relayout", "call_ms": stats(ms), "steps": args.steps}
    relayout["tb_per_s"] = round(2 * nbytes["64"] / (relayout["call_ms"]["median"] * 1e-3) / 1e12, 3)
    cases, sort_ms = [relayout], {}
    lab = np.zeros(A, dtype=np.int32)
    out = torch.zeros((1, T), dtype=torch.float64, device=dev)
    for slab, f32 in (("64", 0), ("32", 1)):
        fresh(f32)
        ctx.set_option("timeline", 1)
        own = []
        for i in range(args.warmup + args.steps):
            ctx.species_self_staged(_lib.SELF_VACF, 1, 1, lab, out.data_ptr())
            torch.cuda.synchronize()
            if i >= args.warmup:
                own.append(dict(ctx.kernel_timeline(64))["k_species_sort"])
        ctx.trim()  # the sorted slab (the input's size as float64) goes before the compound calls allocate theirs
        t = {"case": "sort", "slab": "float" + slab, "kernel_ms": stats(own), "steps": args.steps}
        t["tb_per_s"] = round((nbytes[slab] + nbytes["64"]) / (t["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
        sort_ms[slab] = t["kernel_ms"]["median"]
        cases.append(t)

    u = np.full(A, 1.0 / A)
    for name, (off, mem) in plans(np, A).items():
        C = off.size - 1
        w = np.full(mem.size, 1.0) / np.repeat(np.diff(off), np.diff(off))
        new_bytes = (C * D + 1) // 2 * ((T + 7) // 8 * 8) * 16
        for slab, f32 in (("64", 0), ("32", 1)):
            for frame in (None, u):
                call, own, kernels = [], [], {}
                for i in range(args.warmup + 2 * args.steps):
                    timeline = i >= args.warmup + args.steps
                    fresh(f32)
                    ctx.set_option("timeline", int(timeline))
                    ctx.compound(off, mem, w, frame)
                    if timeline:
                        kernels = {}
                        for k, v in ctx.kernel_timeline(64):
                            kernels[k] = round(kernels.get(k, 0.0) + v, 3)
                        own.append(kernels["k_compound"])
                    elif i >= args.warmup:
                        call.append(ctx.timing_history(1)[0][0])
                t = {"case": "compound", "plan": name, "slab": "float" + slab, "barycentric": frame is not None,
                     "n_compounds": C, "n_members": int(mem.size), "call_ms": stats(call), "kernel_ms": stats(own),
                     "kernels": kernels, "steps": args.steps}
                t["tb_per_s"] = round((nbytes[slab] * mem.size / A + new_bytes) / (t["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
                t["over_sort"] = round(t["kernel_ms"]["median"] / sort_ms[slab], 4)
                cases.append(t)
    result = {"metric": "compound_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A, "dim": D,
              "slab_bytes": nbytes, "relayout_ms": relayout["call_ms"]["median"], "sort_ms": sort_ms, "cases": cases}
    ctx.stage_free()
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
