#!/usr/bin/env python3
"""Green-Kubo species currents (ta_current_staged) on float64 and float32 device slabs against the Onsager moment pass,
one JSON line.

Velocities ta_stage_synth'd straight into two device slabs of the same values (default 10000 frames x 100000 atoms x 3:
24 GB as float64, 12 GB as float32).  In ONE run, per S in --species (default 1 2 4 8), labels interleaved (atom n is
species n % S):
  on the float64 slab
      moment64      : ta_onsager_staged without the cross term -- k_species_moment, the pass the new kernel is modelled on;
      current64     : ta_current_staged without the cross term -- k_species_current<double>;
      whole64       : currents + C (T, S, S) (fft=True);
  on the float32 slab
      current32     : ta_current_staged without the cross term -- k_species_current<float>, no widening;
      whole32       : currents + C;
      widen32       : ta_onsager_staged without the cross term -- k_widen_f32 + k_species_moment, the only route to a
                      collective sum of a float32 slab before this kernel;
      widen32_whole : the same with its cross MSD.
Per case: K timed calls after W warm-ups; `pass_ms` = median / min / max of the main kernel's device-event interval
(ta_timing_history; the pass is the main kernel of a call without the cross term), `call_ms` = the same of the whole call,
`kernels` = the per-kernel split of one more call (ta_kernel_timeline), `hbm_roof_frac` = slab bytes / pass median / 8 TB/s.
Gates per S:
  a_float64 : current64's pass median <= moment64's pass median + (max - min) of moment64's K passes;
  b_pass    : current32's pass median < current64's pass median;
  b_call    : whole32's call median < widen32_whole's, and current32's < widen32's (ratios reported).

    python tools/bench_current.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--species 1 2 4 8]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
SEED = 20240917


def stats(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def timed(torch, ctx, call, steps, warmup):
    """({call_ms, pass_ms}: median / min / max over `steps` calls, {kernel: ms} of one more call)"""
    ctx.set_option("timeline", 0)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    hist = ctx.timing_history(steps)
    ctx.set_option("timeline", 1)
    call()
    torch.cuda.synchronize()
    kernels = {}
    for name, t in ctx.kernel_timeline(64):
        kernels[name] = round(kernels.get(name, 0.0) + t, 3)
    ctx.set_option("timeline", 0)
    return {"call_ms": stats(t for t, _ in hist), "pass_ms": stats(m for _, m in hist), "steps": len(hist)}, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--species", type=int, nargs="+", default=[1, 2, 4, 8])
    args = ap.parse_args()
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

    w = torch.ones(A, dtype=torch.float64, device=dev)
    w[1::2] = -1.0
    cases, gates = [], []
    for S in args.species:
        sums = torch.zeros((S, T, D), dtype=torch.float64, device=dev)
        cross = torch.zeros((T, S, S), dtype=torch.float64, device=dev)
        lab = (torch.arange(A, device=dev) % S).to(torch.int32)

        def current(ctx, d_cross):
            return lambda: ctx.current_staged(True, S, lab.data_ptr(), sums.data_ptr(), w.data_ptr(), d_cross)

        def moment(ctx, d_cross):
            return lambda: ctx.onsager_staged(True, S, lab.data_ptr(), sums.data_ptr(), w.data_ptr(), d_cross)

        plan = [("moment64", "64", moment, 0, "k_species_moment"), ("current64", "64", current, 0, "k_species_current"),
                ("whole64", "64", current, cross.data_ptr(), "k_species_current"),
                ("current32", "32", current, 0, "k_species_current"),
                ("whole32", "32", current, cross.data_ptr(), "k_species_current"),
                ("widen32", "32", moment, 0, "k_species_moment"),
                ("widen32_whole", "32", moment, cross.data_ptr(), "k_species_moment")]
        got = {}
        for case, slab, make, d_cross, kernel in plan:
            t, kernels = timed(torch, slabs[slab], make(slabs[slab], d_cross), args.steps, args.warmup)
            t.update({"n_species": S, "case": case, "slab": "float" + slab, "kernels": kernels, "pass_kernel_ms": kernels[kernel]})
            if not d_cross and not case.startswith("widen"):  # (the call's main kernel is the pass)
                t["hbm_roof_frac"] = round(nbytes[slab] / (t["pass_ms"]["median"] * 1e-3) / HBM_BYTES_PER_S, 4)
            else:
                del t["pass_ms"]  # an FFT evaluation after the pass is the main kernel there
            got[case] = t
            cases.append(t)
        m64, c64, c32 = got["moment64"]["pass_ms"], got["current64"]["pass_ms"], got["current32"]["pass_ms"]
        spread = round(m64["max"] - m64["min"], 3)
        gates.append({
            "n_species": S, "moment64_spread_ms": spread,
            "a_float64": bool(c64["median"] <= m64["median"] + spread),
            "current64_over_moment64": round(c64["median"] / m64["median"], 4),
            "b_pass": bool(c32["median"] < c64["median"]),
            "current32_over_current64": round(c32["median"] / c64["median"], 4),
            "b_call": bool(got["whole32"]["call_ms"]["median"] < got["widen32_whole"]["call_ms"]["median"]
                           and got["current32"]["call_ms"]["median"] < got["widen32"]["call_ms"]["median"]),
            "widen32_whole_over_whole32": round(got["widen32_whole"]["call_ms"]["median"] / got["whole32"]["call_ms"]["median"], 3),
            "widen32_over_current32": round(got["widen32"]["call_ms"]["median"] / got["current32"]["call_ms"]["median"], 3)})
    out = {"metric": "current_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A, "dim": D,
           "fft": True, "slab_bytes": nbytes, "gates": gates, "cases": cases}
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
