#!/usr/bin/env python3
"""Current correlation functions (ta_kcurrent_staged) on float64 and float32 device slabs against a streaming read and the
composed route's lower bound, one JSON line.

Values ta_stage_synth'd straight into two pairs of device slabs (velocities, positions) of the same values (default 10000
frames x 100000 atoms x 3: 2 x 24 GB as float64, 2 x 12 GB as float32).  In ONE run, on the same staged slabs:
  stream     : k_species_current of slab 0 with one species (ta_current_staged without cross term): a pure streaming read
               of the same layout, per slab type;
  kcurrent   : per slab type and K in --kvectors (default 1 4 16): ta_kcurrent_staged(fft=1) with all three outputs --
               k_kcurrent once per KC wavevectors, k_sum_partials, then the projections' correlation;
  scatter    : ta_scatter_staged asked for the density only at the same K: the lower bound of the route composed from
               k_phase and a species sum, which writes and re-reads a phase slab per wavevector.
Per case: `steps` timed calls after `warmup` warm-ups; `call_ms` = median / min / max of the whole call's device-event
interval (ta_timing_history), `kernel_ms` = the same of the named kernel's own interval (all its launches of a call
together) in `steps` MORE calls with the kernel timeline on (ta_kernel_timeline).
  kcurrent_tb_per_s = launches x both slabs' bytes / k_kcurrent median;   stream_tb_per_s = slab bytes / k_species_current median.
No ratio is gated: the figures are the result.

The candidate tiles.  `--build-tiles 2x2 4x1 ...` compiles kcurrent.hip once per KCxF (-DTA_KCURRENT_KC, -DTA_KCURRENT_F)
and links it with the library's other objects (run `make` in csrc first) into tools/kcurrent_tiles/libta_hip_KCxF.so;
`--tiles 2x2 4x1 ...` then times k_kcurrent of each such library at the largest K in a process of its own (`--lib`), so the
shipped (KC, F) is a recorded choice.

    python tools/bench_kcurrent.py [--frames T] [--atoms A] [--steps K] [--warmup W] [--kvectors 1 4 16] [--tiles 2x2 ...]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "transport_analysis_amd", "csrc")
TILES = os.path.join(ROOT, "tools", "kcurrent_tiles")

SEED = 20241019


def tile_lib(name):
    return os.path.join(TILES, f"libta_hip_{name}.so")


def build_tiles(names):
    os.makedirs(TILES, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".o") and f != "kcurrent.o")
    if not objs:
        raise SystemExit("no objects in csrc: run make there first")
    for name in names:
        kc, f = (int(v) for v in name.split("x"))
        obj = os.path.join(TILES, f"kcurrent_{name}.o")
        subprocess.check_call([hipcc, "-O3", "-std=c++20", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast",
                               f"-DTA_KCURRENT_KC={kc}", f"-DTA_KCURRENT_F={f}", "-c", os.path.join(CSRC, "kcurrent.hip"), "-o", obj])
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tile_lib(name), obj, *objs, "-ldl",
                               "-lpthread", "-lgomp"])
        print("built", tile_lib(name))


def stats(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def timed(torch, ctx, call, steps, warmup, kernel):
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
        for name, t in ctx.kernel_timeline(128):
            kernels[name] = round(kernels.get(name, 0.0) + t, 3)
        own.append(kernels[kernel])
    out["kernel_ms"] = stats(own)
    out["launches"] = ctx.kernel_launches(kernel)
    ctx.set_option("timeline", 0)
    out["kernels"] = kernels
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kvectors", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--build-tiles", nargs="+", default=None, metavar="KCxF")
    ap.add_argument("--tiles", nargs="+", default=[], metavar="KCxF")
    ap.add_argument("--lib", default=None, help="a candidate tile's library: time k_kcurrent alone")
    args = ap.parse_args()
    if args.build_tiles:
        build_tiles(args.build_tiles)
        return
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    if args.lib:
        _lib._SO = os.path.abspath(args.lib)
    T, A, D = args.frames, args.atoms, 3
    dev = torch.device("cuda", 0)
    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = _lib.Context(0)
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, A, D, 2)
        ctx.stage_synth(0, SEED, 0, A * D)
        ctx.stage_synth(1, SEED + 1, 0, A * D)
        slabs[name] = ctx
    nbytes = {"64": T * A * D * 8, "32": T * A * D * 4}
    tile = _lib.kcurrent_tile()
    rng = np.random.default_rng(3)
    cases = []

    def kcurrent_case(slab, ctx, K, corr=True):
        k = rng.uniform(-2.0, 2.0, size=(K, D))
        cur = torch.zeros((K, T, D, 2), dtype=torch.float64, device=dev)
        lon = torch.zeros((K, T), dtype=torch.float64, device=dev)
        tr = torch.zeros((K, T), dtype=torch.float64, device=dev)
        t = timed(torch, ctx, lambda: ctx.kcurrent_staged(1, k, cur.data_ptr(), lon.data_ptr() if corr else 0, tr.data_ptr() if corr else 0),
                  args.steps, args.warmup, "k_kcurrent")
        t.update({"case": "kcurrent", "slab": "float" + slab, "n_k": K})
        t["kcurrent_tb_per_s"] = round(t["launches"] * 2 * nbytes[slab] / (t["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
        t["ms_per_wavevector"] = round(t["kernel_ms"]["median"] / K, 3)
        return t

    if args.lib:  # a candidate tile: the pass alone, at the largest K
        K = max(args.kvectors)
        out = {"tile": tile, "n_k": K}
        for slab, ctx in slabs.items():
            t = kcurrent_case(slab, ctx, K, corr=False)
            out["float" + slab] = {key: t[key] for key in ("kernel_ms", "launches", "kcurrent_tb_per_s", "ms_per_wavevector")}
        print(json.dumps(out), flush=True)
        return

    d_lab = torch.zeros(A, dtype=torch.int32, device=dev)
    one = torch.zeros((1, T, D), dtype=torch.float64, device=dev)
    stream = {}
    for slab, ctx in slabs.items():
        t = timed(torch, ctx, lambda ctx=ctx: ctx.current_staged(1, 1, d_lab.data_ptr(), one.data_ptr()), args.steps, args.warmup,
                  "k_species_current")
        t.update({"case": "stream", "slab": "float" + slab})
        t["stream_tb_per_s"] = round(nbytes[slab] / (t["kernel_ms"]["median"] * 1e-3) / 1e12, 3)
        stream[slab] = t
        cases.append(t)
    report = []
    for K in args.kvectors:
        row = {"n_k": K}
        for slab, ctx in slabs.items():
            t = kcurrent_case(slab, ctx, K)
            cases.append(t)
            ctx.trim()
            k = rng.uniform(-2.0, 2.0, size=(K, D))
            rho = torch.zeros((K, T, 2), dtype=torch.float64, device=dev)
            s = timed(torch, ctx, lambda ctx=ctx: ctx.scatter_staged(1, k, 0, rho.data_ptr(), 0), args.steps, args.warmup, "k_phase")
            s.update({"case": "scatter", "slab": "float" + slab, "n_k": K})
            cases.append(s)
            ctx.trim()
            row.update({f"kcurrent{slab}_call_ms": t["call_ms"]["median"], f"kcurrent{slab}_pass_ms": t["kernel_ms"]["median"],
                        f"kcurrent{slab}_tb_per_s": t["kcurrent_tb_per_s"], f"stream{slab}_tb_per_s": stream[slab]["stream_tb_per_s"],
                        f"scatter_density{slab}_call_ms": s["call_ms"]["median"], "launches": t["launches"]})
        report.append(row)
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    tiles = []
    for name in args.tiles:  # each candidate in a process of its own, once this one has let go of the device memory
        cmd = [sys.executable, os.path.abspath(__file__), "--lib", tile_lib(name), "--frames", str(T), "--atoms", str(A), "--steps",
               str(args.steps), "--warmup", str(args.warmup), "--kvectors", str(max(args.kvectors))]
        line = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
        tiles.append(json.loads(line))
    result = {"metric": "kcurrent_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_atoms": A, "dim": D,
              "fft": True, "slab_bytes": nbytes, "tile": tile, "report": report, "tiles": tiles, "cases": cases}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
