#!/usr/bin/env python3
"""Crossovers of the Einstein MSD's evaluations at equal data volume (n_frames x n_atoms = 5e8: 12 GB of float64
positions): k_short (up to 64 frames), k_mid ("mid_all" 1: 65 ... 512 frames), the vector kernel k_direct ("short_max" 0,
"mid_max" 0) and the FFT form (fft=1 with "short_max" 0), with and without the by-particle array; then the FFT form's
accuracy on the closed form x = t^2 / 2 (5001 frames, 1 atom, xyz) and on a random walk offset by 1000 A.
Device time per call (ta_last_timing), best of 2 after a warm-up.

    python tools/sweep_msd.py [n_frames ...]  -> the table recorded in DESIGN.md section 4.7
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from transport_analysis_amd import _lib

FORMS = (  # name, fft, options
    ("short", 0, {"short_max": 64, "mid_max": 0, "mid_all": 0}),
    ("mid", 0, {"short_max": 0, "mid_max": 512, "mid_all": 1}),
    ("vector", 0, {"short_max": 0, "mid_max": 0, "mid_all": 0}),
    ("fft", 1, {"short_max": 0, "mid_max": 512, "mid_all": 0}),
)
DEFAULTS = {"short_max": 64, "mid_max": 512, "mid_all": 0}


def sweep(frames):
    dev = torch.device("cuda:0")
    ctx = _lib.Context(0)
    print("# ms per call, 12 GB of positions: " + " / ".join(f[0] for f in FORMS) + "  (- : the form does not apply)")
    for bp in (True, False):
        for T in frames:
            A = int(5e8 / T)
            ctx.stage_free()
            ctx.trim()
            torch.cuda.empty_cache()
            ctx.stage_alloc_device(T, A, 3, 1)
            ctx.stage_synth(0, 7, 0, A * 3)
            lag = torch.zeros(T, dtype=torch.float64, device=dev)
            out = torch.empty((T, A), dtype=torch.float64, device=dev) if bp else None
            row = []
            for name, fft, opts in FORMS:
                if (name == "short" and T > 64) or (name == "mid" and not 65 <= T <= 512):
                    row.append("        -")
                    continue
                for k, v in opts.items():
                    ctx.set_option(k, v)
                ts = []
                for _ in range(3):
                    ctx.msd_staged(fft, lag.data_ptr(), out.data_ptr() if bp else 0, A if bp else 0)
                    torch.cuda.synchronize()
                    ts.append(ctx.last_timing()[0])
                row.append(f"{min(ts[1:]):9.3f}")
            for k, v in DEFAULTS.items():
                ctx.set_option(k, v)
            del out, lag
            print(f"by_particle={int(bp)} T={T:5d} A={A:9d}: " + " / ".join(row), flush=True)
    ctx.close()


def accuracy():
    """lag-1 relative error of the FFT form against the closed form / the direct form"""
    ctx = _lib.Context(0)
    T = 5001
    t = np.arange(T, dtype=np.float64)
    x = np.repeat((t * t / 2)[:, None, None], 3, axis=2)
    (view,) = ctx.stage_alloc(T, 1, 3)
    view[:] = x
    ctx.stage_commit(0, T)
    ts, _ = ctx.msd(True)
    want1 = 3 * np.mean((t[:-1] + 0.5) ** 2)  # lag 1: x[t + 1] - x[t] = t + 1/2
    print(f"# closed form x = t^2/2, {T} frames, xyz: FFT form lag-1 relative error {abs(ts[1] - want1) / want1:.3e}")
    rng = np.random.default_rng(0)
    T, A = 5000, 64
    w = np.cumsum(rng.standard_normal((T, A, 3)), axis=0) + 1000.0
    (view,) = ctx.stage_alloc(T, A, 3)
    view[:] = w
    ctx.stage_commit(0, T)
    f, _ = ctx.msd(True)
    d, _ = ctx.msd(False)
    rel = np.abs(f[1:] - d[1:]) / np.abs(d[1:])
    print(f"# random walk + 1000 A, {T} frames x {A} atoms: FFT form against the direct form, lag-1 relative "
          f"{rel[0]:.3e}, worst lag {rel.max():.3e}, scale-relative {np.max(np.abs(f - d)) / np.max(np.abs(d)):.3e}")
    ctx.close()


if __name__ == "__main__":
    sweep([int(a) for a in sys.argv[1:]] or [32, 48, 64, 65, 80, 96, 97, 112, 128, 160, 192, 256, 384, 512])
    accuracy()
