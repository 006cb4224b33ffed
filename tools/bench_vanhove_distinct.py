#!/usr/bin/env python3
"""The distinct van Hove passes (ta_vanhove_distinct_staged: k_vhd_gather, k_vhd_pairs) on float64 and float32 device slabs,
one JSON line.

Two device slabs of the same values (default 2000 frames x 20000 items x 3), every `--stride`-th frame (10) an origin, all
items on both sides, B = --bins (200), per `--data`:
  noise   : ta_stage_synth's unit-variance white noise in a box of 8 -- the distances spread over all bins;
  lattice : a simple-cubic lattice of spacing 1 (box = its edge) plus a random walk of `--step` per frame and component,
            built on the device (frame pieces through ta_stage_commit_dev) -- the pairs of a lattice shell fall into one or
            two bins: what same-address LDS atomics cost shows as the difference to `noise`.
Per data kind, slab type, L in --lags (1 8: lag 0, then log-spaced) and r_max in --rmax (fractions of the box: 0.5 0.25):
`steps` calls with the kernel timeline on after `warmup` warm-ups; `pairs_ms` / `gather_ms` = median / min / max of all
launches of k_vhd_pairs / k_vhd_gather of a call together (ta_kernel_timeline).
  pairs_per_ns     = sum_l n_orig[l] N (N - 1) / k_vhd_pairs median
  lds_atomic_share = the share of the pairs inside the binned range (the others cost a register add, no LDS atomic)
  gather_over_pairs = k_vhd_gather median / k_vhd_pairs median
`--cpu`: the CPU backend's wall time on `--cpu-threads` (16) threads at a shape cut down to run in seconds (--cpu-frames 200,
--cpu-items 5000), and that its counts equal the GPU's at that shape.  No time is gated: the figures are the result.
`--profile`: ONE call per slab type (the first of --lags and --rmax) and nothing else -- the run to put under a counters-only
profiler.

    python tools/bench_vanhove_distinct.py [--frames T] [--items N] [--steps K] [--warmup W] [--lags 1 8] [--data noise lattice]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SEED = 20240917


def stats(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def lag_list(np, T, L):
    """lag 0, then L - 1 strictly increasing lags up to about T / 2, logarithmically spaced where integers allow"""
    if L == 1:
        return np.zeros(1, dtype=np.int64)
    lags = np.rint(np.geomspace(1, max(T // 2, L), L - 1)).astype(np.int64)
    for i in range(1, L - 1):
        lags[i] = max(lags[i], lags[i - 1] + 1)
    return np.concatenate([np.zeros(1, dtype=np.int64), lags[lags < T]])


def lattice_edge(N):
    n = 1
    while n ** 3 < N:
        n += 1
    return n


def fill_lattice(torch, np, slabs, T, N, D, step, piece=250):
    """the first N sites of a simple-cubic lattice of spacing 1, each with its own random walk, into both slabs"""
    n = lattice_edge(N)
    g = torch.arange(n, dtype=torch.float64, device="cuda")
    sites = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1).reshape(-1, 3)[:N].reshape(1, N * D)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    carry = sites.clone()
    for lo in range(0, T, piece):
        hi = min(T, lo + piece)
        x = carry + torch.cumsum(torch.randn((hi - lo, N * D), dtype=torch.float64, device="cuda", generator=gen) * step, dim=0)
        carry = x[-1:].clone()
        x32 = x.float()
        slabs["64"].stage_commit_dev(0, x.data_ptr(), N * D, lo, hi, dtype=np.float64)
        slabs["32"].stage_commit_dev(0, x32.data_ptr(), N * D, lo, hi, dtype=np.float32)
        torch.cuda.synchronize()


def timed(torch, ctx, call, steps, warmup):
    ctx.set_option("timeline", 1)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    pairs, gather, total = [], [], []
    for _ in range(steps):
        call()
        torch.cuda.synchronize()
        by_name = {}
        for name, t in ctx.kernel_timeline(4096):
            by_name[name] = by_name.get(name, 0.0) + t
        pairs.append(by_name["k_vhd_pairs"])
        gather.append(by_name["k_vhd_gather"])
        total.append(ctx.timing_history(1)[0][0])
    out = {"pairs_ms": stats(pairs), "gather_ms": stats(gather), "call_ms": stats(total), "steps": steps,
           "launches": {k: ctx.kernel_launches(k) for k in ("k_vhd_gather", "k_vhd_pairs")}}
    ctx.set_option("timeline", 0)
    return out


def cpu_case(np, _lib, torch, args, D):
    """the CPU backend at a cut-down shape, against the GPU on the same values"""
    T, N = args.cpu_frames, args.cpu_items
    x = np.random.default_rng(SEED).uniform(0.0, 8.0, size=(T, N, D))
    lags, dims = np.zeros(1, dtype=np.int64), np.tile([8.0, 8.0, 8.0, 90.0, 90.0, 90.0], (T, 1))
    out = {}
    for name, device in (("cpu", "cpu"), ("gpu", 0)):
        c = _lib.Context(device)
        try:
            if device == "cpu":
                c.set_option("cpu_threads", args.cpu_threads)
            (view,) = c.stage_alloc(T, N, D, dtype=np.float64)
            view[:] = x
            c.stage_commit(0, T)
            t0 = time.perf_counter()
            out[name] = c.vanhove_distinct(lags, args.bins, 4.0 / args.bins, origin_stride=args.stride, dimensions=dims)
            out[name + "_s"] = round(time.perf_counter() - t0, 3)
        finally:
            c.close()
    pairs = float(-(-T // args.stride)) * N * (N - 1)
    return {"case": "cpu_backend", "n_frames": T, "n_items": N, "threads": args.cpu_threads, "pairs": pairs,
            "cpu_s": out["cpu_s"], "cpu_pairs_per_ns": round(pairs / (out["cpu_s"] * 1e9), 4),
            "counts_equal_gpu": bool(np.array_equal(out["cpu"], out["gpu"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--stride", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lags", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--rmax", type=float, nargs="+", default=[0.5, 0.25])
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--data", nargs="+", default=["noise", "lattice"], choices=["noise", "lattice"])
    ap.add_argument("--slabs", nargs="+", default=["64", "32"], choices=["64", "32"])
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=200)
    ap.add_argument("--cpu-items", type=int, default=5000)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from transport_analysis_amd import _lib

    T, N, D, B = args.frames, args.items, 3, args.bins
    dev = torch.device("cuda", 0)
    slabs = {}
    for name, f32 in (("64", 0), ("32", 1)):
        ctx = _lib.Context(0)
        ctx.set_option("stage_device_f32", f32)
        ctx.stage_alloc_device(T, N, D, 1)
        slabs[name] = ctx
    report = []
    for data in args.data:
        if data == "noise":
            box = 8.0
            for ctx in slabs.values():
                ctx.stage_synth(0, SEED, 0, N * D)
        else:
            box = float(lattice_edge(N))
            fill_lattice(torch, np, slabs, T, N, D, args.step)
        torch.cuda.synchronize()
        dims = np.tile([box, box, box, 90.0, 90.0, 90.0], (T, 1))
        for L in args.lags:
            lags = lag_list(np, T, L)
            pairs = float(sum(-(-(T - int(tau)) // args.stride) for tau in lags)) * N * (N - 1)
            for frac in args.rmax:
                dr = frac * box / B
                cnt = torch.zeros((len(lags), B + 1), dtype=torch.int64, device=dev)
                row = {"data": data, "box": box, "n_lags": int(len(lags)), "lag_max": int(lags[-1]), "r_max": frac * box, "pairs": pairs}
                for slab in args.slabs:
                    ctx = slabs[slab]
                    call = lambda ctx=ctx: ctx.vanhove_distinct_staged(lags, B, dr, cnt.data_ptr(), origin_stride=args.stride,  # noqa: E731
                                                                       dimensions=dims)
                    if args.profile:
                        call()
                        torch.cuda.synchronize()
                        continue
                    t = timed(torch, ctx, call, args.steps, args.warmup)
                    ms = t["pairs_ms"]["median"]
                    row["float" + slab] = t
                    row[f"pairs_per_ns{slab}"] = round(pairs / (ms * 1e6), 3)
                    row[f"gather_over_pairs{slab}"] = round(t["gather_ms"]["median"] / ms, 5)
                if args.profile:
                    break
                counts = cnt.cpu().numpy()
                assert counts.sum() == int(pairs)
                row["lds_atomic_share"] = round(1.0 - float(counts[:, -1].sum()) / pairs, 6)
                row["top_bin_share_lag0"] = round(float(counts[0, :-1].max()) / max(1.0, float(counts[0, :-1].sum())), 4)
                report.append(row)
            if args.profile:
                break
    for ctx in slabs.values():
        ctx.stage_free()
        ctx.close()
    if args.profile:
        return
    result = {"metric": "vanhove_distinct_ms_per_call", "device": torch.cuda.get_device_name(0), "n_frames": T, "n_items": N, "dim": D,
              "origin_stride": args.stride, "n_bins": B, "report": report}
    if args.cpu:
        result["cpu_backend"] = cpu_case(np, _lib, torch, args, D)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
