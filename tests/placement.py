"""The ranks of the collective classes' placement tests: IntermediateScattering, CurrentCorrelation, VanHoveSelf,
DynamicSusceptibility, PartialScattering and FourPointStructureFactor under distributed=True, each rank a fresh child
process with its own process group.

A class's test module (test_scattering, test_current_correlation, test_vanhove, test_overlap, test_partial_scattering,
test_overlap_density) gives

    placed_results(A, **place)   the class run on its case of A atoms with the placement keywords: {name: array}
    check_placed(out, A, what)   those arrays against the reference over ALL atoms, at the bar of the single-device test
    INTEGER_KEYS                 the results that are integers: equal to the single-process run's

and ranks() runs placed_results(A, distributed=True) in `world` children.  The CPU halves (device="cpu", gloo; for
FourPointStructureFactor also "cpu-env": $TA_AMD_DEVICE=cpu and no device= keyword) are unmarked tests of those modules;
the GPU halves (gloo with two ranks on one GPU, nccl = RCCL with one rank) are in test_classes_gpu.py."""
import importlib
import os

import numpy as np

#: first port of each module's groups (test_gpu_dist.py's derivation: + pid % 2000 + A, here + 100 per kind of group)
PORTS = {"test_scattering": 42000, "test_current_correlation": 44500, "test_vanhove": 47000, "test_overlap": 49500}
KINDS = {"cpu": 0, "gloo": 100, "nccl": 200, "cpu-env": 300}


def record_ranges(out, results):
    """out["range"] / out["device_ranges"]: the blocks of atoms a run's results name (distributed=True / devices=[...])"""
    if results.get("particle_range") is not None:
        out["range"] = np.array(results.particle_range)
    if results.get("device_ranges") is not None:
        out["device_ranges"] = np.array(results.device_ranges)


def _rank(rank, world, port, kind, module, A, out_dir):
    import torch.distributed as dist

    place = {"distributed": True}
    if kind == "cpu":
        place["device"] = "cpu"
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    elif kind == "cpu-env":
        os.environ.pop("LOCAL_RANK", None)
        os.environ["TA_AMD_DEVICE"] = "cpu"  # no device= keyword: dist.default_device() reads the variable
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    elif kind == "gloo":
        os.environ.pop("LOCAL_RANK", None)
        os.environ["TA_AMD_DEVICE"] = "0"  # the ranks share the box's one GPU
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    else:
        import torch

        from transport_analysis_amd import dist as tad

        os.environ.pop("TA_AMD_DEVICE", None)
        os.environ["LOCAL_RANK"] = "0"
        os.environ["TA_AMD_FORCE_COLLECTIVE"] = "1"  # a group of one rank reduces nothing unless asked
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                device_id=torch.device("cuda", 0))
        assert tad.uses_device_reduce() and tad.default_device() == 0
    out = importlib.import_module(module).placed_results(A, **place)
    np.savez(os.path.join(out_dir, f"{module}_{rank}.npz"), **out)
    dist.destroy_process_group()


def ranks(module, A, world, kind, out_dir):
    """[{name: array}] of the `world` ranks, each with its "range" = results.particle_range"""
    import torch.multiprocessing as mp

    port = PORTS[module] + KINDS[kind] + (os.getpid() % 2000) + A
    mp.spawn(_rank, args=(world, port, kind, module, A, str(out_dir)), nprocs=world, join=True)
    outs = [dict(np.load(os.path.join(str(out_dir), f"{module}_{r}.npz"))) for r in range(world)]
    for r, out in enumerate(outs):
        assert tuple(out.pop("range")) == ((A * r) // world, (A * (r + 1)) // world)
    return outs


def check_ranks(mod, A, world, kind, out_dir, place):
    """every rank's results against the reference over all atoms; the integer results equal to the single-process run's
    (`place`: its placement keywords)"""
    single = mod.placed_results(A, **place)
    for r, out in enumerate(ranks(mod.__name__, A, world, kind, out_dir)):
        mod.check_placed(out, A, f"{kind} rank {r} of {world}")
        for key in mod.INTEGER_KEYS:
            assert out[key].dtype == np.int64 and np.array_equal(out[key], single[key]), (key, r)
