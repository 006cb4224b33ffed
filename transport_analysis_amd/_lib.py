"""ctypes binding of libta_hip.so (the C-ABI declared in include/ta_hip.h).

There is no CPU fallback: if the shared library is missing, or no GPU is
usable, every compute entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libta_hip.so")
_CSRC = os.path.join(_HERE, "csrc")

TA_F32, TA_F64 = 0, 1
#: ta_orient's modes (TA_ORIENT_*)
ORIENT_MODES = {"bond": 0, "bisector": 1, "normal": 2}
#: ta_shell_msd's conditions (TA_SHELL_*)
SHELL_CONDITIONS = {"continuous": 0, "endpoints": 1}

_vp, _i64, _ci, _dbl, _str = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_char_p
_P = ctypes.POINTER
_pf = _P(ctypes.c_float)


def _int(*argtypes):
    return _ci, list(argtypes)


def _text(*argtypes):
    return _str, list(argtypes)


_HOST = _int(_vp, _vp, _vp)  # (handle, h_timeseries, h_by_particle)
_DEV = _int(_vp, _vp, _i64, _i64, _ci, _i64, _vp, _vp, _i64, _vp)
_STAGED = _int(_vp, _vp, _vp, _i64, _vp)
_FRAME = _int(_vp, _ci, _i64, _vp, _ci, _i64, _ci, _ci, _ci, _i64, _vp, _i64)
_COND = _int(_vp, _ci, _vp, _vp, _vp, _vp)
_UNWRAP = _int(_vp, _ci, _vp, _vp)
_ONSAGER = _int(_vp, _ci, _ci, _vp, _vp, _vp, _vp)  # (handle, fft, n_species, h_species, h_weights, h_moments, h_cross)
_SELF = _int(_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp)  # (handle, quantity, fft, n_species, h_species, h_weights, h_self, h_counts)
_SCATTER = _int(_vp, _ci, _ci, _vp, _vp, _vp, _vp)  # (handle, fft, n_k, h_kvecs, h_self, h_density, h_coll)
_KCURRENT = _int(_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp)  # (handle, fft, n_k, h_kvecs, h_weights, h_current, h_long, h_trans)
# (handle, fft, n_k, h_kvecs, n_species, h_species, h_weights, h_density, h_cross)
_PARTIAL = _int(_vp, _ci, _ci, _vp, _ci, _vp, _vp, _vp, _vp)
_VANHOVE = _int(_vp, _ci, _vp, _ci, _dbl, _vp, _vp)  # (handle, n_lags, h_lags, n_bins, dr, h_counts, h_moments)
_OVERLAP = _int(_vp, _ci, _vp, _ci, _vp, _vp)  # (handle, n_lags, h_lags, n_cutoffs, h_cutoffs, h_q)
# (handle, n_k, h_kvecs, n_lags, h_lags, n_cutoffs, h_cutoffs, h_w)
_OVERLAP_DENSITY = _int(_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp)

#: every symbol include/ta_hip.h declares -> (result type, argument types): the one table EXPORTS and lib() are made of
_API = {
    "ta_abi_version": _int(), "ta_device_count": _int(), "ta_stage_threads": _int(),
    "ta_last_error": _text(_vp),
    "ta_ctx_create": _int(_ci, _P(_vp)), "ta_ctx_destroy": _int(_vp),
    "ta_set_option": _int(_vp, _str, _i64), "ta_trim": _int(_vp),
    "ta_fft_plan_info": _int(_i64, _P(_i64), _P(_ci), _P(_ci)),
    "ta_host_alloc": _int(_i64, _P(_vp)), "ta_host_alloc_on": _int(_ci, _i64, _P(_vp)), "ta_host_free": _int(_vp),
    "ta_stage_alloc": _int(_vp, _i64, _i64, _ci, _ci, _ci, _P(_vp)), "ta_stage_alloc_device": _int(_vp, _i64, _i64, _ci, _ci),
    "ta_stage_commit": _int(_vp, _i64, _i64), "ta_stage_frame": _FRAME, "ta_stage_free": _int(_vp),
    "ta_stage_commit_dev": _int(_vp, _ci, _vp, _ci, _i64, _i64, _i64, _vp), "ta_stage_read_dev": _int(_vp, _ci, _vp, _i64, _vp),
    "ta_stage_device": _int(_vp, _ci, _P(_vp), _P(_i64), _P(_i64)),
    "ta_stage_synth": _int(_vp, _ci, ctypes.c_uint64, _i64, _i64, _vp),
    "ta_vacf_fft": _HOST, "ta_vacf_direct": _HOST, "ta_helfand_msd": _int(_vp, _vp, _dbl, _vp, _vp),
    "ta_msd": _int(_vp, _ci, _vp, _vp), "ta_conductivity": _COND, "ta_unwrap": _UNWRAP,
    "ta_onsager": _ONSAGER, "ta_onsager_cross": _int(_vp, _ci, _vp, _ci, _i64, _ci, _vp),
    "ta_onsager_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_onsager_staged": _int(_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_current": _ONSAGER, "ta_current_cross": _int(_vp, _ci, _vp, _ci, _i64, _ci, _vp),
    "ta_current_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_current_staged": _int(_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_species_self": _SELF, "ta_species_self_staged": _int(_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp),
    "ta_species_self_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _ci, _ci, _vp, _vp, _vp, _vp),
    "ta_scatter": _SCATTER, "ta_scatter_collective": _int(_vp, _ci, _vp, _ci, _i64, _vp),
    "ta_scatter_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_scatter_staged": _int(_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp),
    # (handle, fft, mode, n_vectors, h_index, h_dimensions, h_weights, c1, c2, total, coll[, stream])
    "ta_orient": _int(_vp, _ci, _ci, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "ta_orient_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _ci, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "ta_orient_staged": _int(_vp, _ci, _ci, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "ta_chain_modes": _int(_vp, _ci, _i64, _i64, _vp, _ci, _vp, _vp, _vp),
    "ta_chain_modes_staged": _int(_vp, _ci, _i64, _i64, _vp, _ci, _vp, _vp, _vp, _vp),
    "ta_chain_modes_tile": _int(_P(_ci), _P(_ci)),
    "ta_kcurrent": _KCURRENT, "ta_kcurrent_correlate": _int(_vp, _ci, _vp, _ci, _vp, _i64, _ci, _vp, _vp),
    "ta_kcurrent_tile": _int(_P(_ci), _P(_ci), _P(_ci)),
    "ta_kcurrent_staged": _int(_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp),
    "ta_partial_density": _PARTIAL, "ta_partial_cross": _int(_vp, _ci, _vp, _ci, _ci, _i64, _vp),
    "ta_partial_density_tile": _int(_ci, _P(_ci), _P(_ci), _P(_ci), _P(_ci)),
    "ta_partial_density_staged": _int(_vp, _ci, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_vanhove": _VANHOVE, "ta_vanhove_staged": _int(_vp, _ci, _vp, _ci, _dbl, _vp, _vp, _vp),
    "ta_vanhove_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _vp, _ci, _dbl, _vp, _vp, _vp),
    "ta_overlap": _OVERLAP, "ta_overlap_tile": _int(_P(_ci)), "ta_overlap_staged": _int(_vp, _ci, _vp, _ci, _vp, _vp, _vp),
    "ta_overlap_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _vp, _ci, _vp, _vp, _vp),
    "ta_overlap_density": _OVERLAP_DENSITY, "ta_overlap_density_tile": _int(_P(_ci), _P(_ci), _P(_ci)),
    "ta_overlap_density_staged": _int(_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp),
    # (handle, n_lags, h_lags, origin_stride, n_a, h_idx_a, n_b, h_idx_b, h_dimensions, axes, n_bins, dr, counts[, stream])
    "ta_vanhove_distinct": _int(_vp, _ci, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _ci, _dbl, _vp),
    "ta_pair_find": _int(_vp, _i64, _vp, _i64, _vp, _vp, _vp, _dbl, _i64, _vp),
    "ta_pair_find_read": _int(_vp, _i64, _vp),
    "ta_pair_lifetime": _int(_vp, _ci, _i64, _vp, _vp, _vp, _dbl, _vp, _vp, _vp),
    "ta_pair_lifetime_staged": _int(_vp, _ci, _i64, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp),
    # (handle, fft, n_bonds, n_at, h_atoms, h_dimensions, axes, r_cut, r_break, cos_cut, cos_break, gap, ci, runs, nb[, stream])
    "ta_bond_lifetime": _int(_vp, _ci, _i64, _ci, _vp, _vp, _vp, _dbl, _dbl, _dbl, _dbl, _ci, _vp, _vp, _vp),
    "ta_bond_lifetime_staged": _int(_vp, _ci, _i64, _ci, _vp, _vp, _vp, _dbl, _dbl, _dbl, _dbl, _ci, _vp, _vp, _vp, _vp),
    "ta_shell_residence": _int(_vp, _ci, _i64, _vp, _i64, _vp, _vp, _vp, _dbl, _dbl, _ci, _vp, _vp, _vp),
    "ta_shell_residence_staged": _int(_vp, _ci, _i64, _vp, _i64, _vp, _vp, _vp, _dbl, _dbl, _ci, _vp, _vp, _vp, _vp),
    # (handle, condition, max_lag, n_a, idx_a, n_b, idx_b, h_dimensions, axes, r_cut, r_break, gap, sums, count, runs, nb[, stream])
    "ta_shell_msd": _int(_vp, _ci, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _dbl, _dbl, _ci, _vp, _vp, _vp, _vp),
    "ta_shell_msd_staged": _int(_vp, _ci, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _dbl, _dbl, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_shell_orient": _int(_vp, _ci, _i64, _ci, _ci, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _dbl, _dbl, _ci, _vp, _vp, _vp, _vp),
    "ta_shell_orient_staged": _int(_vp, _ci, _i64, _ci, _ci, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _dbl, _dbl, _ci, _vp, _vp, _vp, _vp,
                                   _vp),
    "ta_vanhove_distinct_staged": _int(_vp, _ci, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _ci, _dbl, _vp, _vp),
    "ta_compound": _int(_vp, _i64, _vp, _vp, _vp, _vp, _P(_vp)),
    "ta_vacf_fft_dev": _DEV, "ta_vacf_direct_dev": _DEV,
    "ta_helfand_msd_dev": _int(_vp, _vp, _vp, _vp, _i64, _i64, _ci, _i64, _dbl, _vp, _vp, _i64, _vp),
    "ta_msd_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _vp, _vp, _i64, _vp),
    "ta_conductivity_dev": _int(_vp, _vp, _i64, _i64, _ci, _i64, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_vacf_fft_staged": _STAGED, "ta_vacf_direct_staged": _STAGED,
    "ta_helfand_msd_staged": _int(_vp, _vp, _dbl, _vp, _vp, _i64, _vp), "ta_msd_staged": _int(_vp, _ci, _vp, _vp, _i64, _vp),
    "ta_conductivity_staged": _int(_vp, _ci, _vp, _vp, _vp, _vp, _vp),
    "ta_last_timing": _int(_vp, _pf, _pf), "ta_timing_history": _int(_vp, _ci, _pf, _pf, _P(_ci)),
    "ta_kernel_timeline": _int(_vp, _ci, _P(_str), _pf, _P(_ci)), "ta_kernel_launches": _int(_vp, _str, _P(_ci)),
    "ta_clock_probe": _int(_vp, _ci, _P(_dbl), _P(_dbl), _P(_dbl)),
    "ta_group_create": _int(_P(_ci), _ci, _P(_vp)), "ta_group_destroy": _int(_vp), "ta_group_last_error": _text(_vp),
    "ta_group_size": _int(_vp), "ta_group_member": _int(_vp, _ci, _P(_vp), _P(_ci)),
    "ta_group_shard": _int(_vp, _i64, _ci, _P(_i64), _P(_i64)),
    "ta_group_reduce_kind": _text(_vp), "ta_group_reduce_note": _text(_vp), "ta_group_rccl_ranks": _int(_vp),
    "ta_group_set_option": _int(_vp, _str, _i64),
    "ta_group_stage_alloc": _int(_vp, _i64, _i64, _ci, _ci, _ci, _P(_vp)), "ta_group_stage_alloc_device": _int(_vp, _i64, _i64, _ci, _ci),
    "ta_group_stage_commit": _int(_vp, _i64, _i64), "ta_group_stage_frame": _FRAME, "ta_group_stage_free": _int(_vp),
    "ta_group_stage_synth": _int(_vp, _ci, ctypes.c_uint64, _i64, _i64),
    "ta_group_vacf_fft": _HOST, "ta_group_vacf_direct": _HOST, "ta_group_helfand_msd": _int(_vp, _vp, _dbl, _vp, _vp),
    "ta_group_msd": _int(_vp, _ci, _vp, _vp), "ta_group_conductivity": _COND, "ta_group_unwrap": _UNWRAP,
    "ta_group_onsager": _ONSAGER, "ta_group_current": _ONSAGER, "ta_group_species_self": _SELF,
    "ta_group_scatter": _SCATTER, "ta_group_kcurrent": _KCURRENT, "ta_group_partial_density": _PARTIAL,
    "ta_group_vanhove": _VANHOVE,
    "ta_group_overlap": _OVERLAP,
    "ta_group_overlap_density": _OVERLAP_DENSITY,
}
EXPORTS = tuple(_API)


class TAError(RuntimeError):
    """A C-ABI call returned a negative status."""

    def __init__(self, code, message):
        super().__init__(f"libta_hip error {code}: {message}")
        self.code = code


def build(force=False):
    """Compile libta_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", _CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", _CSRC])
    return _SO


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 with
    the same SONAME as /opt/rocm's; whichever is loaded first serves both libraries, and
    torch.cuda fails ("No HIP GPUs are available") on top of a runtime that is not its own.
    So when torch is installed but not loaded yet, its runtime is loaded first -- without
    importing torch -- and libta_hip.so binds to it exactly as it does when the application
    imported torch before us."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass  # fall back to the system runtime


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(
            f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950). transport_analysis_amd has no CPU fallback."
        )
    _share_hip_runtime_with_torch()
    L = ctypes.CDLL(_SO)
    for name, (restype, argtypes) in _API.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def device_count():
    return int(lib().ta_device_count())


def fft_plan_info(n_frames):
    m, nt, ns = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    rc = lib().ta_fft_plan_info(int(n_frames), ctypes.byref(m), ctypes.byref(nt), ctypes.byref(ns))
    if rc != 0:
        return None
    return {"M": m.value, "n_threads": nt.value, "n_stages": ns.value}


def kcurrent_tile():
    """{"KC", "F64", "F32"}: the wavevectors per launch of k_kcurrent and the frames per thread on a float64 / float32
    slab (a workgroup covers 256 F frames), ta_kcurrent_tile"""
    kc, f64, f32 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib().ta_kcurrent_tile(ctypes.byref(kc), ctypes.byref(f64), ctypes.byref(f32))
    return {"KC": kc.value, "F64": f64.value, "F32": f32.value}


def partial_density_tile(n_species):
    """{"ST", "KC", "F64", "F32"}: the species slots and the wavevectors per launch of the k_species_density tile that serves
    `n_species`, and the frames per thread on a float64 / float32 slab (a workgroup covers 256 F frames),
    ta_partial_density_tile"""
    st, kc, f64, f32 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib().ta_partial_density_tile(int(n_species), ctypes.byref(st), ctypes.byref(kc), ctypes.byref(f64), ctypes.byref(f32))
    if rc != 0:
        raise TAError(rc, lib().ta_last_error(None).decode())
    return {"ST": st.value, "KC": kc.value, "F64": f64.value, "F32": f32.value}


def overlap_tile():
    """the (lag, cutoff) slots of one k_overlap launch: floor(slots / n_cutoffs) lags share a launch, ta_overlap_tile"""
    slots = ctypes.c_int()
    lib().ta_overlap_tile(ctypes.byref(slots))
    return slots.value


def overlap_density_tile():
    """{"SL", "KC", "F"}: the (lag, cutoff) slots and the wavevectors of one k_overlap_density launch -- floor(SL / n_cutoffs)
    lags and KC wavevectors share a launch -- and the origin frames per thread (a workgroup covers 256 F frames),
    ta_overlap_density_tile"""
    sl, kc, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib().ta_overlap_density_tile(ctypes.byref(sl), ctypes.byref(kc), ctypes.byref(f))
    return {"SL": sl.value, "KC": kc.value, "F": f.value}


def chain_modes_tile():
    """{"modes", "frames"}: the modes one k_chain_modes launch serves and the frames per thread (a workgroup covers 256 of
    them), ta_chain_modes_tile"""
    m, f = ctypes.c_int(), ctypes.c_int()
    lib().ta_chain_modes_tile(ctypes.byref(m), ctypes.byref(f))
    return {"modes": m.value, "frames": f.value}


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else ctypes.c_void_p(None)


def _index_list(idx, name):
    """(int64 array, length) of a list of item indices of the pair calls, or (None, 0)"""
    if idx is None:
        return None, 0
    a = np.ascontiguousarray(idx, dtype=np.int64)
    if a.ndim != 1:
        raise ValueError(f"{name}: shape {a.shape}, expected a 1-d list of item indices")
    return a, int(a.shape[0])


def frame_source(arr):
    """(pointer, dtype code, ld_row) of a frame's (n_atoms, n_coord) array if ta_stage_frame can read it in
    place -- float32 / float64, unit stride along the coordinates, a non-negative whole-element row stride --
    else None (the caller then stages through the NumPy view of the slab)."""
    if not isinstance(arr, np.ndarray) or arr.ndim != 2 or arr.dtype not in (np.float32, np.float64):
        return None
    isz = arr.dtype.itemsize
    if arr.shape[1] > 1 and arr.strides[1] != isz:
        return None
    if arr.strides[0] < isz * arr.shape[1] or arr.strides[0] % isz:
        return None
    return arr.ctypes.data, (TA_F32 if arr.dtype == np.float32 else TA_F64), arr.strides[0] // isz


def atom_rows(ix):
    """(atom_lo, index array or None, n) for ta_stage_frame from an AtomGroup's atom indices: a group of
    consecutive atoms is a block (no index array), anything else is gathered by index."""
    ix = np.ascontiguousarray(ix, dtype=np.int64)
    n = int(ix.size)
    if n == 0:
        return 0, None, 0
    if int(ix[-1]) - int(ix[0]) + 1 == n and (n == 1 or bool(np.all(np.diff(ix) == 1))):
        return int(ix[0]), None, n
    return 0, ix, n


class _PinnedBlock:
    """Owner of one ta_host_alloc block: freed when the last NumPy view of it is gone."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                lib().ta_host_free(ctypes.c_void_p(self.ptr))
                self.ptr = 0
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64, device=-1):
    """np.empty in page-locked host memory (ta_host_alloc_on): the home of results.vacf_by_particle /
    results.visc_by_particle, so that the device->host copy runs at the link's rate the first
    time.  The memory lives as long as the array or any view of it.  `device`: the GPU the calling
    thread is bound to before allocating (-1: its current one).  Raises TAError when the
    allocation fails; `result_empty` is the variant that falls back to pageable memory."""
    shape = tuple(int(x) for x in np.atleast_1d(shape))
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    p = ctypes.c_void_p()
    rc = lib().ta_host_alloc_on(int(device), nbytes, ctypes.byref(p))
    if rc != 0:
        raise TAError(rc, lib().ta_last_error(None).decode())
    buf = (ctypes.c_char * max(nbytes, 1)).from_address(p.value)
    buf._owner = _PinnedBlock(p.value)  # the ctypes array is the NumPy array's base
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)


def pinned_results_enabled():
    """$TA_AMD_PINNED_RESULTS=0 keeps result arrays in pageable memory (np.empty, as the reference's
    np.zeros): for hosts whose RLIMIT_MEMLOCK / cgroup leaves no room for 8 GB more of pinned pages
    beside the staging slabs."""
    return os.environ.get("TA_AMD_PINNED_RESULTS", "1") != "0"


def result_empty(shape, device=-1):
    """Home of a by-particle result: pinned when possible, else -- with a warning -- a pageable
    np.empty (the device->host copy is then slower the first time, the values are the same).  The
    analysis must not be lost in _conclude, after every frame has been read, because page-locking
    failed (hipHostMalloc under a memlock limit)."""
    if not pinned_results_enabled():
        return np.empty(tuple(int(x) for x in np.atleast_1d(shape)), dtype=np.float64)
    try:
        return pinned_empty(shape, device=device)
    except TAError as e:
        import warnings

        warnings.warn(f"page-locked result array unavailable ({e}); using pageable memory "
                      "(slower device->host copy, same values)", RuntimeWarning, stacklevel=2)
        return np.empty(tuple(int(x) for x in np.atleast_1d(shape)), dtype=np.float64)


class PinnedResult:
    """The home of a by-particle result, page-locked on a helper thread while the frames are staged
    (page-locking 8 GB takes about as long as copying them); `get()` joins.  The helper thread is
    bound to the analysis' GPU; a failed pinned allocation degrades to pageable memory with a
    warning (result_empty)."""

    def __init__(self, shape, device=-1):
        import threading

        self._arr, self._err = None, None

        def work():
            try:
                self._arr = result_empty(shape, device=device)
            except Exception as e:  # surfaced by get()
                self._err = e

        self._thread = threading.Thread(target=work, daemon=True)
        self._thread.start()

    def get(self):
        self._thread.join()
        if self._err is not None:
            raise self._err
        return self._arr


DEVICE_CPU = -1  # ta_hip.h: TA_DEVICE_CPU
SELF_MSD, SELF_VACF = 0, 1  # ta_hip.h: TA_SELF_MSD, TA_SELF_VACF


def device_index(device):
    """A GPU index, or DEVICE_CPU for "cpu" / -1: the opt-in CPU backend behind the same C symbols
    (csrc/cpu_backend.cpp).  Nothing picks it on the caller's behalf."""
    if isinstance(device, str):
        if device.strip().lower() == "cpu":
            return DEVICE_CPU
        return int(device)
    return int(device)


class _PlainHome:
    """result_home of a CPU context: an ordinary array (there is no device to copy from)"""

    def __init__(self, shape):
        self._shape = tuple(int(x) for x in np.atleast_1d(shape))

    def get(self):
        return np.empty(self._shape, dtype=np.float64)


def _dtype_code(dtype):
    return TA_F64 if np.dtype(dtype) == np.float64 else TA_F32


def _slab_view(p, dtype, shape):
    """NumPy view of the pinned host slab at address p"""
    n = int(np.prod(shape, dtype=np.int64))
    buf = ((ctypes.c_double if _dtype_code(dtype) == TA_F64 else ctypes.c_float) * n).from_address(p)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


class _Staged:
    """What `Context` and `Group` do the same way: the C calls of a handle under its symbol prefix (ta_ / ta_group_),
    the staged shape, the NumPy views of the host slabs and the host-facing compute calls."""

    _prefix = "ta_"
    _h = None
    shape = None  # (n_frames, n_atoms, dim) once staged
    is_cpu = False

    def _call(self, name, *args):
        """ta_<name> / ta_group_<name> on this handle; a negative status raises with the handle's last message"""
        self._check(getattr(lib(), self._prefix + name)(self._h, *args))

    def _check(self, rc):
        if rc != 0:
            raise TAError(rc, getattr(lib(), self._prefix + "last_error")(self._h).decode())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        self._call("set_option", key.encode(), int(value))

    # -- staging --------------------------------------------------------
    def _staged(self, n_frames, n_atoms, dim, views=()):
        self._slabs = list(views)
        self.shape = (int(n_frames), int(n_atoms), int(dim))

    def _drop_views(self):
        # the pinned memory behind the NumPy views goes away with the slabs: writes through a
        # stale view must not land in freed memory silently
        for a in self._slabs:
            try:
                a.setflags(write=False)
            except Exception:
                pass
        self._slabs = []

    def stage_commit(self, frame_lo, frame_hi):
        self._call("stage_commit", int(frame_lo), int(frame_hi))

    def stage_frame(self, slab, frame, source, cols, rows):
        """slab[frame] = source[rows][:, cols] natively (ta_stage_frame; a group: every member's slab gets its atoms).
        source: frame_source(...) of the Timestep's array; cols: the dim_type's column list (an arithmetic
        progression); rows: atom_rows(...)."""
        ptr, code, ld = source
        lo, index, n = rows
        step = cols[1] - cols[0] if len(cols) > 1 else 1
        self._call("stage_frame", int(slab), int(frame), ctypes.c_void_p(ptr), code, int(ld), int(cols[0]), int(step),
                   len(cols), int(lo), _ptr(index), int(n))

    def stage_free(self):
        self._drop_views()
        self._call("stage_free")

    # -- host-facing compute -------------------------------------------
    def _staged_shape(self):
        return self.shape or (1, 1, 1)  # unstaged: the library reports it

    def _per_atom(self, values, dtype, name, unit):
        """`values` as a flat contiguous array of `dtype` with one entry per staged atom (None stays None)"""
        if values is None:
            return None
        a = np.ascontiguousarray(values, dtype=dtype).ravel()
        if a.size != self._staged_shape()[1]:
            raise ValueError(f"{name}: {a.size} {unit} for {self._staged_shape()[1]} atoms")
        return a

    def _host(self, name, by_particle, *extra, out=None):
        """by_particle: False, True (a pinned (n_frames, n_atoms) array is allocated here) or
        `out` = the caller's (n_frames, n_atoms) float64 C-contiguous array (pinned_empty)."""
        T, A, _ = self._staged_shape()
        ts = np.empty(T, dtype=np.float64)
        bp = None
        if out is not None:
            if out.shape != (T, A) or out.dtype != np.float64 or not out.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous float64 array of shape (n_frames, n_atoms)")
            bp = out
        elif by_particle:
            bp = np.empty((T, A), dtype=np.float64) if self.is_cpu else result_empty((T, A), device=self.device)
        self._call(name, *extra, _ptr(ts), _ptr(bp))
        return ts, bp

    def vacf_fft(self, by_particle=False, out=None):
        return self._host("vacf_fft", by_particle, out=out)

    def vacf_direct(self, by_particle=False, out=None):
        return self._host("vacf_direct", by_particle, out=out)

    def helfand_msd(self, masses, scale, by_particle=False, out=None):
        m = np.ascontiguousarray(masses, dtype=np.float64)
        return self._host("helfand_msd", by_particle, _ptr(m), ctypes.c_double(scale), out=out)

    def msd(self, fft, by_particle=False, out=None):
        """Einstein MSD of slab 0 (the positions): (timeseries, by_particle or None)."""
        return self._host("msd", by_particle, int(fft), out=out)

    def conductivity(self, fft, charges, self_term=False, collective=True):
        """Einstein-Helfand conductivity of slab 0 (the positions) with one charge per staged atom:
        (moment (n_frames, dim), Phi (n_frames,) or None, self lag sum sum_n q_n^2 MSD_n (n_frames,) or None)."""
        T, _, D = self._staged_shape()
        q = self._per_atom(charges, np.float64, "charges", "values")
        moment = np.empty((T, D), dtype=np.float64)
        phi = np.empty(T, dtype=np.float64) if collective else None
        self_ls = np.empty(T, dtype=np.float64) if self_term else None
        self._call("conductivity", int(fft), _ptr(q), _ptr(moment), _ptr(phi), _ptr(self_ls))
        return moment, phi, self_ls

    def _species_args(self, species, n_species, weights):
        """(labels int32, n_species as given or the largest label + 1, weights float64 or None, the outputs' species count)"""
        lab = self._per_atom(species, np.int32, "species", "labels")
        S = int(n_species) if n_species is not None else int(lab.max()) + 1
        return lab, S, self._per_atom(weights, np.float64, "weights", "values"), max(S, 1)

    def _species_sums(self, name, fft, species, n_species, weights, cross):
        T, _, D = self._staged_shape()
        lab, S, w, n = self._species_args(species, n_species, weights)
        sums = np.empty((n, T, D), dtype=np.float64)
        c = np.empty((T, n, n), dtype=np.float64) if cross else None
        self._call(name, int(fft), S, _ptr(lab), _ptr(w), _ptr(sums), _ptr(c))
        return sums, c

    def onsager(self, fft, species, n_species=None, weights=None, cross=True):
        """Species moments and their cross MSD of slab 0 (the positions), ta_onsager: `species` one integer label in
        0 ... n_species - 1 per staged atom, in any order (n_species: default the largest label + 1), `weights` one weight
        per atom or None (all 1): (moments (n_species, n_frames, dim), C (n_frames, n_species, n_species) or None)."""
        return self._species_sums("onsager", fft, species, n_species, weights, cross)

    def current(self, fft, species, n_species=None, weights=None, cross=True):
        """Species currents and their cross-correlation of slab 0 (the velocities), ta_current: arguments as `onsager`:
        (currents (n_species, n_frames, dim), C (n_frames, n_species, n_species) with lag 0, or None)."""
        return self._species_sums("current", fft, species, n_species, weights, cross)

    def species_self(self, quantity, fft, species, n_species=None, weights=None):
        """Per-species self terms of slab 0, ta_species_self: `quantity` SELF_MSD (slab 0 = positions) or SELF_VACF
        (velocities), the other arguments as `onsager`: (self (n_species, n_frames) = sum_{n in s} w_n^2 f_n(k), counts
        (n_species,) int64 = the atoms per species)."""
        T, _, _ = self._staged_shape()
        lab, S, w, n = self._species_args(species, n_species, weights)
        out = np.empty((n, T), dtype=np.float64)
        counts = np.zeros(n, dtype=np.int64)
        self._call("species_self", int(quantity), int(fft), S, _ptr(lab), _ptr(w), _ptr(out), _ptr(counts))
        return out, counts

    def _kvectors(self, kvectors, dim):
        """(wavevectors as a C-contiguous float64 (n_k, dim) array, n_k)"""
        k = np.ascontiguousarray(kvectors, dtype=np.float64)
        if k.ndim != 2 or k.shape[1] != dim:
            raise ValueError(f"kvectors: shape {k.shape}, expected (n_k, {dim}) (one component per staged column)")
        return k, int(k.shape[0])

    def scatter(self, fft, kvectors, self_part=True, density=True, collective=True):
        """Intermediate scattering functions of slab 0 (the positions), ta_scatter: `kvectors` (n_k, dim) in rad per length
        unit: (self (n_k, n_frames) = sum_n <cos(k . (x_n(t + tau) - x_n(t)))>, density (n_k, n_frames, 2) = sum_n (cos, sin)
        (k . x_n(t)), coll (n_k, n_frames) = the autocorrelation of the density), None for one not asked for; nothing is
        divided by the number of atoms.  A group: the members' self parts and densities are summed, then ONE collective
        part runs."""
        T, _, D = self._staged_shape()
        k, K = self._kvectors(kvectors, D)
        fs = np.empty((K, T), dtype=np.float64) if self_part else None
        rho = np.empty((K, T, 2), dtype=np.float64) if density else None
        coll = np.empty((K, T), dtype=np.float64) if collective else None
        self._call("scatter", int(fft), K, _ptr(k), _ptr(fs), _ptr(rho), _ptr(coll))
        return fs, rho, coll

    def kcurrent(self, fft, kvectors, weights=None, current=True, longitudinal=True, transverse=True):
        """Current correlation functions of slab 0 (the velocities) and slab 1 (the positions), ta_kcurrent: `kvectors`
        (n_k, dim) in rad per length unit, `weights` one per staged atom or None (all 1): (current (n_k, n_frames, dim, 2) =
        sum_n w_n v_n (cos, sin)(k . x_n), long (n_k, n_frames), trans (n_k, n_frames)), None for one not asked for; nothing
        is divided by the number of atoms.  A group: the members' currents are summed, then ONE correlation runs."""
        T, _, D = self._staged_shape()
        k, K = self._kvectors(kvectors, D)
        w = self._per_atom(weights, np.float64, "weights", "values")
        cur = np.empty((K, T, D, 2), dtype=np.float64) if current else None
        lon = np.empty((K, T), dtype=np.float64) if longitudinal else None
        tr = np.empty((K, T), dtype=np.float64) if transverse else None
        self._call("kcurrent", int(fft), K, _ptr(k), _ptr(w), _ptr(cur), _ptr(lon), _ptr(tr))
        return cur, lon, tr

    def partial_density(self, fft, kvectors, species, n_species=None, weights=None, cross=True):
        """Species-resolved density of slab 0 (the positions) and its cross term, ta_partial_density: `kvectors` (n_k, dim) in
        rad per length unit, `species` one integer label in 0 ... n_species - 1 per staged atom (n_species: default the
        largest label + 1), `weights` one per atom or None (all 1): (density (n_k, n_species, n_frames, 2) = sum_{n in a} w_n
        (cos, sin)(k . x_n), cross (n_k, n_frames, n_species, n_species) with lag 0, or None); nothing is divided by the
        number of atoms.  A group: the members' densities are summed, then ONE cross term runs."""
        T, _, D = self._staged_shape()
        k, K = self._kvectors(kvectors, D)
        lab, S, w, n = self._species_args(species, n_species, weights)
        rho = np.empty((K, n, T, 2), dtype=np.float64)
        c = np.empty((K, T, n, n), dtype=np.float64) if cross else None
        self._call("partial_density", int(fft), K, _ptr(k), S, _ptr(lab), _ptr(w), _ptr(rho), _ptr(c))
        return rho, c

    @staticmethod
    def _lags(lags):
        lg = np.ascontiguousarray(lags, dtype=np.int64)
        if lg.ndim != 1:
            raise ValueError(f"lags: shape {lg.shape}, expected (n_lags,) integer frame lags")
        return lg, int(lg.shape[0])

    def vanhove(self, lags, n_bins, dr, counts=True, moments=True):
        """Self van Hove function of slab 0 (the positions), ta_vanhove: for the integer frame `lags` (strictly increasing,
        below n_frames) the histogram of |x(t + lag) - x(t)| in `n_bins` bins of width `dr` plus the overflow bin, and
        (sum r2, sum r2 r2): (counts (n_lags, n_bins + 1) int64, moments (n_lags, 2)), None for one not asked for; nothing
        is divided by the number of pairs.  A group: the members' counts and moments are summed."""
        lg, L = self._lags(lags)
        n_bins = int(n_bins)
        cnt = np.empty((L, max(n_bins, 0) + 1), dtype=np.int64) if counts else None
        mom = np.empty((L, 2), dtype=np.float64) if moments else None
        self._call("vanhove", L, _ptr(lg), n_bins, float(dr), _ptr(cnt), _ptr(mom))
        return cnt, mom

    @staticmethod
    def _cutoffs(cutoffs):
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(cutoffs, dtype=np.float64)))
        if a.ndim != 1:
            raise ValueError(f"cutoffs: shape {a.shape}, expected a scalar or (n_cutoffs,)")
        return a, int(a.shape[0])

    def overlap(self, lags, cutoffs):
        """Self-overlap per time origin of slab 0 (the positions), ta_overlap: for the integer frame `lags` (strictly
        increasing, below n_frames) and the `cutoffs` a_c (> 0, strictly increasing, at most 4) the int64 array Q (n_cutoffs,
        n_lags, n_frames) of the atoms with |x(t0 + lag) - x(t0)| < a_c, zeros at t0 >= n_frames - lag; nothing is divided.
        A group: the members' Q are summed (a variance over origins comes after that sum)."""
        lg, L = self._lags(lags)
        a, C = self._cutoffs(cutoffs)
        T = self.shape[0] if self.shape is not None else 0
        q = np.empty((C, L, T), dtype=np.int64)
        self._call("overlap", L, _ptr(lg), C, _ptr(a), _ptr(q))
        return q

    def overlap_density(self, kvectors, lags, cutoffs):
        """Density of the overlap field per time origin of slab 0 (the positions), ta_overlap_density: for `kvectors` (n_k,
        dim) in rad per length unit (k = 0 allowed), the integer frame `lags` and the `cutoffs` a_c of `overlap` the
        complex128 array W (n_k, n_cutoffs, n_lags, n_frames) = sum over the atoms with |x(t0 + lag) - x(t0)| < a_c of
        exp(i k . x(t0)), zeros at t0 >= n_frames - lag; nothing is divided.  A group: the members' W are summed (|W|^2
        and a variance over origins come after that sum)."""
        T, D = (self.shape[0], self.shape[2]) if self.shape is not None else (0, 0)
        if D:
            k, K = self._kvectors(kvectors, D)
        else:  # unstaged: the library reports it
            k = np.ascontiguousarray(kvectors, dtype=np.float64)
            K = int(k.shape[0]) if k.ndim else 0
        lg, L = self._lags(lags)
        a, C = self._cutoffs(cutoffs)
        w = np.empty((K, C, L, T, 2), dtype=np.float64)
        self._call("overlap_density", K, _ptr(k), L, _ptr(lg), C, _ptr(a), _ptr(w))
        return w.view(np.complex128)[..., 0]

    def unwrap(self, slab, dimensions, axes):
        """Undo periodic wrapping of staged slab `slab` in place (MDAnalysis' NoJump, ta_unwrap; a group: on every
        member's block of the slab): `dimensions` the (n_frames, 6) boxes [a, b, c, alpha, beta, gamma] of the staged
        frames, `axes` the box axis (0, 1, 2) of each staged column of an atom."""
        dims = np.ascontiguousarray(dimensions, dtype=np.float64)
        if self.shape is not None and dims.shape != (self.shape[0], 6):
            raise ValueError(f"dimensions: shape {dims.shape}, expected ({self.shape[0]}, 6) (one box per staged frame)")
        ax = np.ascontiguousarray(axes, dtype=np.int32).ravel()
        self._call("unwrap", int(slab), _ptr(dims), _ptr(ax))


class Context(_Staged):
    """One ta_ctx: owns a stream, plan tables, workspaces and the staged slabs.  `device`: a GPU index, or
    "cpu" / DEVICE_CPU for the opt-in CPU backend (host slabs, OpenMP; the device-pointer calls are unsupported).
    `member_of`, `handle`: a group's member context, borrowed from it (Group.member_context)."""

    def __init__(self, device=0, *, member_of=None, handle=None):
        self.device = device_index(device)
        self.is_cpu = self.device == DEVICE_CPU
        self._slabs = []
        self._group = member_of  # a member's context lives as long as its group: the view keeps the group alive
        self._h = handle
        if member_of is None:
            self._h = ctypes.c_void_p(None)
            L = lib()
            rc = L.ta_ctx_create(self.device, ctypes.byref(self._h))
            if rc != 0:
                raise TAError(rc, L.ta_last_error(None).decode())

    def close(self):
        if self._h:
            self._drop_views()
            if self._group is None:  # a group member's context belongs to its group
                lib().ta_ctx_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def result_home(self, shape):
        """Start page-locking the by-particle result array of `shape`; `.get()` returns it."""
        return _PlainHome(shape) if self.is_cpu else PinnedResult(shape, device=self.device)

    # -- staging --------------------------------------------------------
    def stage_alloc(self, n_frames, n_atoms, dim, n_slabs=1, dtype=np.float64):
        """Pinned host slabs (n_frames, n_atoms, dim) as NumPy views + device twins."""
        ptrs = (ctypes.c_void_p * n_slabs)()
        self._drop_views()
        self._call("stage_alloc", n_frames, n_atoms, dim, _dtype_code(dtype), n_slabs, ptrs)
        self._staged(n_frames, n_atoms, dim, [_slab_view(p, dtype, (n_frames, n_atoms, dim)) for p in ptrs])
        return list(self._slabs)

    def stage_alloc_device(self, n_frames, n_atoms, dim, n_slabs=1):
        """Device slabs only (pair-major), for data that is already on the GPU."""
        self._drop_views()
        self._call("stage_alloc_device", n_frames, n_atoms, dim, n_slabs)
        self._staged(n_frames, n_atoms, dim)

    def stage_commit_dev(self, slab, d_src, ld_row, frame_lo, frame_hi, dtype=np.float64, stream=0):
        self._call("stage_commit_dev", slab, d_src, _dtype_code(dtype), int(ld_row), int(frame_lo), int(frame_hi), stream or None)

    def stage_synth(self, slab, seed, col_offset, n_cols_total, stream=0):
        self._call("stage_synth", slab, int(seed), int(col_offset), int(n_cols_total), stream or None)

    def stage_read_dev(self, slab, d_dst, ld_row, stream=0):
        self._call("stage_read_dev", slab, d_dst, int(ld_row), stream or None)

    def stage_device(self, slab):
        """(device pointer, rows per column pair, number of pairs) of the pair-major slab."""
        p, pitch, n_pairs = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        self._call("stage_device", slab, ctypes.byref(p), ctypes.byref(pitch), ctypes.byref(n_pairs))
        return p.value, pitch.value, n_pairs.value

    def trim(self):
        self._call("trim")

    def compound(self, offsets, members, weights=None, frame_weights=None):
        """Replace staged slab 0 by the float64 slab of its compounds (ta_compound): compound c = the member entries
        [offsets[c], offsets[c + 1]) of `members` (atom indices, in any order), `weights` one per member entry or None (all
        1), `frame_weights` one per staged atom or None: their weighted mean over all atoms is subtracted (times the
        compound's weight sum).  The context's shape becomes (n_frames, n_compounds, dim) and the host views are dropped:
        nothing can be staged until the next stage_alloc.  Returns the new host slab's view on a CPU context, else None."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
        mem = np.ascontiguousarray(members, dtype=np.int32).ravel()
        n = int(off.size) - 1
        if n >= 1 and int(off[-1]) != mem.size:
            raise ValueError(f"compound: offsets end at {int(off[-1])}, and there are {mem.size} member entries")
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).ravel()
        if w is not None and w.size != mem.size:
            raise ValueError(f"compound: {w.size} weights for {mem.size} member entries")
        u = self._per_atom(frame_weights, np.float64, "frame_weights", "values")
        out = ctypes.c_void_p()
        self._call("compound", n, _ptr(off), _ptr(mem), _ptr(w), _ptr(u), ctypes.byref(out))
        T, _, D = self._staged_shape()
        self._drop_views()
        self._staged(T, n, D)
        if not out.value:
            return None
        view = _slab_view(out.value, np.float64, (T, n, D))
        self._slabs = [view]  # dropped (made read-only) with the slab, like the staging views
        return view

    def moment_msd(self, moment, fft):
        """Phi(k) of a (n_frames, dim) moment, e.g. the sum of several shards' moments: the moment is staged as a
        one-atom slab (replacing this context's slabs) whose conductivity with charge 1 is that moment's MSD."""
        moment = np.asarray(moment, dtype=np.float64)
        T, D = moment.shape
        (view,) = self.stage_alloc(T, 1, D)
        view[:, 0, :] = moment
        self.stage_commit(0, T)
        return self.conductivity(fft, np.ones(1))[1]

    def _cross(self, name, noun, sums, fft):
        a = np.ascontiguousarray(sums, dtype=np.float64)
        if a.ndim != 3:
            raise ValueError(f"{noun}: shape {a.shape}, expected (n_species, n_frames, dim)")
        S, T, D = a.shape
        c = np.empty((T, S, S), dtype=np.float64)
        self._call(name, int(fft), _ptr(a), S, T, D, _ptr(c))
        return c

    def onsager_cross(self, moments, fft):
        """C (n_frames, S, S) of given (S, n_frames, dim) moments, e.g. the sum of several shards' moments
        (ta_onsager_cross): needs no staged slab and leaves the context's slabs as they are."""
        return self._cross("onsager_cross", "moments", moments, fft)

    def current_cross(self, currents, fft):
        """C (n_frames, S, S) of given (S, n_frames, dim) currents, e.g. the sum of several shards' currents
        (ta_current_cross): needs no staged slab and leaves the context's slabs as they are."""
        return self._cross("current_cross", "currents", currents, fft)

    def scatter_collective(self, density, fft):
        """coll (n_k, n_frames) of a given (n_k, n_frames, 2) density, e.g. the sum of several shards' densities
        (ta_scatter_collective): needs no staged slab and leaves the context's slabs as they are."""
        a = np.ascontiguousarray(density, dtype=np.float64)
        if a.ndim != 3 or a.shape[2] != 2:
            raise ValueError(f"density: shape {a.shape}, expected (n_k, n_frames, 2)")
        K, T, _ = a.shape
        c = np.empty((K, T), dtype=np.float64)
        self._call("scatter_collective", int(fft), _ptr(a), K, T, _ptr(c))
        return c

    def kcurrent_correlate(self, current, kvectors, fft):
        """(long, trans) (n_k, n_frames) of a given (n_k, n_frames, dim, 2) current, e.g. the sum of several shards' currents
        (ta_kcurrent_correlate): needs no staged slab and leaves the context's slabs as they are."""
        a = np.ascontiguousarray(current, dtype=np.float64)
        if a.ndim != 4 or a.shape[3] != 2:
            raise ValueError(f"current: shape {a.shape}, expected (n_k, n_frames, dim, 2)")
        K, T, D, _ = a.shape
        k, n_k = self._kvectors(kvectors, D)
        if n_k != K:
            raise ValueError(f"kvectors: {n_k} wavevectors for a current of {K}")
        lon, tr = np.empty((K, T), dtype=np.float64), np.empty((K, T), dtype=np.float64)
        self._call("kcurrent_correlate", int(fft), _ptr(a), K, _ptr(k), T, D, _ptr(lon), _ptr(tr))
        return lon, tr

    def partial_cross(self, density, fft):
        """cross (n_k, n_frames, S, S) of a given (n_k, S, n_frames, 2) density, e.g. the sum of several shards' densities
        (ta_partial_cross): needs no staged slab and leaves the context's slabs as they are."""
        a = np.ascontiguousarray(density, dtype=np.float64)
        if a.ndim != 4 or a.shape[3] != 2:
            raise ValueError(f"density: shape {a.shape}, expected (n_k, n_species, n_frames, 2)")
        K, S, T, _ = a.shape
        c = np.empty((K, T, S, S), dtype=np.float64)
        self._call("partial_cross", int(fft), _ptr(a), K, S, T, _ptr(c))
        return c

    # -- device-pointer compute (asynchronous) --------------------------
    def vacf_fft_dev(self, d_vel, n_frames, n_atoms, dim, ld_row, d_lagsum, d_bp=0, ld_bp=0, stream=0):
        self._call("vacf_fft_dev", d_vel, n_frames, n_atoms, dim, ld_row, d_lagsum, d_bp or None, ld_bp, stream or None)

    def vacf_direct_dev(self, d_vel, n_frames, n_atoms, dim, ld_row, d_lagsum, d_bp=0, ld_bp=0, stream=0):
        self._call("vacf_direct_dev", d_vel, n_frames, n_atoms, dim, ld_row, d_lagsum, d_bp or None, ld_bp, stream or None)

    def helfand_msd_dev(self, d_vel, d_pos, d_masses, n_frames, n_atoms, dim, ld_row, scale, d_lagsum,
                        d_bp=0, ld_bp=0, stream=0):
        self._call("helfand_msd_dev", d_vel, d_pos, d_masses, n_frames, n_atoms, dim, ld_row, scale, d_lagsum,
                   d_bp or None, ld_bp, stream or None)

    def msd_dev(self, d_pos, n_frames, n_atoms, dim, ld_row, fft, d_lagsum, d_bp=0, ld_bp=0, stream=0):
        self._call("msd_dev", d_pos, n_frames, n_atoms, dim, ld_row, int(fft), d_lagsum, d_bp or None, ld_bp, stream or None)

    def conductivity_dev(self, d_pos, n_frames, n_atoms, dim, ld_row, fft, d_charges, d_moment, d_collective=0,
                         d_self=0, stream=0):
        self._call("conductivity_dev", d_pos, n_frames, n_atoms, dim, ld_row, int(fft), d_charges, d_moment,
                   d_collective or None, d_self or None, stream or None)

    def onsager_dev(self, d_pos, n_frames, n_atoms, dim, ld_row, fft, n_species, d_species, d_moments, d_weights=0,
                    d_cross=0, stream=0):
        self._call("onsager_dev", d_pos, n_frames, n_atoms, dim, ld_row, int(fft), int(n_species), d_species,
                   d_weights or None, d_moments, d_cross or None, stream or None)

    def current_dev(self, d_vel, n_frames, n_atoms, dim, ld_row, fft, n_species, d_species, d_currents, d_weights=0,
                    d_cross=0, stream=0):
        self._call("current_dev", d_vel, n_frames, n_atoms, dim, ld_row, int(fft), int(n_species), d_species,
                   d_weights or None, d_currents, d_cross or None, stream or None)

    # -- compute on the staged slabs, device outputs (asynchronous) ------
    def vacf_fft_staged(self, d_lagsum, d_bp=0, ld_bp=0, stream=0):
        self._call("vacf_fft_staged", d_lagsum, d_bp or None, ld_bp, stream or None)

    def vacf_direct_staged(self, d_lagsum, d_bp=0, ld_bp=0, stream=0):
        self._call("vacf_direct_staged", d_lagsum, d_bp or None, ld_bp, stream or None)

    def helfand_msd_staged(self, d_masses, scale, d_lagsum, d_bp=0, ld_bp=0, stream=0):
        self._call("helfand_msd_staged", d_masses, scale, d_lagsum, d_bp or None, ld_bp, stream or None)

    def msd_staged(self, fft, d_lagsum, d_bp=0, ld_bp=0, stream=0):
        self._call("msd_staged", int(fft), d_lagsum, d_bp or None, ld_bp, stream or None)

    def conductivity_staged(self, fft, d_charges, d_moment, d_collective=0, d_self=0, stream=0):
        self._call("conductivity_staged", int(fft), d_charges, d_moment, d_collective or None, d_self or None, stream or None)

    def onsager_staged(self, fft, n_species, d_species, d_moments, d_weights=0, d_cross=0, stream=0):
        self._call("onsager_staged", int(fft), int(n_species), d_species, d_weights or None, d_moments, d_cross or None,
                   stream or None)

    def current_staged(self, fft, n_species, d_species, d_currents, d_weights=0, d_cross=0, stream=0):
        self._call("current_staged", int(fft), int(n_species), d_species, d_weights or None, d_currents, d_cross or None,
                   stream or None)

    def species_self_dev(self, d_x, n_frames, n_atoms, dim, ld_row, quantity, fft, n_species, species, d_self, d_weights=0,
                         stream=0):
        """`species`: HOST labels, one per atom (checked by the library before anything is written)"""
        lab = np.ascontiguousarray(species, dtype=np.int32).ravel()
        if lab.size != n_atoms:
            raise ValueError(f"species: {lab.size} labels for {n_atoms} atoms")
        self._call("species_self_dev", d_x, n_frames, n_atoms, dim, ld_row, int(quantity), int(fft), int(n_species), _ptr(lab),
                   d_weights or None, d_self, stream or None)

    def species_self_staged(self, quantity, fft, n_species, species, d_self, d_weights=0, stream=0):
        """`species`: HOST labels, one per staged atom (checked by the library before anything is written)"""
        lab = self._per_atom(species, np.int32, "species", "labels")
        self._call("species_self_staged", int(quantity), int(fft), int(n_species), _ptr(lab), d_weights or None, d_self,
                   stream or None)

    def scatter_dev(self, d_pos, n_frames, n_atoms, dim, ld_row, fft, kvectors, d_self=0, d_density=0, d_coll=0, stream=0):
        """`kvectors`: HOST wavevectors (n_k, dim) (checked by the library before anything is written)"""
        k, K = self._kvectors(kvectors, dim)
        self._call("scatter_dev", d_pos, n_frames, n_atoms, dim, ld_row, int(fft), K, _ptr(k), d_self or None,
                   d_density or None, d_coll or None, stream or None)

    def scatter_staged(self, fft, kvectors, d_self=0, d_density=0, d_coll=0, stream=0):
        """`kvectors`: HOST wavevectors (n_k, dim) (checked by the library before anything is written)"""
        k, K = self._kvectors(kvectors, self._staged_shape()[2])
        self._call("scatter_staged", int(fft), K, _ptr(k), d_self or None, d_density or None, d_coll or None, stream or None)

    def kcurrent_staged(self, fft, kvectors, d_current=0, d_long=0, d_trans=0, d_weights=0, stream=0):
        """`kvectors`: HOST wavevectors (n_k, dim) (checked by the library before anything is written); d_weights: device"""
        k, K = self._kvectors(kvectors, self._staged_shape()[2])
        self._call("kcurrent_staged", int(fft), K, _ptr(k), d_weights or None, d_current or None, d_long or None,
                   d_trans or None, stream or None)

    def partial_density_staged(self, fft, kvectors, n_species, d_species, d_density, d_cross=0, d_weights=0, stream=0):
        """`kvectors`: HOST wavevectors (n_k, dim) (checked by the library before anything is written); d_species (int32
        labels), d_weights: device"""
        k, K = self._kvectors(kvectors, self._staged_shape()[2])
        self._call("partial_density_staged", int(fft), K, _ptr(k), int(n_species), d_species or None, d_weights or None,
                   d_density or None, d_cross or None, stream or None)

    def vanhove_dev(self, d_pos, n_frames, n_atoms, dim, ld_row, lags, n_bins, dr, d_counts=0, d_moments=0, stream=0):
        """`lags`: HOST frame lags (checked by the library before anything is written); d_counts (n_lags, n_bins + 1) int64"""
        lg, L = self._lags(lags)
        self._call("vanhove_dev", d_pos, n_frames, n_atoms, dim, ld_row, L, _ptr(lg), int(n_bins), float(dr), d_counts or None,
                   d_moments or None, stream or None)

    def vanhove_staged(self, lags, n_bins, dr, d_counts=0, d_moments=0, stream=0):
        """`lags`: HOST frame lags (checked by the library before anything is written); d_counts (n_lags, n_bins + 1) int64"""
        lg, L = self._lags(lags)
        self._call("vanhove_staged", L, _ptr(lg), int(n_bins), float(dr), d_counts or None, d_moments or None, stream or None)

    def overlap_dev(self, d_pos, n_frames, n_atoms, dim, ld_row, lags, cutoffs, d_q, stream=0):
        """`lags`, `cutoffs`: HOST arrays (checked by the library before anything is written); d_q (n_cutoffs, n_lags,
        n_frames) int64 on the device"""
        lg, L = self._lags(lags)
        a, C = self._cutoffs(cutoffs)
        self._call("overlap_dev", d_pos, n_frames, n_atoms, dim, ld_row, L, _ptr(lg), C, _ptr(a), d_q or None, stream or None)

    def overlap_staged(self, lags, cutoffs, d_q, stream=0):
        """`lags`, `cutoffs`: HOST arrays (checked by the library before anything is written); d_q (n_cutoffs, n_lags,
        n_frames) int64 on the device"""
        lg, L = self._lags(lags)
        a, C = self._cutoffs(cutoffs)
        self._call("overlap_staged", L, _ptr(lg), C, _ptr(a), d_q or None, stream or None)

    def overlap_density_staged(self, kvectors, lags, cutoffs, d_w, stream=0):
        """`kvectors`, `lags`, `cutoffs`: HOST arrays (checked by the library before anything is written); d_w (n_k,
        n_cutoffs, n_lags, n_frames, 2) float64 on the device"""
        k, K = self._kvectors(kvectors, self._staged_shape()[2])
        lg, L = self._lags(lags)
        a, C = self._cutoffs(cutoffs)
        self._call("overlap_density_staged", K, _ptr(k), L, _ptr(lg), C, _ptr(a), d_w or None, stream or None)

    def _vhd_args(self, lags, origin_stride, idx_a, idx_b, dimensions, axes, n_bins, dr):
        """the argument tuple ta_vanhove_distinct* share, and the arrays it points into (to be kept until the call is over)"""
        lg, L = self._lags(lags)
        (a, na), (b, nb) = _index_list(idx_a, "idx_a"), _index_list(idx_b, "idx_b")
        dims, ax = self._pair_box(dimensions, axes)
        keep = (lg, a, b, dims, ax)
        return (L, _ptr(lg), int(origin_stride), na, _ptr(a), nb, _ptr(b), _ptr(dims), _ptr(ax), int(n_bins), float(dr)), keep

    def vanhove_distinct(self, lags, n_bins, dr, *, origin_stride=1, idx_a=None, idx_b=None, dimensions=None, axes=None):
        """Distinct van Hove histogram of slab 0 (the positions), ta_vanhove_distinct: for the integer frame `lags` the
        counts (n_lags, n_bins + 1) int64 of the distances between item a_p at an origin frame (every `origin_stride`-th)
        and item b_q a lag later, over ordered pairs of different items, in `n_bins` bins of width `dr` plus the overflow
        bin.  `idx_a`, `idx_b`: strictly increasing item indices (None: all items / the same as a).  `dimensions`: the
        (n_frames, 6) boxes of the staged frames for the minimum image (None: no periodicity), `axes` the box axis of each
        staged column (None: 0, 1, ...).  Nothing is normalised.  One context only: a device group has no such call."""
        args, keep = self._vhd_args(lags, origin_stride, idx_a, idx_b, dimensions, axes, n_bins, dr)
        cnt = np.empty((args[0], max(int(n_bins), 0) + 1), dtype=np.int64)
        self._call("vanhove_distinct", *args, _ptr(cnt))
        del keep
        return cnt

    def vanhove_distinct_staged(self, lags, n_bins, dr, d_counts, *, origin_stride=1, idx_a=None, idx_b=None, dimensions=None,
                                axes=None, stream=0):
        """the lists and boxes are HOST arrays (checked by the library before anything is written); d_counts (n_lags,
        n_bins + 1) int64 on the device"""
        args, keep = self._vhd_args(lags, origin_stride, idx_a, idx_b, dimensions, axes, n_bins, dr)
        self._call("vanhove_distinct_staged", *args, d_counts or None, stream or None)
        del keep

    def _pair_box(self, dimensions, axes):
        """(dimensions, axes) of a pair call as contiguous arrays, or (None, None)"""
        if dimensions is None:
            return None, None
        dims = np.ascontiguousarray(dimensions, dtype=np.float64)
        if self.shape is not None and dims.shape != (self.shape[0], 6):
            raise ValueError(f"dimensions: shape {dims.shape}, expected ({self.shape[0]}, 6) (one box per staged frame)")
        ax = np.ascontiguousarray(np.arange(self._staged_shape()[2]) if axes is None else axes, dtype=np.int32).ravel()
        return dims, ax

    def pair_find(self, r_cut, *, search_stride=1, idx_a=None, idx_b=None, dimensions=None, axes=None):
        """Candidate pairs of slab 0 (the positions), ta_pair_find + ta_pair_find_read: the (n, 2) int32 staged item ids
        (a, b), sorted, of every pair of different items from `idx_a` x `idx_b` (strictly increasing item indices; None: all
        items / the same as a, then only a < b) closer than `r_cut` in at least one of the frames 0, search_stride, ...
        `dimensions`, `axes`: as for vanhove_distinct.  The list stays in the context (pair_lifetime(pairs=None) uses it)
        until trim() or a new staging.  One context only: a device group has no such call."""
        (a, na), (b, nb) = _index_list(idx_a, "idx_a"), _index_list(idx_b, "idx_b")
        dims, ax = self._pair_box(dimensions, axes)
        n = ctypes.c_int64(0)
        self._call("pair_find", na, _ptr(a), nb, _ptr(b), _ptr(dims), _ptr(ax), float(r_cut), int(search_stride), ctypes.byref(n))
        pairs = np.empty((int(n.value), 2), dtype=np.int32)
        if n.value:  # (an empty list is not read: ta_pair_find_read refuses it)
            self._call("pair_find_read", int(n.value), _ptr(pairs))
        return pairs

    def _pair_args(self, fft, pairs, r_cut, dimensions, axes):
        """the argument tuple ta_pair_lifetime* share, and the arrays it points into (to be kept until the call is over)"""
        pr, n = None, 0
        if pairs is not None:
            pr = np.ascontiguousarray(pairs)
            if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer):
                raise ValueError(f"pairs: shape {pr.shape} and dtype {pr.dtype}, expected an integer (n_pairs, 2) array")
            if pr.size and (pr.min() < -2**31 or pr.max() >= 2**31):
                raise ValueError("pairs: entries must fit int32")
            pr, n = np.ascontiguousarray(pr, dtype=np.int32), int(pr.shape[0])
        dims, ax = self._pair_box(dimensions, axes)
        return (int(fft), n, _ptr(pr), _ptr(dims), _ptr(ax), float(r_cut)), (pr, dims, ax)

    def pair_lifetime(self, fft, r_cut, pairs=None, *, dimensions=None, axes=None, ci=True, runs=True, nb=True):
        """Pair population sums of slab 0 (the positions), ta_pair_lifetime, of the (n_pairs, 2) staged item ids `pairs`
        (None: the list pair_find left in the context): (ci (n_frames,) = sum_pairs sum_t h(t) h(t + tau), NOT divided by
        n_frames - tau; runs (n_frames + 1,) int64 = the histogram of the lengths of the runs of bonded frames; nb
        (n_frames,) = the bonded pairs per frame), None for one not asked for.  One context only: a device group has no
        such call."""
        return self._life("pair_lifetime", self._life_outs(ci, runs, nb), self._pair_args(fft, pairs, r_cut, dimensions, axes))

    def pair_lifetime_staged(self, fft, r_cut, pairs=None, *, dimensions=None, axes=None, d_ci=0, d_runs=0, d_nb=0, stream=0):
        """`pairs`, `dimensions`: HOST arrays (checked by the library before anything is written); d_ci (n_frames,), d_runs
        (n_frames + 1,) int64, d_nb (n_frames,) on the device"""
        self._life_staged("pair_lifetime_staged", self._pair_args(fft, pairs, r_cut, dimensions, axes), (d_ci, d_runs, d_nb), stream)

    def _life_outs(self, ci, runs, nb):
        """the outputs (asked for, shape, dtype) of the three-output calls"""
        T = self._staged_shape()[0]
        return (ci, T, np.float64), (runs, T + 1, np.int64), (nb, T, np.float64)

    def _gated_outs(self, max_lag, n_sums, sums, count, runs, nb):
        """the outputs (asked for, shape, dtype) of shell_msd and shell_orient: n_sums sums per lag"""
        L = max(int(max_lag), 0)
        return ((sums, (L + 1, n_sums), np.float64), (count, L + 1, np.int64)) + self._life_outs(False, runs, nb)[1:]

    def _life(self, name, outs, args_keep):
        """what the pair, bond and shell calls share: the outputs asked for allocated, the call, the tuple of them"""
        args, keep = args_keep
        res = tuple(np.empty(shape, dtype=dtype) if want else None for want, shape, dtype in outs)
        self._call(name, *args, *(_ptr(o) for o in res))
        del keep
        return res

    def _life_staged(self, name, args_keep, d_outs, stream):
        args, keep = args_keep
        self._call(name, *args, *(d or None for d in d_outs), stream or None)
        del keep

    def _bond_args(self, fft, atoms, r_cut, r_break, cos_cut, cos_break, gap, dimensions, axes):
        """the argument tuple ta_bond_lifetime* share, and the arrays it points into (to be kept until the call is over)"""
        at = np.ascontiguousarray(atoms)
        if at.ndim != 2 or at.shape[1] not in (2, 3) or not np.issubdtype(at.dtype, np.integer):
            raise ValueError(f"atoms: shape {at.shape} and dtype {at.dtype}, expected an integer (n_bonds, 2) or (n_bonds, 3) array")
        if at.size and (at.min() < -2**31 or at.max() >= 2**31):
            raise ValueError("atoms: entries must fit int32")
        at = np.ascontiguousarray(at, dtype=np.int32)
        dims, ax = self._pair_box(dimensions, axes)
        r_break = r_cut if r_break is None else r_break
        cos_break = cos_cut if cos_break is None else cos_break
        return (int(fft), int(at.shape[0]), int(at.shape[1]), _ptr(at), _ptr(dims), _ptr(ax), float(r_cut), float(r_break),
                float(cos_cut), float(cos_break), int(gap)), (at, dims, ax)

    def bond_lifetime(self, fft, atoms, r_cut, *, r_break=None, cos_cut=0.0, cos_break=None, gap=0, dimensions=None, axes=None,
                      ci=True, runs=True, nb=True):
        """pair_lifetime's sums (ci, runs, nb) of slab 0 for the bonds `atoms`, ta_bond_lifetime: rows (p, q) or (donor,
        hydrogen, acceptor) of staged item ids; a bond forms below `r_cut` with (triplets) the cosine of the D-H-A angle at most
        `cos_cut`, lasts while below `r_break` / `cos_break` (None: the form values), and absences of up to `gap` frames (0 ...
        63) between bonded frames are filled.  One context only: a device group has no such call."""
        return self._life("bond_lifetime", self._life_outs(ci, runs, nb),
                          self._bond_args(fft, atoms, r_cut, r_break, cos_cut, cos_break, gap, dimensions, axes))

    def bond_lifetime_staged(self, fft, atoms, r_cut, *, r_break=None, cos_cut=0.0, cos_break=None, gap=0, dimensions=None, axes=None,
                             d_ci=0, d_runs=0, d_nb=0, stream=0):
        """`atoms`, `dimensions`: HOST arrays (checked by the library before anything is written); d_ci (n_frames,), d_runs
        (n_frames + 1,) int64, d_nb (n_frames,) on the device"""
        self._life_staged("bond_lifetime_staged", self._bond_args(fft, atoms, r_cut, r_break, cos_cut, cos_break, gap, dimensions, axes),
                          (d_ci, d_runs, d_nb), stream)

    def _shell_args(self, fft, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes):
        """the argument tuple ta_shell_residence* share, and the arrays it points into (to be kept until the call is over)"""
        (a, na), (b, nb) = _index_list(idx_a, "idx_a"), _index_list(idx_b, "idx_b")
        dims, ax = self._pair_box(dimensions, axes)
        r_break = r_cut if r_break is None else r_break
        return (int(fft), na, _ptr(a), nb, _ptr(b), _ptr(dims), _ptr(ax), float(r_cut), float(r_break), int(gap)), (a, b, dims, ax)

    def shell_residence(self, fft, r_cut, *, r_break=None, gap=0, idx_a=None, idx_b=None, dimensions=None, axes=None, ci=True,
                        runs=True, nb=True):
        """pair_lifetime's sums (ci, runs, nb) of slab 0 for one series per OBSERVED item of `idx_b` (None: the same as a),
        ta_shell_residence: the item is inside while SOME reference item of `idx_a` (None: all items) other than itself is
        closer than `r_cut`, stays inside while some is closer than `r_break` (None: r_cut), and absences of up to `gap` frames
        (0 ... 63) between frames inside are filled.  The lists: strictly increasing item indices, the same list or disjoint
        ones.  One context only: a device group has no such call."""
        return self._life("shell_residence", self._life_outs(ci, runs, nb),
                          self._shell_args(fft, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes))

    def shell_residence_staged(self, fft, r_cut, *, r_break=None, gap=0, idx_a=None, idx_b=None, dimensions=None, axes=None,
                               d_ci=0, d_runs=0, d_nb=0, stream=0):
        """the lists and `dimensions`: HOST arrays (checked by the library before anything is written); d_ci (n_frames,), d_runs
        (n_frames + 1,) int64, d_nb (n_frames,) on the device"""
        self._life_staged("shell_residence_staged", self._shell_args(fft, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes),
                          (d_ci, d_runs, d_nb), stream)

    def _shell_msd_args(self, condition, max_lag, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes):
        """the argument tuple ta_shell_msd* share, and the arrays it points into (to be kept until the call is over)"""
        code = SHELL_CONDITIONS.get(condition, condition)
        if isinstance(code, str):
            raise ValueError(f"condition: {condition!r}, expected one of {sorted(SHELL_CONDITIONS)}")
        args, keep = self._shell_args(code, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes)
        return (args[0], int(max_lag)) + args[1:], keep

    def shell_msd(self, condition, max_lag, r_cut, *, r_break=None, gap=0, idx_a=None, idx_b=None, dimensions=None, axes=None,
                  sums=True, count=True, runs=True, nb=True):
        """(sums (max_lag + 1, dim), count (max_lag + 1,) int64, runs, nb) of slab 0, ta_shell_msd: the squared displacements
        of the observed items of `idx_b` over the lags 0 ... max_lag, summed over the origins at which the item is in the shell
        of the reference items `idx_a` under `condition`: "continuous" (inside in every frame from the origin to the lag) or
        "endpoints" (inside at both ends); the shell, `runs` and `nb` as shell_residence's.  The positions must be unwrapped.
        One context only: a device group has no such call."""
        D = self._staged_shape()[2]
        args_keep = self._shell_msd_args(condition, max_lag, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes)
        return self._life("shell_msd", self._gated_outs(max_lag, D, sums, count, runs, nb), args_keep)

    def shell_msd_staged(self, condition, max_lag, r_cut, *, r_break=None, gap=0, idx_a=None, idx_b=None, dimensions=None,
                         axes=None, d_sums=0, d_count=0, d_runs=0, d_nb=0, stream=0):
        """the lists and `dimensions`: HOST arrays (checked by the library before anything is written); d_sums (max_lag + 1,
        dim), d_count (max_lag + 1,) int64, d_runs (n_frames + 1,) int64, d_nb (n_frames,) on the device"""
        self._life_staged("shell_msd_staged", self._shell_msd_args(condition, max_lag, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes),
                          (d_sums, d_count, d_runs, d_nb), stream)

    def _shell_orient_args(self, condition, max_lag, index, mode, anchor, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes):
        """the argument tuple ta_shell_orient* share, and the arrays it points into (to be kept until the call is over)"""
        (_, code, n_rows, p_idx, _, _), keep_o = self._orient_args(0, index, mode, None, None)
        args, keep = self._shell_msd_args(condition, max_lag, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes)
        n_a, n_b = args[2], args[4]  # (the library reads one index row per observed item)
        n_obs = n_b if idx_b is not None else n_a if idx_a is not None else self._staged_shape()[1]
        if n_rows != n_obs:
            raise ValueError(f"index: {n_rows} rows for {n_obs} observed items")
        return args[:2] + (code, int(anchor), p_idx) + args[2:], (keep, keep_o)

    def shell_orient(self, condition, max_lag, index, mode, r_cut, *, anchor=0, r_break=None, gap=0, idx_a=None, idx_b=None,
                     dimensions=None, axes=None, sums=True, count=True, runs=True, nb=True):
        """(sums (max_lag + 1, 2), count (max_lag + 1,) int64, runs, nb) of slab 0, ta_shell_orient: (sum c, sum c c) of
        c = u(t) . u(t + lag) over the unit vectors of `index` (rows as orient's for `mode`), each gated as shell_msd's terms
        by the shell series of its anchor atom, column `anchor` of its row; `idx_b` must list the anchors row by row (None:
        the anchors are the reference list `idx_a` itself).  `dimensions` serves the distance pass and the vectors' image
        step.  One context only: a device group has no such call."""
        self._staged_shape()  # (nothing staged is reported before anything about the arguments)
        args_keep = self._shell_orient_args(condition, max_lag, index, mode, anchor, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes)
        return self._life("shell_orient", self._gated_outs(max_lag, 2, sums, count, runs, nb), args_keep)

    def shell_orient_staged(self, condition, max_lag, index, mode, r_cut, *, anchor=0, r_break=None, gap=0, idx_a=None, idx_b=None,
                            dimensions=None, axes=None, d_sums=0, d_count=0, d_runs=0, d_nb=0, stream=0):
        """`index`, the lists and `dimensions`: HOST arrays (checked by the library before anything is written); d_sums
        (max_lag + 1, 2), d_count (max_lag + 1,) int64, d_runs (n_frames + 1,) int64, d_nb (n_frames,) on the device"""
        self._life_staged("shell_orient_staged",
                          self._shell_orient_args(condition, max_lag, index, mode, anchor, r_cut, r_break, gap, idx_a, idx_b, dimensions, axes),
                          (d_sums, d_count, d_runs, d_nb), stream)

    def _orient_args(self, fft, index, mode, dimensions, weights):
        """the argument tuple ta_orient* share, and the arrays it points into (to be kept until the call is over)"""
        code = ORIENT_MODES.get(mode, mode)
        if not isinstance(code, (int, np.integer)):
            raise ValueError(f"mode: {mode!r}, expected one of {sorted(ORIENT_MODES)}")
        width = 2 if code == 0 else 3
        idx = np.ascontiguousarray(index)
        if idx.ndim != 2 or idx.shape[1] != width or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"index: shape {idx.shape} and dtype {idx.dtype}, expected an integer (n_vectors, {width}) array "
                             f"for mode {mode!r}")
        if idx.size and (idx.min() < -2**31 or idx.max() >= 2**31):
            raise ValueError("index: entries must fit int32")
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        dims = w = None
        if dimensions is not None:
            dims = np.ascontiguousarray(dimensions, dtype=np.float64)
            if self.shape is not None and dims.shape != (self.shape[0], 6):
                raise ValueError(f"dimensions: shape {dims.shape}, expected ({self.shape[0]}, 6) (one box per staged frame)")
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
            if w.size != idx.shape[0]:
                raise ValueError(f"weights: {w.size} values for {idx.shape[0]} vectors")
        return (int(fft), int(code), int(idx.shape[0]), _ptr(idx), _ptr(dims), _ptr(w)), (idx, dims, w)

    def orient(self, fft, index, mode, dimensions=None, weights=None, c1=True, c2=True, total=True, collective=True):
        """Rotational correlation functions of slab 0 (the positions, three columns per atom), ta_orient: `index` (n_vectors,
        2) atoms (a, b) for mode "bond", (n_vectors, 3) atoms (a, b, c) for "bisector" and "normal"; `dimensions` the
        (n_frames, 6) boxes of the staged frames for the image step (None: nothing is reduced); `weights` one per vector or
        None (all 1; they enter total and coll only): (c1 (n_frames,) = sum_n <u_n . u_n'>, c2 (n_frames,) = sum_n
        <Q_n : Q_n'> = 2/3 sum_n <P2>, total (n_frames, 3) = sum_n w_n u_n, coll (n_frames,) = the autocorrelation of the
        total), None for one not asked for; nothing is divided by the number of vectors.  One context only: a device group
        has no such call."""
        T = self._staged_shape()[0]
        args, keep = self._orient_args(fft, index, mode, dimensions, weights)
        o1 = np.empty(T, dtype=np.float64) if c1 else None
        o2 = np.empty(T, dtype=np.float64) if c2 else None
        tot = np.empty((T, 3), dtype=np.float64) if total else None
        coll = np.empty(T, dtype=np.float64) if collective else None
        self._call("orient", *args, _ptr(o1), _ptr(o2), _ptr(tot), _ptr(coll))
        del keep
        return o1, o2, tot, coll

    def orient_dev(self, d_pos, n_frames, n_atoms, dim, ld_row, fft, index, mode, dimensions=None, weights=None, d_c1=0, d_c2=0,
                   d_total=0, d_coll=0, stream=0):
        """`index`, `dimensions`, `weights`: HOST arrays (checked by the library before anything is written)"""
        args, keep = self._orient_args(fft, index, mode, dimensions, weights)
        self._call("orient_dev", d_pos, n_frames, n_atoms, dim, ld_row, *args, d_c1 or None, d_c2 or None, d_total or None,
                   d_coll or None, stream or None)
        del keep

    def orient_staged(self, fft, index, mode, dimensions=None, weights=None, d_c1=0, d_c2=0, d_total=0, d_coll=0, stream=0):
        """`index`, `dimensions`, `weights`: HOST arrays (checked by the library before anything is written)"""
        args, keep = self._orient_args(fft, index, mode, dimensions, weights)
        self._call("orient_staged", *args, d_c1 or None, d_c2 or None, d_total or None, d_coll or None, stream or None)
        del keep

    def _chain_args(self, fft, members, coeff, dimensions):
        """the argument tuple ta_chain_modes* share, and the arrays it points into (to be kept until the call is over)"""
        mem = np.ascontiguousarray(members)
        if mem.ndim != 2 or not np.issubdtype(mem.dtype, np.integer):
            raise ValueError(f"members: shape {mem.shape} and dtype {mem.dtype}, expected an integer (n_chains, chain_len) array")
        if mem.size and (mem.min() < -2**31 or mem.max() >= 2**31):
            raise ValueError("members: entries must fit int32")
        mem = np.ascontiguousarray(mem, dtype=np.int32)
        co = np.ascontiguousarray(coeff, dtype=np.float64)
        if co.ndim != 2 or co.shape[1] != mem.shape[1]:
            raise ValueError(f"coeff: shape {co.shape}, expected (n_modes, {mem.shape[1]}) (one coefficient per bead)")
        dims = None
        if dimensions is not None:
            dims = np.ascontiguousarray(dimensions, dtype=np.float64)
            if self.shape is not None and dims.shape != (self.shape[0], 6):
                raise ValueError(f"dimensions: shape {dims.shape}, expected ({self.shape[0]}, 6) (one box per staged frame)")
        return (int(fft), int(mem.shape[0]), int(mem.shape[1]), _ptr(mem), int(co.shape[0]), _ptr(co), _ptr(dims)), (mem, co, dims)

    def chain_modes(self, fft, members, coeff, dimensions=None):
        """Autocorrelations of linear functionals of whole chains of slab 0 (the positions, three columns per atom),
        ta_chain_modes: `members` (n_chains, chain_len) atoms in backbone order, `coeff` (n_modes, chain_len) one row per
        functional of the chain made whole bead by bead (relative to its first bead), `dimensions` the (n_frames, 6) boxes of
        the staged frames for the image step (None: nothing is reduced): acf (n_modes, n_frames), the sum over chains, not
        divided by their number.  One context only: a device group has no such call."""
        T = self._staged_shape()[0]
        args, keep = self._chain_args(fft, members, coeff, dimensions)
        acf = np.empty((args[4], T), dtype=np.float64)
        self._call("chain_modes", *args, _ptr(acf))
        del keep
        return acf

    def chain_modes_staged(self, fft, members, coeff, dimensions=None, d_acf=0, stream=0):
        """`members`, `coeff`, `dimensions`: HOST arrays (checked by the library before anything is written); d_acf (n_modes,
        n_frames) on the device"""
        args, keep = self._chain_args(fft, members, coeff, dimensions)
        self._call("chain_modes_staged", *args, d_acf or None, stream or None)
        del keep

    # -- timing ----------------------------------------------------------
    def timing_history(self, max_n=64):
        """[(total_ms, main_kernel_ms)] of the last compute calls, oldest first."""
        n = ctypes.c_int()
        t = (ctypes.c_float * max_n)()
        m = (ctypes.c_float * max_n)()
        self._call("timing_history", max_n, t, m, ctypes.byref(n))
        return [(t[i], m[i]) for i in range(n.value)]

    def kernel_timeline(self, max_n=32):
        """[(kernel name, ms)] of the last compute call (needs set_option("timeline", 1))."""
        n = ctypes.c_int()
        names = (ctypes.c_char_p * max_n)()
        ms = (ctypes.c_float * max_n)()
        self._call("kernel_timeline", max_n, names, ms, ctypes.byref(n))
        return [(names[i].decode(), ms[i]) for i in range(n.value)]

    def kernel_launches(self, name):
        """launches recorded under `name` in the last compute call's timeline (needs set_option("timeline", 1))"""
        n = ctypes.c_int()
        self._call("kernel_launches", name.encode(), ctypes.byref(n))
        return n.value

    def clock_probe(self, n_launches):
        """{"mhz", "cycles_per_unit_pass", "ms_per_launch"} of the stamped lag-sum forward kernel
        launched n_launches times back to back on the staged slab (ta_clock_probe)."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._call("clock_probe", int(n_launches), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return {"mhz": a.value, "cycles_per_unit_pass": b.value, "ms_per_launch": c.value}

    def last_timing(self):
        t, m = ctypes.c_float(), ctypes.c_float()
        self._call("last_timing", ctypes.byref(t), ctypes.byref(m))
        return t.value, m.value


class Group(_Staged):
    """Several GPUs behind one object (ta_group): ONE frame loop fills every GPU's column block of
    the slab, a compute call fans out, reduces the lag sums once inside the library (RCCL for
    distinct devices; `reduce_kind` says what ran) and copies by-particle blocks into the column
    ranges of one host array.  Same methods as `Context` where the analysis classes use them;
    `stage_alloc` returns, per slab, the list of per-member views, and `shards` the members' atom
    ranges [(lo, hi), ...] (an empty range: more devices than atoms, its view is None)."""

    _prefix = "ta_group_"

    def __init__(self, devices):
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("devices must name at least one GPU")
        self._h = ctypes.c_void_p(None)
        L = lib()
        ids = (ctypes.c_int * len(devices))(*devices)
        rc = L.ta_group_create(ids, len(devices), ctypes.byref(self._h))
        if rc != 0:
            raise TAError(rc, L.ta_group_last_error(None).decode())
        self.devices = devices
        self.device = devices[0]
        self.shards = []
        self._slabs = []  # the members' views, slab by slab (flat)
        self._member_views = []

    def close(self):
        if self._h:
            self._drop_views()
            for ref in self._member_views:
                c = ref()
                if c is not None:  # a borrowed member context must not outlive the group's handle
                    c._h = ctypes.c_void_p(None)
            self._member_views = []
            lib().ta_group_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    @property
    def reduce_kind(self):
        return lib().ta_group_reduce_kind(self._h).decode()

    @property
    def reduce_note(self):
        """why an automatic reduce fell back from RCCL to peer copies ("" when it did not)"""
        return lib().ta_group_reduce_note(self._h).decode()

    @property
    def rccl_ranks(self):
        """ranks of the communicator the last RCCL reduce ran on (ncclCommCount)"""
        return int(lib().ta_group_rccl_ranks(self._h))

    def member_context(self, i):
        """Member i's context as a non-owning `Context` (timing history, options of one member)."""
        import weakref

        h, dev = ctypes.c_void_p(), ctypes.c_int()
        self._call("member", int(i), ctypes.byref(h), ctypes.byref(dev))
        c = Context(dev.value, member_of=self, handle=h)
        self._member_views.append(weakref.ref(c))  # close() invalidates the view
        return c

    def shard(self, n_atoms, i):
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        self._call("shard", int(n_atoms), int(i), ctypes.byref(lo), ctypes.byref(hi))
        return lo.value, hi.value

    def result_home(self, shape):
        return PinnedResult(shape, device=self.device)

    def _staged(self, n_frames, n_atoms, dim, views=()):
        super()._staged(n_frames, n_atoms, dim, [a for a in views if a is not None])
        self.shards = [self.shard(n_atoms, i) for i in range(len(self.devices))]

    def stage_alloc(self, n_frames, n_atoms, dim, n_slabs=1, dtype=np.float64):
        """-> [slab][member] NumPy views (n_frames, hi_i - lo_i, dim) of the members' pinned slabs."""
        n_dev = len(self.devices)
        ptrs = (ctypes.c_void_p * (n_dev * n_slabs))()
        self._drop_views()
        self._call("stage_alloc", n_frames, n_atoms, dim, _dtype_code(dtype), n_slabs, ptrs)
        sizes = [hi - lo for lo, hi in (self.shard(n_atoms, i) for i in range(n_dev))]
        out = [[_slab_view(ptrs[i * n_slabs + s], dtype, (n_frames, sizes[i], dim)) if sizes[i] and ptrs[i * n_slabs + s] else None
                for i in range(n_dev)] for s in range(n_slabs)]
        self._staged(n_frames, n_atoms, dim, [a for views in out for a in views])
        return out

    def stage_alloc_device(self, n_frames, n_atoms, dim, n_slabs=1):
        self._drop_views()
        self._call("stage_alloc_device", n_frames, n_atoms, dim, n_slabs)
        self._staged(n_frames, n_atoms, dim)

    def stage_synth(self, slab, seed, col_offset, n_cols_total):
        self._call("stage_synth", slab, int(seed), int(col_offset), int(n_cols_total))

    def conductivity(self, fft, charges, self_term=False, collective=True):
        """As Context.conductivity, charges of all atoms; the members' moments and self lag sums are summed, then ONE
        collective MSD runs (collective=False is not available here)."""
        if not collective:
            raise ValueError("a device group always evaluates the collective term")
        return super().conductivity(fft, charges, self_term, True)
