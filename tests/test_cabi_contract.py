"""The C-ABI's argument and state contract, pinned row by row: (entry point, state, arguments) -> (status code, exact
ta_last_error / ta_group_last_error text), for the staging, option, timing, host-facing and group entry points; and
the lifetime rules of the workspaces and of the commit queue (ta_trim, "async_commit", a queued commit's failure).

A row names the state its handle is in, a call on the raw ctypes library and what must come back.  Rows on CPU
contexts and on NULL handles need no GPU; the rest are marked gpu.  Where two checks of one call would both fail the
row says so in its id ("A+B": A's message is the one reported).  No row reaches a kernel launch with a made-up
pointer: every made-up "device pointer" below belongs to a call that is rejected before anything is queued."""
import ctypes

import numpy as np
import pytest

from transport_analysis_amd import _lib

INVALID, NOMEM, HIP, STATE, UNSUPPORTED = -1, -2, -3, -4, -5
T, A, D = 8, 3, 3

NO_CPU = "not available on the CPU backend (device pointers, streams and kernel timings belong to GPU contexts)"
NULL_CTX = "null context"
NULL_ARG = "null argument"
NOT_STAGED = "slabs have not been staged"
NO_SLAB = "no such slab"
RANGE = "frame range out of bounds"
LD_ROW = "ld_row smaller than n_atoms*dim"
FFT_FLAG = "fft must be 0 or 1"
SHAPE = "need n_frames >= 1, n_atoms >= 1, 1 <= dim <= 3"
NULL_DEV = "null device pointer"
LD_BP = "ld_bp smaller than n_atoms"
MFMA = ("direct_mfma: 0 vector kernels, 1 by trajectory length (default), 3 matrix cores always "
        "(2, the column-packed forms, left the library in round 6: tools/band/)")
COLUMNS = "columns col0 + k col_step (k < n_col) must lie inside a source row of ld_row elements"
GROUP_SHAPE = "need n_frames >= 1, n_atoms >= 1, 1 <= dim <= 3, 1 <= n_slabs <= 4"
NULL_GROUP = "null group"
SPECIES = "n_species must be 1 ... 8"
LABELS_NULL = "species labels are NULL"
MOMENTS_NULL = "moments output is NULL"
CROSS_NULL = "moments or cross output is NULL"
CROSS_SHAPE = "need 1 <= n_frames <= 2^30, 1 <= dim <= 3"
GROUP_ONS_NULL = "species labels or moments are NULL"
LABEL_NEG = "species label -1 of atom 0 is outside 0 ... n_species - 1"
LABEL_HI = "species label 2 of atom 2 is outside 0 ... n_species - 1"
S = 2

# every option key of ta_set_option with a value it accepts (its default) and, where the key validates, one it rejects
OPTIONS = [
    ("fft_nwg", 0, None), ("direct_nwg", 0, None), ("direct_f32", 0, None), ("direct_groups", 0, None),
    ("direct_chunk", 0, None), ("direct_mfma", 1, None), ("direct_mfma", 0, None), ("direct_mfma", 3, None),
    ("direct_mfma", 2, MFMA), ("direct_mfma", -1, MFMA), ("helfand_fft", 0, None), ("bp_block", 0, None),
    ("bp_spec_atoms", 0, None), ("lock_ahead", 1, None), ("cpu_threads", 2, None), ("cpu_threads", 0, None),
    ("cpu_threads", -1, "cpu_threads: 0 (default) .. 4096"), ("cpu_threads", 4097, "cpu_threads: 0 (default) .. 4096"),
    ("fail_alloc_after", 0, None), ("fail_throw_after", 0, None), ("bp_prefetch", 2, None), ("short_max", 64, None),
    ("direct_subwave", 1, None), ("mid_max", 512, None), ("mid_all", 0, None), ("mid_ncl", 0, None),
    ("short_lags_max", 48, None), ("stage_device_f32", 0, None), ("timeline", 0, None), ("async_commit", 1, None),
    ("async_commit", 0, None), ("nope", 1, "unknown option nope"), ("", 1, "unknown option "),
]


class Bufs:
    """Host arrays the rows point at: big enough for every call that is allowed to write (T x A x D staged)."""

    def __init__(self):
        self.ts = np.zeros(T)
        self.bp = np.zeros((T, A))
        self.m = np.ones(A)
        self.q = np.ones(A)
        self.mom = np.zeros((T, D))
        self.phi = np.zeros(T)
        self.slf = np.zeros(T)
        self.lab = np.array([0, 1, 0], dtype=np.int32)
        self.lab_neg = np.array([-1, 1, 0], dtype=np.int32)
        self.lab_hi = np.array([0, 1, S], dtype=np.int32)
        self.w = np.array([1.0, -0.5, 2.0])
        self.moms = np.zeros((S, T, D))
        self.cross = np.zeros((T, S, S))
        self.box = np.tile(np.array([10.0, 10.0, 10.0, 90.0, 90.0, 90.0]), (T, 1))
        self.badbox = np.tile(np.array([-1.0, 10.0, 10.0, 90.0, 90.0, 90.0]), (T, 1))
        self.tric = np.tile(np.array([10.0, 10.0, 10.0, 80.0, 90.0, 90.0]), (T, 1))
        self.axes = np.array([0, 1, 2], dtype=np.int32)
        self.axes2 = np.array([0, 1, 1], dtype=np.int32)
        self.badaxes = np.array([0, 1, 3], dtype=np.int32)
        self.src = np.zeros((A, D))
        self.f = (ctypes.c_float * 4)()
        self.i = ctypes.c_int(0)
        self.d3 = (ctypes.c_double * 3)()
        self.vp = ctypes.c_void_p()
        self.i64 = (ctypes.c_int64 * 2)()
        self.hs = (ctypes.c_void_p * 8)()
        self.names = (ctypes.c_char_p * 4)()
        # a made-up non-NULL "device pointer": only ever given to calls that are rejected before they queue anything
        self.fake = ctypes.c_void_p(self.ts.ctypes.data)

    def p(self, name):
        return ctypes.c_void_p(getattr(self, name).ctypes.data)


def _state(L, name):
    """-> (handle or None, closer).  Contexts: cpu / gpu, fresh or staged (host slabs, 2 of them, float64, T x A x D);
    gpu_dev: device-only slabs; gpu_f32dev: "stage_device_f32" device slabs.  Groups: two members on device 0."""
    if name in ("null", "gnull"):
        return None, lambda: None
    hs = (ctypes.c_void_p * 8)()
    if name.startswith("g_"):
        h = ctypes.c_void_p()
        assert L.ta_group_create((ctypes.c_int * 2)(0, 0), 2, ctypes.byref(h)) == 0
        if name == "g_staged":
            assert L.ta_group_stage_alloc(h, T, A, D, _lib.TA_F64, 2, hs) == 0
        return h, lambda: L.ta_group_destroy(h)
    h = ctypes.c_void_p()
    assert L.ta_ctx_create(_lib.DEVICE_CPU if name.startswith("cpu") else 0, ctypes.byref(h)) == 0
    if name.endswith("_staged"):
        assert L.ta_stage_alloc(h, T, A, D, _lib.TA_F64, 2, hs) == 0
    elif name.endswith("_staged1"):
        assert L.ta_stage_alloc(h, T, A, D, _lib.TA_F64, 1, hs) == 0
    elif name == "gpu_dev":
        assert L.ta_stage_alloc_device(h, T, A, D, 1) == 0
    elif name == "gpu_f32dev":
        assert L.ta_set_option(h, b"stage_device_f32", 1) == 0
        assert L.ta_stage_alloc_device(h, T, A, D, 1) == 0
    return h, lambda: L.ta_ctx_destroy(h)


BIG = (1 << 30) + 1
F64 = 1

# (id, state, call(L, h, B), status, message).  Context rows read ta_last_error(h), group rows ta_group_last_error(h);
# with a NULL handle both return the calling thread's last message.
CTX_ROWS = [
    # ---- creation, destruction, trim
    ("create-out-null", "null", lambda L, h, B: L.ta_ctx_create(-1, None), INVALID, "out is NULL"),
    ("destroy-null", "null", lambda L, h, B: L.ta_ctx_destroy(None), 0, None),
    ("trim-null", "null", lambda L, h, B: L.ta_trim(None), INVALID, NULL_CTX),
    ("trim-fresh", "*_fresh", lambda L, h, B: L.ta_trim(h), 0, None),
    ("trim-staged", "*_staged", lambda L, h, B: L.ta_trim(h), 0, None),
    ("stage_free-null", "null", lambda L, h, B: L.ta_stage_free(None), INVALID, NULL_CTX),
    ("stage_free-fresh", "*_fresh", lambda L, h, B: L.ta_stage_free(h), 0, None),
    ("plan_info-too-long", "null", lambda L, h, B: L.ta_fft_plan_info(10**9, None, None, None), UNSUPPORTED,
     "n_frames exceeds the largest FFT plan"),
    # ---- options (every key: OPTION_ROWS below)
    ("set_option-null-ctx", "null", lambda L, h, B: L.ta_set_option(None, b"fft_nwg", 1), INVALID, NULL_ARG),
    ("set_option-null-key", "*_fresh", lambda L, h, B: L.ta_set_option(h, None, 1), INVALID, NULL_ARG),
    ("set_option-null-ctx+unknown", "null", lambda L, h, B: L.ta_set_option(None, b"nope", 1), INVALID, NULL_ARG),
    # ---- ta_stage_alloc / ta_stage_alloc_device
    ("alloc-null-ctx", "null", lambda L, h, B: L.ta_stage_alloc(None, T, A, D, F64, 1, B.hs), INVALID, NULL_CTX),
    ("alloc-null-slabs", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, A, D, F64, 1, None), INVALID, "h_slabs is NULL"),
    ("alloc-null-slabs+null-ctx", "null", lambda L, h, B: L.ta_stage_alloc(None, T, A, D, F64, 1, None), INVALID,
     "h_slabs is NULL"),
    ("alloc-null-slabs+shape", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, 0, A, D, F64, 1, None), INVALID,
     "h_slabs is NULL"),
    ("alloc-frames-0", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, 0, A, D, F64, 1, B.hs), INVALID, SHAPE),
    ("alloc-atoms-0", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, 0, D, F64, 1, B.hs), INVALID, SHAPE),
    ("alloc-dim-0", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, A, 0, F64, 1, B.hs), INVALID, SHAPE),
    ("alloc-dim-4", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, A, 4, F64, 1, B.hs), INVALID, SHAPE),
    ("alloc-frames-too-many", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, BIG, 1, 1, F64, 1, B.hs), INVALID,
     "n_frames too large"),
    ("alloc-slabs-0", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, A, D, F64, 0, B.hs), INVALID, "bad slab count"),
    ("alloc-slabs-5", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, A, D, F64, 5, B.hs), INVALID, "bad slab count"),
    ("alloc-dtype", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, A, D, 7, 1, B.hs), INVALID, "bad dtype"),
    ("alloc-shape+slabs", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, 0, A, D, F64, 0, B.hs), INVALID, SHAPE),
    ("alloc-slabs+dtype", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, A, D, 7, 0, B.hs), INVALID, "bad slab count"),
    ("alloc-too-many+dtype", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, BIG, 1, 1, 7, 1, B.hs), INVALID,
     "n_frames too large"),
    ("alloc-good", "*_fresh", lambda L, h, B: L.ta_stage_alloc(h, T, A, D, F64, 2, B.hs), 0, None),
    ("alloc-good-f32-again", "*_staged", lambda L, h, B: L.ta_stage_alloc(h, 4, 2, 1, 0, 4, B.hs), 0, None),
    ("alloc_device-null-ctx", "null", lambda L, h, B: L.ta_stage_alloc_device(None, T, A, D, 1), INVALID, NULL_CTX),
    ("alloc_device-cpu", "cpu_fresh", lambda L, h, B: L.ta_stage_alloc_device(h, T, A, D, 1), UNSUPPORTED,
     "the CPU backend has no device slabs"),
    ("alloc_device-cpu-slabs+no-device-slabs", "cpu_fresh", lambda L, h, B: L.ta_stage_alloc_device(h, T, A, D, 0), INVALID,
     "bad slab count"),
    ("alloc_device-shape", "*_fresh", lambda L, h, B: L.ta_stage_alloc_device(h, T, A, 4, 1), INVALID, SHAPE),
    ("alloc_device-slabs", "gpu_fresh", lambda L, h, B: L.ta_stage_alloc_device(h, T, A, D, 5), INVALID, "bad slab count"),
    ("alloc_device-good", "gpu_fresh", lambda L, h, B: L.ta_stage_alloc_device(h, T, A, D, 2), 0, None),
    # ---- ta_stage_commit
    ("commit-null", "null", lambda L, h, B: L.ta_stage_commit(None, 0, 1), INVALID, NULL_CTX),
    ("commit-fresh", "*_fresh", lambda L, h, B: L.ta_stage_commit(h, 0, 1), STATE, "ta_stage_alloc has not been called"),
    ("commit-fresh+range", "*_fresh", lambda L, h, B: L.ta_stage_commit(h, -1, 1), STATE, "ta_stage_alloc has not been called"),
    ("commit-lo-negative", "*_staged", lambda L, h, B: L.ta_stage_commit(h, -1, 1), INVALID, RANGE),
    ("commit-hi-beyond", "*_staged", lambda L, h, B: L.ta_stage_commit(h, 0, T + 1), INVALID, RANGE),
    ("commit-lo-above-hi", "*_staged", lambda L, h, B: L.ta_stage_commit(h, 3, 2), INVALID, RANGE),
    ("commit-empty", "*_staged", lambda L, h, B: L.ta_stage_commit(h, 3, 3), 0, None),
    ("commit-good", "*_staged", lambda L, h, B: L.ta_stage_commit(h, 0, T), 0, None),
    ("commit-device-only", "gpu_dev", lambda L, h, B: L.ta_stage_commit(h, 0, 1), STATE,
     "device-only slabs: use ta_stage_commit_dev"),
    ("commit-device-only-empty", "gpu_dev", lambda L, h, B: L.ta_stage_commit(h, 1, 1), STATE,
     "device-only slabs: use ta_stage_commit_dev"),
    ("commit-range+device-only", "gpu_dev", lambda L, h, B: L.ta_stage_commit(h, 0, T + 1), INVALID, RANGE),
    # ---- ta_stage_frame
    ("frame-null", "null", lambda L, h, B: L.ta_stage_frame(None, 0, 0, B.p("src"), F64, D, 0, 1, D, 0, None, A), INVALID,
     NULL_CTX),
    ("frame-fresh", "*_fresh", lambda L, h, B: L.ta_stage_frame(h, 0, 0, B.p("src"), F64, D, 0, 1, D, 0, None, A), INVALID, NO_SLAB),
    ("frame-slab", "*_staged", lambda L, h, B: L.ta_stage_frame(h, 2, 0, B.p("src"), F64, D, 0, 1, D, 0, None, A), INVALID, NO_SLAB),
    ("frame-slab+src", "*_staged", lambda L, h, B: L.ta_stage_frame(h, -1, 0, None, F64, D, 0, 1, D, 0, None, A), INVALID, NO_SLAB),
    ("frame-device-only", "gpu_dev", lambda L, h, B: L.ta_stage_frame(h, 0, 0, B.p("src"), F64, D, 0, 1, D, 0, None, A), STATE,
     "device-only slabs have no host side to fill"),
    ("frame-src-null", "*_staged", lambda L, h, B: L.ta_stage_frame(h, 0, 0, None, F64, D, 0, 1, D, 0, None, A), INVALID,
     "h_src is NULL"),
    ("frame-dtype", "*_staged", lambda L, h, B: L.ta_stage_frame(h, 0, 0, B.p("src"), 7, D, 0, 1, D, 0, None, A), INVALID, "bad dtype"),
    ("frame-columns", "*_staged", lambda L, h, B: L.ta_stage_frame(h, 0, 0, B.p("src"), F64, D, 1, 1, D, 0, None, A), INVALID, COLUMNS),
    ("frame-dtype+frame", "*_staged", lambda L, h, B: L.ta_stage_frame(h, 0, T, B.p("src"), 7, D, 0, 1, D, 0, None, A), INVALID,
     "bad dtype"),
    ("frame-out-of-range", "*_staged", lambda L, h, B: L.ta_stage_frame(h, 0, T, B.p("src"), F64, D, 0, 1, D, 0, None, A), INVALID,
     "frame out of range"),
    ("frame-atoms", "*_staged", lambda L, h, B: L.ta_stage_frame(h, 0, 0, B.p("src"), F64, D, 0, 1, D, 0, None, A - 1), INVALID,
     "n_col / n_atoms do not match the staged slab"),
    ("frame-good", "*_staged", lambda L, h, B: L.ta_stage_frame(h, 1, T - 1, B.p("src"), F64, D, 0, 1, D, 0, None, A), 0, None),
    # ---- ta_stage_synth
    ("synth-null", "null", lambda L, h, B: L.ta_stage_synth(None, 0, 1, 0, A * D, None), INVALID, NULL_CTX),
    ("synth-fresh", "*_fresh", lambda L, h, B: L.ta_stage_synth(h, 0, 1, 0, A * D, None), INVALID, NO_SLAB),
    ("synth-slab", "*_staged", lambda L, h, B: L.ta_stage_synth(h, 2, 1, 0, A * D, None), INVALID, NO_SLAB),
    ("synth-slab-negative", "*_staged", lambda L, h, B: L.ta_stage_synth(h, -1, 1, 0, A * D, None), INVALID, NO_SLAB),
    ("synth-offset", "*_staged", lambda L, h, B: L.ta_stage_synth(h, 0, 1, -1, A * D, None), INVALID,
     "column block outside the synthetic tensor"),
    ("synth-total", "*_staged", lambda L, h, B: L.ta_stage_synth(h, 0, 1, 1, A * D, None), INVALID,
     "column block outside the synthetic tensor"),
    ("synth-slab+offset", "*_staged", lambda L, h, B: L.ta_stage_synth(h, 2, 1, -1, A * D, None), INVALID, NO_SLAB),
    ("synth-good", "*_staged", lambda L, h, B: L.ta_stage_synth(h, 1, 7, 2, A * D + 5, None), 0, None),
    # ---- the device-facing staging entries
    ("commit_dev-null", "null", lambda L, h, B: L.ta_stage_commit_dev(None, 0, B.fake, F64, A * D, 0, 1, None), INVALID, NULL_ARG),
    ("commit_dev-src-null", "*_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 0, None, F64, A * D, 0, 1, None), INVALID, NULL_ARG),
    ("commit_dev-cpu", "cpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 0, B.fake, F64, A * D, 0, 1, None), UNSUPPORTED, NO_CPU),
    ("commit_dev-cpu+slab", "cpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 9, B.fake, F64, A * D, 0, 1, None), UNSUPPORTED,
     NO_CPU),
    ("commit_dev-fresh", "gpu_fresh", lambda L, h, B: L.ta_stage_commit_dev(h, 0, B.fake, F64, A * D, 0, 1, None), INVALID, NO_SLAB),
    ("commit_dev-slab", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 2, B.fake, F64, A * D, 0, 1, None), INVALID, NO_SLAB),
    ("commit_dev-slab-negative", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, -1, B.fake, F64, A * D, 0, 1, None), INVALID,
     NO_SLAB),
    ("commit_dev-dtype", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 0, B.fake, 7, A * D, 0, 1, None), INVALID, "bad dtype"),
    ("commit_dev-range", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 0, B.fake, F64, A * D, 0, T + 1, None), INVALID, RANGE),
    ("commit_dev-range-lo", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 0, B.fake, F64, A * D, 2, 1, None), INVALID, RANGE),
    ("commit_dev-ld_row", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 0, B.fake, F64, A * D - 1, 0, 1, None), INVALID, LD_ROW),
    ("commit_dev-slab+dtype", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 2, B.fake, 7, A * D, 0, 1, None), INVALID, NO_SLAB),
    ("commit_dev-dtype+range", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 0, B.fake, 7, A * D, -1, 1, None), INVALID,
     "bad dtype"),
    ("commit_dev-range+ld_row", "gpu_staged", lambda L, h, B: L.ta_stage_commit_dev(h, 0, B.fake, F64, 1, -1, 1, None), INVALID, RANGE),
    ("read_dev-null", "null", lambda L, h, B: L.ta_stage_read_dev(None, 0, B.fake, A * D, None), INVALID, NULL_ARG),
    ("read_dev-dst-null", "*_staged", lambda L, h, B: L.ta_stage_read_dev(h, 0, None, A * D, None), INVALID, NULL_ARG),
    ("read_dev-cpu", "cpu_staged", lambda L, h, B: L.ta_stage_read_dev(h, 0, B.fake, A * D, None), UNSUPPORTED, NO_CPU),
    ("read_dev-slab", "gpu_staged", lambda L, h, B: L.ta_stage_read_dev(h, 2, B.fake, A * D, None), INVALID, NO_SLAB),
    ("read_dev-ld_row", "gpu_staged", lambda L, h, B: L.ta_stage_read_dev(h, 0, B.fake, A * D - 1, None), INVALID, LD_ROW),
    ("read_dev-slab+ld_row", "gpu_staged", lambda L, h, B: L.ta_stage_read_dev(h, 2, B.fake, 1, None), INVALID, NO_SLAB),
    ("stage_device-null", "null", lambda L, h, B: L.ta_stage_device(None, 0, ctypes.byref(B.vp), None, None), INVALID, NULL_ARG),
    ("stage_device-out-null", "*_staged", lambda L, h, B: L.ta_stage_device(h, 0, None, None, None), INVALID, NULL_ARG),
    ("stage_device-cpu", "cpu_staged", lambda L, h, B: L.ta_stage_device(h, 0, ctypes.byref(B.vp), None, None), UNSUPPORTED, NO_CPU),
    ("stage_device-slab", "gpu_staged", lambda L, h, B: L.ta_stage_device(h, 2, ctypes.byref(B.vp), None, None), INVALID, NO_SLAB),
    ("stage_device-fresh", "gpu_fresh", lambda L, h, B: L.ta_stage_device(h, 0, ctypes.byref(B.vp), None, None), INVALID, NO_SLAB),
    ("stage_device-good", "gpu_staged", lambda L, h, B: L.ta_stage_device(h, 1, ctypes.byref(B.vp), None, None), 0, None),
    # ---- timing
    ("last_timing-null", "null", lambda L, h, B: L.ta_last_timing(None, None, None), INVALID, NULL_CTX),
    ("last_timing-cpu", "cpu_staged", lambda L, h, B: L.ta_last_timing(h, None, None), UNSUPPORTED, NO_CPU),
    ("last_timing-fresh", "gpu_fresh", lambda L, h, B: L.ta_last_timing(h, None, None), STATE, "no completed compute call to time"),
    ("timing_history-null", "null", lambda L, h, B: L.ta_timing_history(None, 4, B.f, B.f, ctypes.byref(B.i)), INVALID, NULL_ARG),
    ("timing_history-n-null", "*_fresh", lambda L, h, B: L.ta_timing_history(h, 4, B.f, B.f, None), INVALID, NULL_ARG),
    ("timing_history-cpu", "cpu_fresh", lambda L, h, B: L.ta_timing_history(h, 4, B.f, B.f, ctypes.byref(B.i)), UNSUPPORTED, NO_CPU),
    ("timing_history-fresh", "gpu_fresh", lambda L, h, B: L.ta_timing_history(h, 4, B.f, B.f, ctypes.byref(B.i)), 0, None),
    ("timeline-null", "null", lambda L, h, B: L.ta_kernel_timeline(None, 4, B.names, B.f, ctypes.byref(B.i)), INVALID, NULL_ARG),
    ("timeline-n-null", "*_fresh", lambda L, h, B: L.ta_kernel_timeline(h, 4, B.names, B.f, None), INVALID, NULL_ARG),
    ("timeline-cpu", "cpu_fresh", lambda L, h, B: L.ta_kernel_timeline(h, 4, B.names, B.f, ctypes.byref(B.i)), UNSUPPORTED, NO_CPU),
    ("timeline-fresh", "gpu_fresh", lambda L, h, B: L.ta_kernel_timeline(h, 4, B.names, B.f, ctypes.byref(B.i)), 0, None),
    ("clock_probe-null", "null", lambda L, h, B: L.ta_clock_probe(None, 1, None, None, None), INVALID, NULL_CTX),
    ("clock_probe-cpu", "cpu_staged", lambda L, h, B: L.ta_clock_probe(h, 1, None, None, None), UNSUPPORTED, NO_CPU),
    ("clock_probe-fresh", "gpu_fresh", lambda L, h, B: L.ta_clock_probe(h, 1, None, None, None), STATE, NOT_STAGED),
    ("clock_probe-fresh+launches", "gpu_fresh", lambda L, h, B: L.ta_clock_probe(h, 0, None, None, None), STATE, NOT_STAGED),
    ("clock_probe-launches", "gpu_staged", lambda L, h, B: L.ta_clock_probe(h, 0, None, None, None), INVALID,
     "need at least one launch"),
    ("clock_probe-f32-slabs", "gpu_f32dev", lambda L, h, B: L.ta_clock_probe(h, 1, None, None, None), UNSUPPORTED,
     "clock probe: float64 device slabs only"),
    ("clock_probe-short-plan", "gpu_staged", lambda L, h, B: L.ta_clock_probe(h, 1, None, None, None), UNSUPPORTED,
     "clock probe: plans R0 = 8, 10, 12, 16, 20 without an outer radix only"),
    # ---- host-facing: ta_vacf_fft / ta_vacf_direct / ta_helfand_msd / ta_msd
    ("vacf_fft-null", "null", lambda L, h, B: L.ta_vacf_fft(None, B.p("ts"), None), INVALID, NULL_CTX),
    ("vacf_direct-null", "null", lambda L, h, B: L.ta_vacf_direct(None, B.p("ts"), None), INVALID, NULL_CTX),
    ("helfand-null", "null", lambda L, h, B: L.ta_helfand_msd(None, B.p("m"), 1.0, B.p("ts"), None), INVALID, NULL_CTX),
    ("msd-null", "null", lambda L, h, B: L.ta_msd(None, 1, B.p("ts"), None), INVALID, NULL_CTX),
    ("msd-fft+null", "null", lambda L, h, B: L.ta_msd(None, 2, B.p("ts"), None), INVALID, FFT_FLAG),
    ("vacf_fft-ts-null", "*_staged", lambda L, h, B: L.ta_vacf_fft(h, None, None), INVALID, "h_timeseries is NULL"),
    ("vacf_fft-ts-null+fresh", "*_fresh", lambda L, h, B: L.ta_vacf_fft(h, None, None), INVALID, "h_timeseries is NULL"),
    ("vacf_fft-fresh", "*_fresh", lambda L, h, B: L.ta_vacf_fft(h, B.p("ts"), None), STATE, NOT_STAGED),
    ("vacf_direct-fresh", "*_fresh", lambda L, h, B: L.ta_vacf_direct(h, B.p("ts"), B.p("bp")), STATE, NOT_STAGED),
    ("helfand-fresh", "*_fresh", lambda L, h, B: L.ta_helfand_msd(h, B.p("m"), 1.0, B.p("ts"), None), STATE, NOT_STAGED),
    ("helfand-one-slab", "*_staged1", lambda L, h, B: L.ta_helfand_msd(h, B.p("m"), 1.0, B.p("ts"), None), STATE, NOT_STAGED),
    ("helfand-one-slab+masses", "*_staged1", lambda L, h, B: L.ta_helfand_msd(h, None, 1.0, B.p("ts"), None), STATE, NOT_STAGED),
    ("helfand-masses-null", "*_staged", lambda L, h, B: L.ta_helfand_msd(h, None, 1.0, B.p("ts"), None), INVALID, "h_masses is NULL"),
    ("msd-fresh", "*_fresh", lambda L, h, B: L.ta_msd(h, 0, B.p("ts"), None), STATE, NOT_STAGED),
    ("msd-fft", "*_staged", lambda L, h, B: L.ta_msd(h, 2, B.p("ts"), None), INVALID, FFT_FLAG),
    ("msd-fft-negative", "*_staged", lambda L, h, B: L.ta_msd(h, -1, B.p("ts"), None), INVALID, FFT_FLAG),
    ("msd-fft+ts-null+fresh", "*_fresh", lambda L, h, B: L.ta_msd(h, 2, None, None), INVALID, FFT_FLAG),
    ("vacf_fft-good", "*_staged", lambda L, h, B: L.ta_vacf_fft(h, B.p("ts"), B.p("bp")), 0, None),
    ("vacf_direct-good", "*_staged", lambda L, h, B: L.ta_vacf_direct(h, B.p("ts"), None), 0, None),
    ("helfand-good", "*_staged", lambda L, h, B: L.ta_helfand_msd(h, B.p("m"), 2.0, B.p("ts"), B.p("bp")), 0, None),
    ("msd-good", "*_staged1", lambda L, h, B: L.ta_msd(h, 1, B.p("ts"), B.p("bp")), 0, None),
    # ---- host-facing: ta_conductivity
    ("cond-null", "null", lambda L, h, B: L.ta_conductivity(None, 1, B.p("q"), B.p("mom"), None, None), INVALID, NULL_CTX),
    ("cond-null+fft", "null", lambda L, h, B: L.ta_conductivity(None, 2, B.p("q"), B.p("mom"), None, None), INVALID, NULL_CTX),
    ("cond-fft", "*_staged", lambda L, h, B: L.ta_conductivity(h, 2, B.p("q"), B.p("mom"), None, None), INVALID, FFT_FLAG),
    ("cond-charges", "*_staged", lambda L, h, B: L.ta_conductivity(h, 0, None, B.p("mom"), None, None), INVALID, "charges are NULL"),
    ("cond-moment", "*_staged", lambda L, h, B: L.ta_conductivity(h, 0, B.p("q"), None, None, None), INVALID, "moment output is NULL"),
    ("cond-fft+charges", "*_staged", lambda L, h, B: L.ta_conductivity(h, 2, None, B.p("mom"), None, None), INVALID, FFT_FLAG),
    ("cond-charges+moment", "*_staged", lambda L, h, B: L.ta_conductivity(h, 1, None, None, None, None), INVALID, "charges are NULL"),
    ("cond-fresh", "*_fresh", lambda L, h, B: L.ta_conductivity(h, 1, B.p("q"), B.p("mom"), None, None), STATE, NOT_STAGED),
    ("cond-fft+fresh", "*_fresh", lambda L, h, B: L.ta_conductivity(h, 2, B.p("q"), B.p("mom"), None, None), INVALID, FFT_FLAG),
    ("cond-moment+fresh", "*_fresh", lambda L, h, B: L.ta_conductivity(h, 1, B.p("q"), None, None, None), INVALID,
     "moment output is NULL"),
    ("cond-good", "*_staged", lambda L, h, B: L.ta_conductivity(h, 1, B.p("q"), B.p("mom"), B.p("phi"), B.p("slf")), 0, None),
    ("cond-good-moment-only", "*_staged1", lambda L, h, B: L.ta_conductivity(h, 0, B.p("q"), B.p("mom"), None, None), 0, None),
    # ---- host-facing: ta_onsager (the rows of ta_conductivity, the species count and the labels' range)
    ("ons-null", "null", lambda L, h, B: L.ta_onsager(None, 1, S, B.p("lab"), None, B.p("moms"), None), INVALID, NULL_CTX),
    ("ons-null+fft", "null", lambda L, h, B: L.ta_onsager(None, 2, S, B.p("lab"), None, B.p("moms"), None), INVALID, NULL_CTX),
    ("ons-fft", "*_staged", lambda L, h, B: L.ta_onsager(h, 2, S, B.p("lab"), None, B.p("moms"), None), INVALID, FFT_FLAG),
    ("ons-species-0", "*_staged", lambda L, h, B: L.ta_onsager(h, 0, 0, B.p("lab"), None, B.p("moms"), None), INVALID, SPECIES),
    ("ons-species-9", "*_staged", lambda L, h, B: L.ta_onsager(h, 0, 9, B.p("lab"), None, B.p("moms"), None), INVALID, SPECIES),
    ("ons-labels", "*_staged", lambda L, h, B: L.ta_onsager(h, 0, S, None, None, B.p("moms"), None), INVALID, LABELS_NULL),
    ("ons-moments", "*_staged", lambda L, h, B: L.ta_onsager(h, 0, S, B.p("lab"), None, None, None), INVALID, MOMENTS_NULL),
    ("ons-fft+species-count", "*_staged", lambda L, h, B: L.ta_onsager(h, 2, 0, B.p("lab"), None, B.p("moms"), None), INVALID, FFT_FLAG),
    ("ons-fft+labels", "*_staged", lambda L, h, B: L.ta_onsager(h, 2, S, None, None, B.p("moms"), None), INVALID, FFT_FLAG),
    ("ons-species-count+labels", "*_staged", lambda L, h, B: L.ta_onsager(h, 1, 9, None, None, B.p("moms"), None), INVALID, SPECIES),
    ("ons-labels+moments", "*_staged", lambda L, h, B: L.ta_onsager(h, 1, S, None, None, None, None), INVALID, LABELS_NULL),
    ("ons-fresh", "*_fresh", lambda L, h, B: L.ta_onsager(h, 1, S, B.p("lab"), None, B.p("moms"), None), STATE, NOT_STAGED),
    ("ons-fft+fresh", "*_fresh", lambda L, h, B: L.ta_onsager(h, 2, S, B.p("lab"), None, B.p("moms"), None), INVALID, FFT_FLAG),
    ("ons-moments+fresh", "*_fresh", lambda L, h, B: L.ta_onsager(h, 1, S, B.p("lab"), None, None, None), INVALID, MOMENTS_NULL),
    ("ons-label-negative", "*_staged", lambda L, h, B: L.ta_onsager(h, 1, S, B.p("lab_neg"), None, B.p("moms"), None), INVALID, LABEL_NEG),
    ("ons-label-n_species", "*_staged", lambda L, h, B: L.ta_onsager(h, 1, S, B.p("lab_hi"), None, B.p("moms"), None), INVALID, LABEL_HI),
    ("ons-moments+label", "*_staged", lambda L, h, B: L.ta_onsager(h, 1, S, B.p("lab_neg"), None, None, None), INVALID, MOMENTS_NULL),
    ("ons-good", "*_staged", lambda L, h, B: L.ta_onsager(h, 1, S, B.p("lab"), B.p("w"), B.p("moms"), B.p("cross")), 0, None),
    ("ons-good-moments-only", "*_staged1", lambda L, h, B: L.ta_onsager(h, 0, S, B.p("lab"), None, B.p("moms"), None), 0, None),
    # ---- host-facing: ta_onsager_cross (needs no slab)
    ("ons_cross-null", "null", lambda L, h, B: L.ta_onsager_cross(None, 1, B.p("moms"), S, T, D, B.p("cross")), INVALID, NULL_CTX),
    ("ons_cross-null+fft", "null", lambda L, h, B: L.ta_onsager_cross(None, 2, B.p("moms"), S, T, D, B.p("cross")), INVALID, NULL_CTX),
    ("ons_cross-fft", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 2, B.p("moms"), S, T, D, B.p("cross")), INVALID, FFT_FLAG),
    ("ons_cross-species-0", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), 0, T, D, B.p("cross")), INVALID, SPECIES),
    ("ons_cross-species-9", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), 9, T, D, B.p("cross")), INVALID, SPECIES),
    ("ons_cross-moments-null", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, None, S, T, D, B.p("cross")), INVALID, CROSS_NULL),
    ("ons_cross-cross-null", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), S, T, D, None), INVALID, CROSS_NULL),
    ("ons_cross-frames-0", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), S, 0, D, B.p("cross")), INVALID, CROSS_SHAPE),
    ("ons_cross-dim-4", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), S, T, 4, B.p("cross")), INVALID, CROSS_SHAPE),
    ("ons_cross-dim-0", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), S, T, 0, B.p("cross")), INVALID, CROSS_SHAPE),
    ("ons_cross-frames-too-many", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), S, BIG, D, B.p("cross")), INVALID,
     CROSS_SHAPE),
    ("ons_cross-fft+species-count", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 2, B.p("moms"), 0, T, D, B.p("cross")), INVALID,
     FFT_FLAG),
    ("ons_cross-species-count+null-arrays", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, None, 9, T, D, None), INVALID, SPECIES),
    ("ons_cross-null-arrays+frames", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, None, S, 0, D, None), INVALID, CROSS_NULL),
    ("ons_cross-good", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), S, T, D, B.p("cross")), 0, None),
    ("ons_cross-good-direct-staged", "*_staged", lambda L, h, B: L.ta_onsager_cross(h, 0, B.p("moms"), S, T, D, B.p("cross")), 0, None),
    ("ons_cross-good-one-frame", "*_fresh", lambda L, h, B: L.ta_onsager_cross(h, 1, B.p("moms"), S, 1, D, B.p("cross")), 0, None),
    # ---- host-facing: ta_unwrap
    ("unwrap-null", "null", lambda L, h, B: L.ta_unwrap(None, 0, B.p("box"), B.p("axes")), INVALID, NULL_CTX),
    ("unwrap-dims-null", "*_staged", lambda L, h, B: L.ta_unwrap(h, 0, None, B.p("axes")), INVALID, "dimensions or axes are NULL"),
    ("unwrap-axes-null", "*_staged", lambda L, h, B: L.ta_unwrap(h, 0, B.p("box"), None), INVALID, "dimensions or axes are NULL"),
    ("unwrap-dims-null+fresh", "*_fresh", lambda L, h, B: L.ta_unwrap(h, 0, None, None), INVALID, "dimensions or axes are NULL"),
    ("unwrap-fresh", "*_fresh", lambda L, h, B: L.ta_unwrap(h, 0, B.p("box"), B.p("axes")), STATE, NOT_STAGED),
    ("unwrap-fresh+slab", "*_fresh", lambda L, h, B: L.ta_unwrap(h, -1, B.p("box"), B.p("axes")), STATE, NOT_STAGED),
    ("unwrap-slab", "*_staged", lambda L, h, B: L.ta_unwrap(h, 2, B.p("box"), B.p("axes")), INVALID, NO_SLAB),
    ("unwrap-slab-negative", "*_staged", lambda L, h, B: L.ta_unwrap(h, -1, B.p("box"), B.p("axes")), INVALID, NO_SLAB),
    ("unwrap-slab+box", "*_staged", lambda L, h, B: L.ta_unwrap(h, 2, B.p("badbox"), B.p("axes")), INVALID, NO_SLAB),
    ("unwrap-box", "*_staged", lambda L, h, B: L.ta_unwrap(h, 0, B.p("badbox"), B.p("axes")), INVALID,
     "unwrap: box length <= 0 or not finite in frame 0"),
    ("unwrap-axes", "*_staged", lambda L, h, B: L.ta_unwrap(h, 0, B.p("box"), B.p("badaxes")), INVALID,
     "unwrap: axes: every entry must be 0, 1 or 2"),
    ("unwrap-triclinic-axes", "*_staged", lambda L, h, B: L.ta_unwrap(h, 0, B.p("tric"), B.p("axes2")), INVALID,
     "unwrap: a non-orthogonal box needs the three columns x, y, z (axes {0, 1, 2})"),
    ("unwrap-f32-slabs", "gpu_f32dev", lambda L, h, B: L.ta_unwrap(h, 0, B.p("box"), B.p("axes")), UNSUPPORTED,
     "unwrap: float64 device slabs only (stage_device_f32 is on)"),
    ("unwrap-good", "*_staged", lambda L, h, B: L.ta_unwrap(h, 1, B.p("box"), B.p("axes")), 0, None),
    # ---- device-facing compute: *_dev
    ("vacf_fft_dev-null", "null", lambda L, h, B: L.ta_vacf_fft_dev(None, B.fake, T, A, D, A * D, B.fake, None, 0, None), INVALID,
     NULL_CTX),
    ("vacf_fft_dev-cpu", "cpu_staged", lambda L, h, B: L.ta_vacf_fft_dev(h, B.fake, T, A, D, A * D, B.fake, None, 0, None), UNSUPPORTED,
     NO_CPU),
    ("vacf_direct_dev-cpu", "cpu_staged", lambda L, h, B: L.ta_vacf_direct_dev(h, B.fake, T, A, D, A * D, B.fake, None, 0, None),
     UNSUPPORTED, NO_CPU),
    ("helfand_dev-cpu", "cpu_staged",
     lambda L, h, B: L.ta_helfand_msd_dev(h, B.fake, B.fake, B.fake, T, A, D, A * D, 1.0, B.fake, None, 0, None), UNSUPPORTED, NO_CPU),
    ("msd_dev-cpu", "cpu_staged", lambda L, h, B: L.ta_msd_dev(h, B.fake, T, A, D, A * D, 1, B.fake, None, 0, None), UNSUPPORTED, NO_CPU),
    ("msd_dev-fft+cpu", "cpu_staged", lambda L, h, B: L.ta_msd_dev(h, B.fake, T, A, D, A * D, 2, B.fake, None, 0, None), INVALID,
     FFT_FLAG),
    ("cond_dev-cpu", "cpu_staged", lambda L, h, B: L.ta_conductivity_dev(h, B.fake, T, A, D, A * D, 1, B.fake, B.fake, None, None, None),
     UNSUPPORTED, NO_CPU),
    ("cond_dev-cpu+fft", "cpu_staged", lambda L, h, B: L.ta_conductivity_dev(h, B.fake, T, A, D, A * D, 2, B.fake, B.fake, None, None, None),
     UNSUPPORTED, NO_CPU),
    ("ons_dev-cpu", "cpu_staged", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 1, S, B.fake, None, B.fake, None, None),
     UNSUPPORTED, NO_CPU),
    ("ons_dev-cpu+fft", "cpu_staged", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 2, S, B.fake, None, B.fake, None, None),
     UNSUPPORTED, NO_CPU),
    ("vacf_fft_dev-cpu+shape", "cpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, B.fake, 0, A, D, A * D, B.fake, None, 0, None),
     UNSUPPORTED, NO_CPU),
    ("vacf_fft_dev-shape", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, B.fake, 0, A, D, A * D, B.fake, None, 0, None), INVALID, SHAPE),
    ("vacf_fft_dev-ld_row", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, B.fake, T, A, D, A * D - 1, B.fake, None, 0, None), INVALID,
     LD_ROW),
    ("vacf_fft_dev-shape+ld_row", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, B.fake, T, A, 4, 1, B.fake, None, 0, None), INVALID,
     SHAPE),
    ("vacf_fft_dev-ld_row+too-many", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, B.fake, BIG, A, D, 1, B.fake, None, 0, None),
     INVALID, LD_ROW),
    ("vacf_fft_dev-too-many", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, B.fake, BIG, A, D, A * D, B.fake, None, 0, None), INVALID,
     "n_frames too large"),
    ("vacf_fft_dev-vel-null", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, None, T, A, D, A * D, B.fake, None, 0, None), INVALID,
     NULL_DEV),
    ("vacf_direct_dev-lagsum-null", "gpu_fresh", lambda L, h, B: L.ta_vacf_direct_dev(h, B.fake, T, A, D, A * D, None, None, 0, None),
     INVALID, NULL_DEV),
    ("helfand_dev-pos-null", "gpu_fresh",
     lambda L, h, B: L.ta_helfand_msd_dev(h, B.fake, None, B.fake, T, A, D, A * D, 1.0, B.fake, None, 0, None), INVALID, NULL_DEV),
    ("helfand_dev-masses-null", "gpu_fresh",
     lambda L, h, B: L.ta_helfand_msd_dev(h, B.fake, B.fake, None, T, A, D, A * D, 1.0, B.fake, None, 0, None), INVALID, NULL_DEV),
    ("vacf_fft_dev-ld_bp", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, B.fake, T, A, D, A * D, B.fake, B.fake, A - 1, None), INVALID,
     LD_BP),
    ("vacf_fft_dev-null-pointer+ld_bp", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_dev(h, None, T, A, D, A * D, B.fake, B.fake, 0, None),
     INVALID, NULL_DEV),
    ("msd_dev-fft", "gpu_fresh", lambda L, h, B: L.ta_msd_dev(h, B.fake, T, A, D, A * D, 2, B.fake, None, 0, None), INVALID, FFT_FLAG),
    ("msd_dev-fft+shape", "gpu_fresh", lambda L, h, B: L.ta_msd_dev(h, B.fake, 0, A, D, A * D, 2, B.fake, None, 0, None), INVALID, FFT_FLAG),
    ("msd_dev-fft+null", "null", lambda L, h, B: L.ta_msd_dev(None, B.fake, T, A, D, A * D, 2, B.fake, None, 0, None), INVALID, FFT_FLAG),
    ("msd_dev-ld_row", "gpu_fresh", lambda L, h, B: L.ta_msd_dev(h, B.fake, T, A, D, 1, 0, B.fake, None, 0, None), INVALID, LD_ROW),
    ("cond_dev-null", "null", lambda L, h, B: L.ta_conductivity_dev(None, B.fake, T, A, D, A * D, 1, B.fake, B.fake, None, None, None),
     INVALID, NULL_CTX),
    ("cond_dev-shape", "gpu_fresh", lambda L, h, B: L.ta_conductivity_dev(h, B.fake, T, 0, D, A * D, 1, B.fake, B.fake, None, None, None),
     INVALID, SHAPE),
    ("cond_dev-ld_row", "gpu_fresh", lambda L, h, B: L.ta_conductivity_dev(h, B.fake, T, A, D, 1, 1, B.fake, B.fake, None, None, None),
     INVALID, LD_ROW),
    ("cond_dev-shape+fft", "gpu_fresh", lambda L, h, B: L.ta_conductivity_dev(h, B.fake, T, 0, D, A * D, 2, B.fake, B.fake, None, None, None),
     INVALID, SHAPE),
    ("cond_dev-fft", "gpu_fresh", lambda L, h, B: L.ta_conductivity_dev(h, B.fake, T, A, D, A * D, 2, B.fake, B.fake, None, None, None),
     INVALID, FFT_FLAG),
    ("cond_dev-charges", "gpu_fresh", lambda L, h, B: L.ta_conductivity_dev(h, B.fake, T, A, D, A * D, 1, None, B.fake, None, None, None),
     INVALID, "charges are NULL"),
    ("cond_dev-moment", "gpu_fresh", lambda L, h, B: L.ta_conductivity_dev(h, B.fake, T, A, D, A * D, 1, B.fake, None, None, None, None),
     INVALID, "moment output is NULL"),
    ("cond_dev-pos-null", "gpu_fresh", lambda L, h, B: L.ta_conductivity_dev(h, None, T, A, D, A * D, 1, B.fake, B.fake, None, None, None),
     INVALID, NULL_DEV),
    ("cond_dev-charges+pos-null", "gpu_fresh",
     lambda L, h, B: L.ta_conductivity_dev(h, None, T, A, D, A * D, 1, None, B.fake, None, None, None), INVALID, "charges are NULL"),
    ("ons_dev-null", "null", lambda L, h, B: L.ta_onsager_dev(None, B.fake, T, A, D, A * D, 1, S, B.fake, None, B.fake, None, None),
     INVALID, NULL_CTX),
    ("ons_dev-shape", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, 0, D, A * D, 1, S, B.fake, None, B.fake, None, None),
     INVALID, SHAPE),
    ("ons_dev-ld_row", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, 1, 1, S, B.fake, None, B.fake, None, None),
     INVALID, LD_ROW),
    ("ons_dev-shape+fft", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, 0, D, A * D, 2, S, B.fake, None, B.fake, None, None),
     INVALID, SHAPE),
    ("ons_dev-ld_row+species-count", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, 1, 1, 0, B.fake, None, B.fake, None, None),
     INVALID, LD_ROW),
    ("ons_dev-fft", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 2, S, B.fake, None, B.fake, None, None),
     INVALID, FFT_FLAG),
    ("ons_dev-species-0", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 1, 0, B.fake, None, B.fake, None, None),
     INVALID, SPECIES),
    ("ons_dev-species-9", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 1, 9, B.fake, None, B.fake, None, None),
     INVALID, SPECIES),
    ("ons_dev-fft+species-count", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 2, 9, B.fake, None, B.fake, None, None),
     INVALID, FFT_FLAG),
    ("ons_dev-labels", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 1, S, None, None, B.fake, None, None),
     INVALID, LABELS_NULL),
    ("ons_dev-moments", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 1, S, B.fake, None, None, None, None),
     INVALID, MOMENTS_NULL),
    ("ons_dev-species-count+labels", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 1, 0, None, None, B.fake, None, None),
     INVALID, SPECIES),
    ("ons_dev-labels+moments", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, B.fake, T, A, D, A * D, 1, S, None, None, None, None, None),
     INVALID, LABELS_NULL),
    ("ons_dev-pos-null", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, None, T, A, D, A * D, 1, S, B.fake, None, B.fake, None, None),
     INVALID, NULL_DEV),
    ("ons_dev-labels+pos-null", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, None, T, A, D, A * D, 1, S, None, None, B.fake, None, None),
     INVALID, LABELS_NULL),
    ("ons_dev-moments+pos-null", "gpu_fresh", lambda L, h, B: L.ta_onsager_dev(h, None, T, A, D, A * D, 1, S, B.fake, None, None, None, None),
     INVALID, MOMENTS_NULL),
    # ---- device-facing compute: *_staged
    ("vacf_fft_staged-null", "null", lambda L, h, B: L.ta_vacf_fft_staged(None, B.fake, None, 0, None), INVALID, NULL_CTX),
    ("vacf_fft_staged-cpu", "cpu_staged", lambda L, h, B: L.ta_vacf_fft_staged(h, B.fake, None, 0, None), UNSUPPORTED, NO_CPU),
    ("vacf_direct_staged-cpu", "cpu_staged", lambda L, h, B: L.ta_vacf_direct_staged(h, B.fake, None, 0, None), UNSUPPORTED, NO_CPU),
    ("helfand_staged-cpu", "cpu_staged", lambda L, h, B: L.ta_helfand_msd_staged(h, B.fake, 1.0, B.fake, None, 0, None), UNSUPPORTED,
     NO_CPU),
    ("msd_staged-cpu", "cpu_staged", lambda L, h, B: L.ta_msd_staged(h, 1, B.fake, None, 0, None), UNSUPPORTED, NO_CPU),
    ("msd_staged-fft+cpu", "cpu_staged", lambda L, h, B: L.ta_msd_staged(h, 2, B.fake, None, 0, None), INVALID, FFT_FLAG),
    ("cond_staged-cpu", "cpu_staged", lambda L, h, B: L.ta_conductivity_staged(h, 1, B.fake, B.fake, None, None, None), UNSUPPORTED,
     NO_CPU),
    ("cond_staged-cpu+fft", "cpu_fresh", lambda L, h, B: L.ta_conductivity_staged(h, 2, None, None, None, None, None), UNSUPPORTED,
     NO_CPU),
    ("ons_staged-cpu", "cpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 1, S, B.fake, None, B.fake, None, None), UNSUPPORTED, NO_CPU),
    ("ons_staged-cpu+fft", "cpu_fresh", lambda L, h, B: L.ta_onsager_staged(h, 2, 0, None, None, None, None, None), UNSUPPORTED, NO_CPU),
    ("vacf_fft_staged-cpu+fresh", "cpu_fresh", lambda L, h, B: L.ta_vacf_fft_staged(h, None, None, 0, None), UNSUPPORTED, NO_CPU),
    ("vacf_fft_staged-fresh", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_staged(h, B.fake, None, 0, None), STATE, NOT_STAGED),
    ("vacf_fft_staged-fresh+null-pointer", "gpu_fresh", lambda L, h, B: L.ta_vacf_fft_staged(h, None, None, 0, None), STATE, NOT_STAGED),
    ("helfand_staged-one-slab", "gpu_staged1", lambda L, h, B: L.ta_helfand_msd_staged(h, B.fake, 1.0, B.fake, None, 0, None), STATE,
     NOT_STAGED),
    ("vacf_direct_staged-lagsum-null", "gpu_staged", lambda L, h, B: L.ta_vacf_direct_staged(h, None, None, 0, None), INVALID, NULL_DEV),
    ("helfand_staged-masses-null", "gpu_staged", lambda L, h, B: L.ta_helfand_msd_staged(h, None, 1.0, B.fake, None, 0, None), INVALID,
     NULL_DEV),
    ("vacf_fft_staged-ld_bp", "gpu_staged", lambda L, h, B: L.ta_vacf_fft_staged(h, B.fake, B.fake, A - 1, None), INVALID, LD_BP),
    ("vacf_fft_staged-null-pointer+ld_bp", "gpu_staged", lambda L, h, B: L.ta_vacf_fft_staged(h, None, B.fake, 0, None), INVALID, NULL_DEV),
    ("msd_staged-fft", "gpu_staged", lambda L, h, B: L.ta_msd_staged(h, 2, B.fake, None, 0, None), INVALID, FFT_FLAG),
    ("msd_staged-fft+fresh", "gpu_fresh", lambda L, h, B: L.ta_msd_staged(h, 2, B.fake, None, 0, None), INVALID, FFT_FLAG),
    ("msd_staged-fft+null", "null", lambda L, h, B: L.ta_msd_staged(None, 2, B.fake, None, 0, None), INVALID, FFT_FLAG),
    ("msd_staged-fresh", "gpu_fresh", lambda L, h, B: L.ta_msd_staged(h, 0, B.fake, None, 0, None), STATE, NOT_STAGED),
    ("cond_staged-null", "null", lambda L, h, B: L.ta_conductivity_staged(None, 1, B.fake, B.fake, None, None, None), INVALID, NULL_CTX),
    ("cond_staged-fft", "gpu_staged", lambda L, h, B: L.ta_conductivity_staged(h, 2, B.fake, B.fake, None, None, None), INVALID, FFT_FLAG),
    ("cond_staged-charges", "gpu_staged", lambda L, h, B: L.ta_conductivity_staged(h, 1, None, B.fake, None, None, None), INVALID,
     "charges are NULL"),
    ("cond_staged-moment", "gpu_staged", lambda L, h, B: L.ta_conductivity_staged(h, 1, B.fake, None, None, None, None), INVALID,
     "moment output is NULL"),
    ("cond_staged-fresh", "gpu_fresh", lambda L, h, B: L.ta_conductivity_staged(h, 1, B.fake, B.fake, None, None, None), STATE, NOT_STAGED),
    ("cond_staged-charges+fresh", "gpu_fresh", lambda L, h, B: L.ta_conductivity_staged(h, 1, None, B.fake, None, None, None), INVALID,
     "charges are NULL"),
    ("ons_staged-null", "null", lambda L, h, B: L.ta_onsager_staged(None, 1, S, B.fake, None, B.fake, None, None), INVALID, NULL_CTX),
    ("ons_staged-fft", "gpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 2, S, B.fake, None, B.fake, None, None), INVALID, FFT_FLAG),
    ("ons_staged-species-0", "gpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 1, 0, B.fake, None, B.fake, None, None), INVALID, SPECIES),
    ("ons_staged-species-9", "gpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 1, 9, B.fake, None, B.fake, None, None), INVALID, SPECIES),
    ("ons_staged-fft+species-count", "gpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 2, 0, B.fake, None, B.fake, None, None), INVALID, FFT_FLAG),
    ("ons_staged-labels", "gpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 1, S, None, None, B.fake, None, None), INVALID, LABELS_NULL),
    ("ons_staged-moments", "gpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 1, S, B.fake, None, None, None, None), INVALID, MOMENTS_NULL),
    ("ons_staged-species-count+labels", "gpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 1, 9, None, None, B.fake, None, None), INVALID, SPECIES),
    ("ons_staged-labels+moments", "gpu_staged", lambda L, h, B: L.ta_onsager_staged(h, 1, S, None, None, None, None, None), INVALID, LABELS_NULL),
    ("ons_staged-fresh", "gpu_fresh", lambda L, h, B: L.ta_onsager_staged(h, 1, S, B.fake, None, B.fake, None, None), STATE, NOT_STAGED),
    ("ons_staged-labels+fresh", "gpu_fresh", lambda L, h, B: L.ta_onsager_staged(h, 1, S, None, None, B.fake, None, None), INVALID, LABELS_NULL),
    ("ons_staged-species-count+fresh", "gpu_fresh", lambda L, h, B: L.ta_onsager_staged(h, 1, 0, B.fake, None, B.fake, None, None), INVALID, SPECIES),
]

GROUP_ROWS = [
    # ---- no group needed
    ("create-out-null", "gnull", lambda L, g, B: L.ta_group_create((ctypes.c_int * 1)(0), 1, None), INVALID, "out is NULL"),
    ("create-ids-null", "gnull", lambda L, g, B: L.ta_group_create(None, 1, ctypes.byref(B.vp)), INVALID, "need 1..64 device ids"),
    ("create-none", "gnull", lambda L, g, B: L.ta_group_create((ctypes.c_int * 1)(0), 0, ctypes.byref(B.vp)), INVALID,
     "need 1..64 device ids"),
    ("create-65", "gnull", lambda L, g, B: L.ta_group_create((ctypes.c_int * 65)(), 65, ctypes.byref(B.vp)), INVALID,
     "need 1..64 device ids"),
    ("create-cpu-member", "gnull", lambda L, g, B: L.ta_group_create((ctypes.c_int * 2)(0, -1), 2, ctypes.byref(B.vp)), UNSUPPORTED,
     "device groups are made of GPU contexts (TA_DEVICE_CPU is a context of its own)"),
    ("destroy-null", "gnull", lambda L, g, B: L.ta_group_destroy(None), 0, None),
    ("member-null", "gnull", lambda L, g, B: L.ta_group_member(None, 0, None, None), INVALID, "no such member"),
    ("shard-null", "gnull", lambda L, g, B: L.ta_group_shard(None, 10, 0, B.i64, B.i64), INVALID, "bad argument"),
    ("set_option-null", "gnull", lambda L, g, B: L.ta_group_set_option(None, b"reduce_mode", 1), INVALID, NULL_ARG),
    ("alloc-null", "gnull", lambda L, g, B: L.ta_group_stage_alloc(None, T, A, D, F64, 1, B.hs), INVALID, NULL_GROUP),
    ("alloc-null+slabs-null", "gnull", lambda L, g, B: L.ta_group_stage_alloc(None, T, A, D, F64, 1, None), INVALID, NULL_GROUP),
    ("alloc_device-null", "gnull", lambda L, g, B: L.ta_group_stage_alloc_device(None, T, A, D, 1), INVALID, NULL_GROUP),
    ("synth-null", "gnull", lambda L, g, B: L.ta_group_stage_synth(None, 0, 1, 0, A * D), INVALID, NULL_GROUP),
    ("commit-null", "gnull", lambda L, g, B: L.ta_group_stage_commit(None, 0, 1), INVALID, NULL_GROUP),
    ("stage_free-null", "gnull", lambda L, g, B: L.ta_group_stage_free(None), INVALID, NULL_GROUP),
    ("vacf_fft-null", "gnull", lambda L, g, B: L.ta_group_vacf_fft(None, B.p("ts"), None), INVALID, NULL_GROUP),
    ("vacf_direct-null", "gnull", lambda L, g, B: L.ta_group_vacf_direct(None, B.p("ts"), None), INVALID, NULL_GROUP),
    ("helfand-null", "gnull", lambda L, g, B: L.ta_group_helfand_msd(None, B.p("m"), 1.0, B.p("ts"), None), INVALID, NULL_GROUP),
    ("msd-null", "gnull", lambda L, g, B: L.ta_group_msd(None, 1, B.p("ts"), None), INVALID, NULL_GROUP),
    ("msd-fft+null", "gnull", lambda L, g, B: L.ta_group_msd(None, 2, B.p("ts"), None), INVALID, FFT_FLAG),
    ("cond-null", "gnull", lambda L, g, B: L.ta_group_conductivity(None, 2, None, None, None, None), INVALID, NULL_GROUP),
    ("ons-null", "gnull", lambda L, g, B: L.ta_group_onsager(None, 2, 0, None, None, None, None), INVALID, NULL_GROUP),
    ("unwrap-null", "gnull", lambda L, g, B: L.ta_group_unwrap(None, 0, None, None), INVALID, NULL_GROUP),
    # ---- options
    ("set_option-key-null", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, None, 1), INVALID, NULL_ARG),
    ("set_option-reduce_mode-3", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, b"reduce_mode", 3), INVALID,
     "reduce_mode: 0 auto, 1 peer copies, 2 RCCL"),
    ("set_option-reduce_mode-negative", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, b"reduce_mode", -1), INVALID,
     "reduce_mode: 0 auto, 1 peer copies, 2 RCCL"),
    ("set_option-reduce_mode-1", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, b"reduce_mode", 1), 0, None),
    ("set_option-force_rccl-0", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, b"force_rccl", 0), 0, None),
    ("set_option-force_rccl-7", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, b"force_rccl", 7), 0, None),
    ("set_option-member-key", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, b"bp_block", 64), 0, None),
    ("set_option-unknown", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, b"nope", 1), INVALID,
     "device member 0: unknown option nope"),
    ("set_option-member-rejects", "g_fresh", lambda L, g, B: L.ta_group_set_option(g, b"direct_mfma", 2), INVALID,
     "device member 0: " + MFMA),
    # ---- members and shards
    ("member-5", "g_fresh", lambda L, g, B: L.ta_group_member(g, 5, None, None), INVALID, "no such member"),
    ("member-negative", "g_fresh", lambda L, g, B: L.ta_group_member(g, -1, None, None), INVALID, "no such member"),
    ("member-good", "g_fresh", lambda L, g, B: L.ta_group_member(g, 1, ctypes.byref(B.vp), ctypes.byref(B.i)), 0, None),
    ("shard-member", "g_fresh", lambda L, g, B: L.ta_group_shard(g, 10, 2, B.i64, B.i64), INVALID, "bad argument"),
    ("shard-atoms", "g_fresh", lambda L, g, B: L.ta_group_shard(g, -1, 0, B.i64, B.i64), INVALID, "bad argument"),
    ("shard-out-null", "g_fresh", lambda L, g, B: L.ta_group_shard(g, 10, 0, None, B.i64), INVALID, "bad argument"),
    ("shard-good", "g_fresh", lambda L, g, B: L.ta_group_shard(g, 10, 1, B.i64, B.i64), 0, None),
    # ---- staging
    ("alloc-slabs-null", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, T, A, D, F64, 1, None), INVALID, "h_slabs is NULL"),
    ("alloc-slabs-null+shape", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, 0, A, D, F64, 1, None), INVALID, "h_slabs is NULL"),
    ("alloc-frames-0", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, 0, A, D, F64, 1, B.hs), INVALID, GROUP_SHAPE),
    ("alloc-dim-4", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, T, A, 4, F64, 1, B.hs), INVALID, GROUP_SHAPE),
    ("alloc-slabs-5", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, T, A, D, F64, 5, B.hs), INVALID, GROUP_SHAPE),
    ("alloc-shape+dtype", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, T, 0, D, 7, 1, B.hs), INVALID, GROUP_SHAPE),
    ("alloc-dtype", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, T, A, D, 7, 1, B.hs), INVALID, "device member 0: bad dtype"),
    ("alloc-too-many", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, BIG, A, 1, F64, 1, B.hs), INVALID,
     "device member 0: n_frames too large"),
    ("alloc-good-more-members-than-atoms", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc(g, T, 1, D, F64, 1, B.hs), 0, None),
    ("alloc_device-shape", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc_device(g, T, A, D, 0), INVALID, GROUP_SHAPE),
    ("alloc_device-good", "g_fresh", lambda L, g, B: L.ta_group_stage_alloc_device(g, T, A, D, 2), 0, None),
    ("commit-fresh", "g_fresh", lambda L, g, B: L.ta_group_stage_commit(g, 0, 1), STATE, "ta_group_stage_alloc has not been called"),
    ("commit-range", "g_staged", lambda L, g, B: L.ta_group_stage_commit(g, 0, T + 1), INVALID, "device member 0: " + RANGE),
    ("commit-good", "g_staged", lambda L, g, B: L.ta_group_stage_commit(g, 0, T), 0, None),
    ("synth-fresh", "g_fresh", lambda L, g, B: L.ta_group_stage_synth(g, 0, 1, 0, A * D), STATE, NOT_STAGED),
    ("synth-slab", "g_staged", lambda L, g, B: L.ta_group_stage_synth(g, 2, 1, 0, A * D), INVALID, "device member 0: " + NO_SLAB),
    ("synth-offset", "g_staged", lambda L, g, B: L.ta_group_stage_synth(g, 0, 1, -1, A * D), INVALID,
     "device member 0: column block outside the synthetic tensor"),
    ("synth-total", "g_staged", lambda L, g, B: L.ta_group_stage_synth(g, 0, 1, 0, A * D - 1), INVALID,
     "device member 1: column block outside the synthetic tensor"),
    ("synth-good", "g_staged", lambda L, g, B: L.ta_group_stage_synth(g, 1, 3, 0, A * D), 0, None),
    ("stage_free-good", "g_staged", lambda L, g, B: L.ta_group_stage_free(g), 0, None),
    # ---- compute
    ("vacf_fft-ts-null", "g_staged", lambda L, g, B: L.ta_group_vacf_fft(g, None, None), INVALID, "h_timeseries is NULL"),
    ("vacf_fft-ts-null+fresh", "g_fresh", lambda L, g, B: L.ta_group_vacf_fft(g, None, None), INVALID, "h_timeseries is NULL"),
    ("vacf_fft-fresh", "g_fresh", lambda L, g, B: L.ta_group_vacf_fft(g, B.p("ts"), None), STATE, NOT_STAGED),
    ("vacf_direct-fresh", "g_fresh", lambda L, g, B: L.ta_group_vacf_direct(g, B.p("ts"), None), STATE, NOT_STAGED),
    ("helfand-fresh+masses", "g_fresh", lambda L, g, B: L.ta_group_helfand_msd(g, None, 1.0, B.p("ts"), None), STATE, NOT_STAGED),
    ("helfand-masses-null", "g_staged", lambda L, g, B: L.ta_group_helfand_msd(g, None, 1.0, B.p("ts"), None), INVALID,
     "h_masses is NULL"),
    ("msd-fft", "g_staged", lambda L, g, B: L.ta_group_msd(g, 2, B.p("ts"), None), INVALID, FFT_FLAG),
    ("msd-fft+fresh", "g_fresh", lambda L, g, B: L.ta_group_msd(g, -1, None, None), INVALID, FFT_FLAG),
    ("msd-fresh", "g_fresh", lambda L, g, B: L.ta_group_msd(g, 0, B.p("ts"), None), STATE, NOT_STAGED),
    ("vacf_fft-good", "g_staged", lambda L, g, B: L.ta_group_vacf_fft(g, B.p("ts"), B.p("bp")), 0, None),
    ("helfand-good", "g_staged", lambda L, g, B: L.ta_group_helfand_msd(g, B.p("m"), 1.0, B.p("ts"), None), 0, None),
    ("msd-good", "g_staged", lambda L, g, B: L.ta_group_msd(g, 0, B.p("ts"), B.p("bp")), 0, None),
    ("cond-fft", "g_staged", lambda L, g, B: L.ta_group_conductivity(g, 2, B.p("q"), B.p("mom"), B.p("phi"), None), INVALID, FFT_FLAG),
    ("cond-fft+charges", "g_staged", lambda L, g, B: L.ta_group_conductivity(g, 2, None, B.p("mom"), B.p("phi"), None), INVALID, FFT_FLAG),
    ("cond-charges", "g_staged", lambda L, g, B: L.ta_group_conductivity(g, 1, None, B.p("mom"), B.p("phi"), None), INVALID,
     "charges, moment or collective is NULL"),
    ("cond-moment", "g_staged", lambda L, g, B: L.ta_group_conductivity(g, 1, B.p("q"), None, B.p("phi"), None), INVALID,
     "charges, moment or collective is NULL"),
    ("cond-collective", "g_staged", lambda L, g, B: L.ta_group_conductivity(g, 1, B.p("q"), B.p("mom"), None, None), INVALID,
     "charges, moment or collective is NULL"),
    ("cond-collective+fresh", "g_fresh", lambda L, g, B: L.ta_group_conductivity(g, 1, B.p("q"), B.p("mom"), None, None), INVALID,
     "charges, moment or collective is NULL"),
    ("cond-fresh", "g_fresh", lambda L, g, B: L.ta_group_conductivity(g, 1, B.p("q"), B.p("mom"), B.p("phi"), None), STATE, NOT_STAGED),
    ("cond-good", "g_staged", lambda L, g, B: L.ta_group_conductivity(g, 0, B.p("q"), B.p("mom"), B.p("phi"), B.p("slf")), 0, None),
    ("ons-fft", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 2, S, B.p("lab"), None, B.p("moms"), None), INVALID, FFT_FLAG),
    ("ons-fft+species-count", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 2, 0, B.p("lab"), None, B.p("moms"), None), INVALID, FFT_FLAG),
    ("ons-species-0", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 1, 0, B.p("lab"), None, B.p("moms"), None), INVALID, SPECIES),
    ("ons-species-9", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 1, 9, B.p("lab"), None, B.p("moms"), None), INVALID, SPECIES),
    ("ons-species-count+labels", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 1, 9, None, None, B.p("moms"), None), INVALID, SPECIES),
    ("ons-labels", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 1, S, None, None, B.p("moms"), None), INVALID, GROUP_ONS_NULL),
    ("ons-moments", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 1, S, B.p("lab"), None, None, None), INVALID, GROUP_ONS_NULL),
    ("ons-moments+fresh", "g_fresh", lambda L, g, B: L.ta_group_onsager(g, 1, S, B.p("lab"), None, None, None), INVALID, GROUP_ONS_NULL),
    ("ons-fresh", "g_fresh", lambda L, g, B: L.ta_group_onsager(g, 1, S, B.p("lab"), None, B.p("moms"), None), STATE, NOT_STAGED),
    ("ons-fresh+label", "g_fresh", lambda L, g, B: L.ta_group_onsager(g, 1, S, B.p("lab_neg"), None, B.p("moms"), None), STATE, NOT_STAGED),
    ("ons-label-negative", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 1, S, B.p("lab_neg"), None, B.p("moms"), None), INVALID, LABEL_NEG),
    ("ons-label-n_species", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 1, S, B.p("lab_hi"), None, B.p("moms"), None), INVALID, LABEL_HI),
    ("ons-good", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 0, S, B.p("lab"), B.p("w"), B.p("moms"), B.p("cross")), 0, None),
    ("ons-good-moments-only", "g_staged", lambda L, g, B: L.ta_group_onsager(g, 1, S, B.p("lab"), None, B.p("moms"), None), 0, None),
    ("unwrap-dims-null", "g_staged", lambda L, g, B: L.ta_group_unwrap(g, 0, None, B.p("axes")), INVALID, "dimensions or axes are NULL"),
    ("unwrap-axes-null+fresh", "g_fresh", lambda L, g, B: L.ta_group_unwrap(g, 0, B.p("box"), None), INVALID,
     "dimensions or axes are NULL"),
    ("unwrap-fresh", "g_fresh", lambda L, g, B: L.ta_group_unwrap(g, 0, B.p("box"), B.p("axes")), STATE, NOT_STAGED),
    ("unwrap-slab", "g_staged", lambda L, g, B: L.ta_group_unwrap(g, 2, B.p("box"), B.p("axes")), INVALID, NO_SLAB),
    ("unwrap-slab+box", "g_staged", lambda L, g, B: L.ta_group_unwrap(g, -1, B.p("badbox"), B.p("axes")), INVALID, NO_SLAB),
    ("unwrap-box", "g_staged", lambda L, g, B: L.ta_group_unwrap(g, 0, B.p("badbox"), B.p("axes")), INVALID,
     "unwrap: box length <= 0 or not finite in frame 0"),
    ("unwrap-good", "g_staged", lambda L, g, B: L.ta_group_unwrap(g, 0, B.p("box"), B.p("axes")), 0, None),
]


def _expand(rows, prefix):
    """"*_x" states run once on a CPU context (no mark) and once on a GPU context (gpu mark)."""
    out = []
    for rid, state, call, code, msg in rows:
        states = [state.replace("*", "cpu"), state.replace("*", "gpu")] if state.startswith("*") else [state]
        for s in states:
            marks = [pytest.mark.gpu] if s.startswith(("gpu", "g_")) else []
            out.append(pytest.param(s, call, code, msg, id=f"{prefix}{rid}[{s}]", marks=marks))
    return out


def _run_row(state, call, code, msg, last_error):
    L = _lib.lib()
    h, close = _state(L, state)
    try:
        rc = call(L, h, Bufs())
        text = last_error(L, h).decode()
        assert rc == code, (rc, text)
        if msg is not None:
            assert text == msg
    finally:
        close()


@pytest.mark.parametrize("state,call,code,msg", _expand(CTX_ROWS, ""))
def test_context_contract(state, call, code, msg):
    _run_row(state, call, code, msg, lambda L, h: L.ta_last_error(h))


@pytest.mark.parametrize("state,call,code,msg", _expand(GROUP_ROWS, "group-"))
def test_group_contract(state, call, code, msg):
    _run_row(state, call, code, msg, lambda L, g: L.ta_group_last_error(g))


def _option_rows():
    out = []
    for key, value, msg in OPTIONS:
        for s in ("cpu_fresh", "gpu_fresh", "gpu_staged"):
            marks = [pytest.mark.gpu] if s.startswith("gpu") else []
            out.append(pytest.param(s, key, value, msg, id=f"{key}={value}[{s}]", marks=marks))
    return out


@pytest.mark.parametrize("state,key,value,msg", _option_rows())
def test_option_contract(state, key, value, msg):
    """Every key of ta_set_option: accepted values return TA_OK and leave the message alone, rejected ones and unknown
    keys return TA_E_INVALID with their text."""
    _run_row(state, lambda L, h, B: L.ta_set_option(h, key.encode(), value), 0 if msg is None else INVALID, msg,
             lambda L, h: L.ta_last_error(h))


def test_group_stage_frame_null_group():
    """ta_group_stage_frame reports through its members: a NULL group has none, and there is no message to pin."""
    B = Bufs()
    assert _lib.lib().ta_group_stage_frame(None, 0, 0, B.p("src"), F64, D, 0, 1, D, 0, None, A) == INVALID


def test_failed_call_keeps_its_message_until_the_next_failure():
    """ta_last_error(ctx) is the context's LAST failure: calls that succeed in between do not clear it."""
    L = _lib.lib()
    h, close = _state(L, "cpu_fresh")
    try:
        assert L.ta_set_option(h, b"nope", 1) == INVALID
        assert L.ta_set_option(h, b"fft_nwg", 0) == 0 and L.ta_trim(h) == 0
        assert L.ta_last_error(h) == b"unknown option nope"
        assert L.ta_stage_commit(h, 0, 1) == STATE
        assert L.ta_last_error(h) == b"ta_stage_alloc has not been called"
    finally:
        close()


# ---- lifetimes: what ta_trim, the option "async_commit" and the commit queue promise -------------------------------------

def _fill(ctx, T_, A_, D_, n_slabs, seed):
    rng = np.random.default_rng(seed)
    data = [rng.standard_normal((T_, A_, D_)) for _ in range(n_slabs)]
    views = ctx.stage_alloc(T_, A_, D_, n_slabs=n_slabs)
    return data, views


def _every_quantity(ctx, A_):
    m = np.linspace(1.0, 2.0, A_)
    q = np.where(np.arange(A_) % 2 == 0, 1.0, -0.5)
    lab = np.arange(A_) % 3
    out = []
    for r in (ctx.vacf_fft(by_particle=True), ctx.vacf_fft(), ctx.vacf_direct(by_particle=True), ctx.vacf_direct(),
              ctx.helfand_msd(m, 3.0, by_particle=True), ctx.helfand_msd(m, 3.0), ctx.msd(True, by_particle=True),
              ctx.msd(False, by_particle=True), ctx.msd(True), ctx.conductivity(True, q, self_term=True),
              ctx.conductivity(False, q, self_term=True), ctx.onsager(True, lab, 3, weights=q),
              ctx.onsager(False, lab, 3, weights=q), ctx.onsager(True, lab, 3, cross=False)):
        out += [np.array(a, copy=True) for a in r if a is not None]
    return out


@pytest.mark.parametrize("device,T_", [pytest.param("cpu", 40), pytest.param(0, 40, marks=pytest.mark.gpu),
                                       pytest.param(0, 700, marks=pytest.mark.gpu)])
def test_trim_between_calls_changes_no_result(device, T_):
    """After ta_trim every quantity comes out bit-identical: no workspace that a later call relies on without
    re-creating is released, none that is released is used stale (40 frames: k_short; 700: the FFT and band forms)."""
    ctx = _lib.Context(device)
    try:
        A_ = 70
        data, views = _fill(ctx, T_, A_, 3, 2, seed=3)
        for v, d in zip(views, data):
            v[...] = d
        ctx.stage_commit(0, T_)
        first = _every_quantity(ctx, A_)
        ctx.trim()
        second = _every_quantity(ctx, A_)
        ctx.trim()
        ctx.trim()
        third = _every_quantity(ctx, A_)
        assert len(first) == len(second) == len(third) > 0
        for a, b, c in zip(first, second, third):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        ctx.unwrap(0, np.tile(np.array([7.0, 8.0, 9.0, 90.0, 90.0, 90.0]), (T_, 1)), [0, 1, 2])
        u1 = ctx.msd(False)[0].copy()
        ctx.trim()
        assert np.array_equal(ctx.msd(False)[0], u1)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_async_commit_toggled_between_commits_loses_no_frame():
    """"async_commit" 0 / 1 between ta_stage_commit calls: the option flushes the queue before it changes, so every
    committed frame is on the device whichever path took it (read back with ta_stage_read_dev)."""
    import torch

    T_, A_, D_ = 64, 50, 3
    ctx = _lib.Context(0)
    try:
        data, (view,) = _fill(ctx, T_, A_, D_, 1, seed=5)
        for i, lo in enumerate(range(0, T_, 8)):
            view[lo:lo + 8] = data[0][lo:lo + 8]
            ctx.set_option("async_commit", i % 2)
            ctx.stage_commit(lo, lo + 8)
        back = torch.zeros((T_, A_ * D_), dtype=torch.float64, device="cuda:0")
        ctx.stage_read_dev(0, back.data_ptr(), A_ * D_)
        torch.cuda.synchronize()
        assert np.array_equal(back.cpu().numpy().reshape(T_, A_, D_), data[0])
        want = ctx.vacf_direct()[0]
        ref = _lib.Context(0)
        try:
            (v2,) = ref.stage_alloc(T_, A_, D_)
            v2[...] = data[0]
            ref.set_option("async_commit", 0)
            ref.stage_commit(0, T_)
            assert np.array_equal(ref.vacf_direct()[0], want)
        finally:
            ref.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_queued_commit_failure_surfaces_once_at_the_next_flush():
    """A commit that fails on the worker thread (here: a refused host allocation, the "fail_alloc_after" hook in the
    worker's first workspace request) returns TA_OK to its caller; the NEXT call that flushes the queue returns the
    failure with the documented prefix, and the one after that does not see it again."""
    L = _lib.lib()
    T_, A_, D_ = 16, 5, 3
    ctx = _lib.Context(0)
    try:
        (view,) = ctx.stage_alloc(T_, A_, D_)
        view[...] = 1.0
        ctx.set_option("fail_alloc_after", 1)
        assert L.ta_stage_commit(ctx._h, 0, T_) == 0
        assert L.ta_trim(ctx._h) == NOMEM
        assert L.ta_last_error(ctx._h) == b"queued ta_stage_commit: out of host memory (std::bad_alloc inside the library)"
        assert L.ta_trim(ctx._h) == 0
        ctx.stage_commit(0, T_)  # the frames were never copied: commit them again
        ts = ctx.vacf_direct()[0]
        np.testing.assert_allclose(ts, np.full(T_, 3.0), rtol=1e-12)  # sum_d 1 * 1 at every lag: the frames arrived
    finally:
        ctx.close()
