"""The three launch loops of the pair family that only a long series turns: more than 65535 origins or searched frames.

  vhd_pm        one k_vhd_pairs launch per 65535 origins: the second launch starts at o0 = 65535
  k_vhd_gather  its grid holds at most 65535 origins in y: the others are reached by o += gridDim.y
  pair_find_pm  at most 65535 searched frames per chunk: the second chunk's o_base is 65535 (or what "pair_find_chunk" makes
                it), and with per-frame boxes frame y of a chunk reads the box of frame (o_base + y) stride

The inputs are the smallest that reach them: D = 1 (the box axis 1, the dyadic length 2), three walk items (and for the search
three constructed ones), so the gathered scratch is T x 1280 x 8 bytes per slot and the pair work is trivial.  The references
are vanhove_distinct_ref's and pair_ref's, exact in float64 at these lengths (they assert it), and everything is compared for
equality.  Every case runs once on the CPU backend (unmarked: it has no chunks, but proves the inputs and the expected values
without a GPU) and on both slab types on the GPU, where the launch counts are asserted too."""
import functools

import numpy as np
import pytest

import pair_ref
import vanhove_distinct_ref as ref
from test_pair_lifetime_shapes import run_find
from test_vanhove_distinct_shapes import SLABS, run_staged, slab_bits, stage, staged_bits
from transport_analysis_amd import _lib

ORIGINS = 65535  # origins per k_vhd_pairs launch, per y extent of k_vhd_gather's grid, searched frames per chunk at most

# (T, origin stride, boxed): exactly one launch; a second launch of one origin (with the box and without); 65537 origins with
# t = 2 o; per-frame boxes read at o >= 65535 (lag 0 only)
VHD_CASES = [(65535, 1, True), (65536, 1, True), (65536, 1, False), (131073, 2, True), (65537, 1, "frames")]
VHD_IDS = [f"T{T}-stride{s}-box{b}" for T, s, b in VHD_CASES]


def vhd_case(T, stride, boxed):
    """vanhove_distinct_ref.case of 3 items in one dimension: lags 0, 1, 2, T // 2, T - 1 (at the last only origin 0 survives,
    every later workgroup leaves before its barrier); "frames": lag 0.  references() asserts the sum invariant."""
    return ref.case(T, 3, 1, stride, "same", boxed)


def vhd_launches(T, stride):
    return -(-int(ref.n_origins(T, [0], stride)[0]) // ORIGINS)


def test_the_cases_turn_the_loops():
    assert [vhd_launches(T, s) for T, s, _ in VHD_CASES] == [1, 2, 2, 2, 2]
    assert int(ref.n_origins(131073, [0], 2)[0]) == 65537 and int(ref.n_origins(65536, [65535], 1)[0]) == 1


@pytest.mark.parametrize("T,stride,boxed", VHD_CASES, ids=VHD_IDS)
def test_vanhove_distinct_cpu(T, stride, boxed):
    x, lags, a, b, dims, axes, refs = vhd_case(T, stride, boxed)
    c = _lib.Context("cpu")
    try:
        (view,) = c.stage_alloc(T, 3, 1, dtype=np.float32)
        view[:] = x
        c.stage_commit(0, T)
        for bins in ref.BINS:
            got = c.vanhove_distinct(lags, *bins, origin_stride=stride, dimensions=dims, axes=axes)
            ref.assert_counts(got, refs[bins], what=f"cpu T={T} stride={stride} box={boxed} bins={bins}")
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,stride,boxed", VHD_CASES, ids=VHD_IDS)
def test_vanhove_distinct_gpu(T, stride, boxed, dtype):
    """counts equal to the reference with the lags in chunks of 1, 2 and all at once (5 lags of 65537 origins gather 2.8 GB,
    below the 4 GiB of one pass), the launch counts of each, the host-facing entry and the slab's bits"""
    x, lags, a, b, dims, axes, refs = vhd_case(T, stride, boxed)
    kw = dict(origin_stride=stride, dimensions=dims, axes=axes)
    per_chunk, L = vhd_launches(T, stride), len(lags)
    c = stage(_lib.Context(0), x, dtype)
    try:
        for bins in ref.BINS:
            runs = []
            for chunk in (1, 2, 0):
                c.set_option("vanhove_distinct_chunk", chunk)
                runs.append(run_staged(c, lags, *bins, repeat=1, **kw))
                chunks = -(-L // chunk) if chunk else 1
                n_gather, n_pairs = c.kernel_launches("k_vhd_gather"), c.kernel_launches("k_vhd_pairs")
                print(f"    T={T} stride={stride} chunk={chunk}: k_vhd_gather x {n_gather}, k_vhd_pairs x {n_pairs}")
                assert n_gather == chunks and n_pairs == chunks * per_chunk
                assert "k_widen_f32" not in [n for n, _ in c.kernel_timeline(64)]
            ref.assert_counts(runs[0], refs[bins], what=f"T={T} stride={stride} box={boxed} bins={bins}")
            assert all(np.array_equal(runs[0], r) for r in runs[1:]), "the chunk size changed the counts"
            assert np.array_equal(c.vanhove_distinct(lags, *bins, **kw), runs[0]), "the host-facing entry differs from the staged one"
        assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    finally:
        c.close()


# ---- ta_pair_find ---------------------------------------------------------------------------------------------------------
R_CUT = 0.25  # dyadic, an eighth of the shortest box
BASE = 4096.0  # where the constructed items rest: a multiple of every box length, and without a box far from the walk
FIND_CASES = [(65537, 1), (131073, 2)]
BOXES = [False, True, "frames"]
# the box lengths of the three marked frames, and of every other frame
MARKED_BOXES, OTHER_BOX = (8.0, 2.0, 4.0), 16.0


@functools.lru_cache(maxsize=None)
def find_case(T, stride, boxed):
    """(x (T, 6, 1), dims or None, found list, the three constructed pairs, their frames).  Items 0 ... 2 are the walk; items
    3, 4, 5 rest at BASE + 0, 0.5 and 1: no two of them within R_CUT under any box here.  In the searched frames o = 65534,
    65535 and 65536 (t = stride o: the last of the first chunk of 65535, the first and the last of the second) one of them sits
    1/8 from another: (3, 4), then (3, 5), then (4, 5).  boxed "frames": it sits one box length of ITS frame further, and
    every other frame's box is 16 -- the pair is bonded under its own frame's box only."""
    assert T == stride * 65536 + 1
    frames = [stride * o for o in (65534, 65535, 65536)]
    pairs = [(3, 4), (3, 5), (4, 5)]
    shift = MARKED_BOXES if boxed == "frames" else (0.0, 0.0, 0.0)
    x = np.empty((T, 6, 1))
    x[:, :3] = ref.positions(T, 3, 1)
    x[:, 3:, 0] = BASE + np.array([0.0, 0.5, 1.0])[None, :]
    x[frames[0], 4, 0] = BASE + 0.125 + shift[0]
    x[frames[1], 5, 0] = BASE + 0.125 + shift[1]
    x[frames[2], 5, 0] = BASE + 0.625 + shift[2]
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    dims = box = None
    if boxed:
        lengths = np.full(T, OTHER_BOX if boxed == "frames" else ref.BOX[1])
        if boxed == "frames":
            lengths[frames] = MARKED_BOXES
        dims = np.array([[4.0, h, 4.0, 90.0, 90.0, 90.0] for h in lengths])
        box = lengths[:, None]
    want = pair_ref.found(x, None, None, box, R_CUT, stride)
    # each constructed pair is bonded in its frame and in no other, and is in the list
    h = pair_ref.indicator(x, pairs, box, R_CUT)
    for row, t, pair in zip(h, frames, pairs):
        assert np.flatnonzero(row).tolist() == [t], (pair, np.flatnonzero(row)[:5])
        assert (want == np.array(pair)).all(axis=1).any(), pair
    if boxed == "frames":  # ... and under the box of frame 0 (what a chunk without its o_base would read) it is not
        wrong = pair_ref.indicator(x, pairs, np.full((T, 1), OTHER_BOX), R_CUT)
        assert not wrong.any()
    x.setflags(write=False)
    return x, dims, want.astype(np.int32), pairs, frames


@pytest.mark.parametrize("boxed", BOXES, ids=["nobox", "box", "frames"])
@pytest.mark.parametrize("T,stride", FIND_CASES)
def test_pair_find_cpu(T, stride, boxed):
    x, dims, want, pairs, _ = find_case(T, stride, boxed)
    c = _lib.Context("cpu")
    try:
        (view,) = c.stage_alloc(T, 6, 1, dtype=np.float32)
        view[:] = x
        c.stage_commit(0, T)
        got = c.pair_find(R_CUT, search_stride=stride, dimensions=dims, axes=ref.AXES[1])
        print(f"    cpu T={T} stride={stride} box={boxed}: found {got.shape[0]} pairs, expected {want.shape[0]}")
        assert np.array_equal(got, want)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("boxed", BOXES, ids=["nobox", "box", "frames"])
@pytest.mark.parametrize("T,stride", FIND_CASES)
def test_pair_find_gpu(T, stride, boxed, dtype):
    """65537 searched frames in chunks of 65535 (the clamp of the automatic size), 1000 and 65535 (asked for)"""
    x, dims, want, pairs, _ = find_case(T, stride, boxed)
    c = stage(_lib.Context(0), x, dtype)
    try:
        for chunk, launches in ((0, 2), (1000, 66), (65535, 2)):
            c.set_option("pair_find_chunk", chunk)
            run_find(c, dtype, x, R_CUT, want, repeat=1, search_stride=stride, dimensions=dims, axes=ref.AXES[1])
            n_gather, n_find = c.kernel_launches("k_vhd_gather"), c.kernel_launches("k_pair_find")
            print(f"    T={T} stride={stride} box={boxed} chunk={chunk}: k_vhd_gather x {n_gather}, k_pair_find x {n_find}")
            assert n_gather == launches == n_find
    finally:
        c.close()
