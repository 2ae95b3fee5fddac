"""Case lists and helpers of the joint-volume domain tests (tests/test_volume_domain_host.py on the CPU, tests/test_gpu_volume_domain.py
on the device): the corners of the domain that include/sceneego_hip.h promises for se_volume_filter_f32, se_skeleton_couple_f32 and
se_shell_correlate_f32 and that the operators' own test files never enter.  No device code.

Why they were never entered: the operators' own tests softmax their inputs on the device with se_softargmax3d_f32, which refuses
voxels & 3, so every grid there is even.  The inputs here are softmaxed ON THE HOST (volume_filter_cases.softmax32: float64, rounded to
float32) and copied to the device, which makes odd grids, and the same inputs in the host test and in the GPU test, possible.

The generators, the seed rules and the models are the operators' own (volume_filter_cases, skeleton_prior_cases, volume_filter_model,
skeleton_prior_model).  Two shapes are out of their reach and are said so here:
  * volume_filter_cases.make_logits standardises by the std of a bump that is constant on a 2^3 grid (0 / 0): G = 2 takes plain normal
    logits x 2 instead;
  * skeleton_prior_cases.make_pose cannot place a pose on a 2^3 grid (its box [0.5, G - 1.5] is one point): G = 2 is left out for the
    skeleton operators.
"""
import functools

import numpy as np

import skeleton_prior_cases as SC
import volume_filter_cases as FC
from skeleton_prior_model import skeleton_couple_model
from volume_filter_model import volume_filter_model

SIDE = FC.SIDE
assert SC.SIDE == SIDE

# ------------------------------------------------------------------------------------------------------------------ 1. the filter
# rows, G, R, floor, T
FILTER_CASES = [
    (2, 3, 2, 1e-3, 4),          # 27 voxels: the scalar finish pass, R = G - 1
    (4, 5, 2, 0.0, 4),
    (3, 9, 3, 1e-3, 4),
    (2, 17, 16, 1e-3, 3),        # R = 16 = G - 1: the longest taps, every window clipped on both sides
    (1, 127, 16, 1e-3, 2),       # the largest odd grid: W = 128 lanes for 127 columns
    (3, 2, 0, 1e-3, 3),          # the smallest grid: one lane row serves 128 plane rows
    (3, 2, 1, 1e-3, 3),
]
FILTER_ALIGN_CASE = (4, 10, 3, 1e-3, 5)      # an even grid of the operator's own list: the fast finish pass unless a base is offset
FILTER_CUT_CASE = (3, 9, 3, 1e-3, 4)
FILTER_NAN_CASE = (3, 9, 3, 1e-3, 4)


def filter_seed(rows, G, R):
    return 1000 * G + 10 * rows + R


@functools.lru_cache(maxsize=None)
def filter_inputs(rows, G, R, T):
    """Host arrays of one sequence, computed once and shared (nothing modifies them): p [T, rows, N] float32 softmaxed on the host, c
    [N, 3] float32, taps [2R+1] float32."""
    seed = filter_seed(rows, G, R)
    if G == 2:
        logits = (2.0 * np.random.default_rng(seed).standard_normal((T, rows, 8))).astype(np.float32)
    else:
        logits = FC.make_logits(T, rows, G, R, seed=seed)
    return {"p": FC.softmax32(logits), "c": FC.coord_grid(G), "taps": FC.taps_for(G, R)}


@functools.lru_cache(maxsize=None)
def filter_want(rows, G, R, floor, T):
    """volume_filter_model on filter_inputs: (belief, joints, evidence, restarted), float64."""
    k = filter_inputs(rows, G, R, T)
    return volume_filter_model(k["p"], k["c"], k["taps"], G, floor)


def filter_condition(want, N):
    """The condition on the inputs, on the model: every update has evidence x N >= 1e-3 and only frame 0 restarts.  Returns the
    smallest evidence x N."""
    _, _, we, wr = want
    low = float(np.nanmin(we[1:])) * N
    assert (we[1:] * N >= 1e-3).all(), f"evidence x N down to {low}"
    assert wr[0].all() and not wr[1:].any()
    return low


# ------------------------------------------------------------------------------------------------------------------ 2. the skeleton
J_MAX = 32
TREES = {
    "chain3": SC.CHAIN3,
    "chain32": tuple(max(j - 1, 0) for j in range(J_MAX)),            # depth 31: the longest walk over the levels
    "heap2_32": tuple(max(j - 1, 0) // 2 for j in range(J_MAX)),      # two children per joint
    "heap4_32": tuple(max(j - 1, 0) // 4 for j in range(J_MAX)),      # four: the general product loop at J = 32
}
# A wide star is no case: 31 children give a normaliser of 2e-56 and 9 children 3e-15 with these generators, below the 1e-12 of the
# condition, so the float32 kernel would fall back and the test would measure nothing.  star5 (the operator's own list) stays the widest.

# frames, tree, G, R, floor
SKELETON_CASES = [
    (1, "chain3", 3, 2, 1e-3),
    (1, "chain3", 5, 4, 0.0),
    (1, "chain3", 7, 3, 1e-3),
    (2, "chain3", 9, 4, 0.0),            # odd G: ragged row and column tiles together, an odd chunk of the row sums
    (1, "chain3", 65, 4, 1e-3),          # the second column tile holds one column
    (1, "chain3", 80, 24, 1e-3),         # R at its maximum: the deepest LDS tile and the longest runs
    (1, "chain3", 127, 6, 1e-3),
    (1, "chain3", 128, 20, 1e-3),
    (1, "chain32", 8, 3, 1e-3),
    (1, "heap2_32", 8, 3, 1e-3),
    (1, "heap4_32", 8, 3, 1e-3),
]
SKELETON_ALIGN_CASE = (2, "chain3", 9, 4, 0.0)
SKELETON_BATCH_CASE = (5, "chain3", 9, 4, 0.0)       # five frames: a group of four and one more
# G, R of se_shell_correlate_f32 alone over two column tiles; and one small grid where every voxel is compared
CORRELATE_CASES = [(65, 4), (127, 4)]
CORRELATE_SMALL = (9, 8)
# ... and two thin shells (3.2 and 1.6 voxels) inside a block of the largest radius at a two-tile grid: the deepest LDS tile with few
# non-zero taps, so that (nnz + 2) u holds the second column tile far tighter than the coupling's bound at R = 24 can
CORRELATE_DEEP = (80, 24, (3.2, 1.6))


def skeleton_seed(tree, G, R):
    return 1000 * G + 10 * len(TREES[tree]) + R


def skeleton_method(G):
    """The form of the float64 model: the FFT form from 64^3 up (the direct one is too slow there), which needs floor > 0."""
    return "fft" if G >= 64 else "direct"


@functools.lru_cache(maxsize=None)
def skeleton_inputs(frames, tree, G, R):
    """Host arrays of one case, computed once and shared (nothing modifies them): p [frames, J, N] float32 softmaxed on the host, c
    [N, 3] float32, taps [J, (2R+1)^3] float32, the tree and the bone lengths."""
    parents = TREES[tree]
    seed = skeleton_seed(tree, G, R)
    lengths = SC.lengths_for(parents, G, R, seed)
    logits = SC.make_logits(frames, parents, lengths, G, seed)[0]
    return {"p": FC.softmax32(logits), "c": FC.coord_grid(G), "taps": SC.taps_for(lengths, G, R), "parents": parents, "lengths": lengths}


@functools.lru_cache(maxsize=None)
def skeleton_want(frames, tree, G, R, floor):
    """skeleton_couple_model on skeleton_inputs: (beliefs, joints, evidence, coupled, norms), float64."""
    k = skeleton_inputs(frames, tree, G, R)
    assert floor > 0 or skeleton_method(G) == "direct"
    return skeleton_couple_model(k["p"], k["c"], k["taps"], k["parents"], G, floor, method=skeleton_method(G))


def skeleton_condition(want):
    """The condition on the inputs, on the model: no frame falls back and every s, t, Z is >= 1e-12.  Returns the smallest."""
    norms, coupled = want[4], want[3]
    small = min(float(np.nanmin(norms[k])) for k in ("s", "t", "Z") if np.isfinite(norms[k]).any())
    assert coupled.all() and small >= 1e-12, f"a normaliser of {small}"
    return small


@functools.lru_cache(maxsize=None)
def correlate_inputs(G, R):
    """Two volumes and two different shells for se_shell_correlate_f32: a [2, N] float32 (the first two joints of the chain3 case of
    SKELETON_CASES at this grid, whatever its R: the pose generator is not asked for a second pose), taps [3, (2R+1)^3] float32 (rows 1
    and 2 hold two bone lengths that fit R), tap_row (2, 1), s and the scale."""
    frames, tree, _, pose_r, _ = next(c for c in SKELETON_CASES if c[1] == "chain3" and c[2] == G)
    lengths = SC.lengths_for(SC.CHAIN3, G, R, skeleton_seed("chain3", G, R))
    assert lengths[1] != lengths[2]
    return {"a": np.ascontiguousarray(skeleton_inputs(frames, tree, G, pose_r)["p"][0, :2]), "taps": SC.taps_for(lengths, G, R),
            "tap_row": np.array([2, 1], dtype=np.int32), "s": np.array([0.37, 2.5], dtype=np.float32), "scale": np.float32(0.999)}


def correlate_voxels(G):
    """The flat voxels compared at a two-tile grid: every voxel of the last plane i = G - 1, of the columns k >= 64 and 4096 sampled."""
    n = np.arange(G ** 3)
    region = n[(n // (G * G) == G - 1) | (n % G >= 64)]
    sample = np.random.default_rng(3 + G).choice(G ** 3, size=4096, replace=False)
    return np.unique(np.concatenate([region, sample]))


# ------------------------------------------------------------------------------------------------------------------ 3. split rows
SPLIT_GRIDS = (96, 128)
SPLIT_ROWS = 2                   # se_sa_splits(rows < 30) = 256 chunks per row
# rows, G, K, radius
MODES_CASES = [(2, 96, 4, 2),    # 24 lanes per row: idle lanes in every band
               (2, 128, 16, 3)]  # 32 lanes per row, bands of 8 rows


@functools.lru_cache(maxsize=None)
def split_logits(rows, G):
    """Normal logits x 3, float32 [rows, G^3]."""
    return (3.0 * np.random.default_rng(7000 + G).standard_normal((rows, G ** 3))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ 4. guards
GUARD_BYTES = 128 * 1024         # per band: at least 64 KiB and at least one G^2 plane of float32 at G = 128 (64 KiB)
GUARD_FILL = 0xA5                # 0xA5A5A5A5 is -2.87e-16 as a float32 and -1515870811 as an int32: no result of these operators
NAN_FILL = 0xFF                  # 0xFFFFFFFF is a NaN as a float32


def _banded(numel, dtype, offset_bytes, device, fill):
    import torch
    assert offset_bytes >= 0 and offset_bytes % 4 == 0
    size = torch.empty((), dtype=dtype).element_size()
    start, nbytes = GUARD_BYTES + offset_bytes, numel * size
    buf = torch.full((start + nbytes + GUARD_BYTES,), fill, dtype=torch.uint8, device=device)
    view = buf[start:start + nbytes].view(dtype)
    assert view.data_ptr() == buf.data_ptr() + start and view.is_contiguous() and view.numel() == numel
    return buf, view, start, nbytes


def guarded(numel, dtype, offset_bytes=0, device="cuda:0"):
    """(view, check): a contiguous 1-D ``view`` of ``numel`` elements of ``dtype`` inside one larger allocation, a band of GUARD_BYTES
    bytes of GUARD_FILL before it and one after it (the payload is filled with it too, so an element that the operator leaves unwritten
    shows as well).  ``offset_bytes`` (a multiple of 4) moves the view that far off the allocation's alignment; the bytes skipped belong
    to the band before.  ``check()`` asserts that both bands are unchanged: an overrun is a failed assertion, not a fault."""
    import torch
    buf, view, start, nbytes = _banded(numel, dtype, offset_bytes, device, GUARD_FILL)

    def check(what=""):
        torch.cuda.synchronize() if buf.is_cuda else None
        before, after = buf[:start], buf[start + nbytes:]
        bad_b, bad_a = int((before != GUARD_FILL).sum()), int((after != GUARD_FILL).sum())
        assert bad_b == 0 and bad_a == 0, f"{what}: {bad_b} bytes written before and {bad_a} after a view of {numel} x {dtype}"
    check.buffer = buf               # the whole allocation, bands included, as bytes
    return view, check


def nan_banded(array, offset_bytes=0, device="cuda:0"):
    """An input on the device: ``array`` (numpy or tensor) flattened into a 1-D view with NaN bands (bytes 0xFF) around it, so that a
    read outside the input that reaches a result shows as a NaN or a missed bound."""
    import torch
    t = torch.as_tensor(array).contiguous()
    buf, view, _, _ = _banded(t.numel(), t.dtype, offset_bytes, device, NAN_FILL)
    view.copy_(t.reshape(-1))
    view.buffer = buf                # the whole allocation, bands included, as bytes
    return view
