"""GPU: the joint-volume operators over the part of their documented domain (include/sceneego_hip.h) that their own test files never
enter: odd grids and the smallest grid of se_volume_filter_f32 (vf_finish_kernel<false>, also reached by any base that is only 4-byte
aligned), the second column tile, odd grids, R up to 24 and J = 32 of se_skeleton_couple_f32 / se_shell_correlate_f32, the split-row
operators at 96^3 and 128^3, and for all of them the memory contract: every output and the exactly sized scratch lie between guard
bands, every input between NaN bands (tests/volume_domain_cases.py: guarded, nan_banded).

INPUTS.  The operators' own tests softmax on the device with se_softargmax3d_f32, which refuses voxels & 3; that is why no odd grid was
ever tested.  Parts 1 and 2 here softmax ON THE HOST (volume_filter_cases.softmax32) and copy: the arrays are those that
tests/test_volume_domain_host.py has already put through the float64 models on the CPU.  Part 3 feeds normal logits x 3 through the
operator under test, or through se_softargmax3d_f32 for the operators that read probabilities.

TOLERANCES.  None is new; every comparison goes through the operator's own bound function, imported from its test file:
  filter     test_gpu_volume_filter: beliefs 2 t e1 want + 2^-90, evidence 2 t e1, joints max(2 t e1, (L + 2) u) sum b |c|, restarted
             exact, e1 = (6 R + 20 + L) u.  L = _lib.FILTER_CHAIN = 80 was derived for G = 128: a thread of the update kernel owns one
             column and every (256 / W)-th row of the G x G slab, W the power of two >= G, so it adds ceil(G W / 256) <= 64 terms, then
             6 + 2 (workgroup) + 2 + 6 (the G records, two per lane above 64).  At G = 127: W = 128, 64 terms, two records for lanes
             0..62: the same 80.  At G = 2, 3, 5, 9, 17: W = 2..32, at most 3 terms per thread (G = 17: 8 thread rows for 17 slab rows),
             one record per lane: 3 + 6 + 2 + 1 + 6 = 18 <= 80.
             The scalar finish pass divides each element by the same Z as the vector pass: no term is added.
  skeleton   test_gpu_skeleton_prior: compare() with B = 1.01 (2 (J - 1) + 1) e_msg, e_msg = (T(R) + L + 8 + kids) u.  T(R) =
             _lib.SHELL_CHAIN(R) depends on R alone (2449 at R = 24).  L = _lib.SKELETON_SUM_CHAIN = 142 was derived for 128^3: CH =
             min(64, ceil(N / 256)) chunks of ceil(N / CH) values, a thread adds ceil(chunk / 256) of them: 128 at 128^3 (chunk
             32768), 126 at 127^3 (chunk 32006), 32 at 80^3, 17 at 65^3, at most 1 below 9^3; then 6 + 2 + 6.  All <= 142.
             se_shell_correlate_f32 alone: (nnz + 2) u, as test_shell_correlation_at_the_production_shape.
  split rows test_gpu_volume_io.check_softargmax computes its chain T = ceil(chunk / 1024) + 23 from (rows, voxels) itself: with 2 or 4
             rows se_sa_splits is 256, the chunk 3456 at 96^3 (T = 27) and 8192 at 128^3 (T = 31).  The covariance, entropy and masked
             sums keep their 1e-4: it stands for a lane chain of up to 1024 terms plus 12 levels; here a lane adds 4 ceil(chunk / 1024)
             = 16 and 32 terms.  The peak and se_joint_modes_f32 are exact.
A launch through VolumeFilter.step / SkeletonPrior.couple uses the buffers the class allocates and cannot be guarded; every _lib-level
launch of parts 1 and 2 is, and every launch of part 3."""
import functools

import numpy as np
import pytest
import torch

import scene_constraint_model as SCM
import test_gpu_joint_modes as TM
import test_gpu_joint_stats as TS
import test_gpu_scene_constraint as TC
import test_gpu_skeleton_prior as TK
import test_gpu_volume_filter as TF
import test_gpu_volume_io as TV
import volume_domain_cases as D
from conftest import synthetic_state_dict
from joint_modes_model import joint_modes_model
from sceneego_amd import _lib, load_config, op, synth
from sceneego_amd.skeleton_prior import SkeletonPrior, shell_taps
from sceneego_amd.volume_filter import gaussian_taps
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
from skeleton_prior_model import corr_direct

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def all_same(got, want):
    return all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))


class Guards:
    """The guarded views of one launch: ``out(numel, dtype)`` hands one out, ``check()`` asserts every band after the launch."""

    def __init__(self, what):
        self.what, self.checks = what, []

    def out(self, numel, dtype, offset_bytes=0):
        view, check = D.guarded(numel, dtype, offset_bytes, DEV)
        self.checks.append(check)
        return view

    def check(self):
        torch.cuda.synchronize()
        for c in self.checks:
            c(self.what)


# ================================================================================================================== 1. the filter
@functools.lru_cache(maxsize=None)
def filter_dev(rows, G, R, T):
    """filter_inputs and plain device copies of them, shared (nothing modifies them)."""
    k = dict(D.filter_inputs(rows, G, R, T))
    k.update(prob=dev(k["p"]), coord=dev(k["c"]), taps_dev=dev(k["taps"]))
    return k


def filter_guarded(k, G, R, floor, offsets=None, prob=None):
    """One _lib-level call over all frames with every output and the exactly sized scratch between guard bands and every input between
    NaN bands; ``offsets`` {name: bytes} moves the named buffers off their alignment.  Host arrays as TF.launch returns them."""
    off = offsets or {}
    p = k["p"] if prob is None else prob
    T, rows, N = p.shape
    g = Guards(f"volume_filter rows {rows} G {G} R {R} offsets {off}")
    pd = D.nan_banded(p, off.get("prob", 0), DEV)
    cd, td = D.nan_banded(k["c"], 0, DEV), D.nan_banded(k["taps"], 0, DEV)
    state = g.out(rows * N, F32, off.get("state", 0))
    out = g.out(T * rows * N, F32, off.get("belief_out", 0))
    joints, evidence, restarted = g.out(T * rows * 3, F32), g.out(T * rows, F32), g.out(T * rows, I32)
    scratch = g.out(_lib.volume_filter_scratch_bytes(rows, G, R), U8, off.get("scratch", 0))
    for name, t in (("prob", pd), ("state", state), ("belief_out", out), ("scratch", scratch)):
        assert t.data_ptr() % 16 == off.get(name, 0) % 16
    _lib.volume_filter(pd, cd, td, state, out, joints, evidence, restarted, T, rows, N, G, R, floor, scratch=scratch)
    g.check()
    return (out.view(T, rows, N).cpu().numpy(), joints.view(T, rows, 3).cpu().numpy(), evidence.view(T, rows).cpu().numpy(),
            restarted.view(T, rows).cpu().numpy(), state.view(rows, N).cpu().numpy())


def compare_filter(k, got, want, R, tag):
    """The bounds of TF.test_against_the_model_over_chained_frames, frame by frame."""
    gb, gj, ge, gr, gs = got
    wb, wj, we, wr = want
    T = gb.shape[0]
    assert np.array_equal(gr != 0, wr)
    assert same_bits(gb[0], k["p"][0]) and same_bits(gs, gb[-1])
    assert np.isnan(ge[0]).all()
    sabs = np.einsum("trn,na->tra", wb, np.abs(k["c"].astype(np.float64)))
    worst = {"belief": 0.0, "evidence": 0.0, "joints": 0.0}
    for t in range(T):
        bound = 2 * t * TF.e1(R)
        err = np.abs(gb[t].astype(np.float64) - wb[t])
        tol = bound * wb[t] + 2.0 ** -90
        rel = None
        if t:
            worst["belief"] = max(worst["belief"], float((err / (wb[t] + 2.0 ** -60)).max()) / U)
            rel = np.abs(ge[t].astype(np.float64) - we[t]) / we[t]
            worst["evidence"] = max(worst["evidence"], float(rel.max()) / U)
        jerr = np.abs(gj[t].astype(np.float64) - wj[t])
        jtol = max(bound, (TF.L + 2) * U) * sabs[t]
        worst["joints"] = max(worst["joints"], float((jerr / sabs[t]).max()) / U)
        at = np.unravel_index(int(np.argmax(err - tol)), err.shape)
        assert (err <= tol).all(), (f"{tag} frame {t}: belief at (row, voxel) {at} is {gb[t][at]!r}, the model {wb[t][at]!r}: off by "
                                    f"{err[at] / max(wb[t][at], 2.0 ** -126) / U:.1f} u of the {bound / U:.0f} u allowed")
        if t:
            assert (rel <= bound).all(), f"{tag} frame {t}: evidence relative error {float(rel.max()) / U:.1f} u > {bound / U:.0f} u"
        assert (jerr <= jtol).all(), f"{tag} frame {t}: joints off by {float((jerr / sabs[t]).max()) / U:.1f} u of sum b|c|"
    print(f"{tag}: last frame's bound {2 * (T - 1) * TF.e1(R) / U:.0f} u; worst (units of 2^-24) {worst}")
    return worst


@pytest.mark.parametrize("rows,G,R,floor,T", D.FILTER_CASES)
def test_filter_against_the_model(rows, G, R, floor, T):
    k = filter_dev(rows, G, R, T)
    want = D.filter_want(rows, G, R, floor, T)
    D.filter_condition(want, G ** 3)
    got = filter_guarded(k, G, R, floor)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    compare_filter(k, got, want, R, f"filter rows {rows} G {G} R {R} floor {floor}")
    plain = TF.launch(k["prob"], k["coord"], k["taps_dev"], G, R, floor)
    assert all_same(got, plain), "the guarded launch and the launch into plain tensors differ"


def test_filter_alignment_does_not_change_a_bit():
    """An even grid, so that the fast finish pass runs when every base is 16-byte aligned and the scalar one when prob, state,
    belief_out or scratch starts 4 bytes into its buffer: both divide each element by the same Z."""
    rows, G, R, floor, T = D.FILTER_ALIGN_CASE
    k = filter_dev(rows, G, R, T)
    want = D.filter_want(rows, G, R, floor, T)
    D.filter_condition(want, G ** 3)
    base = filter_guarded(k, G, R, floor)
    compare_filter(k, base, want, R, "filter, every base aligned")
    assert all_same(base, TF.launch(k["prob"], k["coord"], k["taps_dev"], G, R, floor))
    names = ("prob", "state", "belief_out", "scratch")
    for moved in [(n,) for n in names] + [names]:
        got = filter_guarded(k, G, R, floor, offsets={n: 4 for n in moved})
        assert all_same(got, base), f"offset {moved}: the results differ from the aligned launch"
        compare_filter(k, got, want, R, f"filter, {'+'.join(moved)} offset by 4 bytes")


def test_filter_cuts_at_an_odd_grid():
    rows, G, R, floor, T = D.FILTER_CUT_CASE
    k = filter_dev(rows, G, R, T)
    runs = [TF.steps(TF.make_filter(k, G, R, floor), k["prob"], cuts, G) for cuts in ((4,), (1, 3), (2, 2))]
    for other in runs[1:]:
        for key in ("beliefs", "joints", "evidence", "state"):
            assert same_bits(runs[0][key], other[key]), key
        assert np.array_equal(runs[0]["restarted"], other["restarted"])
    assert runs[0]["restarted"][0].all() and not runs[0]["restarted"][1:].any()
    gb, gj, ge, gr, gs = filter_guarded(k, G, R, floor)
    assert same_bits(runs[0]["beliefs"].reshape(gb.shape), gb) and same_bits(runs[0]["joints"], gj)
    assert same_bits(runs[0]["evidence"], ge) and same_bits(runs[0]["state"].reshape(gs.shape), gs)


def test_filter_nan_restart_on_the_scalar_path():
    rows, G, R, floor, T = D.FILTER_NAN_CASE
    k = filter_dev(rows, G, R, T)
    clean = TF.steps(TF.make_filter(k, G, R, floor), k["prob"], (4,), G)
    prob = k["prob"].clone()
    prob[1, 1, 300] = float("nan")
    bad = TF.steps(TF.make_filter(k, G, R, floor), prob, (2, 2), G)
    want = np.zeros((T, rows), dtype=bool)
    want[0] = True
    want[1, 1] = want[2, 1] = True
    assert np.array_equal(bad["restarted"], want)
    for key in ("beliefs", "joints", "evidence"):
        assert same_bits(bad[key][:, [0, 2]], clean[key][:, [0, 2]]), key
    assert same_bits(bad["state"][[0, 2]], clean["state"][[0, 2]])
    assert same_bits(bad["beliefs"][1, 1].reshape(-1), prob[1, 1].cpu().numpy())
    assert same_bits(bad["beliefs"][2, 1].reshape(-1), k["p"][2, 1])
    assert np.isnan(bad["evidence"][1, 1]) and np.isnan(bad["evidence"][2, 1]) and np.isfinite(bad["evidence"][3, 1])
    assert np.isnan(bad["joints"][1, 1]).all() and np.isfinite(bad["joints"][2:, 1]).all()
    assert same_bits(bad["beliefs"][0, 1], clean["beliefs"][0, 1])
    # the same through one guarded _lib-level call
    got = filter_guarded(k, G, R, floor, prob=prob.cpu().numpy())
    assert same_bits(got[0], bad["beliefs"].reshape(got[0].shape)) and np.array_equal(got[3] != 0, want)


# ================================================================================================================== 2. the skeleton
@functools.lru_cache(maxsize=None)
def skeleton_dev(frames, tree, G, R):
    k = dict(D.skeleton_inputs(frames, tree, G, R))
    k.update(prob=dev(k["p"]), coord=dev(k["c"]), taps_dev=dev(k["taps"]))
    return k


def skeleton_guarded(k, G, R, floor, offsets=None, frames=None):
    """One guarded _lib-level call over the frames ``frames`` (a slice; default all): host arrays as TK.launch returns them."""
    off = offsets or {}
    p = k["p"] if frames is None else k["p"][frames]
    F, J, N = p.shape
    g = Guards(f"skeleton_couple frames {F} J {J} G {G} R {R} offsets {off}")
    pd = D.nan_banded(p, off.get("prob", 0), DEV)
    cd, td = D.nan_banded(k["c"], 0, DEV), D.nan_banded(k["taps"], 0, DEV)
    out = g.out(F * J * N, F32, off.get("beliefs", 0))
    joints, evidence, coupled = g.out(F * J * 3, F32), g.out(F * J, F32), g.out(F, I32)
    scratch = g.out(_lib.skeleton_couple_scratch_bytes(F, J, G, R), U8, off.get("scratch", 0))
    _lib.skeleton_couple(pd, cd, td, k["parents"], out, joints, evidence, coupled, F, N, G, R, floor, scratch=scratch)
    g.check()
    return out.view(F, J, N).cpu().numpy(), joints.view(F, J, 3).cpu().numpy(), evidence.view(F, J).cpu().numpy(), coupled.cpu().numpy()


@pytest.mark.parametrize("frames,tree,G,R,floor", D.SKELETON_CASES)
def test_skeleton_against_the_model(frames, tree, G, R, floor):
    k = skeleton_dev(frames, tree, G, R)
    want = D.skeleton_want(frames, tree, G, R, floor)
    D.skeleton_condition(want)
    got = skeleton_guarded(k, G, R, floor)
    TK.compare(k, got, want, R, f"skeleton frames {frames} {tree} G {G} R {R} floor {floor}")
    plain = TK.launch(k["prob"], k["coord"], k["taps_dev"], k["parents"], G, R, floor)
    assert all_same(got, plain), "the guarded launch and the launch into plain tensors differ"


def test_skeleton_alignment_does_not_change_a_bit():
    frames, tree, G, R, floor = D.SKELETON_ALIGN_CASE
    k = skeleton_dev(frames, tree, G, R)
    base = skeleton_guarded(k, G, R, floor)
    names = ("prob", "beliefs", "scratch")
    for moved in [(n,) for n in names] + [names]:
        got = skeleton_guarded(k, G, R, floor, offsets={n: 4 for n in moved})
        assert all_same(got, base), f"offset {moved}: the results differ from the aligned launch"


def test_skeleton_batching_at_an_odd_grid():
    """Five frames in one call walk a group of four and a group of one; each frame alone gives the same bits."""
    frames, tree, G, R, floor = D.SKELETON_BATCH_CASE
    k = skeleton_dev(frames, tree, G, R)
    want = D.skeleton_want(frames, tree, G, R, floor)
    D.skeleton_condition(want)
    five = skeleton_guarded(k, G, R, floor)
    TK.compare(k, five, want, R, "skeleton five frames at G 9")
    singles = [skeleton_guarded(k, G, R, floor, frames=slice(f, f + 1)) for f in range(frames)]
    for x in range(4):
        assert same_bits(np.concatenate([s[x] for s in singles]), five[x]), x
    # the first two frames are the two-frame case of the list
    two = D.skeleton_inputs(2, tree, G, R)
    assert same_bits(two["p"], k["p"][:2])


def correlate_guarded(a, taps, tap_row, s, G, R, scale_mul, add):
    rows, N = a.shape
    g = Guards(f"shell_correlate rows {rows} G {G} R {R}")
    ad, td = D.nan_banded(a, 0, DEV), D.nan_banded(taps, 0, DEV).view(taps.shape)
    rd, sd = D.nan_banded(tap_row, 0, DEV), D.nan_banded(s, 0, DEV)
    out = g.out(rows * N, F32)
    scratch = g.out(_lib.shell_correlate_scratch_bytes(taps.shape[0], R), U8)
    _lib.shell_correlate(ad, td, rd, sd, out, rows, G, R, scale_mul, add, scratch=scratch)
    g.check()
    plain = TK.correlate(dev(a), dev(taps), dev(tap_row), dev(s), G, R, scale_mul, add)
    got = out.view(rows, N).cpu().numpy()
    assert same_bits(got, plain), "the guarded launch and the launch into plain tensors differ"
    return got


@pytest.mark.parametrize("G,R", D.CORRELATE_CASES)
def test_shell_correlation_over_two_column_tiles(G, R):
    """Two rows with different shells at a grid of two column tiles: every voxel of the last plane, of the columns k >= 64 and 4096
    sampled ones against float64 dot products within (nnz + 2) u."""
    k = D.correlate_inputs(G, R)
    got = correlate_guarded(k["a"], k["taps"], k["tap_row"], k["s"], G, R, float(k["scale"]), 0.0)
    assert np.isfinite(got).all()
    voxels = D.correlate_voxels(G)
    for r, tr in enumerate(k["tap_row"]):
        nnz = int(np.count_nonzero(k["taps"][tr]))
        want = float(k["scale"]) * TK.dots(k["a"][r].astype(np.float64), k["taps"][tr], G, R, voxels) / float(k["s"][r])
        err = np.abs(got[r, voxels].astype(np.float64) - want)
        worst = int(np.argmax(err / want))
        print(f"shell G {G} R {R} row {r}: {nnz} taps, {len(voxels)} voxels; worst {float((err / want).max()) / U:.1f} u of the {nnz + 2} u "
              f"allowed, at voxel {voxels[worst]} (k = {voxels[worst] % G})")
        assert (want > 0).all()
        assert (err <= (nnz + 2) * U * want).all(), (f"shell G {G} R {R} row {r}: voxel {voxels[worst]} (k = {voxels[worst] % G}) is "
                                                     f"{got[r, voxels[worst]]!r}, float64 {want[worst]!r}: {float((err / want).max()) / U:.1f} u of "
                                                     f"the {nnz + 2} u allowed")


def test_shell_correlation_thin_shells_in_the_deepest_tile():
    """R = 24 (a 64 x 112 LDS tile) at G = 80, two thin shells: a few hundred taps, so the bound is a few hundred u in both column tiles."""
    G, R, bones = D.CORRELATE_DEEP
    h = D.SIDE / G
    taps = shell_taps([0.0] + [b * h for b in bones], 0.5 * h, h, R)
    a = np.ascontiguousarray(D.skeleton_inputs(1, "chain3", G, R)["p"][0, :2])
    tap_row, s, scale = np.array([1, 2], dtype=np.int32), np.array([0.37, 2.5], dtype=np.float32), np.float32(0.999)
    got = correlate_guarded(a, taps, tap_row, s, G, R, float(scale), 0.0)
    voxels = D.correlate_voxels(G)
    for r, tr in enumerate(tap_row):
        nnz = int(np.count_nonzero(taps[tr]))
        want = float(scale) * TK.dots(a[r].astype(np.float64), taps[tr], G, R, voxels) / float(s[r])
        err = np.abs(got[r, voxels].astype(np.float64) - want)
        worst = int(np.argmax(err / want))
        print(f"shell G {G} R {R} row {r}: {nnz} taps, {len(voxels)} voxels; worst {float((err / want).max()) / U:.1f} u of the {nnz + 2} u "
              f"allowed, at voxel {voxels[worst]} (k = {voxels[worst] % G})")
        assert (want > 0).all() and nnz + 2 < 1000
        assert (err <= (nnz + 2) * U * want).all(), (f"shell G {G} R {R} row {r}: voxel {voxels[worst]} (k = {voxels[worst] % G}) is "
                                                     f"{got[r, voxels[worst]]!r}, float64 {want[worst]!r}: {float((err / want).max()) / U:.1f} u of "
                                                     f"the {nnz + 2} u allowed")


def test_shell_correlation_every_voxel_at_an_odd_grid():
    G, R = D.CORRELATE_SMALL
    N, h = G ** 3, D.SIDE / G
    taps = shell_taps([0.0, 6.4 * h, 3.2 * h], 0.5 * h, h, R)
    a = np.ascontiguousarray(D.skeleton_inputs(2, "chain3", 9, 4)["p"][1, :2])
    tap_row, s = np.array([1, 2], dtype=np.int32), np.array([0.5, 1.5], dtype=np.float32)
    add = np.float32(1e-3 / N)
    got = correlate_guarded(a, taps, tap_row, s, G, R, 0.75, float(add))
    for r in (0, 1):
        nnz = int(np.count_nonzero(taps[r + 1]))
        want = 0.75 * corr_direct(a[r].astype(np.float64), taps[r + 1], G, R) / float(s[r]) + float(add)
        err = np.abs(got[r].astype(np.float64) - want)
        print(f"shell G {G} R {R} row {r}: {nnz} taps; worst {float((err / want).max()) / U:.1f} u of the {nnz + 2} u allowed")
        assert (err <= (nnz + 2) * U * want).all(), f"shell G {G} R {R} row {r}: {float((err / want).max()) / U:.1f} u of the {nnz + 2} u allowed"


# ================================================================================================================== 3. split rows
@functools.lru_cache(maxsize=None)
def split_case(G):
    """Two rows of normal logits x 3 at G^3, softmaxed by se_softargmax3d_f32: device tensors and host copies, shared."""
    rows, N = D.SPLIT_ROWS, G ** 3
    lg = D.split_logits(rows, G)
    coord = op.build_coord_volume(G, D.SIDE).reshape(N, 3).contiguous().to(DEV)
    prob, joints = torch.empty((rows, N), device=DEV), torch.empty((rows, 3), device=DEV)
    _lib.softargmax3d(dev(lg), coord, prob, joints, rows, N, 1)
    torch.cuda.synchronize()
    return {"logits": lg, "prob": prob, "coord": coord, "joints": joints, "p": prob.cpu().numpy(), "c": coord.cpu().numpy(),
            "j": joints.cpu().numpy()}


def softargmax_guarded(logits, coord, mode):
    rows, N = logits.shape
    g = Guards(f"softargmax3d rows {rows} voxels {N} mode {mode}")
    out, joints = g.out(rows * N, F32), g.out(rows * 3, F32)
    scratch = g.out(_lib.softargmax3d_scratch_elems(rows), F32)
    _lib.softargmax3d(D.nan_banded(logits, 0, DEV), D.nan_banded(coord, 0, DEV), out, joints, rows, N, mode, scratch)
    g.check()
    return {"vol": out.view(rows, N).cpu().numpy(), "joints": joints.view(rows, 3).cpu().numpy()}


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("G", D.SPLIT_GRIDS)
def test_softargmax_at_large_grids(G, mode):
    """At 128^3 in mode 1 two more rows ride along: one whose chunk 5 (8192 values) is -inf throughout and one that holds a NaN."""
    k = split_case(G)
    lg, c = k["logits"], k["c"]
    extra = G == 128 and mode == 1
    if extra:
        chunk = TV.C.sa_chunk(4, G ** 3)
        assert chunk == 8192
        lg = np.concatenate([lg, lg[:1], lg[1:]])
        lg[2, 5 * chunk:6 * chunk] = -np.inf
        lg[3, 777777] = np.nan
    got = softargmax_guarded(lg, c, mode)
    TV.check_softargmax(got, lg, c, mode, f"softargmax G {G} mode {mode}", rows_to_check=[0, 1, 2] if extra else None)
    plain = TV.run_softargmax(lg, c, mode)
    assert same_bits(got["vol"], plain["vol"]) and same_bits(got["joints"], plain["joints"])
    if extra:
        assert (got["vol"][2, 5 * chunk:6 * chunk] == 0).all() and np.isnan(got["vol"][3]).all() and np.isnan(got["joints"][3]).all()
    elif mode == 1:
        assert same_bits(got["vol"], k["p"]) and same_bits(got["joints"], k["j"])


@pytest.mark.parametrize("G", D.SPLIT_GRIDS)
def test_joint_stats_at_large_grids(G):
    k = split_case(G)
    rows, N = k["p"].shape
    g = Guards(f"joint_stats G {G}")
    stats, idx = g.out(rows * 12, F32), g.out(rows, I32)
    scratch = g.out(_lib.joint_stats_scratch_elems(rows), F32)
    _lib.joint_stats(D.nan_banded(k["p"], 0, DEV), D.nan_banded(k["c"], 0, DEV), D.nan_banded(k["j"], 0, DEV), stats, idx, rows, N,
                     scratch=scratch)
    g.check()
    stats, idx = stats.view(rows, 12).cpu().numpy(), idx.cpu().numpy()
    plain = TS.launch(k["prob"], k["coord"], k["joints"])
    assert same_bits(stats, plain[0]) and np.array_equal(idx, plain[1])
    cov, ent = TS.model(k["p"], k["c"], k["j"])
    assert np.isfinite(stats).all()
    TS.check_peak(stats, idx, k["p"], k["c"])
    TS.check_cov(stats, cov, f"joint_stats G {G}")
    TS.check_entropy(stats, ent, f"joint_stats G {G}")
    TS.check_sigma(stats)


@pytest.mark.parametrize("G", D.SPLIT_GRIDS)
def test_masked_softargmax_at_large_grids(G):
    """Two frames of one row each under random masks; then frame 1 blocked throughout."""
    k = split_case(G)
    rows, N = k["p"].shape
    rng = np.random.default_rng(77 * G + rows)
    f = (rng.random((rows, N)) < 0.5).astype(np.uint8)
    f[f == 1] = rng.choice(np.array([1, 1, 1, 255, 2], dtype=np.uint8), size=int((f == 1).sum()))      # any non-zero byte is free

    def run(free):
        g = Guards(f"softargmax3d_masked G {G}")
        out, idx = g.out(rows * 8, F32), g.out(rows, I32)
        scratch = g.out(_lib.softargmax3d_masked_scratch_elems(rows), F32)
        _lib.softargmax3d_masked(D.nan_banded(k["p"], 0, DEV), D.nan_banded(k["c"], 0, DEV), D.nan_banded(free, 0, DEV), out, idx, rows,
                                 1, N, scratch=scratch)
        g.check()
        out, idx = out.view(rows, 8).cpu().numpy(), idx.cpu().numpy()
        plain = TC.launch(k["prob"], k["coord"], dev(free), 1)
        assert same_bits(out, plain[0]) and np.array_equal(idx, plain[1])
        return out, idx

    out, idx = run(f)
    want, want_idx, mag = SCM.masked_reduction(k["p"], k["c"], f, 1)
    assert np.isfinite(out).all() and (f[np.arange(rows), idx] != 0).all()
    TC.check_peak(out, idx, want, want_idx, k["c"])
    TC.check_sums(out, want, mag, f"masked G {G}")
    blocked = f.copy()
    blocked[1] = 0
    out2, idx2 = run(blocked)
    assert same_bits(out2[:1], out[:1]) and idx2[0] == idx[0]
    assert (out2[1, :5] == 0).all() and not np.signbit(out2[1, :5]).any() and np.isnan(out2[1, 5:8]).all() and idx2[1] == -1


def modes_guarded(prob, coord, G, K, radius):
    rows = prob.shape[0]
    g = Guards(f"joint_modes G {G} K {K} radius {radius}")
    modes, index, count, total = g.out(rows * K * 8, F32), g.out(rows * K, I32), g.out(rows, I32), g.out(rows, I32)
    scratch = g.out(_lib.joint_modes_scratch_bytes(rows, G, K), U8)
    _lib.joint_modes(D.nan_banded(prob, 0, DEV), D.nan_banded(coord, 0, DEV), modes, index, count, total, rows, G ** 3, G, K, radius, 0.0,
                     scratch=scratch)
    g.check()
    got = (modes.view(rows, K, 8).cpu().numpy(), index.view(rows, K).cpu().numpy(), count.cpu().numpy(), total.cpu().numpy())
    TM.assert_same(got, TM.launch(dev(prob), dev(coord), G, K, radius), "guarded against plain")
    return got


@pytest.mark.parametrize("rows,G,K,radius", D.MODES_CASES)
def test_joint_modes_at_large_grids(rows, G, K, radius):
    k = split_case(G)
    assert rows == k["p"].shape[0]
    got = modes_guarded(k["p"], k["c"], G, K, radius)
    want = joint_modes_model(k["p"], k["c"], G, K, radius)
    print(f"joint_modes G {G} K {K} radius {radius}: totals {want[3].tolist()}")
    assert (want[3] > K).all()
    TM.assert_same(got, want, f"joint_modes G {G} K {K} radius {radius}")


def test_joint_modes_ties_across_a_band_and_a_slab_at_128():
    """128^3: 32 lanes per row, bands of 8 j-rows, slabs of 4 i-planes.  Row 0 holds an equal pair at j = 7 | 8, row 1 one at
    i = 3 | 4, above everything else: one mode each, the lower index."""
    G = 128
    k = split_case(G)
    p = k["p"].copy()
    v = TM.above(p[0])
    assert v > p[1].max()
    pairs = [(TM.flat(G, 10, 7, 20), TM.flat(G, 10, 8, 20)), (TM.flat(G, 3, 40, 50), TM.flat(G, 4, 40, 50))]
    for r, (lo, hi) in enumerate(pairs):
        p[r, lo] = p[r, hi] = v
    got = modes_guarded(p, k["c"], G, 4, 2)
    want = joint_modes_model(p, k["c"], G, 4, 2)
    assert got[1][:, 0].tolist() == [pairs[0][0], pairs[1][0]] and not np.isin([pairs[0][1], pairs[1][1]], got[1]).any()
    TM.assert_same(got, want, "ties at 128^3")


# ================================================================================================================== 6. the module at 96^3
def test_module_heads_at_96_equal_the_library_calls():
    G, J = 96, 15
    N = G ** 3
    cfg = load_config()
    cfg.model.volume_size = G
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    net = net.to(DEV).eval()
    img, depth = synth.make_inputs(3200 + G, 1, "floor")
    with torch.no_grad():
        kp, _, vols, _ = net(img.to(DEV), net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth.to(DEV))
    torch.cuda.synchronize()
    kp, vols = kp.clone(), vols.clone()
    assert tuple(vols.shape) == (1, J, G, G, G)
    coord = net.coord_volumes[0].reshape(N, 3).float().contiguous().to(DEV)
    flat = vols.reshape(J, N)

    stats = net.joint_statistics(vols, kp)
    raw, raw_idx = TS.launch(flat, coord, kp.reshape(J, 3).contiguous())
    assert np.array_equal(stats["peak_index"].cpu().numpy().reshape(J), raw_idx)
    for key, cols in (("entropy", 6), ("peak_prob", 7), ("sigma", 11), ("peak_coord", slice(8, 11))):
        assert same_bits(stats[key].cpu().numpy().reshape(raw[:, cols].shape), raw[:, cols]), key
    assert same_bits(stats["cov"].cpu().numpy().reshape(J, 9), raw[:, [0, 3, 4, 3, 1, 5, 4, 5, 2]])

    modes = net.joint_modes(vols, k=4, radius=2)
    rm, ri, rc, rt = TM.launch(flat, coord, G, 4, 2)
    assert np.array_equal(modes["index"].cpu().numpy().reshape(J, 4), ri) and np.array_equal(modes["count"].cpu().numpy().reshape(J), rc)
    assert np.array_equal(modes["total"].cpu().numpy().reshape(J), rt)
    for key, cols in (("peak_prob", 0), ("mass", 1), ("peak_coord", slice(5, 8))):
        assert same_bits(modes[key].cpu().numpy().reshape(rm[:, :, cols].shape), rm[:, :, cols]), key
    assert torch.equal(modes["index"][..., 0], stats["peak_index"])

    f = net.volume_filter()
    assert f.radius == 15 and f.grid == G
    res = [f.step(vols, return_beliefs=True) for _ in range(2)]
    torch.cuda.synchronize()
    taps = gaussian_taps(0.10, f.radius, net.cuboid_side / G)
    gb, gj, ge, gr, gs = TF.launch(torch.cat([flat[None], flat[None]]), coord, dev(taps), G, f.radius, 1e-3)
    assert same_bits(torch.cat([r["beliefs"] for r in res]).reshape(2, J, N).cpu().numpy(), gb)
    assert same_bits(torch.cat([r["joints"] for r in res]).cpu().numpy(), gj)
    assert same_bits(torch.cat([r["evidence"] for r in res]).cpu().numpy(), ge)
    assert np.array_equal(torch.cat([r["restarted"] for r in res]).cpu().numpy(), gr != 0) and gr[0].all() and not gr[1].any()
    assert same_bits(f.state.reshape(J, N).cpu().numpy(), gs)
    del res, gb

    bones = np.linspace(0.15, 0.40, 14)
    sp = net.skeleton_prior(bones)
    assert isinstance(sp, SkeletonPrior) and sp.radius == 24
    r = sp.couple(vols, joints=kp, return_beliefs=True)
    torch.cuda.synchronize()
    taps = shell_taps(np.concatenate([[0.0], bones]), 0.03, net.cuboid_side / G, sp.radius)
    gb, gj, ge, gc = TK.launch(flat[None], coord, dev(taps), TK.TREE, G, sp.radius, 1e-3)
    assert same_bits(r["beliefs"].reshape(1, J, N).cpu().numpy(), gb) and same_bits(r["joints"].cpu().numpy(), gj)
    assert same_bits(r["evidence"].cpu().numpy(), ge) and np.array_equal(r["coupled"].cpu().numpy(), gc != 0)
    print(f"module at 96^3: coupled {gc.tolist()}, skeleton evidence x N {ge.min() * N:.3g} .. {ge.max() * N:.3g}")
    assert np.isfinite(gj).all()
