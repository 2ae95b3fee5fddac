"""GPU: the trajectory sampler (csrc/volume_sample.hip, se_volume_sample_f32) against its numpy model (tests/volume_sampler_model.py),
BIT FOR BIT in ``index``, ``kind`` and ``next``: the definition is float64 with one rounding per operation, sequential sums and
Philox4x32-10, so there is one right answer and no tolerance.  Then its independence of how the frames and the samples are cut into
calls, NaN frames, denormal and sparse beliefs, the argument gate, the public method and the command line.

Inputs and forward pass: those of tests/test_gpu_volume_smoother.py (``sequence``, ``forward``, ``filtered``): the filter's float32
beliefs and restart flags go to the kernel and to the model alike.
"""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD
from sceneego_amd import _lib, op, synth
from sceneego_amd.volume_smoother import VolumeSmoother
from test_gpu_volume_smoother import filtered, forward, same_bits, sequence
from volume_filter_cases import SIDE
from volume_sampler_model import FRESH, JUMP, STEP, sample_in_chunks, volume_sampler_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# rows, G, R, floor, T, S
CASES = [
    (1, 2, 1, 1e-3, 3, 8),
    (1, 8, 0, 0.0, 5, 8),
    (1, 8, 2, 1e-3, 5, 8),
    (3, 6, 5, 1e-3, 4, 8),          # R = G - 1: every window clipped on both sides
    (4, 10, 3, 0.3, 5, 8),          # jumps really occur
    (15, 16, 5, 1e-3, 3, 8),
    (2, 24, 8, 1.0, 4, 4),
    (15, 64, 10, 1e-3, 3, 4),       # the production shape
    (1, 128, 16, 1e-3, 2, 2),
]


def bound(prob, S):
    return 5.0 * np.sqrt(prob * (1.0 - prob) / S) + 1.0 / S


def sample(belief, restarted, taps_dev, G, R, floor, S, cuts=None, seed=0, first_sample=0):
    """The _lib-level sampler over ``belief`` [T, rows, N] in calls of ``cuts`` frames each (in frame order; issued last chunk first,
    ``next`` and ``have_link`` carried).  Host arrays: index and kind [S, T, rows], next [S, rows]."""
    T, rows, N = belief.shape
    cuts = (T,) if cuts is None else tuple(cuts)
    assert sum(cuts) == T
    index = torch.full((S, T, rows), -7, device=DEV, dtype=torch.int32)
    kind = torch.full((S, T, rows), -7, device=DEV, dtype=torch.int32)
    nxt = torch.full((S, rows), -7, device=DEV, dtype=torch.int32)
    starts = np.concatenate([[0], np.cumsum(cuts)]).tolist()
    for i in range(len(cuts) - 1, -1, -1):
        t0, t1 = starts[i], starts[i + 1]
        link = None if t1 == T else (restarted[t1] == 0).to(torch.int32)
        idx = torch.full((S, t1 - t0, rows), -7, device=DEV, dtype=torch.int32)
        knd = torch.full((S, t1 - t0, rows), -7, device=DEV, dtype=torch.int32)
        _lib.volume_sample(belief[t0:t1], restarted[t0:t1], taps_dev, nxt, idx, knd, t1 - t0, rows, N, G, R, floor, S,
                           first_sample=first_sample, first_frame=t0, seed=seed, have_link=link)
        index[:, t0:t1], kind[:, t0:t1] = idx, knd
    torch.cuda.synchronize()
    return {"index": index.cpu().numpy(), "kind": kind.cpu().numpy(), "next": nxt.cpu().numpy()}


def equal(got, want, label=""):
    for key in ("index", "kind", "next"):
        same = np.array_equal(got[key], want[key])
        assert same, f"{label}: {key} differs in {int((got[key] != want[key]).sum())} of {got[key].size} entries"


# ------------------------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("rows,G,R,floor,T,S", CASES)
def test_bit_for_bit_against_the_model(rows, G, R, floor, T, S):
    k = filtered(rows, G, R, floor, T)
    got = sample(k["belief"], k["restarted"], k["taps_dev"], G, R, floor, S, seed=0)
    want = volume_sampler_model(k["b"], k["rs"], k["taps"], G, floor, S, seed=0)
    equal(got, want, f"rows {rows} G {G} R {R} floor {floor}")
    assert (got["index"] < G ** 3).all() and np.array_equal(got["next"], got["index"][:, 0])
    if G == 2:
        # the filter tests' logits are constant at G = 2 (both voxels of an axis lie as far from the bump) and standardise to NaN: the
        # case holds the kernel to the model where every frame is invalid; test_the_smallest_grid below draws at G = 2
        assert np.isnan(k["b"]).all() and (got["index"] == -1).all() and (got["kind"] == FRESH).all()
        return
    assert (got["index"] >= 0).all()
    assert (got["kind"][:, T - 1] == FRESH).all() and (got["kind"][:, :T - 1] != FRESH).all()
    kinds = set(np.unique(got["kind"][:, :T - 1]).tolist())
    if floor == 0.3:
        assert kinds == {STEP, JUMP}                            # jumps really occur, and steps beside them
    if floor == 1.0:
        assert kinds == {JUMP}
    if floor == 0.0:
        assert kinds == {STEP}
    print(f"rows {rows} G {G} R {R} floor {floor}: {S * T * rows} draws equal; kinds {sorted(kinds)}")


def test_the_smallest_grid():
    """G = 2, R = 1 on beliefs of its own (see the first case above): every window is clipped to the two voxels of an axis."""
    rows, G, R, T, S = 3, 2, 1, 4, 64
    rng = np.random.default_rng(12)
    b = rng.random((T, rows, 8))
    b = (b / b.sum(axis=2, keepdims=True)).astype(np.float32)
    rs = np.zeros((T, rows), dtype=np.int32)
    rs[0] = 1
    taps = np.array([0.25, 0.5, 0.25], dtype=np.float32)
    for floor in (1e-3, 0.3):
        got = sample(torch.from_numpy(b).to(DEV), torch.from_numpy(rs).to(DEV), torch.from_numpy(taps).to(DEV), G, R, floor, S, seed=1)
        equal(got, volume_sampler_model(b, rs, taps, G, floor, S, seed=1), f"G 2 floor {floor}")
        assert (got["index"] >= 0).all() and (got["index"] < 8).all() and len(np.unique(got["index"])) == 8
    assert {STEP, JUMP, FRESH} == set(np.unique(got["kind"]).tolist())


def test_asymmetric_taps():
    """The window of y is x = y + d with w[d] as given: no reversal.  With the taps reversed the model draws other voxels here."""
    rows, G, R, floor, T, S = 2, 8, 2, 1e-3, 4, 32
    k = sequence(rows, G, R, T)
    w = np.array([0.05, 0.10, 0.20, 0.30, 0.35], dtype=np.float64)
    taps = (w / w.sum()).astype(np.float32)
    taps_dev = torch.from_numpy(taps).to(DEV)
    belief, restarted = forward(k["prob"], k["coord"], taps_dev, G, R, floor)
    b, rs = belief.cpu().numpy(), restarted.cpu().numpy()
    got = sample(belief, restarted, taps_dev, G, R, floor, S, seed=4)
    equal(got, volume_sampler_model(b, rs, taps, G, floor, S, seed=4), "asymmetric taps")
    wrong = volume_sampler_model(b, rs, np.ascontiguousarray(taps[::-1]), G, floor, S, seed=4)
    assert not np.array_equal(wrong["index"], got["index"])


def test_denormal_and_sparse_beliefs():
    rows, G, R, floor, T, S = 4, 10, 3, 1e-3, 5, 16
    k = filtered(rows, G, R, floor, T)
    # scaled into the float32 denormals: the peak near 2^-130, most of the volume flushed to exact zeros by the scaling itself
    t = (k["b"].astype(np.float64) * 2.0 ** -128).astype(np.float32)       # rounded on the host: gradual underflow
    tiny = torch.from_numpy(t).to(DEV)
    assert (t[t > 0] < 2.0 ** -126).all() and (t > 0).any(axis=2).all() and (t == 0).any()
    got = sample(tiny, k["restarted"], k["taps_dev"], G, R, floor, S, seed=5)
    equal(got, volume_sampler_model(t, k["rs"], k["taps"], G, floor, S, seed=5), "denormal beliefs")
    for f in range(T):
        for row in range(rows):
            x = got["index"][:, f, row]
            assert (x >= 0).all() and (t[f, row, x] > 0).all()
    # a few non-zero cells per row
    gen = torch.Generator(device="cpu").manual_seed(3)
    mask = (torch.rand(k["belief"].shape, generator=gen) > 0.99).to(DEV)
    mask.scatter_(2, k["belief"].argmax(dim=2, keepdim=True), True)        # the peak of every row stays
    sparse = (k["belief"] * mask).contiguous()
    sp = sparse.cpu().numpy()
    assert ((sp > 0).sum(axis=2) >= 1).all() and (sp == 0).mean() > 0.98
    got = sample(sparse, k["restarted"], k["taps_dev"], G, R, 0.3, S, seed=6)
    equal(got, volume_sampler_model(sp, k["rs"], k["taps"], G, 0.3, S, seed=6), "sparse beliefs")
    for f in range(T):
        for row in range(rows):
            x = got["index"][:, f, row]
            assert (x >= 0).all() and (sp[f, row, x] > 0).all()


def test_a_nan_frame():
    rows, G, R, floor, T, S = 15, 16, 5, 1e-3, 5, 8
    k = filtered(rows, G, R, floor, T)
    clean = sample(k["belief"], k["restarted"], k["taps_dev"], G, R, floor, S, seed=2)
    prob = k["prob"].clone()
    prob[2, 7, 1234] = float("nan")
    belief, restarted = forward(prob, k["coord"], k["taps_dev"], G, R, floor)
    rs = restarted.cpu().numpy()
    assert rs[:, 7].tolist() == [1, 0, 1, 1, 0]
    got = sample(belief, restarted, k["taps_dev"], G, R, floor, S, cuts=(3, 2), seed=2)
    equal(got, volume_sampler_model(belief.cpu().numpy(), rs, k["taps"], G, floor, S, seed=2), "NaN frame")
    assert (got["index"][:, 2, 7] == -1).all() and (got["kind"][:, [1, 2, 4], 7] == FRESH).all()
    assert (got["kind"][:, [0, 3], 7] != FRESH).all() and (got["index"][:, [0, 1, 3, 4], 7] >= 0).all()
    others = [r for r in range(rows) if r != 7]
    assert np.array_equal(got["index"][:, :, others], clean["index"][:, :, others])
    assert np.array_equal(got["kind"][:, :, others], clean["kind"][:, :, others])
    # an invalid voxel handed over in `next` links nothing: the call's last frame is a fresh draw for that chain alone
    nxt = torch.from_numpy(clean["index"][:, 3].copy()).to(DEV)
    nxt[1, 3], nxt[2, 4] = -1, G ** 3
    idx = torch.empty((S, 3, rows), device=DEV, dtype=torch.int32)
    knd = torch.empty_like(idx)
    _lib.volume_sample(k["belief"][:3], k["restarted"][:3], k["taps_dev"], nxt, idx, knd, 3, rows, G ** 3, G, R, floor, S, seed=2,
                       have_link=torch.ones(rows, device=DEV, dtype=torch.int32))
    torch.cuda.synchronize()
    knd = knd.cpu().numpy()
    fresh = np.zeros((S, rows), dtype=bool)
    fresh[1, 3] = fresh[2, 4] = True
    assert np.array_equal(knd[:, 2] == FRESH, fresh)
    keep = np.broadcast_to(~fresh[:, None, :], (S, 3, rows))     # every other chain is the clean one
    assert np.array_equal(idx.cpu().numpy()[keep], clean["index"][:, :3][keep]) and np.array_equal(knd[keep], clean["kind"][:, :3][keep])


# ------------------------------------------------------------------------------------------------------------------ 2. cuts, runs
def test_results_do_not_depend_on_how_frames_and_samples_are_cut():
    rows, G, R, floor, T, S = 4, 10, 3, 0.3, 5, 16
    k = filtered(rows, G, R, floor, T)
    args = (k["belief"], k["restarted"], k["taps_dev"], G, R, floor)
    whole = sample(*args, S, seed=9)
    cuts = [c for n in range(2, 6) for c in _compositions(T, n)]
    assert len(cuts) == 15                                      # every cut of five frames into two or more calls
    for c in cuts:
        equal(sample(*args, S, cuts=c, seed=9), whole, f"cuts {c}")
    lo, hi = sample(*args, 8, seed=9), sample(*args, 8, seed=9, first_sample=8, cuts=(2, 3))
    for key in ("index", "kind", "next"):
        assert np.array_equal(np.concatenate([lo[key], hi[key]]), whole[key]), key
    equal(sample(*args, S, seed=9), whole, "a second run")     # two runs, bitwise
    assert not np.array_equal(sample(*args, S, seed=10)["index"], whole["index"])
    equal(whole, sample_in_chunks(k["b"], k["rs"], k["taps"], G, floor, S, (2, 3), seed=9), "the model in chunks")
    # a 64-bit seed reaches the key's second word
    big = sample(*args, 4, seed=(5 << 32) | 9)
    equal(big, volume_sampler_model(k["b"], k["rs"], k["taps"], G, floor, 4, seed=(5 << 32) | 9), "64-bit seed")
    assert not np.array_equal(big["index"], whole["index"][:4])


def _compositions(total, parts):
    if parts == 1:
        return [(total,)]
    return [(first,) + rest for first in range(1, total - parts + 2) for rest in _compositions(total - first, parts - 1)]


# ------------------------------------------------------------------------------------------------------------------ 3. arguments
def test_bad_arguments_raise_and_do_not_launch():
    rows, G, R, T, floor, S = 4, 10, 3, 5, 1e-3, 4
    k = filtered(rows, G, R, floor, T)
    N = G ** 3
    belief, restarted = k["belief"][:2].contiguous(), k["restarted"][:2].contiguous()
    nxt = torch.full((S, rows), -7, device=DEV, dtype=torch.int32)
    index = torch.full((S, 2, rows), -7, device=DEV, dtype=torch.int32)
    kind = torch.full((S, 2, rows), -7, device=DEV, dtype=torch.int32)

    def call(**kw):
        a = {"belief": belief, "restarted": restarted, "taps": k["taps_dev"], "next_voxel": nxt, "index": index, "kind": kind,
             "frames": 2, "rows": rows, "voxels": N, "grid": G, "radius": R, "floor": floor, "samples": S}
        a.update(kw)
        return _lib.volume_sample(**a)

    for kw in ({"radius": 17}, {"radius": -1}, {"radius": G}, {"floor": -0.1}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0},
               {"frames": 3}, {"rows": 0}, {"grid": G + 1}, {"voxels": N + 1}, {"grid": 1, "voxels": 1, "radius": 0},
               {"samples": 0}, {"samples": S + 1}, {"first_sample": -1}, {"first_sample": 2 ** 32 - S + 1}, {"first_frame": -1},
               {"first_frame": 2 ** 32 - 1}, {"seed": -1}, {"seed": 2 ** 64},
               {"belief": belief.cpu()}, {"belief": belief.double()}, {"belief": belief[:, :, ::2]}, {"belief": belief[:1]},
               {"restarted": restarted != 0}, {"restarted": restarted[:1]}, {"taps": k["taps_dev"][:-1]}, {"taps": k["taps"]},
               {"next_voxel": nxt[:-1]}, {"next_voxel": nxt.long()}, {"index": index[:, :1]}, {"kind": kind.float()}, {"kind": index},
               {"have_link": torch.ones(rows, device=DEV)}, {"have_link": torch.ones(rows + 1, device=DEV, dtype=torch.int32)},
               {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    torch.cuda.synchronize()
    assert (index == -7).all() and (kind == -7).all() and (nxt == -7).all()                # nothing was launched
    # the C entry point refuses on its own what the wrapper checks first
    lib = _lib.load()
    ws = torch.empty(_lib.volume_sample_scratch_bytes(2, rows, G) + 8, device=DEV, dtype=torch.uint8)
    P = _lib._ptr

    def raw(radius=R, floor=1e-3, frames=2, grid=G, voxels=N, samples=S, first_sample=0, first_frame=0, scratch_bytes=ws.numel(),
            nxt=nxt, index=index, scratch=ws, rows=rows):
        return lib.se_volume_sample_f32(P(belief), P(restarted), P(k["taps_dev"]), P(nxt), P(index), P(kind), P(scratch), scratch_bytes,
                                        frames, rows, voxels, grid, radius, floor, samples, first_sample, first_frame, 0, 0, None,
                                        _lib._stream())
    assert raw(radius=17) == raw(radius=G) == raw(floor=2.0) == raw(floor=float("nan")) == raw(frames=0) == raw(voxels=N + 4) \
        == raw(grid=129) == raw(samples=0) == raw(first_sample=-1) == raw(first_sample=2 ** 32 - S + 1) == raw(first_frame=2 ** 32 - 1) \
        == raw(rows=0) == raw(rows=65536) == -1
    assert raw(scratch_bytes=_lib.volume_sample_scratch_bytes(2, rows, G) - 1) == -1 and raw(nxt=None) == -1 and raw(index=None) == -1
    assert raw(scratch=ws[4:]) == -1                            # the float64 sums want 8-byte alignment
    torch.cuda.synchronize()
    assert (index == -7).all() and (kind == -7).all() and (nxt == -7).all()
    assert raw() == 0 and raw(first_sample=2 ** 32 - S, first_frame=2 ** 32 - 2) == 0
    torch.cuda.synchronize()
    assert (index >= 0).all() and (kind >= 0).all() and (nxt >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ 4. public surface
def make_smoother(k, G, R, floor, **kw):
    return VolumeSmoother(k["coord"], G, SIDE, sigma=R * (SIDE / G) / 3.0, radius=R, floor=floor, **kw)


def test_the_public_method_draws_from_the_smoothed_marginals_and_leaves_finish_alone():
    rows, G, R, floor, T, S = 2, 4, 2, 1e-2, 4, 4096
    N = G ** 3
    k = filtered(rows, G, R, floor, T)
    vols = k["prob"].view(T, rows, G, G, G)
    s = make_smoother(k, G, R, floor)
    given = torch.zeros((2, rows, 3), device=DEV)
    s.push(vols[:2], joints=given)
    s.push(vols[2:])
    res = s.sample(samples=S, seed=0)
    again = s.sample(samples=16, seed=0)                        # nothing was consumed; fewer samples are the first of more
    assert s.frames_stored == T
    fin = s.finish(return_beliefs=True)
    torch.cuda.synchronize()
    assert tuple(res) == ("index", "coord", "kind", "valid", "mean", "spread", "shift")
    assert tuple(res["index"].shape) == (S, T, rows) == tuple(res["kind"].shape) == tuple(res["valid"].shape)
    assert tuple(res["coord"].shape) == (S, T, rows, 3) and tuple(res["mean"].shape) == (T, rows, 3)
    assert tuple(res["spread"].shape) == (T, rows) == tuple(res["shift"].shape)
    assert res["index"].dtype == torch.int32 and res["valid"].dtype == torch.bool and bool(res["valid"].all())
    assert torch.equal(again["index"], res["index"][:16]) and torch.equal(again["kind"], res["kind"][:16])
    index = res["index"].cpu().numpy()
    # the class is the library call, which is the model
    want = volume_sampler_model(k["b"], k["rs"], k["taps"], G, floor, S, seed=0)
    assert np.array_equal(index, want["index"]) and np.array_equal(res["kind"].cpu().numpy(), want["kind"])
    # the frequencies against the smoothed beliefs finish() returns afterwards
    gamma = torch.cat(fin["beliefs"]).reshape(T, rows, N).cpu().numpy().astype(np.float64)
    worst = 0.0
    for t in range(T):
        for row in range(rows):
            f = np.bincount(index[:, t, row], minlength=N) / S
            worst = max(worst, float((np.abs(f - gamma[t, row]) - bound(gamma[t, row], S)).max()))
    assert worst <= 0.0, f"a frequency is {worst:.3e} beyond five sigma of the smoothed belief"
    # coordinates, mean, spread and shift are what they say
    c = k["c"].astype(np.float64)
    coord = res["coord"].cpu().numpy()
    assert same_bits(coord, k["c"][index])
    mean = c[index].mean(axis=0)
    spread = np.sqrt(((c[index] - mean) ** 2).sum(axis=(0, 3)) / (S - 1))
    assert np.allclose(res["mean"].cpu().numpy(), mean, rtol=0, atol=1e-5) and np.allclose(res["spread"].cpu().numpy(), spread, rtol=1e-4)
    shift = res["shift"].cpu().numpy()
    assert np.allclose(shift[:2], np.linalg.norm(mean[:2], axis=-1), atol=1e-5) and np.isnan(shift[2:]).all()
    frames = op.volume_samples_to_numpy(res)
    assert len(frames) == T and tuple(frames[0]) == ("index", "coord", "kind", "valid", "mean", "spread", "shift")
    assert frames[1]["index"].shape == (S, rows) and frames[1]["coord"].shape == (S, rows, 3) and frames[1]["spread"].shape == (rows,)
    assert np.array_equal(frames[3]["index"], index[:, 3])
    # finish() after sample() returns the bits of a finish() without
    ref = make_smoother(k, G, R, floor)
    ref.push(vols[:2], joints=given)
    ref.push(vols[2:])
    want_fin = ref.finish(return_beliefs=True)
    torch.cuda.synchronize()
    assert tuple(fin) == tuple(want_fin)
    for key in fin:
        if key == "beliefs":
            for a, b in zip(fin[key], want_fin[key]):
                assert same_bits(a.cpu().numpy(), b.cpu().numpy())
        elif fin[key].dtype == torch.bool:
            assert torch.equal(fin[key], want_fin[key])
        else:
            assert same_bits(fin[key].cpu().numpy(), want_fin[key].cpu().numpy()), key
    # nothing is stored any more
    with pytest.raises(ValueError, match="nothing is stored"):
        s.sample()
    s.push(vols[:1])
    s.reset()
    with pytest.raises(ValueError, match="nothing is stored"):
        s.sample()
    # one sample: no spread
    s.push(vols[:3])
    one = s.sample(samples=1, seed=3, stream=torch.cuda.Stream(device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(one["spread"]).all()) and "shift" not in one and bool(torch.isfinite(one["mean"]).all())


# ------------------------------------------------------------------------------------------------------------------ 5. command line
def test_run_sequence_sample_output(tmp_path, capsys):
    import evaluate
    import run_sequence
    demo_exr = os.path.join(GOLD, "demo", "img_001000.jpg.exr")
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 3, [demo_exr], estimated_depth_name="est_depth", seed=5)
    cfg_path = tmp_path / "batch2.yaml"
    with open(os.path.join(os.path.dirname(GOLD), "..", "experiments", "sceneego", "test", "sceneego.yaml")) as f:
        text = f.read()
    assert text.count("  batch_size: 8\n") == 1
    cfg_path.write_text(text.replace("  batch_size: 8\n", "  batch_size: 2\n"))
    common = ["--config", str(cfg_path), "--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth",
              "--weights", "synthetic"]
    res = run_sequence.main(common + ["--smooth_output", str(tmp_path / "s" / "smoothed.pkl"),
                                      "--sample_output", str(tmp_path / "s" / "samples.pkl"), "--samples", "8", "--sample_seed", "11"])
    out = capsys.readouterr().out
    line = [text for text in out.splitlines() if text.startswith("trajectory samples")]
    assert len(line) == 1 and "mean spread" in line[0] and "best-of-8 mpjpe" in line[0] and "smoothed" in line[0]
    with open(tmp_path / "s" / "samples.pkl", "rb") as f:
        frames = pickle.load(f)
    assert len(frames) == 3 and tuple(frames[0]) == ("index", "coord", "kind", "valid", "mean", "spread", "shift")
    for t, fr in enumerate(frames):
        assert fr["index"].shape == (8, 15) and fr["coord"].shape == (8, 15, 3) and fr["valid"].all() and np.isfinite(fr["spread"]).all()
        assert (fr["kind"] == FRESH).all() == (t == 2)
    assert np.isfinite(res["best_of_n_mpjpe"]) and np.isfinite(res["mean_sample_spread"]) and len(res["samples"]) == 3
    assert len(res["smoothed"]) == 3 and np.isfinite(res["smoothed_mpjpe"])
    with pytest.raises(SystemExit):
        run_sequence.main(common + ["--samples", "8"])
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((3, 15, 3)), f)
    ev = evaluate.main(["--pred_dir", str(tmp_path / "s" / "smoothed.pkl"), "--gt", str(tmp_path / "gt.pkl"),
                        "--samples", str(tmp_path / "s" / "samples.pkl")])
    out = capsys.readouterr().out
    assert "best-of-8 MPJPE" in out and "spearman(error, spread)" in out
    a = ev["samples"]
    assert a["samples_per_joint"] == 8 and a["draws"] == a["valid_draws"] == 3 * 8 * 15
    assert np.isfinite(a["best_of_n_mpjpe"]) and np.isfinite(a["mean_sample_spread"])
    assert -1.0 <= a["spearman_error_spread"] <= 1.0 or np.isnan(a["spearman_error_spread"])
