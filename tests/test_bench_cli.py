"""CPU: bench.py's --dump-outputs writer and the options that need --full (nothing here touches a GPU)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float32_and_a_fixed_bounded_sample(tmp_path):
    """The headline shape (B=8, 64^3): joints and features whole, volumes (31 M elements) as the stratified sample the docstring
    describes - the same positions in every call - and the three files together within 64 MB."""
    import bench
    g = torch.Generator().manual_seed(5)
    joints = torch.randn((8, 15, 3), generator=g)
    feats = torch.randn((8, 32, 64, 64), generator=g)
    vols = torch.rand((8, 15, 64, 64, 64), generator=g)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), (joints, feats, vols))
    names = ("joints", "features", "volumes")
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["joints"], joints.numpy()) and np.array_equal(got["features"], feats.numpy())
    n, k = vols.numel(), bench.DUMP_SAMPLE
    stride = n // k
    idx = np.arange(k) * stride + np.random.default_rng(0).integers(0, stride, k)
    assert got["volumes"].shape == (k,) and np.array_equal(got["volumes"], vols.reshape(-1).numpy()[idx])
    for name in names:
        assert np.array_equal(got[name], np.load(tmp_path / "b" / (name + ".npy")))
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in names) <= 64 << 20
    assert 3 * 4 * k + 3 * 4096 <= 64 << 20        # the bound for any shape: no array is written with more than DUMP_SAMPLE elements


def test_profiling_pass_options_need_full():
    """--dump-kernel-events / --dump-launch-order come from the per-launch timing pass, which only a --full run makes: without
    --full the run stops at argument parsing (exit 2) and says so."""
    for opt in (["--dump-kernel-events"], ["--dump-launch-order", os.devnull]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + opt, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--full" in r.stderr, (r.returncode, r.stderr[-500:])
