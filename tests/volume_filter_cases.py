"""Inputs of the grid Bayes filter tests: logits of a moving Gaussian bump per row, the taps and a host softmax.

Per row one bump (1-3 voxels wide up to 32^3, G / 32 times that above) whose centre takes a random walk of at most max(R / 2, 0.5)
voxels per axis per frame (inside the grid); odd rows get a second, static bump: the two-lobed volumes the filter is for.  The logits
of every frame are standardised to a std of 5-10 (one scale per row for the whole sequence) plus 0.01 noise, as the joint-mode tests
build theirs.  The GPU tests softmax them with
se_softargmax3d_f32 on the device; the host tests with ``softmax32`` below.
"""
import numpy as np

from sceneego_amd.volume_filter import gaussian_taps

SIDE = 2.0          # metres: the cuboid of the test grids


def taps_for(G, R):
    """Taps of radius ``R`` on a G^3 grid of side SIDE with sigma = R h / 3 (so that R is the 3-sigma truncation); R = 0: [1]."""
    h = SIDE / G
    return gaussian_taps(R * h / 3.0, R, h)


def make_logits(T, rows, G, R, seed):
    """float32 [T, rows, G^3]."""
    rng = np.random.default_rng(seed)
    ax = np.arange(G, dtype=np.float64)
    step = max(R / 2.0, 0.5)
    wide = max(1.0, G / 32.0)       # bumps of 1-3 voxels at 32^3 and below, as wide in proportion above: at 128^3 a bump of 1-3 voxels
    #                                 under logits of this scale is one-hot after the softmax and would test one voxel of the blur
    out = np.empty((T, rows, G, G, G), dtype=np.float32)

    def bump(c, w):
        g = [np.exp(-(ax - c[a]) ** 2 / (2 * w * w)) for a in range(3)]
        return g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]

    for r in range(rows):
        c = rng.uniform(0.5, G - 1.5, size=3)
        w = wide * rng.uniform(1.0, 3.0)
        amp = rng.uniform(0.6, 1.0)
        static = None
        if r % 2:
            static = rng.uniform(0.6, 1.0) * bump(rng.uniform(0.5, G - 1.5, size=3), wide * rng.uniform(1.0, 3.0))
        scale = rng.uniform(5.0, 10.0)
        for t in range(T):
            if t:
                c = np.clip(c + rng.uniform(-step, step, size=3), 0.5, G - 1.5)
            v = amp * bump(c, w)
            if static is not None:
                v = v + static
            v = (v - v.mean()) / v.std() * scale
            out[t, r] = (v + 0.01 * rng.standard_normal(v.shape)).astype(np.float32)
    return out.reshape(T, rows, G ** 3)


def softmax32(logits):
    """Softmax over the last axis in float64, rounded to float32."""
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def coord_grid(G):
    """Voxel-centre coordinates [G^3, 3] float32 of the test cuboid (op.build_coord_volume)."""
    from sceneego_amd import op
    return op.build_coord_volume(G, SIDE).reshape(G ** 3, 3).contiguous().numpy().astype(np.float32)
