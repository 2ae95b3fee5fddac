"""Inputs of the skeleton-prior tests: a random pose with given bone lengths, logits of one bump per joint around it, the taps and the
two-lobe demonstration.

``make_pose`` walks the tree from a root near the middle of the grid: every child lies its bone length away from its parent in a random
direction that keeps it inside the grid.  ``make_logits`` puts a bump (1-1.6 voxels wide up to 32^3, G / 32 times that above) of logit
amplitude 10-14 at every joint; odd joints get a second, static bump of 0.6-1.1 times that amplitude somewhere else: the two-lobed
volumes the coupling is for, the false lobe sometimes the stronger one.  0.01 noise is added.  The amplitudes are not standardised to
a std as the filter's cases are: a message can weigh two lobes against each other by at most the ratio of its shell value to its
floor, about N / (floor x the voxels of a shell), e^9 at 16^3 and floor 1e-3, so a false lobe that leads by more logits than that is
beyond any bone prior and would only measure the generator.  The GPU tests softmax the logits with se_softargmax3d_f32 on the device;
the host tests with ``softmax32`` of the filter's cases.
"""
import numpy as np

from sceneego_amd.skeleton_prior import shell_taps

SIDE = 2.0          # metres: the cuboid of the test grids
CHAIN3 = (0, 0, 1)
STAR5 = (0, 0, 0, 0, 0)


def lengths_for(parents, G, R, seed, tau_voxels=0.5):
    """Bone lengths in metres for a G^3 grid of side SIDE whose shells of tau = ``tau_voxels`` voxels fit a block of radius R: between
    1.5 voxels and R - 3 tau - 0.01 voxels, the longest one at that upper end (so that R is the radius the definition asks for, when
    R >= 3).  [J] float64, entry 0 is 0."""
    J = len(parents)
    h = SIDE / G
    rng = np.random.default_rng(seed)
    hi = R - 3.0 * tau_voxels - 0.01
    lo = min(1.5, hi)
    L = np.zeros(J)
    if J > 1:
        L[1:] = rng.uniform(lo, hi, size=J - 1)
        L[1 + int(rng.integers(J - 1))] = hi
    return L * h


def taps_for(lengths, G, R, tau_voxels=0.5):
    h = SIDE / G
    return shell_taps(lengths, tau_voxels * h, h, R)


def make_pose(parents, lengths_vox, G, rng):
    """Joint positions [J, 3] in voxel units inside [0.5, G - 1.5], bone j of length lengths_vox[j] (kept exactly unless no direction
    out of 2000 fits, which the callers' shapes do not reach)."""
    J = len(parents)
    lo, hi = 0.5, G - 1.5
    for _ in range(200):
        x = np.empty((J, 3))
        x[0] = rng.uniform(0.35 * G, 0.65 * G, size=3)
        ok = True
        for j in range(1, J):
            for _ in range(2000):
                v = rng.standard_normal(3)
                cand = x[parents[j]] + lengths_vox[j] * v / np.linalg.norm(v)
                if (cand >= lo).all() and (cand <= hi).all():
                    x[j] = cand
                    break
            else:
                ok = False
                break
        if ok:
            return x
    raise RuntimeError("no pose fits the grid")


def _bump(ax, c, w):
    g = [np.exp(-(ax - c[a]) ** 2 / (2 * w * w)) for a in range(3)]
    return g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]


def make_logits(frames, parents, lengths, G, seed, second=True):
    """float32 [frames, J, G^3] and the poses [frames, J, 3] in voxel units."""
    rng = np.random.default_rng(seed)
    J = len(parents)
    h = SIDE / G
    ax = np.arange(G, dtype=np.float64)
    wide = max(1.0, G / 32.0)
    out = np.empty((frames, J, G, G, G), dtype=np.float32)
    poses = np.empty((frames, J, 3))
    for f in range(frames):
        x = make_pose(parents, np.asarray(lengths) / h, G, rng)
        poses[f] = x
        for j in range(J):
            amp = rng.uniform(10.0, 14.0)
            v = amp * _bump(ax, x[j], wide * rng.uniform(1.0, 1.6))
            if second and j % 2:
                v = v + amp * rng.uniform(0.6, 1.1) * _bump(ax, rng.uniform(0.5, G - 1.5, size=3), wide * rng.uniform(1.0, 1.6))
            out[f, j] = (v + 0.01 * rng.standard_normal(v.shape)).astype(np.float32)
    return out.reshape(frames, J, G ** 3), poses


def voxel_coord(G):
    """Coordinates in voxel units: [G^3, 3] float32 with coord[(i G + j) G + k] = (i, j, k)."""
    ax = np.arange(G, dtype=np.float32)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(G ** 3, 3)


def two_lobe_logits():
    """The demonstration: 16^3, chain [0, 0, 1]; lobes of 0.8 voxel sigma and logit amplitude 12 at (8,8,3), (8,8,6.5), (8,8,10); a
    false wrist lobe of 1.5x the amplitude at (8,12,12.5).  Returns (logits [1, 3, 4096] float64, truth [3, 3])."""
    G = 16
    ax = np.arange(G, dtype=np.float64)
    truth = np.array([[8, 8, 3], [8, 8, 6.5], [8, 8, 10]], dtype=np.float64)
    logits = np.stack([12.0 * _bump(ax, truth[j], 0.8) for j in range(3)])
    logits[2] += 18.0 * _bump(ax, np.array([8, 12, 12.5]), 0.8)
    return logits.reshape(1, 3, G ** 3), truth
