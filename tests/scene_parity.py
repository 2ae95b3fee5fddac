"""What the scene tools that existed before the scene distance field compute on fixed inputs, as one hash per tool: the hashes were
recorded on the commit before the field was added, and tests/test_gpu_scene_field.py holds the library that carries the field to
them.  Only entry points of that earlier commit are used (``_lib.softargmax3d``, ``VoxelNetwork_depth.constrain_to_scene``,
``SceneConsistency.check``); no forward runs, so no convolution kernel takes part."""
import hashlib
import os

import numpy as np
import torch

G, B, J = 64, 2, 15
DEPTHS = ("img_001000.jpg.exr", "img_001796.jpg.exr")


def volumes(device):
    """[B,15,G,G,G] softmaxed volumes of one or two Gaussian bumps per joint (seeded numpy, float32 logits through the library's own
    soft-argmax), with the joints it returns."""
    from sceneego_amd import _lib, load_config, op
    g = np.random.default_rng(20240)
    ax = np.arange(G, dtype=np.float64)
    logits = np.empty((B * J, G, G, G), dtype=np.float32)
    for r in range(B * J):
        v = np.zeros((G, G, G))
        for _ in range(1 + r % 2):
            c, w = g.uniform(8.0, G - 9.0, size=3), g.uniform(1.5, 4.0)
            e = [np.exp(-(ax - c[a]) ** 2 / (2 * w * w)) for a in range(3)]
            v += g.uniform(0.6, 1.0) * e[0][:, None, None] * e[1][None, :, None] * e[2][None, None, :]
        logits[r] = (12.0 * v).astype(np.float32)
    cfg = load_config()
    coord = op.build_coord_volume(G, cfg.model.cuboid_side).reshape(-1, 3).contiguous().to(device)
    x = torch.from_numpy(logits.reshape(B * J, -1)).to(device)
    prob = torch.empty_like(x)
    joints = torch.empty((B * J, 3), device=device, dtype=torch.float32)
    _lib.softargmax3d(x, coord, prob, joints, B * J, G ** 3, 1)
    return prob.view(B, J, G, G, G), joints.view(B, J, 3)


def _hash(result, keys):
    h = hashlib.sha256()
    for k in keys:
        a = np.ascontiguousarray(result[k].cpu().numpy())
        h.update(k.encode() + b"\0" + str(a.dtype).encode() + b"\0" + repr(a.shape).encode() + b"\0" + a.tobytes())
    return h.hexdigest()


def digests(gold, device="cuda:0"):
    """{"constrain_to_scene": sha256, "scene_check": sha256} of the two tools on the golden demo depth maps under ``gold``."""
    from sceneego_amd import load_config, op
    from sceneego_amd.config import resolve_calibration_path
    from sceneego_amd.preprocess import load_depth, prepare_depth
    from sceneego_amd.scene_check import SceneConsistency
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    cfg = load_config()
    assert cfg.model.volume_size == G
    depth = torch.stack([prepare_depth(load_depth(os.path.join(gold, "demo", n))) for n in DEPTHS]).to(device)
    vol, kp = volumes(device)
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)      # the heads follow the device of the volumes; no weights are used
    con = net.constrain_to_scene(vol, kp, depth)
    sc = SceneConsistency(resolve_calibration_path(cfg.dataset.camera_calibration_path),
                          frame_size=(cfg.dataset.image_height, cfg.dataset.image_width), device=device, config=cfg).check(depth, kp)
    torch.cuda.synchronize()
    return {"constrain_to_scene": _hash(con, op.CONSTRAINT_KEYS + ("free",)), "scene_check": _hash(sc, op.SCENE_KEYS)}
