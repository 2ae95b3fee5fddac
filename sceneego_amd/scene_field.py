"""The scene of a depth map as a field on the network's own voxel grid: for every voxel the exact distance to the nearest voxel that
holds scene, and which voxel that is.  Built once per frame on the device; any joint distribution, sampled pose or returned voxel
index can then be asked what the method is named for: how close to the scene, how much of the belief inside geometry.

No counterpart in the reference.  The scene is the one ``SceneConsistency`` probes and ``SceneRenderer`` draws: the point cloud of
the depth map under the drop rules of ``se_scene_probe_f64`` (d > 0, d <= 100, z > 0.1, a finite ray).  Each point marks the voxel
whose centre is nearest (``se_scene_sites_u8``); the exact Euclidean distance transform of those sites follows
(``se_scene_distance_i32``; include/sceneego_hip.h states both).  Distances are therefore QUANTISED TO VOXEL CENTRES: a field distance
and the distance to the true nearest scene point differ by up to half a voxel diagonal, (sqrt(3) / 2) * spacing, either way.  Square
roots and the conversion to metres are taken here, in float32 torch on the device.

Frame: the camera frame of the head-mounted fisheye; voxel centres as ``op.build_coord_volume`` places them, spacing
``cuboid_side / (volume_size - 1)``; flat voxel index n = (i G + j) G + k over x, y, z.
"""
from __future__ import annotations

import torch

from . import _lib, op
from .render import MAX_DEPTH, MIN_Z, calibrated_ray_table


class SceneField:
    """Owns the calibrated ray table (built and uploaded once, or shared with a ``SceneConsistency`` / ``SceneRenderer`` through
    ``ray_tab``: 31 MB at 1024 x 1280) and the transform's workspace.  ``config``: the configuration the grid comes from
    (``model.volume_size``, ``model.cuboid_side``; the package's default YAML otherwise)."""

    def __init__(self, calibration_path, frame_size=(1024, 1280), config=None, ray_tab=None, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipExtensionError(f"SceneField needs a HIP device, got {self.device}: the scene field has no CPU fallback")
        _lib.load()
        if config is None:
            from .config import load_config
            config = load_config()
        self.grid, self.side = int(config.model.volume_size), float(config.model.cuboid_side)
        if not 2 <= self.grid <= _lib.SCENE_DISTANCE_MAX_GRID:
            raise _lib.HipExtensionError(f"SceneField: volume_size {self.grid} outside 2..{_lib.SCENE_DISTANCE_MAX_GRID}")
        self.spacing = self.side / (self.grid - 1)
        self.H, self.W = int(frame_size[0]), int(frame_size[1])
        if ray_tab is None:
            ray_tab = torch.from_numpy(calibrated_ray_table(calibration_path, self.H, self.W)).to(self.device)
        elif (not isinstance(ray_tab, torch.Tensor) or ray_tab.dtype != torch.float64 or tuple(ray_tab.shape) != (self.H, self.W, 3)
              or ray_tab.device.type != "cuda" or not ray_tab.is_contiguous()):
            raise _lib.HipExtensionError(f"SceneField: ray_tab must be a contiguous float64 [{self.H},{self.W},3] tensor on a HIP device")
        self.ray_tab = ray_tab
        self._scratch = {}

    def _depth(self, depth):
        d = torch.as_tensor(depth)
        if d.dim() == 2:
            d = d[None]
        if d.dim() == 4 and d.shape[1] == 1:
            d = d[:, 0]
        if d.dim() != 3:
            raise ValueError(f"depth must be [B,dh,dw], got {tuple(d.shape)}")
        return d.to(self.device, torch.float32).contiguous()

    def build(self, depth):
        """``depth`` [B,dh,dw] (or [dh,dw], or [B,1,dh,dw]) metres, any size: it is looked up by nearest index as the scene check
        does.  One memset and three launches on the current stream.  Returns a dict, device tensors but for ``spacing``:

          ``sites``      [B,G,G,G] uint8    1 where a scene point rounds to the voxel
          ``d2``         [B,G,G,G] int32    squared distance to the nearest site in voxel index units (0x7fffffff without a site)
          ``nearest``    [B,G,G,G] int32    flat index of that site, the lowest among the nearest (-1 without a site)
          ``distance``   [B,G,G,G] float32  sqrt(d2) * spacing in metres, +inf without a site
          ``has_scene``  [B] bool           the frame has at least one site
          ``spacing``    float              metres between neighbouring voxel centres, cuboid_side / (G - 1)

        The tensors are fresh; only the transform's workspace is reused by the next call with the same B."""
        d = self._depth(depth)
        B, G = int(d.shape[0]), self.grid
        sites = op.scene_sites(d, self.ray_tab, G, self.side, MIN_Z, MAX_DEPTH)
        if B not in self._scratch:
            self._scratch[B] = torch.empty(_lib.scene_distance_scratch_bytes(B, G), device=self.device, dtype=torch.uint8)
        d2, nearest = op.scene_distance(sites, scratch=self._scratch[B])
        return field_of(sites, d2, nearest, self.spacing)


def field_of(sites, d2, nearest, spacing):
    """The dict of ``SceneField.build`` from the kernels' outputs: the float32 distance and the per-frame flag are taken here."""
    none = d2 == _lib.SCENE_NO_SITE
    distance = torch.where(none, torch.full((), float("inf"), device=d2.device, dtype=torch.float32),
                           torch.sqrt(d2.to(torch.float32)) * float(spacing))
    return {"sites": sites, "d2": d2, "nearest": nearest, "distance": distance, "has_scene": nearest[:, 0, 0, 0] >= 0,
            "spacing": float(spacing)}
