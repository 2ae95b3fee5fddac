"""Does a predicted skeleton agree with the scene of its own depth map?  Collision, clearance and contact of the joints and bones
against the scene point cloud, on the device.

No counterpart in the reference: its depth maps are scene depth with the body removed, so a joint that lies behind the depth
surface along its own line of sight is inside scene geometry (or hidden by it), and a foot whose nearest scene point is
centimetres away is in contact.  The scene is the one ``SceneRenderer`` draws: the point cloud of the depth map under the drop rules
of ``se_render_splat_f64`` (d > 0, d <= 100, z > 0.1).  The kernel is ``csrc/scene_probe.hip`` (``se_scene_probe_f64``;
include/sceneego_hip.h states its arithmetic): every scene point against every probe point, brute force, bitwise reproducible.
Square roots, divisions and thresholds are taken here, in float64 torch on the device.

Frame: the camera frame of the head-mounted fisheye, as in ``render.py``; lengths in metres.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .op import SCENE_KEYS, scene_check_to_numpy  # noqa: F401
from .render import MAX_DEPTH, MIN_Z, calibrated_ray_table

JOINTS = _lib.RENDER_JOINTS
BONES = _lib.SKELETON_LINES
CHECK_KEYS = SCENE_KEYS


def _voxel_edge(config=None) -> float:
    """One voxel edge of the configured grid, ``cuboid_side / volume_size``: the finest length the network resolves."""
    if config is None:
        from .config import load_config
        config = load_config()
    return float(config.model.cuboid_side) / float(config.model.volume_size)


class SceneConsistency:
    """Owns the calibrated ray table (built and uploaded once, or shared with a ``SceneRenderer`` through ``ray_tab``: 31 MB at
    1024 x 1280) and the kernel's workspace.  ``config``: the configuration the default thresholds of ``check`` come from (the
    package's default YAML otherwise)."""

    def __init__(self, calibration_path, frame_size=(1024, 1280), device="cuda", ray_tab=None, config=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipExtensionError(f"SceneConsistency needs a HIP device, got {self.device}: the scene check has no CPU fallback")
        _lib.load()
        self.H, self.W = int(frame_size[0]), int(frame_size[1])
        if ray_tab is None:
            ray_tab = torch.from_numpy(calibrated_ray_table(calibration_path, self.H, self.W)).to(self.device)
        elif (not isinstance(ray_tab, torch.Tensor) or ray_tab.dtype != torch.float64 or tuple(ray_tab.shape) != (self.H, self.W, 3)
              or ray_tab.device.type != "cuda" or not ray_tab.is_contiguous()):
            raise _lib.HipExtensionError(f"SceneConsistency: ray_tab must be a contiguous float64 [{self.H},{self.W},3] tensor on a HIP device")
        self.ray_tab = ray_tab
        self.voxel_edge = _voxel_edge(config)
        self._buf = {}

    # -------------------------------------------------------------------------------------------- probes
    @staticmethod
    def probes(joints, samples_per_bone=3) -> torch.Tensor:
        """[B, 15 + 15 S, 3] float64 on the device of ``joints`` [B,15,3] (or [15,3]): the 15 joints, then for bone e = (a, b) of
        ``Skeleton.lines`` the S points A + (B - A) k / (S + 1), k = 1..S, at rows 15 + e S + (k - 1)."""
        S = int(samples_per_bone)
        if S < 0 or JOINTS + len(BONES) * S > _lib.SCENE_PROBE_MAX:
            raise ValueError(f"samples_per_bone = {samples_per_bone}: 15 + 15 S probes must not pass {_lib.SCENE_PROBE_MAX} (S <= 3)")
        j = torch.as_tensor(joints)
        if j.dim() == 2:
            j = j[None]
        if j.dim() != 3 or tuple(j.shape[1:]) != (JOINTS, 3):
            raise ValueError(f"joints must be [B,15,3], got {tuple(j.shape)}")
        j = j.to(torch.float64)
        if S == 0:
            return j.contiguous()
        bones = torch.tensor(BONES, device=j.device, dtype=torch.long)
        A, Bn = j[:, bones[:, 0]], j[:, bones[:, 1]]                                  # [B,15,3]
        k = torch.arange(1, S + 1, device=j.device, dtype=torch.float64)              # [S]
        pts = A[:, :, None, :] + ((Bn - A)[:, :, None, :] * k[None, None, :, None]) / float(S + 1)
        return torch.cat([j, pts.reshape(j.shape[0], len(BONES) * S, 3)], dim=1).contiguous()

    # -------------------------------------------------------------------------------------------- kernel call
    def _depth(self, depth):
        d = torch.as_tensor(depth)
        if d.dim() == 2:
            d = d[None]
        if d.dim() != 3:
            raise ValueError(f"depth must be [B,dh,dw], got {tuple(d.shape)}")
        return d.to(self.device, torch.float32).contiguous()

    def _buffers(self, B, P):
        if (B, P) not in self._buf:
            self._buf[(B, P)] = (torch.empty((B, P, _lib.SCENE_PROBE_SLOTS), device=self.device, dtype=torch.float64),
                                 torch.empty((B, P, 2), device=self.device, dtype=torch.int32),
                                 torch.empty((_lib.scene_probe_scratch_bytes(B, self.H, self.W, P),), device=self.device,
                                             dtype=torch.uint8))
        return self._buf[(B, P)]

    def probe(self, depth, points, tolerance=None, max_sight_angle_deg=1.0):
        """Any probe points [B,P,3] (1 <= P <= 64) against the scene of ``depth`` [B,dh,dw]: one ``se_scene_probe_f64`` call, then the
        per-probe quantities of ``check`` for all P probes, as a dict of device tensors:

          ``nearest_q`` [B,P] (squared distance), ``nearest_dist`` [B,P], ``nearest_point`` [B,P,3], ``nearest_index`` [B,P] int32,
          ``range`` [B,P], ``sight_dot`` [B,P], ``sight_index`` [B,P] int32, ``surface`` [B,P], ``in_view`` [B,P] bool,
          ``clearance`` [B,P], ``penetration_depth`` [B], ``penetrating`` [B] bool.

        The tensors are fresh; the kernel's own buffers are reused by the next call with the same B and P."""
        d = self._depth(depth)
        c = torch.as_tensor(points)
        if c.dim() != 3 or c.shape[0] != d.shape[0] or c.shape[2] != 3:
            raise ValueError(f"points must be [B,P,3] with B = {d.shape[0]}, got {tuple(c.shape)}")
        c = c.to(self.device, torch.float64).contiguous()
        B, P = c.shape[:2]
        if not 1 <= P <= _lib.SCENE_PROBE_MAX:
            raise ValueError(f"{P} probes per frame, 1..{_lib.SCENE_PROBE_MAX} supported")
        out, index, scratch = self._buffers(B, P)
        _lib.scene_probe(d, self.ray_tab, c, out, index, scratch=scratch, min_z=MIN_Z, max_depth=MAX_DEPTH)
        tol = self.voxel_edge if tolerance is None else float(tolerance)
        rng = torch.sqrt(out[..., 4])
        # unit rays: sight_dot / range is the cosine of the angle between the probe and the ray that points at it best
        cosine = out[..., 5] / rng
        in_view = (rng > 0) & (cosine >= math.cos(math.radians(float(max_sight_angle_deg))))           # a NaN is not in view
        nan = torch.full_like(rng, float("nan"))
        clearance = torch.where(in_view, out[..., 6] - rng, nan)
        worst = torch.where(torch.isnan(clearance), torch.zeros_like(clearance), clearance).amin(dim=1)
        depth_in = torch.clamp(-worst, min=0.0)
        return {"nearest_q": out[..., 0].clone(), "nearest_dist": torch.sqrt(out[..., 0]), "nearest_point": out[..., 1:4].clone(),
                "nearest_index": index[..., 0].clone(), "range": rng, "sight_dot": out[..., 5].clone(),
                "sight_index": index[..., 1].clone(), "surface": out[..., 6].clone(), "in_view": in_view, "clearance": clearance,
                "penetration_depth": depth_in, "penetrating": depth_in > tol}

    # -------------------------------------------------------------------------------------------- the check
    def check(self, depth, joints, samples_per_bone=3, contact_radius=None, tolerance=None, max_sight_angle_deg=1.0):
        """``depth`` [B,dh,dw] (or [dh,dw]) metres, ``joints`` [B,15,3] (or [15,3]) in the camera frame -> a dict of device tensors:

          ``nearest_dist``      [B,15]    distance of each joint to its nearest scene point (+inf in a frame without one)
          ``nearest_point``     [B,15,3]  that scene point (NaN without one)
          ``nearest_index``     [B,15]    int32, its pixel y * W + x, the lowest among equals (-1 without one)
          ``range``             [B,15]    distance of each joint from the camera
          ``sight_index``       [B,15]    int32, the pixel whose ray points at the joint best (the lowest among equals)
          ``in_view``           [B,15]    bool: the angle between the joint and that ray is <= ``max_sight_angle_deg``; a joint at the
                                          origin, or outside the calibrated field of view, is not in view
          ``clearance``         [B,15]    depth surface at the sight pixel - range: positive is free space in front of the surface,
                                          negative is behind it; NaN where that pixel has no surface or the joint is not in view
          ``bone_clearance``    [B,15]    per bone of ``Skeleton.lines``: the minimum clearance over its ``samples_per_bone`` interior
                                          samples and its two end joints, ignoring NaN (NaN if all are)
          ``penetration_depth`` [B]       max(0, -min clearance) over all probes (joints and bone samples) of the frame; 0 if none
                                          is defined
          ``penetrating``       [B]       bool: penetration_depth > ``tolerance``
          ``contact``           [B,15]    bool: nearest_dist <= ``contact_radius``

        ``tolerance`` defaults to one voxel edge of the configured grid (``cuboid_side / volume_size``, 31.25 mm for the shipped
        YAML) and ``contact_radius`` to two.  These are conventions tied to what the network can resolve; they are NOT calibrated
        against data, because no annotated data ships with the method.  A non-finite joint gives NaN / -1 / False in its own
        entries and in the bones it ends; the other entries are unaffected."""
        S = int(samples_per_bone)
        c = self.probes(torch.as_tensor(joints).to(self.device), S)
        r = self.probe(depth, c, tolerance=tolerance, max_sight_angle_deg=max_sight_angle_deg)
        radius = 2.0 * self.voxel_edge if contact_radius is None else float(contact_radius)
        B = c.shape[0]
        clear = r["clearance"]                                                        # [B,P]
        bones = torch.tensor(BONES, device=self.device, dtype=torch.long)
        members = [bones[:, 0], bones[:, 1]] + [JOINTS + torch.arange(len(BONES), device=self.device) * S + k for k in range(S)]
        group = clear[:, torch.stack(members, dim=1)]                                 # [B,15,S+2]
        inf = torch.full_like(group, float("inf"))
        low = torch.where(torch.isnan(group), inf, group).amin(dim=2)                 # a clearance is finite or NaN, never +inf
        bone_clearance = torch.where(torch.isinf(low), torch.full_like(low, float("nan")), low)
        J = slice(0, JOINTS)
        assert clear.shape == (B, JOINTS + len(BONES) * S)
        return {"nearest_dist": r["nearest_dist"][:, J], "nearest_point": r["nearest_point"][:, J], "nearest_index": r["nearest_index"][:, J],
                "range": r["range"][:, J], "sight_index": r["sight_index"][:, J], "in_view": r["in_view"][:, J],
                "clearance": clear[:, J], "bone_clearance": bone_clearance, "penetration_depth": r["penetration_depth"],
                "penetrating": r["penetrating"], "contact": r["nearest_dist"][:, J] <= radius}

