"""Headless rendering of a frame's result on the device: the coloured point cloud of the depth map together with the predicted
skeleton from a free third-person view, and the skeleton drawn into the fisheye frame.

Stands in for the reference's ``visualize.py`` (``utils/depth2pointcloud.py: get_point_cloud_single_image`` with ``post_process``,
``utils/skeleton.py: joints_2_mesh``, an open3d window); the kernels are ``csrc/render.hip`` (``se_render_splat_f64``,
``se_render_resolve_f64``, ``se_render_overlay_f64``; include/sceneego_hip.h states their arithmetic).

Frames: the camera frame of the head-mounted fisheye (x right, y down in the image, +z from the camera down into the cuboid, whose
centre is (0, 0, 1)); a view is 12 float64, row-major ``R[3][3]`` then ``t[3]``, taking a camera-frame point p to view space
``R p + t`` (x right, y down, z forward).
"""
from __future__ import annotations

import math
import struct

import numpy as np
import torch

from . import _lib
from .fisheye import FishEyeCameraCalibrated

MIN_Z = 0.1          # the reference drops points with z <= 0.1 (depth2pointcloud.py postprocess)
MAX_DEPTH = 100.0    # ... and zeroes depths above 100 (get_point_cloud_single_image)
NEAR = 0.05          # near plane of the rendered view, metres


def look_at(eye, target, up) -> np.ndarray:
    """view[12] (float64) of a camera at ``eye`` looking at ``target``; ``up`` points to the top of the image."""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    z = target - eye
    n = np.linalg.norm(z)
    if not n > 0:
        raise ValueError("look_at: eye and target coincide")
    z = z / n
    x = np.cross(-up, z)                 # image x = down x forward (right-handed: x cross y = z with y down)
    n = np.linalg.norm(x)
    if not n > 1e-12:
        raise ValueError("look_at: up is parallel to the viewing direction")
    x = x / n
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R.reshape(9), -(R @ eye)])


def orbit_view(azimuth_deg=35.0, elevation_deg=25.0, distance=3.5, target=(0.0, 0.0, 1.0)) -> np.ndarray:
    """A camera on a sphere around ``target`` (default: the cuboid centre).  Up is (0, 0, -1): towards the head camera, so a positive
    elevation looks at the scene from above the person's feet, like a bystander."""
    up = np.array([0.0, 0.0, -1.0])
    az, el = math.radians(azimuth_deg), math.radians(elevation_deg)
    target = np.asarray(target, dtype=np.float64)
    eye = target + distance * (math.cos(el) * np.array([math.cos(az), math.sin(az), 0.0]) + math.sin(el) * up)
    return look_at(eye, target, up)


def calibrated_ray_table(calibration_path, height, width) -> np.ndarray:
    """[height, width, 3] float64 unit rays of the frame's pixels, in ``FishEyeCameraCalibrated.camera2world_ray``'s arithmetic."""
    cam = FishEyeCameraCalibrated(calibration_path)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    pts = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)
    return np.ascontiguousarray(cam.camera2world_ray(pts).reshape(height, width, 3))


def pinhole_ray_table(out_h, out_w, f, cx, cy) -> np.ndarray:
    """[out_h, out_w, 3] float64: ((px + 0.5 - cx) / f, (py + 0.5 - cy) / f, 1), the ray through the centre of output pixel (px, py)."""
    rays = np.ones((out_h, out_w, 3), dtype=np.float64)
    rays[:, :, 0] = ((np.arange(out_w, dtype=np.float64) + 0.5 - cx) / f)[None, :]
    rays[:, :, 1] = ((np.arange(out_h, dtype=np.float64) + 0.5 - cy) / f)[:, None]
    return rays


def parse_joint_list(text):
    """"9,10,13,14" -> (9, 10, 13, 14), the form of the tools' ``--volume_joints``; None stays None (all joints).  ValueError with
    the message the tools print for anything else."""
    if text is None:
        return None
    try:
        joints = tuple(int(t) for t in str(text).split(","))
    except ValueError:
        raise ValueError(f"--volume_joints wants joint indices separated by commas, e.g. 9,10,13,14; got {text!r}") from None
    if not joints or any(not 0 <= j < _lib.RENDER_JOINTS for j in joints):
        raise ValueError(f"--volume_joints wants joint indices 0..{_lib.RENDER_JOINTS - 1}; got {text!r}")
    return joints


class SceneRenderer:
    """Owns the two ray tables (built and uploaded once), the z-buffer and the output images.  The arrays ``render`` / ``overlay``
    return are the renderer's own buffers: the next call with the same batch size overwrites them."""

    def __init__(self, calibration_path, frame_size=(1024, 1280), out_size=(720, 960), fov_y_deg=50.0, splat=2, device="cuda",
                 background=(255, 255, 255)):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipExtensionError(f"SceneRenderer needs a HIP device, got {self.device}: the renderer has no CPU fallback")
        _lib.load()
        self.H, self.W = int(frame_size[0]), int(frame_size[1])
        self.Hout, self.Wout = int(out_size[0]), int(out_size[1])
        if not 1 <= int(splat) <= 4:
            raise ValueError(f"splat must be 1..4, got {splat}")
        self.splat = int(splat)
        self.background = tuple(int(c) for c in background)
        self.f = (self.Hout / 2.0) / math.tan(math.radians(fov_y_deg) / 2.0)
        self.cx, self.cy = self.Wout / 2.0, self.Hout / 2.0
        self.ray_tab = torch.from_numpy(calibrated_ray_table(calibration_path, self.H, self.W)).to(self.device)
        self.pinhole = torch.from_numpy(pinhole_ray_table(self.Hout, self.Wout, self.f, self.cx, self.cy)).to(self.device)
        self._buf = {}

    def _buffers(self, B):
        if B not in self._buf:
            self._buf[B] = (torch.empty((B, self.Hout, self.Wout), device=self.device, dtype=torch.int64),
                            torch.empty((B, self.Hout, self.Wout, 3), device=self.device, dtype=torch.uint8),
                            torch.empty((B, self.H, self.W, 3), device=self.device, dtype=torch.uint8))
        return self._buf[B]

    def _frames(self, image_bgr_u8):
        img = torch.as_tensor(image_bgr_u8)
        if img.dim() == 3:
            img = img[None]
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise ValueError(f"frames must be uint8 [B,H,W,3] (B, G, R), got {img.dtype} {tuple(img.shape)}")
        if tuple(img.shape[1:3]) != (self.H, self.W):
            raise ValueError(f"this renderer was built for {self.H}x{self.W} frames (its ray table is per pixel), got "
                             f"{img.shape[1]}x{img.shape[2]}: build a SceneRenderer with frame_size=({img.shape[1]}, {img.shape[2]})")
        return img.to(self.device).contiguous()

    def _depth(self, depth, B):
        d = torch.as_tensor(depth)
        if d.dim() == 2:
            d = d[None]
        if d.dim() != 3 or d.shape[0] != B:
            raise ValueError(f"depth must be [B,dh,dw] with B = {B}, got {tuple(d.shape)}")
        return d.to(self.device, torch.float32).contiguous()

    def _joints(self, joints, B):
        j = torch.as_tensor(joints)
        if j.dim() == 2:
            j = j[None]
        if tuple(j.shape) != (B, _lib.RENDER_JOINTS, 3):
            raise ValueError(f"joints must be [B,15,3] with B = {B}, got {tuple(j.shape)}")
        return j.to(self.device, torch.float64)

    def render(self, depth, image_bgr_u8, joints, view=None) -> torch.Tensor:
        """uint8 [B,Hout,Wout,3] (R, G, B) on the device: the point cloud of ``depth`` coloured by the frame, with the skeleton."""
        img = self._frames(image_bgr_u8)
        B = img.shape[0]
        d, j = self._depth(depth, B), self._joints(joints, B)
        v = np.asarray(orbit_view() if view is None else view, dtype=np.float64).reshape(12)
        vt = torch.from_numpy(v).to(self.device)
        R, t = vt[:9].view(3, 3), vt[9:]
        jv = (j @ R.T + t).contiguous()            # the joints in view space, float64 on the device
        zbuf, out, _ = self._buffers(B)
        _lib.render_splat(d, self.ray_tab, img, vt, zbuf, self.f, self.cx, self.cy, splat=self.splat, min_z=MIN_Z,
                          max_depth=MAX_DEPTH, near=NEAR)
        return _lib.render_resolve(self.pinhole, jv, zbuf, out, near=NEAR, background=self.background)

    def overlay(self, image_bgr_u8, joints, depth=None) -> torch.Tensor:
        """uint8 [B,H,W,3] (R, G, B) on the device: the frame with the skeleton drawn into it; with ``depth`` the skeleton is hidden
        where the depth map is nearer."""
        img = self._frames(image_bgr_u8)
        B = img.shape[0]
        j = self._joints(joints, B).contiguous()
        d = None if depth is None else self._depth(depth, B)
        return _lib.render_overlay(self.ray_tab, j, img, self._buffers(B)[2], depth=d, near=NEAR)

    # -------------------------------------------------------------------------------------------- the joint probability volumes
    @staticmethod
    def _joint_mask(joint_mask) -> int:
        """None (all joints) or an iterable of joint indices -> the bit mask of se_render_volume_*_f64."""
        if joint_mask is None:
            return _lib.RENDER_VOLUME_ALL
        if isinstance(joint_mask, (str, bytes)) or not hasattr(joint_mask, "__iter__"):
            raise ValueError(f"joint_mask must be None or an iterable of joint indices 0..14, got {joint_mask!r}")
        mask = 0
        for j in joint_mask:
            if isinstance(j, bool) or int(j) != j or not 0 <= int(j) < _lib.RENDER_JOINTS:
                raise ValueError(f"joint_mask must hold joint indices 0..14, got {j!r}")
            mask |= 1 << int(j)
        return mask

    @staticmethod
    def _volume_options(cuboid_side, gain, opacity):
        side, gain, opacity = float(cuboid_side), float(gain), float(opacity)
        if not (math.isfinite(side) and side > 0):
            raise ValueError(f"cuboid_side must be a positive number of metres, got {cuboid_side}")
        if not 0 <= gain <= 1e30:
            raise ValueError(f"gain must lie in [0, 1e30], got {gain}")
        if not 0 <= opacity <= 1:
            raise ValueError(f"opacity must lie in [0, 1], got {opacity}")
        return side, gain, opacity

    def _volumes(self, volumes, B):
        v = volumes if isinstance(volumes, torch.Tensor) else torch.as_tensor(volumes)
        if v.dim() == 4:
            v = v[None]
        if v.dtype != torch.float32 or v.dim() != 5 or v.shape[1] != _lib.RENDER_JOINTS or not v.shape[2] == v.shape[3] == v.shape[4]:
            raise ValueError(f"volumes must be float32 [B,15,G,G,G], got {v.dtype} {tuple(v.shape)}")
        if v.shape[0] != B:
            raise ValueError(f"volumes must be [B,15,G,G,G] with B = {B}, got {tuple(v.shape)}")
        if v.shape[2] < 2:
            raise ValueError(f"volumes need a grid of at least 2 cells per axis, got {tuple(v.shape)}")
        return v.to(self.device).contiguous()

    def _scale(self, scale, vol):
        B = vol.shape[0]
        if scale is None:
            # the brightest finite cell of every joint maps to 1 (a NaN or infinite cell counts as 0 here, as a NaN cell never wins
            # in the march); a joint without a positive cell gets an infinite scale, which switches it off
            return 1.0 / torch.nan_to_num(vol, nan=0.0, posinf=0.0, neginf=0.0).amax(dim=(2, 3, 4)).double()
        s = torch.as_tensor(scale)
        if s.dim() == 1:
            s = s[None]
        if tuple(s.shape) != (B, _lib.RENDER_JOINTS):
            raise ValueError(f"scale must be [B,15] with B = {B}, got {tuple(s.shape)}")
        return s.to(self.device, torch.float64).contiguous()

    def _packed(self, vol):
        """The cell-interleaved copy of ``vol`` (se_render_volume_pack_f32) in a buffer the renderer keeps per (B, G)."""
        B, G = vol.shape[0], vol.shape[2]
        key = ("packed", B, G)
        if key not in self._buf:
            self._buf[key] = torch.empty(_lib.render_volume_packed_elems(B, G), device=self.device, dtype=torch.float32)
        return _lib.render_volume_pack(vol, self._buf[key])

    def render_volumes(self, depth, image_bgr_u8, joints, volumes, cuboid_side, view=None, joint_mask=None, scale=None, gain=1.0,
                       opacity=0.8, occlude=True) -> torch.Tensor:
        """``render`` with the maximum of every joint's volume along each pixel's ray drawn over it in the joint's colour
        (include/sceneego_hip.h: se_render_volume_view_f64).  ``volumes``: the float32 [B,15,G,G,G] device tensor ``forward()`` returns,
        over a cuboid of ``cuboid_side`` metres; ``scale`` [B,15] (default 1 / the joint's largest finite value: its brightest cell maps to 1, a NaN cell is passed over);
        ``joint_mask``: an iterable of joint indices (default all); ``occlude``: hidden behind the point cloud.  Under
        ``enable_graphs(True)`` the volumes are the graph's static buffers: render before the next forward."""
        side, gain, opacity = self._volume_options(cuboid_side, gain, opacity)
        mask = self._joint_mask(joint_mask)
        img = self._frames(image_bgr_u8)
        B = img.shape[0]
        vol = self._volumes(volumes, B)
        sc = self._scale(scale, vol)
        v = np.asarray(orbit_view() if view is None else view, dtype=np.float64).reshape(12)
        out = self.render(depth, img, joints, view=v)
        zbuf = self._buffers(B)[0]
        return _lib.render_volume_view(self._packed(vol), sc, self.pinhole, v, zbuf if occlude else None, out, vol.shape[2], side,
                                       near=NEAR, joint_mask=mask, gain=gain, opacity=opacity)

    def overlay_volumes(self, image_bgr_u8, joints, volumes, cuboid_side, depth=None, joint_mask=None, scale=None, gain=1.0,
                        opacity=0.8, occlude=True) -> torch.Tensor:
        """``overlay`` with the volumes drawn into the fisheye frame (se_render_volume_overlay_f64); with ``depth`` and ``occlude`` the
        skeleton and the volumes are hidden where the depth map is nearer.  Arguments as for ``render_volumes``."""
        side, gain, opacity = self._volume_options(cuboid_side, gain, opacity)
        mask = self._joint_mask(joint_mask)
        img = self._frames(image_bgr_u8)
        B = img.shape[0]
        vol = self._volumes(volumes, B)
        sc = self._scale(scale, vol)
        d = None if depth is None else self._depth(depth, B)
        out = self.overlay(img, joints, depth=d)
        return _lib.render_volume_overlay(self._packed(vol), sc, self.ray_tab, out, vol.shape[2], side, depth=d if occlude else None,
                                          near=NEAR, joint_mask=mask, gain=gain, opacity=opacity)

    def scene_points(self, depth, image_bgr_u8):
        """(points float32 [n,3], rgb uint8 [n,3]) on the device: the reference's ``get_point_cloud_single_image`` with
        ``post_process``, with the drop rules of the splat (d > 0, d <= 100, z > 0.1); the frames of a batch are concatenated."""
        img = self._frames(image_bgr_u8)
        B = img.shape[0]
        d = self._depth(depth, B)
        dh, dw = d.shape[1:]
        sy = (torch.arange(self.H, device=self.device) * dh) // self.H
        sx = (torch.arange(self.W, device=self.device) * dw) // self.W
        dd = d[:, sy][:, :, sx].double()                       # [B,H,W]
        p = self.ray_tab[None] * dd[..., None]
        keep = (dd > 0) & (dd <= MAX_DEPTH) & (p[..., 2] > MIN_Z)
        return p[keep].float(), img[keep].flip(-1).contiguous()


# ------------------------------------------------------------------------------------------------ files
def write_ply(path, points, rgb) -> None:
    """Binary little-endian PLY: x y z float, red green blue uchar."""
    pts = np.ascontiguousarray(torch.as_tensor(points).cpu().numpy(), dtype="<f4").reshape(-1, 3)
    col = np.ascontiguousarray(torch.as_tensor(rgb).cpu().numpy(), dtype=np.uint8).reshape(-1, 3)
    if len(pts) != len(col):
        raise ValueError(f"{len(pts)} points but {len(col)} colours")
    rec = np.empty(len(pts), dtype=[("p", "<f4", 3), ("c", "u1", 3)])
    rec["p"], rec["c"] = pts, col
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(pts))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path):
    """(points float32 [n,3], rgb uint8 [n,3]) of a file ``write_ply`` wrote."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    n = next(int(ln.split()[2]) for ln in lines if ln.startswith("element vertex"))
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    if props != [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]:
        raise ValueError(f"{path}: unexpected properties {props}")
    if len(data) - end != n * struct.calcsize("<3f3B"):
        raise ValueError(f"{path}: {len(data) - end} payload bytes for {n} vertices")
    rec = np.frombuffer(data, dtype=[("p", "<f4", 3), ("c", "u1", 3)], count=n, offset=end)
    return rec["p"].astype(np.float32), rec["c"].copy()


def save_png(path, rgb) -> None:
    """uint8 [H,W,3] (R, G, B), tensor or array -> PNG (PIL, on the host)."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(torch.as_tensor(rgb).cpu().numpy())).save(path, format="PNG")


def save_jpeg(path, rgb, quality=90, subsampling="444") -> None:
    """uint8 [H,W,3] (R, G, B), tensor or array -> baseline JPEG encoded on the device (``sceneego_amd/jpeg_encode.py``); only the
    compressed bytes cross to the host."""
    from .jpeg_encode import save_jpeg as _save
    _save(path, rgb, quality=quality, subsampling=subsampling)
