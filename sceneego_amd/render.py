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
