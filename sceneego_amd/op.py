"""Host-side geometry of the hot path + the operator surface of the reference's ``utils/op.py``.

Init-time constants (run once on the host, exactly as the reference does):
  * ``build_coord_volume``                      <- ``network/voxel_net_depth.py:110-134``
  * ``get_projected_2d_points_with_coord_volumes`` <- ``utils/op.py:98-116`` (-> ``utils/multiview.py:114-132``)
  * ``get_grid_coord_proj_batch``               <- ``utils/op.py:177-184``
  * ``calculated_ray_direction_numpy``          <- ``network/voxel_net_depth.py:147-155``
plus two tables that exist only in this build (they are what the HIP kernels read):
  * ``build_gather_table``  — per voxel 4 texel indices + 4 bilinear weights into the 64x64 map
    (fuses Upsample(1024^2, nearest) + ConstantPad2d(128) + grid_sample);
  * ``build_voxelizer_ray_table`` — the float64 rays of the centre 1024 columns, in the order the
    voxeliser kernel walks the depth map.

Per-forward operators (device; thin wrappers over the C-ABI in ``include/sceneego_hip.h``):
  * ``unproject_heatmaps_one_view_batch``       <- ``utils/op.py:194-214``
  * ``integrate_tensor_3d_with_coordinates``    <- ``utils/op.py:83-96``
These two keep the reference's names and argument meaning; they run on HIP tensors only and raise
if the extension is missing (there is no CPU fallback in the product path).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

# Geometry the reference hard-codes (voxel_net_depth.py:60-61,197-198): the 64x64 feature map is
# nearest-upsampled to 1024x1024 and zero-padded by 128 columns left/right to the 1280-wide image.
UPSAMPLED = 1024
PAD_X = 128


# ----------------------------------------------------------------------------------------------
# init-time constants
# ----------------------------------------------------------------------------------------------
def build_coord_volume(volume_size: int, cuboid_side: float) -> torch.Tensor:
    """[G,G,G,3] float32 voxel-centre coordinates in metres (reference ``voxel_net_depth.py:110-134``)."""
    sides = np.array([cuboid_side, cuboid_side, cuboid_side])
    position = np.array([-cuboid_side / 2, -cuboid_side / 2, 0])
    r = torch.arange(volume_size)
    xxx, yyy, zzz = torch.meshgrid(r, r, r, indexing="ij")
    grid = torch.stack([xxx, yyy, zzz], dim=-1).type(torch.float).reshape((-1, 3))
    coord = torch.zeros_like(grid)
    for a in range(3):
        coord[:, a] = position[a] + (sides[a] / (volume_size - 1)) * grid[:, a]
    return coord.reshape(volume_size, volume_size, volume_size, 3)


def get_projected_2d_points_with_coord_volumes(fisheye_model, coord_volume: torch.Tensor) -> torch.Tensor:
    """[N,2] pixel position of every voxel centre (reference ``utils/op.py:98-116``)."""
    return fisheye_model.world2camera_pytorch(coord_volume.reshape((-1, 3)))


def get_grid_coord_proj_batch(grid_coord_proj: torch.Tensor, batch_size: int, heatmap_shape) -> torch.Tensor:
    """Normalise to grid_sample's [-1,1] and expand (stride 0) to the batch (reference ``utils/op.py:177-184``)."""
    g = torch.zeros_like(grid_coord_proj)
    g[:, 0] = 2 * (grid_coord_proj[:, 0] / heatmap_shape[1] - 0.5)
    g[:, 1] = 2 * (grid_coord_proj[:, 1] / heatmap_shape[0] - 0.5)
    g = g.unsqueeze(1).unsqueeze(0)
    return g.expand(batch_size, -1, -1, -1)


def calculated_ray_direction_numpy(fisheye_model, image_width: int, image_height: int) -> np.ndarray:
    """[W*H,3] float64 unit rays, pixel order x-major (flat = x*H + y) (reference ``voxel_net_depth.py:147-155``)."""
    xs = np.arange(image_width, dtype=np.float64)
    ys = np.arange(image_height, dtype=np.float64)
    points = np.zeros((image_width, image_height, 2))
    points[:, :, 0] = xs[:, None]
    points[:, :, 1] = ys[None, :]
    return fisheye_model.camera2world_ray(points.reshape((-1, 2)))


def _nearest_src(dst: torch.Tensor, in_size: int, out_size: int) -> torch.Tensor:
    """Source index of ``nn.Upsample(mode='nearest')`` (ATen ``nearest_neighbor_compute_source_index``): min(floor(dst * scale), in - 1) with
    scale = in / out evaluated in float32 (exact for the power-of-two ratios of the 256x256 crop, and the reference's rounding elsewhere)."""
    scale = torch.tensor(float(in_size), dtype=torch.float32) / torch.tensor(float(out_size), dtype=torch.float32)
    src = torch.floor(dst.to(torch.float32) * scale).to(torch.int64)
    return torch.clamp(src, max=in_size - 1)


def build_gather_table(grid_coord_proj_norm: torch.Tensor, heatmap_shape, feat_hw=64):
    """Per-voxel 4-tap lookup into the compact feature map.

    ``grid_coord_proj_norm`` is [N,2] in grid_sample's normalised coordinates for an image of
    ``heatmap_shape`` = (H=1024, W=1280).  grid_sample(align_corners=True, bilinear, zeros) un-normalises
    ix = (gx+1)/2*(W-1), iy = (gy+1)/2*(H-1) and blends the 4 neighbouring texels; a texel (x,y) of the
    virtual 1024x1280 image is ``F[src(y), src(x-128)]`` inside the 1024 centre columns and 0 elsewhere, src = the nearest-neighbour
    source index of ``nn.Upsample(size=(1024, 1024))`` for a feature map of ``feat_hw`` = (h, w) (an int means square; the reference
    upsamples ANY feature-map size, ``network/voxel_net_depth.py:59-60,238``; 64 x 64 for the 256 x 256 crop: src = dst >> 4).
    Returns (idx int32 [N,4], w float32 [N,4]); idx = fy * w + fx, -1 marks a zero tap.
    """
    H, W = int(heatmap_shape[0]), int(heatmap_shape[1])
    fh, fw = (int(feat_hw), int(feat_hw)) if isinstance(feat_hw, int) else (int(feat_hw[0]), int(feat_hw[1]))
    if fh <= 0 or fw <= 0 or H != UPSAMPLED or W != UPSAMPLED + 2 * PAD_X:
        raise ValueError("gather table: heatmap %dx%d / feature map %dx%d not representable" % (H, W, fh, fw))
    g = grid_coord_proj_norm.detach().to(torch.float32).cpu()
    # same float32 arithmetic as ATen's grid_sampler_unnormalize(align_corners=True): ((g + 1) / 2) * (size - 1)
    ix = ((g[:, 0] + 1) / 2) * (W - 1)
    iy = ((g[:, 1] + 1) / 2) * (H - 1)
    x0 = torch.floor(ix)
    y0 = torch.floor(iy)
    x1 = x0 + 1
    y1 = y0 + 1
    # ATen weights: nw=(x1-ix)(y1-iy)  ne=(ix-x0)(y1-iy)  sw=(x1-ix)(iy-y0)  se=(ix-x0)(iy-y0)
    w = torch.stack([(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)], dim=1)
    taps_x = torch.stack([x0, x1, x0, x1], dim=1).to(torch.int64)
    taps_y = torch.stack([y0, y0, y1, y1], dim=1).to(torch.int64)
    inside = (taps_x >= PAD_X) & (taps_x < PAD_X + UPSAMPLED) & (taps_y >= 0) & (taps_y < H)
    fx = _nearest_src(torch.clamp(taps_x - PAD_X, 0, UPSAMPLED - 1), fw, UPSAMPLED)
    fy = _nearest_src(torch.clamp(taps_y, 0, UPSAMPLED - 1), fh, UPSAMPLED)
    idx = torch.where(inside, fy * fw + fx, torch.full_like(fx, -1)).to(torch.int32)
    w = torch.where(inside, w, torch.zeros_like(w)).to(torch.float32)
    return idx.contiguous(), w.contiguous()


def build_voxelizer_ray_table(ray: np.ndarray, image_width: int, image_height: int) -> np.ndarray:
    """Rays of the centre ``UPSAMPLED`` columns, laid out [y, x', 3] float64 (row-major like the depth map).

    The reference multiplies ``ray`` (x-major, [W*H,3]) with the padded depth transposed
    (``voxel_net_depth.py:198-200``); the 2x128 pad columns carry depth 0 and need no ray.
    """
    assert image_width == UPSAMPLED + 2 * PAD_X
    r = ray.reshape(image_width, image_height, 3)[PAD_X:PAD_X + UPSAMPLED]  # [x', y, 3]
    return np.ascontiguousarray(r.transpose(1, 0, 2))                        # [y, x', 3]


# ----------------------------------------------------------------------------------------------
# per-forward operators (HIP)
# ----------------------------------------------------------------------------------------------
def unproject_heatmaps_one_view_batch(heatmaps, grid_coord_proj_transformed_batch, volume_size):
    """Reference ``utils/op.py:194-214``: sample ``heatmaps`` [B,C,H,W] at the projected voxel centres.

    Generic form (any H,W, bilinear, zeros padding, align_corners=True) on the HIP gather kernel;
    returns [B,C,G,G,G] like the reference.  The network's forward uses the fused table-driven form
    instead (no 1024x1280 intermediate), see ``VoxelNetwork_depth.forward``.
    """
    _lib.require_hip(heatmaps)
    B, C, H, W = heatmaps.shape
    G = int(volume_size)
    grid = grid_coord_proj_transformed_batch[0].reshape(-1, 2)   # identical for every sample (stride-0 expand)
    idx, w = build_gather_table_generic(grid, H, W)
    idx = idx.to(heatmaps.device)
    w = w.to(heatmaps.device)
    feat = heatmaps.permute(0, 2, 3, 1).contiguous().float()     # NHWC
    out = torch.empty((B, G * G * G, C), device=heatmaps.device, dtype=torch.float32)
    _lib.unproject_gather(feat, idx, w, out, B, H * W, C, G * G * G, C, 0)
    return out.view(B, G, G, G, C).permute(0, 4, 1, 2, 3)


def build_gather_table_generic(grid_norm: torch.Tensor, H: int, W: int):
    """4-tap table for a plain [H,W] image (no upsample/pad folding)."""
    g = grid_norm.detach().to(torch.float32).cpu()
    ix = ((g[:, 0] + 1) / 2) * (W - 1)
    iy = ((g[:, 1] + 1) / 2) * (H - 1)
    x0 = torch.floor(ix)
    y0 = torch.floor(iy)
    x1 = x0 + 1
    y1 = y0 + 1
    w = torch.stack([(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)], dim=1)
    tx = torch.stack([x0, x1, x0, x1], dim=1).to(torch.int64)
    ty = torch.stack([y0, y0, y1, y1], dim=1).to(torch.int64)
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    idx = torch.where(inside, ty * W + tx, torch.full_like(tx, -1)).to(torch.int32)
    w = torch.where(inside, w, torch.zeros_like(w)).to(torch.float32)
    return idx.contiguous(), w.contiguous()


def integrate_tensor_3d_with_coordinates(volumes, coord_volumes, softmax=True):
    """Reference ``utils/op.py:83-96``: softmax over all voxels per (b,joint), then expectation of the coordinates.

    ``volumes`` [B,J,X,Y,Z] float32 (NCDHW, contiguous), ``coord_volumes`` [B,X,Y,Z,3] (any batch stride;
    sample 0 is used for all — the reference's grid is a stride-0 expand).  Returns
    (coordinates [B,J,3], volumes [B,J,X,Y,Z]) with the softmax (or ReLU, ``softmax=False``) applied.
    """
    _lib.require_hip(volumes)
    B, J, X, Y, Z = volumes.shape
    vol = volumes.contiguous().float()
    coord = coord_volumes[0].contiguous().float()
    out_vol = torch.empty_like(vol)
    joints = torch.empty((B, J, 3), device=vol.device, dtype=torch.float32)
    _lib.softargmax3d(vol, coord, out_vol, joints, B * J, X * Y * Z, 1 if softmax else 0)
    return joints, out_vol


def _volume_args(what, volumes, coord_volumes, joints=None, cubic=False):
    """What the operators over the softmaxed volumes check alike: ``volumes`` [B,J,X,Y,Z] float32 on a HIP device (X = Y = Z when
    ``cubic``), ``coord_volumes`` [>=1,X,Y,Z,3], ``joints`` None or [B,J,3] on a HIP device.  Returns B, J, (X, Y, Z) and the flat
    float32 [X Y Z, 3] coordinates of sample 0 on the device of the volumes."""
    _lib.require_hip(volumes, joints)
    if volumes.dim() != 5 or volumes.dtype != torch.float32 or (cubic and not volumes.shape[2] == volumes.shape[3] == volumes.shape[4]):
        raise _lib.HipExtensionError("%s: volumes must be [B,J,%s] float32, got %s %s"
                                     % (what, "G,G,G" if cubic else "X,Y,Z", tuple(volumes.shape), volumes.dtype))
    B, J = int(volumes.shape[0]), int(volumes.shape[1])
    shape = tuple(int(v) for v in volumes.shape[2:])
    if tuple(coord_volumes.shape[1:]) != shape + (3,) or coord_volumes.shape[0] < 1:
        raise _lib.HipExtensionError("%s: coord_volumes %s does not match volumes %s"
                                     % (what, tuple(coord_volumes.shape), tuple(volumes.shape)))
    if joints is not None and tuple(joints.shape) != (B, J, 3):
        raise _lib.HipExtensionError("%s: joints %s, expected %s" % (what, tuple(joints.shape), (B, J, 3)))
    return B, J, shape, coord_volumes[0].to(device=volumes.device, dtype=torch.float32).contiguous()


def _per_frame(result, keys, size_key):
    """A dict of device tensors with a leading batch dimension as a list of per-frame dicts of numpy arrays (``keys`` without the
    batch dimension; ``size_key`` names the entry whose length is the batch)."""
    host = {k: result[k].cpu().numpy() for k in keys}
    return [{k: host[k][b].copy() for k in keys} for b in range(host[size_key].shape[0])]


STAT_KEYS = ("cov", "sigma", "entropy", "peak_prob", "peak_index", "peak_coord")


def joint_statistics(volumes, coord_volumes, joints, scratch=None):
    """How far to trust each soft-argmax joint (no counterpart in the reference): statistics of the softmaxed ``volumes``
    [B,J,X,Y,Z] float32 as ``integrate_tensor_3d_with_coordinates`` returns them, about the ``joints`` [B,J,3] it returned with
    them.  ``coord_volumes`` [>=1,X,Y,Z,3]: sample 0 is used, as there.  One pass over the volumes on the device
    (``se_joint_stats_f32``); returns a dict of device tensors:

      ``cov``        [B,J,3,3]  sum_n p_n (c_n - joint)(c_n - joint)^T in m^2, symmetric
      ``sigma``      [B,J]      sqrt(trace(cov)) in metres
      ``entropy``    [B,J]      -sum_n p_n ln p_n in nats
      ``peak_prob``  [B,J]      max_n p_n
      ``peak_index`` [B,J]      int32, the lowest flat voxel index that holds it
      ``peak_coord`` [B,J,3]    that voxel's centre

    A (sample, joint) whose volume holds a NaN gets NaN in every float entry and peak_index -1.  ``scratch``: an optional float32
    workspace of at least ``_lib.joint_stats_scratch_elems(B * J)`` elements (allocated per call otherwise)."""
    B, J, (X, Y, Z), coord = _volume_args("joint_statistics", volumes, coord_volumes, joints)
    return _joint_statistics_flat(volumes.contiguous(), coord, joints.contiguous().float(), B, J, X * Y * Z, scratch)


def _joint_statistics_flat(vol, coord, joints, B, J, N, scratch):
    rows = B * J
    stats = torch.empty((rows, _lib.JOINT_STATS_SLOTS), device=vol.device, dtype=torch.float32)
    peak_index = torch.empty((rows,), device=vol.device, dtype=torch.int32)
    _lib.joint_stats(vol, coord, joints, stats, peak_index, rows, N, scratch=scratch)
    s = stats.view(B, J, _lib.JOINT_STATS_SLOTS)
    #                  xx xy xz  xy yy yz  xz yz zz   from cxx cyy czz cxy cxz cyz
    cov = s[..., [0, 3, 4, 3, 1, 5, 4, 5, 2]].view(B, J, 3, 3)
    return {"cov": cov, "sigma": s[..., 11], "entropy": s[..., 6], "peak_prob": s[..., 7],
            "peak_index": peak_index.view(B, J), "peak_coord": s[..., 8:11]}


def joint_statistics_to_numpy(stats):
    """The dict of ``joint_statistics`` as a list of per-frame dicts of numpy arrays (the keys without the batch dimension): what
    demo.py --stats and run_sequence.py --stats_output write."""
    return _per_frame(stats, STAT_KEYS, "sigma")


SCENE_KEYS = ("nearest_dist", "nearest_point", "nearest_index", "range", "sight_index", "in_view", "clearance", "bone_clearance",
              "penetration_depth", "penetrating", "contact")


def scene_check_to_numpy(result):
    """The dict of ``scene_check.SceneConsistency.check`` as a list of per-frame dicts of numpy arrays (the keys without the batch
    dimension): what demo.py --scene_check and run_sequence.py --scene_output write."""
    host = {k: result[k].cpu().numpy() for k in SCENE_KEYS}
    return [{k: np.array(host[k][b]) for k in SCENE_KEYS} for b in range(host["range"].shape[0])]      # 0-d entries stay arrays


# ----------------------------------------------------------------------------------------------
# scene-constrained joints (csrc/scene_constraint.hip; no counterpart in the reference)
# ----------------------------------------------------------------------------------------------
CONSTRAINT_KEYS = ("joints", "constrained", "free_mass", "moved", "free_peak_prob", "free_peak_index", "free_peak_coord")


def build_sight_table(grid_coord_proj, coord_volume, height, width):
    """The sight table of ``include/sceneego_hip.h`` (host, once per grid and frame size): for every voxel the pixel its centre
    projects to and its distance from the camera.  ``grid_coord_proj`` [N,2] float32 (u, v) as the module holds it, ``coord_volume``
    [..., 3] float32 voxel centres with N rows in all.  Returns CPU tensors (pix int32 [N], rng float32 [N]):
    x = floor((double)u + 0.5), y = floor((double)v + 0.5); pix = y * width + x when u, v are finite and the pixel lies in the
    ``height`` x ``width`` frame, else -1; rng = (float)sqrt(((double)cx cx + (double)cy cy) + (double)cz cz)."""
    height, width = int(height), int(width)
    if height <= 0 or width <= 0 or height * width > 0x7fff0000:
        raise ValueError(f"sight table: frame {height}x{width} not representable")
    uv = grid_coord_proj.detach().to(torch.float32).cpu().numpy().reshape(-1, 2).astype(np.float64)
    c = coord_volume.detach().to(torch.float32).cpu().numpy().reshape(-1, 3).astype(np.float64)
    if uv.shape[0] != c.shape[0]:
        raise ValueError(f"sight table: {uv.shape[0]} projections for {c.shape[0]} voxel centres")
    finite = np.isfinite(uv).all(axis=1)
    with np.errstate(invalid="ignore"):
        x = np.floor(np.where(finite, uv[:, 0], -1.0) + 0.5)
        y = np.floor(np.where(finite, uv[:, 1], -1.0) + 0.5)
    inside = finite & (x >= 0) & (x < width) & (y >= 0) & (y < height)
    pix = np.where(inside, np.where(inside, y, 0.0) * width + np.where(inside, x, 0.0), -1.0).astype(np.int32)
    rng = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(np.float32)
    return torch.from_numpy(pix), torch.from_numpy(rng)


def scene_free_mask(depth, pix, rng, height, width, margin, max_depth, out=None):
    """The free space of the voxel grid, per frame (``se_scene_free_mask_u8``): ``depth`` [B,dh,dw] float32 on the device, the sight
    table ``pix`` / ``rng`` of ``build_sight_table`` on the same device -> uint8 [B,N], 1 where the voxel is free: it projects outside
    the frame, its pixel has no surface (depth <= 0, > ``max_depth`` or NaN), or it is no more than ``margin`` metres behind the
    surface: blocked iff (double)d + margin < (double)rng.  ``out``: an optional uint8 [B,N] buffer."""
    _lib.require_hip(depth, pix, rng)
    if depth.dim() != 3:
        raise _lib.HipExtensionError("scene_free_mask: depth [B,dh,dw] expected, got %s" % (tuple(depth.shape),))
    if out is None:
        out = torch.empty((depth.shape[0], pix.numel()), device=depth.device, dtype=torch.uint8)
    return _lib.scene_free_mask(depth, pix, rng, out, height, width, margin, max_depth)


def constrained_joints(volumes, coord_volumes, free, joints=None, scratch=None):
    """The soft-argmax over the free voxels alone (``se_softargmax3d_masked_f32``; one pass over the volumes on the device).
    ``volumes`` [B,J,X,Y,Z] float32 softmaxed, as ``integrate_tensor_3d_with_coordinates`` returns them; ``coord_volumes``
    [>=1,X,Y,Z,3] (sample 0 is used); ``free`` uint8 [B,X,Y,Z] (or [B,N]) of ``scene_free_mask``; ``joints`` [B,J,3]: the unconstrained
    joints, kept where a row cannot be constrained (NaN there without them).  Returns a dict of device tensors:

      ``joints``          [B,J,3]  sum_n f_n p_n c_n / sum_n f_n p_n (float32 division), or the input joint where free_mass is 0 or NaN
      ``constrained``     [B,J]    bool: the masked expectation was used
      ``free_mass``       [B,J]    sum_n f_n p_n: the probability in front of the depth surface
      ``moved``           [B,J]    metres between the input and the returned joint (NaN without ``joints``)
      ``free_peak_prob``  [B,J]    the largest p_n over the free voxels (0 without a free voxel)
      ``free_peak_index`` [B,J]    int32, the lowest free flat index that holds it (-1 without one)
      ``free_peak_coord`` [B,J,3]  that voxel's centre (NaN without one): the one output that is guaranteed to be free

    Masking and renormalising is a convention, not validated against annotated data, and the mean of a masked distribution is not
    itself guaranteed to lie in free space.  A (sample, joint) whose volume holds a NaN keeps its input joint, with NaN in free_mass,
    free_peak_prob and free_peak_coord and index -1."""
    _lib.require_hip(free)
    B, J, (X, Y, Z), coord = _volume_args("constrained_joints", volumes, coord_volumes, joints)
    N = X * Y * Z
    if free.dtype != torch.uint8 or free.shape[0] != B or free.numel() != B * N:
        raise _lib.HipExtensionError("constrained_joints: free must be uint8 [%d,%d,%d,%d], got %s %s"
                                     % (B, X, Y, Z, tuple(free.shape), free.dtype))
    return _constrained_joints_flat(volumes.contiguous(), coord, free.contiguous(),
                                    None if joints is None else joints.contiguous().float(), B, J, N, scratch)


def _constrained_joints_flat(vol, coord, free, joints, B, J, N, scratch):
    rows = B * J
    out = torch.empty((rows, _lib.MASKED_SLOTS), device=vol.device, dtype=torch.float32)
    peak_index = torch.empty((rows,), device=vol.device, dtype=torch.int32)
    _lib.softargmax3d_masked(vol, coord, free, out, peak_index, rows, J, N, scratch=scratch)
    o = out.view(B, J, _lib.MASKED_SLOTS)
    mass = o[..., 0]
    constrained = mass > 0                                   # false for an empty row (0) and for a NaN row
    before = joints if joints is not None else torch.full((B, J, 3), float("nan"), device=vol.device, dtype=torch.float32)
    after = torch.where(constrained[..., None], o[..., 1:4] / mass[..., None], before)
    d = after - before
    moved = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return {"joints": after, "constrained": constrained, "free_mass": mass, "moved": moved, "free_peak_prob": o[..., 4],
            "free_peak_index": peak_index.view(B, J), "free_peak_coord": o[..., 5:8]}


def scene_constraint_to_numpy(result):
    """The dict of ``VoxelNetwork_depth.constrain_to_scene`` / ``constrained_joints`` as a list of per-frame dicts of numpy arrays (the
    keys without the batch dimension and without the ``free`` mask): what demo.py --constrained_dir and run_sequence.py
    --constrain_output write."""
    return _per_frame(result, CONSTRAINT_KEYS, "free_mass")


# ----------------------------------------------------------------------------------------------
# scene distance field (csrc/scene_field.hip; no counterpart in the reference)
# ----------------------------------------------------------------------------------------------
FIELD_KEYS = ("sites", "d2", "nearest", "distance", "has_scene")                    # of SceneField.build, beside the float "spacing"
EXPECT_KEYS = ("contact_prob", "contact_free_prob", "blocked_prob", "expected_distance", "expected_free_distance", "mass")
LOOKUP_KEYS = ("distance", "nearest_index", "blocked", "contact")
DEFAULT_RADII2 = (1, 4, 9)       # contact radii of 1, 2 and 3 voxel spacings, squared, in voxel index units


def scene_sites(depth, ray_tab, grid, side, min_z, max_depth, out=None):
    """Which voxels of a ``grid``^3 cuboid of ``side`` metres hold scene, per frame (``se_scene_sites_u8``): ``depth`` [B,dh,dw]
    float32 and the calibrated ``ray_tab`` [H,W,3] float64 on the device -> uint8 [B,G,G,G], 1 where a scene point of
    ``se_scene_probe_f64`` (d > 0, d <= ``max_depth``, z > ``min_z``, a finite ray) has the voxel's centre as its nearest:
    q = rint((s - origin) * (G - 1) / side) per axis, half to even, points outside the grid dropped.  ``out``: an optional uint8
    buffer of B * G^3 elements."""
    _lib.require_hip(depth, ray_tab)
    if depth.dim() != 3:
        raise _lib.HipExtensionError("scene_sites: depth [B,dh,dw] expected, got %s" % (tuple(depth.shape),))
    B, G = int(depth.shape[0]), int(grid)
    if out is None:
        out = torch.empty((B, G, G, G), device=depth.device, dtype=torch.uint8)
    return _lib.scene_sites(depth, ray_tab, out, G, side, min_z, max_depth).view(B, G, G, G)


def scene_distance(sites, scratch=None, out=None):
    """The exact Euclidean distance transform of ``sites`` uint8 [B,G,G,G] (any non-zero byte is a site; 2 <= G <= 128), per frame
    (``se_scene_distance_i32``).  Returns (d2, nearest), both int32 [B,G,G,G]: the squared distance to the nearest site in voxel index
    units, and that site's flat index (the lowest among the nearest); 0x7fffffff and -1 in a frame without a site.  ``scratch``: an
    optional uint8 workspace of ``_lib.scene_distance_scratch_bytes(B, G)`` bytes; ``out``: an optional (d2, nearest) pair to fill."""
    _lib.require_hip(sites)
    if sites.dim() != 4 or not sites.shape[1] == sites.shape[2] == sites.shape[3]:
        raise _lib.HipExtensionError("scene_distance: sites [B,G,G,G] expected, got %s" % (tuple(sites.shape),))
    B, G = int(sites.shape[0]), int(sites.shape[1])
    if out is None:
        out = (torch.empty((B, G, G, G), device=sites.device, dtype=torch.int32),
               torch.empty((B, G, G, G), device=sites.device, dtype=torch.int32))
    d2, nearest = _lib.scene_distance(sites, out[0], out[1], B, G, scratch=scratch)
    return d2.view(B, G, G, G), nearest.view(B, G, G, G)


def _radii2(radii2, device):
    """The squared contact radii as (tuple of ints, int32 device tensor): 1..8 of them, non-negative and ascending."""
    r = tuple(int(v) for v in (DEFAULT_RADII2 if radii2 is None else radii2))
    if not 1 <= len(r) <= _lib.EXPECT_MAX_RADII or any(v < 0 or v >= _lib.SCENE_NO_SITE for v in r) or list(r) != sorted(r):
        raise ValueError(f"radii2 = {r}: 1..{_lib.EXPECT_MAX_RADII} ascending non-negative squared radii expected")
    return r, torch.tensor(r, device=device, dtype=torch.int32)


def contact_radii2(contact_radii, spacing):
    """Contact radii in metres -> squared radii in voxel index units, floor((r / spacing)^2) in float64; None -> the default of 1, 2
    and 3 voxel spacings, (1, 4, 9) exactly."""
    if contact_radii is None:
        return DEFAULT_RADII2
    return tuple(int(np.floor((float(r) / float(spacing)) ** 2)) for r in contact_radii)


def scene_expect(volumes, d2, free, radii2=None, scratch=None):
    """The raw sums of ``se_scene_expect_f32``: ``volumes`` [B,J,X,Y,Z] float32 against ``d2`` int32 and ``free`` uint8, both
    [B,X,Y,Z] (or [B,N]) -> float32 [B,J,24] (include/sceneego_hip.h states every slot; nothing is divided)."""
    _lib.require_hip(volumes, d2, free)
    if volumes.dim() != 5 or volumes.dtype != torch.float32:
        raise _lib.HipExtensionError("scene_expect: volumes must be [B,J,X,Y,Z] float32, got %s %s" % (tuple(volumes.shape), volumes.dtype))
    B, J = int(volumes.shape[0]), int(volumes.shape[1])
    N = int(volumes[0, 0].numel())
    for name, t, dtype in (("d2", d2, torch.int32), ("free", free, torch.uint8)):
        if t.dtype != dtype or t.shape[0] != B or t.numel() != B * N:
            raise _lib.HipExtensionError("scene_expect: %s must be %s with %d x %d elements, got %s %s"
                                         % (name, dtype, B, N, tuple(t.shape), t.dtype))
    _, rad = _radii2(radii2, volumes.device)
    return _scene_expect_flat(volumes.contiguous(), d2.contiguous(), free.contiguous(), rad, B, J, N, scratch)


def _scene_expect_flat(vol, d2, free, rad, B, J, N, scratch):
    out = torch.empty((B * J, _lib.EXPECT_SLOTS), device=vol.device, dtype=torch.float32)
    _lib.scene_expect(vol, d2, free, rad, out, B * J, J, N, scratch=scratch)
    return out.view(B, J, _lib.EXPECT_SLOTS)


def scene_expectations(volumes, field, free, radii2=None, scratch=None):
    """A distribution against the scene field, one pass over the volumes on the device (``se_scene_expect_f32``).  ``volumes``
    [B,J,G,G,G] float32 softmaxed (``forward()``'s volumes, the filtered / smoothed / coupled beliefs, the normalised max-marginals);
    ``field``: the dict of ``SceneField.build``; ``free`` uint8 [B,G,G,G] of ``scene_free_mask``; ``radii2``: 1..8 ascending squared
    contact radii in voxel index units (default 1, 4, 9).  Divisions, square roots and thresholds are taken here, in float32 torch.
    Returns a dict of device tensors:

      ``contact_prob``            [B,J,K]  the share of the mass within each radius of the scene: sum p [d2 <= radii2[k]] / mass
      ``contact_free_prob``       [B,J,K]  the same over the free voxels alone (still divided by the whole mass)
      ``blocked_prob``            [B,J]    the share of the mass in blocked voxels, behind the depth surface
      ``expected_distance``       [B,J]    sum p distance / mass in metres; NaN in a frame without a scene
      ``expected_free_distance``  [B,J]    the same over the free voxels, divided by the free mass (mass - blocked mass); NaN in a
                                           frame without a scene or without free mass
      ``mass``                    [B,J]    sum p (1 up to rounding for a softmaxed volume)
      ``radii2``                  [K]      int32, the squared radii used

    Distance is quantised to voxel centres; the radii are conventions, not calibrated.  A (sample, joint) whose volume holds a NaN
    gets NaN everywhere."""
    _, rad = _radii2(radii2, volumes.device)
    raw = scene_expect(volumes, field["d2"], free, radii2, scratch=scratch)
    return _scene_expectations_of(raw, rad, field["has_scene"], float(field["spacing"]))


def _scene_expectations_of(raw, rad, has_scene, spacing):
    K = int(rad.numel())
    mass = raw[..., 0]
    nan = torch.full_like(mass, float("nan"))
    scene = has_scene[:, None].expand_as(mass)
    free_mass = mass - raw[..., 1]
    return {"contact_prob": raw[..., 4:4 + K] / mass[..., None], "contact_free_prob": raw[..., 12:12 + K] / mass[..., None],
            "blocked_prob": raw[..., 1] / mass,
            "expected_distance": torch.where(scene, raw[..., 2] / mass * spacing, nan),
            "expected_free_distance": torch.where(scene & (free_mass > 0), raw[..., 3] / free_mass * spacing, nan),
            "mass": mass, "radii2": rad}


def scene_field_lookup(field, free, index, radii2=None):
    """The field at given voxels: a plain gather.  ``field``: the dict of ``SceneField.build`` for B frames; ``free`` uint8
    [B,G,G,G] of ``scene_free_mask`` (None: nothing counts as blocked); ``index``: any integer tensor [..., B, J] of flat voxel
    indices, -1 (any negative) for an invalid entry - ``SkeletonPrior.sample``'s and ``VolumeSmoother.sample``'s ``index`` (with the
    frames as B), ``solve``'s and the path's ``index``, ``alt_index``, ``free_peak_index``.  Returns a dict of device tensors shaped
    like ``index``:

      ``distance``       float32 metres to the nearest scene voxel (+inf in a frame without a scene, NaN for an invalid entry)
      ``nearest_index``  int32 flat index of that voxel (-1 without one or for an invalid entry)
      ``blocked``        bool: the voxel lies behind the depth surface (False for an invalid entry)
      ``contact``        [..., K] bool: d2 <= radii2[k] (False for an invalid entry)
      ``radii2``         [K] int32, the squared radii used (default 1, 4, 9)"""
    d2 = field["d2"]
    _lib.require_hip(d2, index)
    B = int(d2.shape[0])
    N = int(d2[0].numel())
    if index.dim() < 2 or index.shape[-2] != B or index.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise _lib.HipExtensionError("scene_field_lookup: index must be an integer tensor [..., %d, J], got %s %s"
                                     % (B, tuple(index.shape), index.dtype))
    _, rad = _radii2(radii2, d2.device)
    idx = index.to(device=d2.device, dtype=torch.int64)
    valid = (idx >= 0) & (idx < N)
    base = torch.arange(B, device=d2.device, dtype=torch.int64)[:, None] * N                    # broadcasts over [..., B, J]
    at = torch.where(valid, idx, torch.zeros_like(idx)) + base
    g_d2 = d2.reshape(-1)[at]
    dist = field["distance"].reshape(-1)[at]
    near = field["nearest"].reshape(-1)[at]
    blocked = (free.reshape(-1)[at] == 0) if free is not None else torch.zeros_like(valid)
    return {"distance": torch.where(valid, dist, torch.full_like(dist, float("nan"))),
            "nearest_index": torch.where(valid, near, torch.full_like(near, -1)),
            "blocked": blocked & valid,
            "contact": (g_d2[..., None] <= rad.to(g_d2.dtype)) & valid[..., None], "radii2": rad}


def scene_field_to_numpy(result):
    """A dict of ``scene_expectations`` (or of ``scene_field_lookup`` with ``index`` [B,J]) as a list of per-frame dicts of numpy
    arrays, the keys without the batch dimension and ``radii2`` copied into every frame: what demo.py --scene_field and
    run_sequence.py --scene_field_output write.  A lookup of samples [S,B,J] gives per-frame arrays [S,J]."""
    keys = EXPECT_KEYS if "mass" in result else LOOKUP_KEYS
    host = {k: result[k].cpu().numpy() for k in keys}
    rad = result["radii2"].cpu().numpy()
    lead = host[keys[0]].ndim - (3 if keys[0] in ("contact_prob",) else 2)                        # dimensions before the batch
    nb = host[keys[0]].shape[lead]
    return [{**{k: np.take(host[k], b, axis=lead).copy() for k in keys}, "radii2": rad.copy()} for b in range(nb)]


# ----------------------------------------------------------------------------------------------
# multi-hypothesis joints (csrc/joint_modes.hip; no counterpart in the reference)
# ----------------------------------------------------------------------------------------------
MODES_KEYS = ("coord", "peak_coord", "peak_prob", "mass", "index", "count", "total", "valid")


def joint_modes(volumes, coord_volumes, k=4, radius=2, min_prob=0.0, min_rel=0.02, scratch=None):
    """Where the peaks of each joint's distribution are and how much probability each holds (``se_joint_modes_f32``; one pass over
    the volumes on the device).  ``volumes`` [B,J,G,G,G] float32 softmaxed, as ``integrate_tensor_3d_with_coordinates`` returns them;
    ``coord_volumes`` [>=1,G,G,G,3] (sample 0 is used).  A mode is a voxel with p > 0 and p >= ``min_prob`` whose key (p, -index) is
    greater than that of each of its up to 26 neighbours; the ``k`` (1..16) strongest are returned, strongest first, each with the sums
    over its window of ``radius`` (0..3) voxels each way, clipped to the grid.  Returns a dict of device tensors (``MODES_KEYS``):

      ``coord``      [B,J,K,3]  the window's centroid sum p c / sum p (float32 division): the sub-voxel position of the mode; NaN
                                where the record is unfilled.  With ``radius`` 0 the window is the mode's voxel: its centre is returned
      ``peak_coord`` [B,J,K,3]  the mode voxel's centre (NaN where unfilled)
      ``peak_prob``  [B,J,K]    its probability (0 where unfilled)
      ``mass``       [B,J,K]    the probability inside the window (0 where unfilled); windows of close modes overlap
      ``index``      [B,J,K]    int32 flat voxel index (-1 where unfilled)
      ``count``      [B,J]      int32, the number of filled records, min(K, total)
      ``total``      [B,J]      int32, the number of modes in the volume, uncapped: how multi-modal it is
      ``valid``      [B,J,K]    bool: the record is filled and peak_prob >= ``min_rel`` * peak_prob of mode 0

    A (sample, joint) whose volume holds a NaN gets NaN in every float entry, index -1, count = total = -1 and no valid mode.
    ``scratch``: an optional uint8 workspace of at least ``_lib.joint_modes_scratch_bytes(B * J, G, k)`` bytes."""
    B, J, (G, _, _), coord = _volume_args("joint_modes", volumes, coord_volumes, cubic=True)
    return _joint_modes_flat(volumes.contiguous(), coord, B, J, G, k, radius, min_prob, min_rel, scratch)


def _joint_modes_flat(vol, coord, B, J, G, k, radius, min_prob, min_rel, scratch):
    rows, k = B * J, int(k)
    if not 1 <= k <= _lib.MODES_MAX_K:
        raise _lib.HipExtensionError(f"joint_modes: k = {k} (1..{_lib.MODES_MAX_K}) expected")
    modes = torch.empty((rows, k, _lib.MODES_SLOTS), device=vol.device, dtype=torch.float32)
    index = torch.empty((rows, k), device=vol.device, dtype=torch.int32)
    count = torch.empty((rows,), device=vol.device, dtype=torch.int32)
    total = torch.empty((rows,), device=vol.device, dtype=torch.int32)
    _lib.joint_modes(vol, coord, modes, index, count, total, rows, G ** 3, G, k, radius, min_prob, scratch=scratch)
    m = modes.view(B, J, k, _lib.MODES_SLOTS)
    index = index.view(B, J, k)
    peak, mass = m[..., 0], m[..., 1]
    filled = index >= 0
    nan = torch.full((), float("nan"), device=vol.device, dtype=torch.float32)
    # radius 0: the window is the mode's own voxel and its centroid that voxel's centre; fl(fl(p c) / p) would only add rounding to it
    centroid = torch.where(filled[..., None], m[..., 5:8] if int(radius) == 0 else m[..., 2:5] / mass[..., None], nan)
    valid = filled & (peak >= float(min_rel) * peak[..., :1])
    return {"coord": centroid, "peak_coord": m[..., 5:8], "peak_prob": peak, "mass": mass, "index": index,
            "count": count.view(B, J), "total": total.view(B, J), "valid": valid}


def joint_modes_to_numpy(result):
    """The dict of ``joint_modes`` / ``VoxelNetwork_depth.joint_modes`` as a list of per-frame dicts of numpy arrays (the keys without
    the batch dimension): what demo.py --modes and run_sequence.py --modes_output write."""
    return _per_frame(result, MODES_KEYS, "mass")


# ----------------------------------------------------------------------------------------------
# grid Bayes filter over a sequence (csrc/volume_filter.hip; sceneego_amd/volume_filter.py; no counterpart in the reference)
# ----------------------------------------------------------------------------------------------
FILTER_KEYS = ("joints", "evidence", "restarted")


def volume_filter_to_numpy(result):
    """The dict of ``VolumeFilter.step`` as a list of per-frame dicts of numpy arrays (the keys without the batch dimension and
    without the ``beliefs``; ``shift`` when the step was given joints): what run_sequence.py --filter_info_output writes."""
    return _per_frame(result, FILTER_KEYS + (("shift",) if "shift" in result else ()), "evidence")


SMOOTHER_KEYS = ("joints", "smoothed", "agreement", "filtered_joints", "shift_filtered")


def volume_smoother_to_numpy(result):
    """The dict of ``VolumeSmoother.finish`` as a list of per-frame dicts of numpy arrays (the keys without the frame dimension and
    without the ``beliefs``; ``shift`` when joints were pushed): what run_sequence.py --smooth_info_output writes."""
    return _per_frame(result, SMOOTHER_KEYS + (("shift",) if "shift" in result else ()), "agreement")


SAMPLE_KEYS = ("index", "coord", "kind", "valid")              # [S,T,...]: the frame is the second dimension
SAMPLE_FRAME_KEYS = ("mean", "spread")                          # [T,...]


def volume_samples_to_numpy(result):
    """The dict of ``VolumeSmoother.sample`` as a list of per-frame dicts of numpy arrays: ``index`` [S,J], ``coord`` [S,J,3], ``kind``
    [S,J], ``valid`` [S,J], ``mean`` [J,3], ``spread`` [J] and ``shift`` [J] when joints were pushed: what run_sequence.py
    --sample_output writes."""
    host = {k: result[k].cpu().numpy() for k in SAMPLE_KEYS}
    frame_keys = SAMPLE_FRAME_KEYS + (("shift",) if "shift" in result else ())
    host.update({k: result[k].cpu().numpy() for k in frame_keys})
    return [{**{k: host[k][:, t].copy() for k in SAMPLE_KEYS}, **{k: host[k][t].copy() for k in frame_keys}}
            for t in range(host["mean"].shape[0])]


POSE_SAMPLE_KEYS = ("index", "coord", "kind", "valid", "bone_error")   # [S,B,...]
POSE_SAMPLE_FRAME_KEYS = ("mean", "spread", "sampled")                 # [B,...]


def skeleton_samples_to_numpy(result):
    """The dict of ``SkeletonPrior.sample`` as a list of per-frame dicts of numpy arrays: ``index`` [S,J], ``coord`` [S,J,3], ``kind``
    [S,J], ``valid`` [S,J], ``bone_error`` [S,J-1], ``mean`` [J,3], ``spread`` [J], ``sampled`` (a bool) and ``shift`` [J] when joints
    were given: what run_sequence.py --pose_samples_output writes, and the keys ``metrics.best_of_samples`` and
    ``metrics.best_pose_of_samples`` read."""
    host = {k: result[k].cpu().numpy() for k in POSE_SAMPLE_KEYS}
    frame_keys = POSE_SAMPLE_FRAME_KEYS + (("shift",) if "shift" in result else ())
    host.update({k: result[k].cpu().numpy() for k in frame_keys})
    return [{**{k: host[k][:, t].copy() for k in POSE_SAMPLE_KEYS}, **{k: host[k][t].copy() for k in frame_keys}}
            for t in range(host["mean"].shape[0])]


PATH_KEYS = ("joints", "index", "coord", "jumped", "segment_start", "log_score", "moved")


def volume_path_to_numpy(result):
    """The dict of ``VolumeViterbi.finish`` as a list of per-frame dicts of numpy arrays (the keys without the frame dimension;
    ``shift`` when joints were pushed): what run_sequence.py --path_info_output writes."""
    return _per_frame(result, PATH_KEYS + (("shift",) if "shift" in result else ()), "index")


PATH_ALTERNATIVE_KEYS = ("complete", "margin", "alt_index", "alt_coord", "alt_log_score", "max_marginal_peak_index", "path_is_peak",
                         "runner_up_index", "runner_up_coord", "runner_up_joints", "runner_up_jumped", "runner_up_anchor",
                         "runner_up_margin")


def volume_path_alternatives_to_numpy(result):
    """The dict of ``VolumeViterbi.alternatives`` as a list of per-frame dicts of numpy arrays: the keys of ``volume_path_to_numpy``,
    then the margins, the alternative voxels and the runner-up trajectory (``max_marginals`` is left out: volumes stay on the
    device).  What run_sequence.py --path_alternatives_output writes."""
    return _per_frame(result, PATH_KEYS + (("shift",) if "shift" in result else ()) + PATH_ALTERNATIVE_KEYS, "index")


def _fit_to_json(result, keys, extra):
    """``result[k]`` for k in ``keys`` as plain Python values that ``json.dump`` takes (NaN as null, arrays as lists), with ``extra``."""
    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        if isinstance(v, np.ndarray):
            return plain(v.tolist())
        if isinstance(v, (bool, np.bool_)):
            return bool(v)
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return float(v) if np.isfinite(v) else None
        return v

    out = {k: plain(result[k]) for k in keys}
    out.update({k: plain(v) for k, v in extra.items()})
    return out


def motion_fit_to_json(result, **extra):
    """The dict of ``MotionModelFit.fit`` as plain Python values that ``json.dump`` takes (NaN as null, the per-joint arrays as lists;
    the keys of ``motion_fit.FIT_KEYS``), with ``extra`` added: what run_sequence.py --fit_output writes."""
    from .motion_fit import FIT_KEYS
    return _fit_to_json(result, FIT_KEYS, extra)


def skeleton_fit_to_json(result, **extra):
    """The dict of ``SkeletonModelFit.fit`` in the same plain form (the keys of ``skeleton_fit.FIT_KEYS``), with ``extra`` added: what
    run_sequence.py --skeleton_fit_output writes."""
    from .skeleton_fit import FIT_KEYS
    return _fit_to_json(result, FIT_KEYS, extra)


# ----------------------------------------------------------------------------------------------
# skeleton-coupled joints (csrc/skeleton_prior.hip; sceneego_amd/skeleton_prior.py; the reference has only Skeleton._skeleton_resize)
# ----------------------------------------------------------------------------------------------
SKELETON_KEYS = ("joints", "evidence", "coupled", "bone_error")


def skeleton_couple_to_numpy(result):
    """The dict of ``SkeletonPrior.couple`` as a list of per-frame dicts of numpy arrays (the keys without the batch dimension and
    without the ``beliefs``; ``shift`` and ``bone_error_before`` when the call was given joints): what run_sequence.py
    --skeleton_info_output writes."""
    extra = tuple(k for k in ("shift", "bone_error_before") if k in result)
    return _per_frame(result, SKELETON_KEYS + extra, "evidence")


POSE_KEYS = ("joints", "index", "coord", "jumped", "solved", "log_score", "bone_error")


def skeleton_pose_to_numpy(result):
    """The dict of ``SkeletonPose.solve`` as a list of per-frame dicts of numpy arrays (the keys without the batch dimension; ``shift``
    and ``bone_error_before`` when the call was given joints): what run_sequence.py --map_info_output writes."""
    extra = tuple(k for k in ("shift", "bone_error_before") if k in result)
    return _per_frame(result, POSE_KEYS + extra, "solved")


ALTERNATIVES_KEYS = ("complete", "margin", "alt_log_score", "alt_index", "alt_coord", "alt_pose_index", "alt_pose_jumped", "alt_pose_joints",
                     "max_marginal_peak_index", "pose_is_peak", "runner_up", "runner_up_joints", "runner_up_margin", "runner_up_bone_error")


def skeleton_alternatives_to_numpy(result):
    """The dict of ``SkeletonPose.alternatives`` as a list of per-frame dicts of numpy arrays (the keys of ``skeleton_pose_to_numpy``,
    then ``ALTERNATIVES_KEYS``, then ``max_marginals`` when the call returned them): what run_sequence.py --map_alternatives_output
    writes."""
    extra = tuple(k for k in ("shift", "bone_error_before") if k in result)
    return _per_frame(result, POSE_KEYS + extra + ALTERNATIVES_KEYS + tuple(k for k in ("max_marginals",) if k in result), "solved")
