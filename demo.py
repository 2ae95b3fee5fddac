#!/usr/bin/env python3
"""Drop-in for the reference's ``demo.py`` (``demo.py:19-101``) on MI355X: image dir + depth dir -> one pickle of
15x3 joints per image.

    python demo.py --config experiments/sceneego/test/sceneego.yaml --img_dir data/demo/imgs \\
                   --depth_dir data/demo/depths --output_dir data/demo/out [--weights synthetic] [--stats true] [--scene_check true]

Differences: ``--vis`` (open3d GUI) is out of scope; depth maps are read from ``<img_name>.exr`` (the reference's format:
scanline OpenEXR, NONE/ZIP/PIZ, decoded by ``sceneego_amd/exr.py``) or ``.npy`` / ``.npz``; ``--weights synthetic`` uses the portable seeded weights when no checkpoint exists
(``config.test.model_path`` is loaded strictly otherwise, exactly like ``demo.py:29-31``); ``--stats true`` writes
``<img_name>.stats.pkl`` beside each ``<img_name>.pkl``: the per-joint statistics of ``VoxelNetwork_depth.joint_statistics``.
``--render_dir DIR`` writes ``<img_name>.render.png`` (scene point cloud and skeleton from a third-person view) and
``<img_name>.overlay.png`` (the skeleton in the fisheye frame) per frame, rendered on the device (``sceneego_amd/render.py``);
``--render_format jpg`` writes ``.render.jpg`` / ``.overlay.jpg`` instead: quality-90 4:4:4 JPEG files encoded on the device
(``sceneego_amd/jpeg_encode.py``), so that only compressed bytes cross to the host.  ``--png_encoder device`` does the same for
the PNG files (``sceneego_amd/png_encode.py``: lossless, the same pixels as PIL's files).
``--render_volumes true`` (with ``--render_dir``) also writes ``<img_name>.volumes.render.*`` and ``<img_name>.volumes.overlay.*``: the same
two pictures with the joint probability volumes drawn over them as a maximum-intensity projection in per-joint colours
(``SceneRenderer.render_volumes`` / ``overlay_volumes``); ``--volume_joints 9,10,13,14`` draws only those joints.
``--save_volumes true`` writes ``<img_name>.volumes.npy`` (float32 [15, G, G, G]) beside each ``<img_name>.pkl``, the file
``visualize.py --volumes_path`` reads.
``--scene_check true`` writes ``<img_name>.scene.pkl`` beside each ``<img_name>.pkl``: collision, clearance and contact of the
predicted skeleton against the scene of its own depth map (``sceneego_amd/scene_check.py``: ``SceneConsistency.check``).
``--constrained_dir DIR`` writes ``DIR/<img_name>.pkl``: the joints re-estimated over the free space in front of the depth surface
(``VoxelNetwork_depth.constrain_to_scene``), float32 [15,3] like the prediction, so ``evaluate.py --pred_dir DIR`` reads them; and
``DIR/<img_name>.constraint.pkl``: free_mass, moved, constrained, the free peak, ... of every joint.
``--modes true [--modes_k 4]`` writes ``<img_name>.modes.pkl`` beside each ``<img_name>.pkl``: the strongest peaks of every joint's
volume with their mass and sub-voxel centroid (``VoxelNetwork_depth.joint_modes``); ``evaluate.py --modes`` reads them.
``--scene_field true`` writes ``<img_name>.scene_field.pkl`` beside each ``<img_name>.pkl``: contact probability, blocked probability
and expected distance to the scene of every joint's volume (``VoxelNetwork_depth.scene_expectations``: the volumes against the distance
field of the frame's depth map on the voxel grid; distances are quantised to voxel centres, the contact radii are conventions).
"""
import argparse
import os
import pickle

import numpy as np
import torch

from sceneego_amd import load_config, synth
from sceneego_amd.jpeg_device import JpegFile, decode_jpeg_batch
from sceneego_amd.op import (joint_modes_to_numpy, joint_statistics_to_numpy, scene_check_to_numpy, scene_constraint_to_numpy,
                             scene_field_to_numpy, skeleton_couple_to_numpy)
from sceneego_amd.preprocess import (DEPTH_CLAMP, load_depth, load_image_bgr, prepare_depth, preprocess_image,
                                     preprocess_image_device)
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth

JOINT_NAMES = ["Neck", "Right_shoulder", "Right_elbow", "Right_wrist", "Left_shoulder", "Left_elbow", "Left_wrist",
               "Right_hip", "Right_knee", "Right_ankle", "Right_foot", "Left_hip", "Left_knee", "Left_ankle",
               "Left_foot"]   # heatmap_sequence, reference utils/skeleton.py:17-19


class Demo:
    def __init__(self, config, img_dir, depth_dir, weights=None, image_decode="device", stats=False, render_dir=None, scene_check=False,
                 render_format="png", render_volumes=False, volume_joints=None, save_volumes=None, constrain=False, modes=0,
                 bone_lengths=None, scene_field=False, png_encoder="host"):
        if not torch.cuda.is_available():
            raise RuntimeError("demo.py needs an MI355X (HIP device); the hot path has no CPU fallback")
        self.device = torch.device("cuda")
        self.config = config
        self.image_decode = image_decode
        self.stats = stats
        self.render_dir = render_dir
        if render_format not in ("png", "jpg"):
            raise ValueError(f"render_format must be png or jpg, got {render_format!r}")
        self.render_format = render_format
        if png_encoder not in ("host", "device"):
            raise ValueError(f"png_encoder must be host or device, got {png_encoder!r}")
        self.png_encoder = png_encoder
        self.renderer = None
        self.render_volumes = render_volumes
        self.volume_joints = volume_joints
        self.save_volumes = save_volumes
        self.scene_check = scene_check
        self.constrain = constrain
        self.scene_field = scene_field
        self.modes = int(modes)                # modes kept per joint; 0: off
        self.bone_lengths = bone_lengths       # 14 or 15 metres: couple the joints over the skeleton (--skeleton_dir); None: off
        self.skeleton = None
        self.scene = None
        self.items = []
        for img_name in sorted(os.listdir(img_dir)):
            img_path = os.path.join(img_dir, img_name)
            cands = [os.path.join(depth_dir, img_name + ext) for ext in (".npy", ".npz", ".exr")]
            depth_path = next((c for c in cands if os.path.exists(c)), None)
            if depth_path is None:
                raise Exception(f"The depth map {cands[-1]} does not exist!")
            self.items.append((img_path, depth_path))
        self.network = VoxelNetwork_depth(config, device="cpu")
        if weights == "synthetic":
            self.network.load_state_dict(synth.make_state_dict(self.network.state_dict(), seed=0), strict=True)
        else:
            loads = torch.load(weights or config.test.model_path, map_location="cpu")
            self.network.load_state_dict(loads["state_dict"])
        self.network = self.network.to(self.device).eval()
        self.network.enable_graphs(True)       # batch 1: replay the captured forward
        if self.bone_lengths is not None:
            self.skeleton = self.network.skeleton_prior(self.bone_lengths)

    def run(self):
        results = []
        with torch.no_grad():
            for img_path, depth_path in self.items:
                W, H = self.config.dataset.image_width, self.config.dataset.image_height
                full = (4 * self.config.image_shape[0], 4 * self.config.image_shape[1] + 256)
                jpeg = JpegFile(img_path) if self.image_decode == "device" else None
                if jpeg is not None and jpeg.device and (jpeg.H, jpeg.W) == full:
                    # JPEG decoded on the device (bit-identical to load_image_bgr), then se_preprocess_image_u8
                    frame_u8 = decode_jpeg_batch([jpeg], self.device)
                    img = preprocess_image_device(frame_u8, self.config.image_shape)
                elif (frame := load_image_bgr(img_path)).shape[:2] == full:
                    # raw uint8 frame to the device; crop / quarter-resize / normalise there (se_preprocess_image_u8)
                    frame_u8 = torch.from_numpy(frame).to(self.device)[None]
                    img = preprocess_image_device(frame_u8, self.config.image_shape)
                else:
                    frame_u8 = torch.from_numpy(frame)[None]
                    img = preprocess_image(frame, self.config.image_shape)[None].to(self.device)
                d = load_depth(depth_path)
                if d.shape == (H // 2, W // 2):
                    # half-size depth map (the demo EXRs): upload as is, clamp on the device; the voxeliser's nearest
                    # lookup floor(x * 640 / 1024) equals the reference's two nearest resizes floor(floor(1.25 x) / 2)
                    depth = torch.from_numpy(d).to(self.device).clamp_(max=DEPTH_CLAMP)[None]
                else:
                    depth = prepare_depth(d, W, H)[None].to(self.device)
                kp, _, volumes, _ = self.network(img, self.network.grid_coord_proj_batch, self.network.coord_volumes,
                                                 depth_map_batch=depth)
                assert len(kp) == 1
                results.append({"img_path": img_path, "predicted_keypoints": kp.cpu().numpy()[0]})
                if self.stats:
                    # the volumes are the replayed graph's static buffers: reduced here, before the next frame overwrites them
                    results[-1]["stats"] = joint_statistics_to_numpy(self.network.joint_statistics(volumes, kp))[0]
                if self.constrain:
                    # likewise before the next frame: the volumes are the graph's static buffers
                    results[-1]["constraint"] = scene_constraint_to_numpy(self.network.constrain_to_scene(volumes, kp, depth))[0]
                if self.scene_field:
                    # likewise before the next frame
                    results[-1]["scene_field"] = scene_field_to_numpy(self.network.scene_expectations(volumes, depth=depth))[0]
                if self.modes:
                    # likewise before the next frame
                    results[-1]["modes"] = joint_modes_to_numpy(self.network.joint_modes(volumes, k=self.modes))[0]
                if self.skeleton is not None:
                    # likewise before the next frame
                    results[-1]["skeleton"] = skeleton_couple_to_numpy(self.skeleton.couple(volumes, joints=kp))[0]
                if self.scene_check:
                    results[-1]["scene"] = scene_check_to_numpy(self.check_scene(depth, kp))[0]
                if self.save_volumes is not None:
                    # written frame by frame: a frame's volumes are 15.7 MB, too much to keep for a whole directory
                    os.makedirs(self.save_volumes, exist_ok=True)
                    np.save(os.path.join(self.save_volumes, os.path.split(img_path)[1] + ".volumes.npy"), volumes[0].cpu().numpy())
                if self.render_dir is not None:
                    self.render(os.path.split(img_path)[1], frame_u8, depth, kp, volumes if self.render_volumes else None)
        return results

    def check_scene(self, depth, kp):
        """The scene check of one frame's joints (device tensors); reads the forward's results, changes none."""
        if self.scene is None:
            from sceneego_amd.config import resolve_calibration_path
            from sceneego_amd.scene_check import SceneConsistency
            calib = resolve_calibration_path(self.config.dataset.camera_calibration_path)
            size = (self.config.dataset.image_height, self.config.dataset.image_width)
            shared = self.renderer.ray_tab if self.renderer is not None else None      # one upload of the 31 MB table
            self.scene = SceneConsistency(calib, frame_size=size, device=self.device, ray_tab=shared, config=self.config)
        return self.scene.check(depth, kp)

    def render(self, img_name, frame_u8, depth, kp, volumes=None):
        """<img_name>.render.png and <img_name>.overlay.png (or .jpg) into render_dir, with ``volumes`` also <img_name>.volumes.render.*
        and <img_name>.volumes.overlay.*; reads the forward's results (the volumes before the next forward overwrites them), changes
        none."""
        from sceneego_amd.render import SceneRenderer, save_jpeg, save_png
        if self.renderer is None:
            from sceneego_amd.config import resolve_calibration_path
            calib = resolve_calibration_path(self.config.dataset.camera_calibration_path)
            self.renderer = SceneRenderer(calib, frame_size=(self.config.dataset.image_height, self.config.dataset.image_width),
                                          device=self.device)
            if self.scene is not None:
                self.renderer.ray_tab = self.scene.ray_tab                              # the same table: keep one copy
        os.makedirs(self.render_dir, exist_ok=True)
        save = save_jpeg if self.render_format == "jpg" else save_png
        if self.render_format == "png" and self.png_encoder == "device":
            from sceneego_amd.png_encode import save_png_device as save
        ext = "." + self.render_format
        save(os.path.join(self.render_dir, img_name + ".render" + ext), self.renderer.render(depth, frame_u8, kp)[0])
        save(os.path.join(self.render_dir, img_name + ".overlay" + ext), self.renderer.overlay(frame_u8, kp, depth=depth)[0])
        if volumes is not None:
            side = self.network.cuboid_side
            save(os.path.join(self.render_dir, img_name + ".volumes.render" + ext),
                 self.renderer.render_volumes(depth, frame_u8, kp, volumes, side, joint_mask=self.volume_joints)[0])
            save(os.path.join(self.render_dir, img_name + ".volumes.overlay" + ext),
                 self.renderer.overlay_volumes(frame_u8, kp, volumes, side, depth=depth, joint_mask=self.volume_joints)[0])


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default="experiments/sceneego/test/sceneego.yaml")
    ap.add_argument("--img_dir", type=str, default="data/demo/imgs")
    ap.add_argument("--depth_dir", type=str, default="data/demo/depths")
    ap.add_argument("--output_dir", type=str, default="data/demo/out")
    ap.add_argument("--vis", type=str, default="false")
    ap.add_argument("--weights", type=str, default=None, help="checkpoint path, or 'synthetic'")
    ap.add_argument("--stats", type=str, default="false",
                    help="true: also write <img_name>.stats.pkl (per-joint cov, sigma, entropy, peak_prob, peak_index, peak_coord)")
    ap.add_argument("--render_dir", type=str, default=None,
                    help="also write <img_name>.render.png and <img_name>.overlay.png here (rendered on the device; no display needed)")
    ap.add_argument("--render_format", type=str, default="png", choices=("png", "jpg"),
                    help="with --render_dir: png (PIL on the host) or jpg (quality-90 4:4:4 JPEG encoded on the device)")
    ap.add_argument("--png_encoder", type=str, default="host", choices=("host", "device"),
                    help="with --render_format png: host (PIL) or device (lossless, sceneego_amd/png_encode.py: the same pixels, only "
                         "the compressed bytes cross to the host)")
    ap.add_argument("--render_volumes", type=str, default="false",
                    help="true (with --render_dir): also write <img_name>.volumes.render.* and <img_name>.volumes.overlay.*, the two "
                         "pictures with the joint probability volumes drawn over them")
    ap.add_argument("--volume_joints", type=str, default=None,
                    help="with --render_volumes true: the joints to draw, e.g. 9,10,13,14 (default: all 15)")
    ap.add_argument("--save_volumes", type=str, default="false",
                    help="true: also write <img_name>.volumes.npy (float32 [15,G,G,G]; visualize.py --volumes_path reads it)")
    ap.add_argument("--scene_check", type=str, default="false",
                    help="true: also write <img_name>.scene.pkl (nearest_dist, clearance, bone_clearance, penetration_depth, penetrating, "
                         "contact, ... of the skeleton against the depth map's scene)")
    ap.add_argument("--constrained_dir", type=str, default=None,
                    help="also write <img_name>.pkl here: the joints re-estimated over the free space in front of the depth surface "
                         "(float32 [15,3], readable by evaluate.py --pred_dir), and <img_name>.constraint.pkl (free_mass, moved, ...)")
    ap.add_argument("--scene_field", type=str, default="false",
                    help="true: also write <img_name>.scene_field.pkl (contact_prob, contact_free_prob, blocked_prob, expected_distance, "
                         "expected_free_distance, mass, radii2 of every joint's volume against the depth map's scene on the voxel grid)")
    ap.add_argument("--modes", type=str, default="false",
                    help="true: also write <img_name>.modes.pkl (the strongest peaks of every joint's volume: coord, peak_coord, "
                         "peak_prob, mass, index, count, total, valid)")
    ap.add_argument("--modes_k", type=int, default=4, help="with --modes true: modes kept per joint, 1..16")
    ap.add_argument("--skeleton_dir", type=str, default=None,
                    help="also write <img_name>.pkl here: the joints coupled over the kinematic tree with the bone lengths of "
                         "--bone_lengths (float32 [15,3], readable by evaluate.py --pred_dir), and <img_name>.skeleton.pkl (evidence, "
                         "coupled, bone_error, shift, bone_error_before)")
    ap.add_argument("--bone_lengths", type=str, default=None,
                    help="with --skeleton_dir: a .npy of 14 bone lengths in metres (edges 1..14 of the kinematic tree) or 15 (entry 0 ignored)")
    return ap


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if (args.skeleton_dir is None) != (args.bone_lengths is None):
        raise SystemExit("--skeleton_dir and --bone_lengths go together: single frames cannot estimate the bone lengths")
    if args.vis.lower() == "true":
        raise SystemExit("--vis true (open3d visualisation) is out of scope of this build")
    if args.stats.lower() not in ("true", "false"):
        raise SystemExit("--stats must be true or false")
    args.stats = args.stats.lower() == "true"
    if args.scene_check.lower() not in ("true", "false"):
        raise SystemExit("--scene_check must be true or false")
    args.scene_check = args.scene_check.lower() == "true"
    if not 1 <= args.modes_k <= 16:
        raise SystemExit("--modes_k must be in 1..16")
    for flag in ("render_volumes", "save_volumes", "modes", "scene_field"):
        if getattr(args, flag).lower() not in ("true", "false"):
            raise SystemExit(f"--{flag} must be true or false")
        setattr(args, flag, getattr(args, flag).lower() == "true")
    if args.render_volumes and args.render_dir is None:
        raise SystemExit("--render_volumes true needs --render_dir")
    if args.volume_joints is not None and not args.render_volumes:
        raise SystemExit("--volume_joints needs --render_volumes true")
    from sceneego_amd.render import parse_joint_list
    try:
        args.volume_joints = parse_joint_list(args.volume_joints)
    except ValueError as e:
        raise SystemExit(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)
    config = load_config(args.config)
    demo = Demo(config, args.img_dir, args.depth_dir, weights=args.weights, stats=args.stats, render_dir=args.render_dir,
                scene_check=args.scene_check, render_format=args.render_format, render_volumes=args.render_volumes,
                volume_joints=args.volume_joints, save_volumes=args.output_dir if args.save_volumes else None,
                constrain=args.constrained_dir is not None, modes=args.modes_k if args.modes else 0,
                bone_lengths=np.load(args.bone_lengths) if args.bone_lengths is not None else None, scene_field=args.scene_field,
                png_encoder=args.png_encoder)
    os.makedirs(args.output_dir, exist_ok=True)
    if args.constrained_dir is not None:
        os.makedirs(args.constrained_dir, exist_ok=True)
    for r in demo.run():
        out_path = os.path.join(args.output_dir, os.path.split(r["img_path"])[1] + ".pkl")
        with open(out_path, "wb") as f:
            pickle.dump(r["predicted_keypoints"], f)      # np.float32 [15,3], reference demo.py:88-97
        print(out_path, r["predicted_keypoints"][0])
        if args.stats:
            with open(out_path[:-4] + ".stats.pkl", "wb") as f:
                pickle.dump(r["stats"], f)                # dict of numpy arrays, the keys of op.joint_statistics
        if args.modes:
            with open(out_path[:-4] + ".modes.pkl", "wb") as f:
                pickle.dump(r["modes"], f)                # dict of numpy arrays, the keys of op.MODES_KEYS
        if args.scene_check:
            with open(out_path[:-4] + ".scene.pkl", "wb") as f:
                pickle.dump(r["scene"], f)                # dict of numpy arrays, the keys of SceneConsistency.check
        if args.scene_field:
            with open(out_path[:-4] + ".scene_field.pkl", "wb") as f:
                pickle.dump(r["scene_field"], f)          # dict of numpy arrays, the keys of op.EXPECT_KEYS and radii2
        if args.constrained_dir is not None:
            c = dict(r["constraint"])
            name = os.path.join(args.constrained_dir, os.path.split(r["img_path"])[1])
            with open(name + ".pkl", "wb") as f:
                pickle.dump(np.asarray(c.pop("joints"), dtype=np.float32), f)      # [15,3], the format of the prediction
            with open(name + ".constraint.pkl", "wb") as f:
                pickle.dump(c, f)                         # dict of numpy arrays, the other keys of op.CONSTRAINT_KEYS
        if args.skeleton_dir is not None:
            c = dict(r["skeleton"])
            os.makedirs(args.skeleton_dir, exist_ok=True)
            name = os.path.join(args.skeleton_dir, os.path.split(r["img_path"])[1])
            with open(name + ".pkl", "wb") as f:
                pickle.dump(np.asarray(c.pop("joints"), dtype=np.float32), f)      # [15,3], the format of the prediction
            with open(name + ".skeleton.pkl", "wb") as f:
                pickle.dump(c, f)                         # dict of numpy arrays, the other keys of op.SKELETON_KEYS


if __name__ == "__main__":
    main()
