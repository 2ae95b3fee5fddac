#!/usr/bin/env python3
"""Sequence evaluation of the reference (``test.py`` + ``dataset/test_dataset.py``) on this project's forward: one recorded sequence
-> predicted joints of every frame, MPJPE / PA-MPJPE against its ground truth, frames/s of the whole run.

    python run_sequence.py --root_dir data --seq_name new_diogo1 --estimated_depth_name matterport_green \\
                           --output out/no_body_diogo1.pkl [--weights synthetic] [--depth_decode device|host]
                           [--image_decode device|host] [--streams 2] [--stats_output out/no_body_diogo1.stats.pkl]
                           [--render_dir out/frames [--render_every 10] [--render_format jpg]]
                           [--render_video out/seq.avi [--render_fps 25] [--render_view render|overlay|both] [--render_quality 90]]
                           [--scene_output out/no_body_diogo1.scene.pkl] [--constrain_output out/no_body_diogo1.constraint.pkl]
                           [--modes_output out/no_body_diogo1.modes.pkl [--modes_k 4] [--track_output out/tracked.pkl [--track_sigma 0.1]]]
                           [--filter_output out/filtered.pkl [--filter_info_output out/filter.pkl] [--filter_sigma 0.1]
                            [--filter_radius R] [--filter_floor 1e-3]] [--render_volumes filtered]
                           [--skeleton_output out/skeleton.pkl [--skeleton_info_output out/skeleton_info.pkl] [--bone_lengths FILE.npy]
                            [--bone_frames 64] [--skeleton_tau 0.03] [--skeleton_floor 1e-3]] [--render_volumes coupled]
                           [--map_output out/map.pkl [--map_info_output out/map_info.pkl] [--map_refine 1]]
                           [--map_alternatives_output out/alt.pkl [--map_separation 2]]
                           [--fit_frames 64 [--fit_iterations 8] [--fit_output out/fit.json]]
                           [--skeleton_fit_frames 64 [--skeleton_fit_iterations 8] [--skeleton_fit_output out/skeleton_fit.json]]

Frame list (``TestDataset.get_gt_data``): ``<root>/<seq>/syn.json`` (``ego``, ``ext`` start frames) and ``local_pose_gt.pkl`` (items
with ``ext_id`` and ``ego_pose_gt``); items whose pose is None or whose image ``imgs/img_%06d.jpg`` is missing are skipped; the depth
map is ``<seq>/<estimated_depth_name>/img_%06d.jpg.exr`` or ``<seq>/rendered/depths/img_%06d/Image0001.exr``.  Frames run in
batches of ``config.test.batch_size`` (a partial last batch included).  A small host thread pool reads and parses the JPEGs one batch
ahead; they are decoded on the device (``jpeg_device.decode_jpeg_batch``, bit-identical to PIL) or, with ``--image_decode host``, by
PIL in that pool; the image path is then demo.py's (``se_preprocess_image_u8`` for 1280x1024 frames); depth maps go through
``exr_device.decode_depth_exr_batch(..., out_hw=(1024, 1280))`` (PIZ, ZIP, ZIPS and NONE decoded on the device) or, with
``--depth_decode host``,
through ``exr.py`` + ``prepare_depth`` - the same values either way (``TestDataset.__getitem__``: nearest resize to 1280x1024, clamp
to 10 m).  The pickle holds the list of float32 [15, 3] predictions, as ``test.py`` writes it.  ``--stats_output`` adds a second
pickle: the per-joint statistics of every frame (``VoxelNetwork_depth.joint_statistics``), taken per batch on the stream it ran on.
``--render_format jpg`` writes the pair as JPEG files and ``--render_video`` the picked frames as one Motion-JPEG AVI, both encoded
on the device (``sceneego_amd/jpeg_encode.py``).  ``--render_dir`` writes ``<img_name>.render.png`` and ``<img_name>.overlay.png`` (``sceneego_amd/render.py``: the scene point cloud
with the skeleton from a third-person view, and the skeleton in the fisheye frame) for every ``--render_every``-th frame, batched
through one ``SceneRenderer`` once the joints of the batch are final; the forward is the same with and without it.
``--scene_output`` adds a pickle of the per-frame scene checks (``sceneego_amd/scene_check.py``: collision, clearance and contact of
each predicted skeleton against the scene of its own depth map), taken per batch on the stream it ran on, and prints their summary
(``metrics.scene_summary``) at the end.
``--constrain_output`` adds a pickle of the per-frame scene constraints (``VoxelNetwork_depth.constrain_to_scene``: the joints
re-estimated over the free space in front of the depth surface, free_mass, moved, ...), taken per batch on the stream it ran on; with
``--scene_output`` the scene check also runs on the constrained joints and both summaries are printed.
``--modes_output`` adds a pickle of the per-frame joint modes (``VoxelNetwork_depth.joint_modes``: the ``--modes_k`` strongest peaks of
every joint's volume with their mass and sub-voxel centroid), taken per batch on the stream it ran on.  ``--track_output`` then writes
a pickle in the format of ``--output`` whose joints are one mode per joint and frame, picked over the whole sequence by
``sceneego_amd.track.select_modes`` (``--track_sigma`` metres per frame; the soft-argmax joint where a frame has no valid mode), and
prints its MPJPE beside the soft-argmax's: mass as likelihood and a Gaussian step are a convention, not calibrated.
``--filter_output`` writes a pickle in the format of ``--output`` whose joints are those of a grid Bayes filter run over the volumes of
the sequence on the device (``VoxelNetwork_depth.volume_filter``, ``sceneego_amd/volume_filter.py``: the whole [15,G,G,G] belief is
blurred by a Gaussian step of ``--filter_sigma`` metres truncated at ``--filter_radius`` voxels, mixed with a uniform floor
``--filter_floor`` and multiplied by the next frame's volumes), once per batch on the stream the batch ran on and in frame order
across the pipelined streams; ``--filter_info_output`` adds the per-frame dicts (joints, evidence, restarted, shift) and
``--render_volumes filtered`` draws the beliefs instead of the raw volumes.  It prints its MPJPE beside the soft-argmax's: the volume
as likelihood, the Gaussian step and the floor are a convention, not calibrated.
``--smooth_output`` writes a pickle in the format of ``--output`` whose joints are those of the forward-backward smoother that goes with
that filter (``VoxelNetwork_depth.volume_smoother``, ``sceneego_amd/volume_smoother.py``): the filter runs as above, the volumes and the
beliefs of every frame stay on the device (31.4 MB per frame at 15 x 64^3; at most ``--smooth_max_gb``, default half of the free device
memory) and a backward pass at the end of the sequence conditions every frame on the whole track.  It uses ``--filter_sigma``,
``--filter_radius`` and ``--filter_floor`` and implies the filter, so ``--filter_output`` may be given as well and gets the same joints
as without it; ``--smooth_info_output`` adds the per-frame dicts (joints, smoothed, agreement, filtered_joints, shift_filtered, shift).
Smoothed beliefs are not rendered: frames are rendered per batch, before the future exists.
``--sample_output`` writes a pickle of per-frame dicts of ``--samples`` (default 16) whole trajectories per joint drawn from the posterior
of that smoother's model (``VolumeSmoother.sample``, seed ``--sample_seed``): index, coord, kind, valid [S,15,...], mean, spread and shift.
It implies the smoother, draws before the smoother finishes, and prints the mean spread and the best-of-N MPJPE (the closest valid sample
of every joint) beside the smoothed MPJPE.  The samples are from the model's posterior given the volumes read as likelihoods: not calibrated.
``--scene_field_output sf.pkl [--contact_radii 1,2,3]`` writes a pickle of per-frame dicts of the volumes against the scene distance
field of each frame's depth map on the voxel grid (``VoxelNetwork_depth.scene_expectations``: contact probability within the radii,
given in voxel spacings, blocked probability and expected distance of every joint): ``volumes`` for the raw volumes, ``coupled`` and
``filtered`` for the beliefs of ``--skeleton_output`` / ``--filter_output`` where those are on, and with ``--pose_samples_output``
``pose_samples``, the sampled poses looked up in the field (``op.scene_field_lookup``); prints ``metrics.scene_field_summary``.
Distances are quantised to voxel centres and the radii are conventions: nothing is calibrated.
``--pose_samples_output`` writes a pickle of per-frame dicts of ``--pose_samples`` (default 16) whole poses drawn from the posterior of
the skeleton model (``SkeletonPrior.sample``, seed ``--pose_sample_seed``, the frame's number in the sequence as its global index):
index, coord, kind, valid [S,15,...], bone_error [S,14], mean, spread, sampled and shift.  It uses ``--bone_lengths`` /
``--bone_frames``, ``--skeleton_tau`` and ``--skeleton_floor`` exactly as ``--skeleton_output`` does, and the fitted values with
``--skeleton_fit_frames``.

``--skeleton_output`` writes a pickle in the format of ``--output`` whose joints are coupled over the kinematic tree inside every frame
(``VoxelNetwork_depth.skeleton_prior``, ``sceneego_amd/skeleton_prior.py``: belief propagation over the fifteen volumes with a
bone-length shell of ``--skeleton_tau`` metres on every edge and a uniform floor ``--skeleton_floor``), per batch on the stream the
batch ran on.  The bone lengths come from ``--bone_lengths`` (a .npy of 14 or 15 metres) or, without it, from a first forward pass over
at most ``--bone_frames`` evenly spaced frames (``estimate_bone_lengths``: the per-bone median of the soft-argmax joints' distances).
``--skeleton_info_output`` adds the per-frame dicts (joints, evidence, coupled, bone_error, shift, bone_error_before) and
``--render_volumes coupled`` draws the coupled beliefs.  With ``--filter_output`` as well the order is couple, then filter (with
``--smooth_output``: couple, filter, smooth): the filter runs on the coupled beliefs.  The volume as likelihood, the shell and the floor are a convention, not calibrated.
``--map_output`` writes a pickle in the format of ``--output`` whose joints are the single most probable pose of every frame under
the same bone-length model (``VoxelNetwork_depth.skeleton_pose``, ``sceneego_amd/skeleton_pose.py``: the max-product pass over the
kinematic tree, where ``--skeleton_output`` gives the expectations of the marginals), taken from the raw volumes per batch on the stream
the batch ran on; each pose voxel is refined to the centroid of its joint's volume over a window of ``--map_refine`` voxels (0..3,
default 1).  ``--bone_lengths``, ``--bone_frames``, ``--skeleton_tau`` and ``--skeleton_floor`` are used exactly as ``--skeleton_output``
uses them.  ``--map_info_output`` adds the per-frame dicts (joints, index, coord, jumped, solved, log_score, bone_error, shift,
bone_error_before).  ``evaluate.py --pred_dir map.pkl [--bones]`` reads the file.  The pose is all-or-nothing where the marginals hedge.
``--map_alternatives_output`` says how close the second-best pose was (``SkeletonPose.alternatives``: the downward max-product pass;
it implies the ``--map_*`` model options and runs in place of ``solve``, with the same pose bit for bit): a pickle of per-frame dicts
with the pose's entries and, per joint, the log margin to the best pose that places it more than ``--map_separation`` voxels (default
2) away, that pose, and the runner-up pose of the frame; prints the mean runner-up margin and the share of frames below ln 2.
``evaluate.py --pred_dir map.pkl --alternatives alt.pkl [--gt gt.pkl]`` reads it.  A convention of its own: a window on one joint.
``--path_output`` writes a pickle in the format of ``--output`` whose joints lie on the most probable trajectory of every joint through
the sequence's volumes (``VoxelNetwork_depth.volume_path``, ``sceneego_amd/volume_viterbi.py``: the max-product pass on the filter's
motion model, ``--filter_sigma``, ``--filter_radius`` and ``--filter_floor``): every batch is pushed on the stream it ran on, the
back-pointers and, with ``--path_refine`` > 0 (default 1), the volumes stay on the device (31.4 MB per frame at 15 x 64^3; at most
``--path_max_gb``) and a walk back at the end of the sequence picks the path.  ``--path_info_output`` adds the per-frame dicts (joints,
index, coord, jumped, segment_start, log_score, moved, shift).  With ``--skeleton_output`` it runs on the coupled beliefs.  It prints
its MPJPE beside the others; ``evaluate.py --pred_dir path.pkl`` reads the file like ``--output``.
``--path_alternatives_output`` implies those options, keeps every frame's scores as well (47.2 MB per frame in all) and runs the
backward max-product pass at the end of the sequence (``VolumeViterbi.alternatives``): the per-frame dicts also carry the margin by
which every frame of the path was decided, the best trajectory that lies further than ``--path_separation`` voxels (default 2) from
the path in that frame, and the runner-up trajectory of every segment.  It prints the mean runner-up margin and the share of the
joint-frames whose margin is below ln 2; ``evaluate.py --pred_dir path.pkl --path_alternatives alt.pkl [--gt gt.pkl]`` reads it.
``--fit_frames F`` fits the motion model of those three to the sequence before the main pass (``VoxelNetwork_depth.motion_fit``,
``sceneego_amd/motion_fit.py``: at most ``--fit_iterations`` EM iterations for sigma and floor over the raw volumes of the first F
consecutive frames, from ``--filter_sigma`` / ``--filter_floor`` at the fixed ``--filter_radius``), prints the start and end values
with their log-likelihoods, writes the whole result to ``--fit_output`` (JSON) and runs ``--filter_output``, ``--smooth_output`` and
``--path_output`` on the fitted values; their per-frame info dicts then carry ``sigma``, ``floor`` and ``radius``.  It is a
maximum-likelihood fit to the network's own volumes read as likelihoods, on this one sequence: not a validation against ground truth.
``--skeleton_fit_frames F`` fits the skeleton model the same way (``VoxelNetwork_depth.skeleton_fit``, ``sceneego_amd/skeleton_fit.py``:
at most ``--skeleton_fit_iterations`` EM iterations for the bone lengths, tau and floor over the raw volumes of F evenly spaced frames,
chosen as ``--bone_frames`` chooses its frames, from ``--bone_lengths`` or the median estimate, ``--skeleton_tau`` and
``--skeleton_floor``), prints the start and fitted values with their log-likelihoods, writes the whole result to
``--skeleton_fit_output`` (JSON) and runs ``--skeleton_output`` and ``--map_output`` on the fitted values; their per-frame info dicts
then carry ``bone_lengths``, ``tau`` and ``floor``.  If the fitted shells need more than min(24, G - 1) voxels it exits with
``SkeletonPrior``'s message.  The same caveat holds: a fit to the volumes, not a validation.
"""
import argparse
import json
import os
import pickle
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_WORKERS = 16


def frame_list(root_dir, seq_name, estimated_depth_name=None):
    """(image paths, ground-truth poses, depth paths) of a sequence, in the order and with the skips of ``TestDataset.get_gt_data``."""
    base = os.path.join(root_dir, seq_name)
    img_dir = os.path.join(base, "imgs")
    depth_dir = os.path.join(base, estimated_depth_name) if estimated_depth_name is not None else os.path.join(base, "rendered", "depths")
    with open(os.path.join(base, "syn.json")) as f:
        syn = json.load(f)
    with open(os.path.join(base, "local_pose_gt.pkl"), "rb") as f:
        pose_gt = pickle.load(f)
    images, poses, depths = [], [], []
    for item in pose_gt:
        pose = item["ego_pose_gt"]
        if pose is None:
            continue
        ego_id = item["ext_id"] - syn["ext"] + syn["ego"]
        img = os.path.join(img_dir, "img_%06d.jpg" % ego_id)
        if not os.path.exists(img):
            continue
        images.append(img)
        if estimated_depth_name is not None:
            depths.append(os.path.join(depth_dir, "img_%06d.jpg.exr" % ego_id))
        else:
            depths.append(os.path.join(depth_dir, "img_%06d" % ego_id, "Image0001.exr"))
        poses.append(pose)
    return images, poses, depths


class SequenceRunner:
    def __init__(self, config, weights=None, streams=1, depth_decode="device", workers=8, image_decode="device"):
        from sceneego_amd import synth
        from sceneego_amd.pipeline import PipelinedForward
        from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
        if not torch.cuda.is_available():
            raise RuntimeError("run_sequence.py needs an MI355X (HIP device); the hot path has no CPU fallback")
        if depth_decode not in ("device", "host"):
            raise ValueError(f"--depth_decode must be device or host, got {depth_decode}")
        if image_decode not in ("device", "host"):
            raise ValueError(f"--image_decode must be device or host, got {image_decode}")
        self.image_decode = image_decode
        self.device = torch.device("cuda")
        self.config = config
        self.depth_decode = depth_decode
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        net = VoxelNetwork_depth(config, device="cpu", verbose=False)
        if weights == "synthetic":
            net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
        else:
            loads = torch.load(weights or config.test.model_path, map_location="cpu")
            net.load_state_dict(loads["state_dict"])
        self.net = net.to(self.device).eval()
        self.pipe = PipelinedForward(self.net, n_streams=streams) if streams > 1 else None
        self.renderer = None
        self.encoder = None
        self.png_encoder = None
        self.video = None
        self.render_options = {"format": "png", "png_encoder": "host", "video": None, "fps": 25, "view": "render", "quality": 90,
                               "renderer": {}}
        self.scenes = {}

    def _scene(self, slot=0):
        """The SceneConsistency of a stream slot: one workspace per slot, one ray table for all (and for the renderer)."""
        from sceneego_amd.config import resolve_calibration_path
        from sceneego_amd.scene_check import SceneConsistency
        if slot not in self.scenes:
            shared = next((s.ray_tab for s in self.scenes.values()), self.renderer.ray_tab if self.renderer is not None else None)
            size = (self.config.dataset.image_height, self.config.dataset.image_width)
            if shared is not None and tuple(shared.shape[:2]) != size:
                shared = None
            self.scenes[slot] = SceneConsistency(resolve_calibration_path(self.config.dataset.camera_calibration_path), frame_size=size,
                                                 device=self.device, ray_tab=shared, config=self.config)
        return self.scenes[slot]

    def _images(self, frames):
        from sceneego_amd.preprocess import preprocess_image, preprocess_image_device, preprocess_jpeg_batch
        shape = self.config.image_shape
        if self.image_decode == "device":             # parsed JpegFile objects
            return preprocess_jpeg_batch(frames, self.device, shape)
        full = (4 * shape[0], 4 * shape[1] + 256)
        if all(f.shape[:2] == full for f in frames):
            u8 = torch.from_numpy(np.stack(frames)).to(self.device)
            return preprocess_image_device(u8, shape)
        return torch.stack([preprocess_image(f, shape) for f in frames]).to(self.device)

    def _depths(self, paths):
        from sceneego_amd.exr_device import decode_depth_exr_batch
        from sceneego_amd.preprocess import DEPTH_CLAMP, load_depth, prepare_depth
        W, H = self.config.dataset.image_width, self.config.dataset.image_height
        if self.depth_decode == "device":
            return decode_depth_exr_batch(paths, self.device, out_hw=(H, W), clamp=DEPTH_CLAMP)
        return torch.stack([prepare_depth(load_depth(p), W, H) for p in paths]).to(self.device)

    def _frames_u8(self, frames):
        """uint8 [n, H, W, 3] (B, G, R) on the device of the frames picked for rendering: a second decode of those frames only, so
        that the image path of the forward stays exactly what it is without --render_dir."""
        from sceneego_amd.jpeg_device import decode_jpeg_batch
        if self.image_decode == "device":
            if all(f.device for f in frames) and len({(f.H, f.W) for f in frames}) == 1:
                return decode_jpeg_batch(frames, self.device)
            frames = [f.host_decode() for f in frames]
        return torch.from_numpy(np.stack(frames)).to(self.device)

    def _render(self, job, kp):
        """The image pair of every picked frame of one batch and / or their video frames; ``kp``: the batch's final joints on the
        host.  PNG files go through the host unless ``--png_encoder device``; those, JPEG files and video frames are encoded on the
        device in the batch they were rendered in, and only their compressed bytes cross to the host."""
        from sceneego_amd.config import resolve_calibration_path
        from sceneego_amd.render import SceneRenderer, save_png
        render_dir, pick, names, frames_u8, depth, vol = job
        opt = self.render_options
        if self.renderer is None:
            self.renderer = SceneRenderer(resolve_calibration_path(self.config.dataset.camera_calibration_path),
                                          frame_size=tuple(frames_u8.shape[1:3]), device=self.device, **opt["renderer"])
        joints = kp[pick]

        def write(view, images):
            if render_dir is None:
                return
            if opt["format"] == "png" and opt["png_encoder"] == "device":
                for name, data in zip(names, self._png_encoder().encode(images)):
                    with open(os.path.join(render_dir, f"{name}.{view}.png"), "wb") as f:
                        f.write(data)
            elif opt["format"] == "png":
                images_h = images.cpu()
                for k, name in enumerate(names):
                    save_png(os.path.join(render_dir, f"{name}.{view}.png"), images_h[k])
            else:
                for name, data in zip(names, self._encoder().encode(images, quality=90, subsampling="444")):
                    with open(os.path.join(render_dir, f"{name}.{view}.jpg"), "wb") as f:
                        f.write(data)

        volumes = bool(opt.get("volumes"))
        if not volumes or render_dir is not None:           # with volumes and a video only, nobody looks at the plain pair
            scene = self.renderer.render(depth, frames_u8, joints)
            over = self.renderer.overlay(frames_u8, joints, depth=depth)
            write("render", scene)
            write("overlay", over)
        if volumes:
            # drawn into the buffers the plain pair was in: that pair has been written by now
            side, which = self.net.cuboid_side, opt.get("volume_joints")
            scene = self.renderer.render_volumes(depth, frames_u8, joints, vol[pick], side, joint_mask=which)
            over = self.renderer.overlay_volumes(frames_u8, joints, vol[pick], side, depth=depth, joint_mask=which)
            write("volumes.render", scene)
            write("volumes.overlay", over)
        if opt["video"] is not None:
            if opt["view"] == "both":
                if scene.shape[1] != over.shape[1]:
                    raise ValueError(f"--render_view both puts the views side by side and needs equal heights: the rendered view is "
                                     f"{scene.shape[1]} rows, the frame {over.shape[1]}; pass --render_size {over.shape[1]}xW")
                images = torch.cat([scene, over], dim=2)
            else:
                images = scene if opt["view"] == "render" else over
            if self.video is None:
                from sceneego_amd.jpeg_encode import MjpegWriter
                os.makedirs(os.path.dirname(os.path.abspath(opt["video"])), exist_ok=True)
                self.video = MjpegWriter(opt["video"], images.shape[2], images.shape[1], opt["fps"])
            for data in self._encoder().encode(images, quality=opt["quality"], subsampling="420"):      # what players expect of MJPG
                self.video.write(data)

    def _encoder(self):
        if self.encoder is None:
            from sceneego_amd.jpeg_encode import JpegEncoder
            self.encoder = JpegEncoder(self.device)
        return self.encoder

    def _png_encoder(self):
        if self.png_encoder is None:
            from sceneego_amd.png_encode import PngEncoder
            self.png_encoder = PngEncoder(self.device)
        return self.png_encoder

    @torch.no_grad()
    def fit_motion(self, images, depths, batch_size, model, iterations=8, max_bytes=None):
        """The first pass of ``--fit_frames``: the forward over the consecutive frames ``images`` / ``depths`` in batches, their raw
        volumes pushed into ``VoxelNetwork_depth.motion_fit(**model)`` (``model``: a dict of ``sigma`` / ``radius`` / ``floor``, the
        values the fit starts from) and the dict of its ``fit(iterations=iterations)``."""
        from sceneego_amd.jpeg_device import JpegFile
        from sceneego_amd.preprocess import load_image_bgr
        load = JpegFile if self.image_decode == "device" else load_image_bgr
        fit = self.net.motion_fit(**model, max_bytes=max_bytes)
        for i in range(0, len(images), batch_size):
            img = self._images([load(p) for p in images[i:i + batch_size]])
            depth = self._depths(depths[i:i + batch_size])
            _, _, vol, _ = self.net(img, self.net.grid_coord_proj_batch, self.net.coord_volumes, depth_map_batch=depth)
            fit.push(vol)                                     # a copy: the next forward overwrites the volumes
        result = fit.fit(iterations=iterations)
        fit.reset()
        return result

    @torch.no_grad()
    def fit_skeleton(self, images, depths, batch_size, model, iterations=8, max_bytes=None):
        """The first pass of ``--skeleton_fit_frames``: the forward over the frames ``images`` / ``depths`` in batches, their raw
        volumes pushed into ``VoxelNetwork_depth.skeleton_fit(**model)`` (``model``: a dict of ``bone_lengths`` / ``tau`` / ``floor``,
        the values the fit starts from) and the dict of its ``fit(iterations=iterations)``."""
        from sceneego_amd.jpeg_device import JpegFile
        from sceneego_amd.preprocess import load_image_bgr
        load = JpegFile if self.image_decode == "device" else load_image_bgr
        fit = self.net.skeleton_fit(**model, max_bytes=max_bytes)
        for i in range(0, len(images), batch_size):
            img = self._images([load(p) for p in images[i:i + batch_size]])
            depth = self._depths(depths[i:i + batch_size])
            _, _, vol, _ = self.net(img, self.net.grid_coord_proj_batch, self.net.coord_volumes, depth_map_batch=depth)
            fit.push(vol)                                     # a copy: the next forward overwrites the volumes
        result = fit.fit(iterations=iterations)
        fit.reset()
        return result

    @torch.no_grad()
    def run(self, images, depths, batch_size, stats=False, render_dir=None, render_every=1, scene=False, render_format="png",
            render_video=None, render_fps=25, render_view="render", render_quality=90, render_size=None, render_volumes=False,
            volume_joints=None, constrain=False, modes=0, filter=None, render_filtered=False, skeleton=None, render_coupled=False,
            smooth=None, path=None, map_pose=None, sample=None, pose_sample=None, scene_field=None, png_encoder="host"):
        """Predicted [15,3] joints of every frame; with ``stats`` a pair (joints, per-frame statistics dicts).  ``render_dir``: also
        write the rendered image pair (``render_format``: png or jpg) of every ``render_every``-th frame there.  ``render_video``:
        those frames (``render_view``: render, overlay or both side by side) as one Motion-JPEG AVI.  ``scene``: the per-frame
        scene-check dicts are appended to what is returned (joints, [statistics,] scene checks).  ``render_volumes``: also write
        ``<img_name>.volumes.render.*`` / ``.volumes.overlay.*`` (the joint probability volumes of ``volume_joints``, default all, drawn
        over the pair), and the video shows those views.  ``constrain``: the per-frame scene-constraint dicts are appended after
        those, and with ``scene`` the scene checks of the constrained joints after them.  ``modes`` = k > 0: the per-frame joint-mode
        dicts (``VoxelNetwork_depth.joint_modes(k=modes)``) are appended after those.  ``filter``: a dict of ``sigma`` / ``radius`` /
        ``floor`` for ``VoxelNetwork_depth.volume_filter``: the whole sequence is one track, filtered batch by batch in frame order on
        the stream each batch ran on, and the per-frame filter dicts are appended last; ``render_filtered`` (with ``render_volumes``)
        draws its beliefs instead of the raw volumes.  ``skeleton``: a dict of ``bone_lengths`` / ``tau`` / ``floor`` for
        ``VoxelNetwork_depth.skeleton_prior``: every batch's joints are coupled over the kinematic tree on the stream the batch ran on
        and the per-frame skeleton dicts are appended after the filter's; ``render_coupled`` (with ``render_volumes``) draws the
        coupled beliefs.  With ``filter`` as well the order is couple, then filter: the filter runs on the coupled beliefs (its
        ``shift`` is still measured from the soft-argmax joints).  ``smooth`` (with ``filter``): a dict with ``max_bytes`` for
        ``VoxelNetwork_depth.volume_smoother``: the filter is the smoother's own, every batch is pushed instead of stepped, and the
        per-frame dicts of its ``finish()``, run once behind the last batch, are appended after the skeleton's.  ``path``: a dict of
        ``sigma`` / ``radius`` / ``floor`` / ``refine`` / ``max_bytes`` for ``VoxelNetwork_depth.volume_path``: every batch's volumes
        (with ``skeleton`` the coupled beliefs) are pushed on the stream the batch ran on, and the per-frame dicts of its ``finish()``
        are appended after those.  ``map_pose``: a dict of ``bone_lengths`` / ``tau`` / ``floor`` / ``refine`` for
        ``VoxelNetwork_depth.skeleton_pose``, and optionally ``separation`` (then ``SkeletonPose.alternatives`` runs in place of
        ``solve`` and the dicts carry its entries too): the most probable pose of every frame is taken from the batch's raw volumes on the stream
        the batch ran on and the per-frame pose dicts are appended after those.  ``sample`` (with ``smooth``): a dict of ``samples`` /
        ``seed`` for ``VolumeSmoother.sample``, drawn once behind the last batch and before ``finish()``; the per-frame sample dicts
        are appended after those.  ``pose_sample``: a dict of ``bone_lengths`` / ``tau`` / ``floor`` / ``samples`` / ``seed``: whole poses
        drawn from the skeleton posterior of every batch's raw volumes (``SkeletonPrior.sample`` with the running frame count as
        ``first_frame``) on the stream the batch ran on; the per-frame pose-sample dicts are appended after those.  ``scene_field``: a dict
        with ``radii2`` (squared contact radii in voxel spacings, or None for 1, 4, 9): every batch's volumes - and the coupled and filtered
        beliefs, and the sampled poses, where those are on - against the scene distance field of the batch's depth maps
        (``VoxelNetwork_depth.scene_expectations``, ``op.scene_field_lookup``) on the stream the batch ran on; the per-frame dicts
        (``volumes``, ``coupled``, ``filtered``, ``pose_samples``) are appended last."""
        from sceneego_amd.jpeg_device import JpegFile
        from sceneego_amd.op import (joint_modes_to_numpy, joint_statistics_to_numpy, scene_check_to_numpy, scene_constraint_to_numpy,
                                     scene_field_lookup, scene_field_to_numpy, skeleton_alternatives_to_numpy,
                                     skeleton_couple_to_numpy, skeleton_pose_to_numpy,
                                     skeleton_samples_to_numpy, volume_filter_to_numpy, volume_path_to_numpy,
                                     volume_smoother_to_numpy)
        from sceneego_amd.preprocess import load_image_bgr
        load = JpegFile if self.image_decode == "device" else load_image_bgr
        batches = [(images[i:i + batch_size], depths[i:i + batch_size]) for i in range(0, len(images), batch_size)]
        preds, frame_stats, frame_scene, pending = [], [], [], []
        frame_constraint, frame_scene_constrained, frame_modes, frame_filter, frame_skeleton, frame_map = [], [], [], [], [], []
        if render_filtered and (filter is None or not render_volumes):
            raise ValueError("render_filtered needs filter and render_volumes")
        if smooth is not None and filter is None:
            raise ValueError("smooth needs filter")
        if sample is not None and smooth is None:
            raise ValueError("sample needs smooth")
        vs = self.net.volume_smoother(**filter, **smooth) if smooth is not None else None
        vf = vs.filter if vs is not None else self.net.volume_filter(**filter) if filter is not None else None
        if render_coupled and (skeleton is None or not render_volumes or render_filtered):
            raise ValueError("render_coupled needs skeleton and render_volumes, and excludes render_filtered")
        sp = self.net.skeleton_prior(**skeleton) if skeleton is not None else None
        frame_pose_samples, frame_scene_field = [], []
        psp = self.net.skeleton_prior(**{k: pose_sample[k] for k in ("bone_lengths", "tau", "floor")}) if pose_sample is not None else None
        path_separation = None
        if path is not None:                # "separation": the backward pass too (--path_alternatives_output)
            path = dict(path)
            path_separation = path.pop("separation", None)
        vp = self.net.volume_path(alternatives=path_separation is not None, **path) if path is not None else None
        separation = map_pose.get("separation") if map_pose is not None else None
        mpose = self.net.skeleton_pose(**{k: v for k, v in map_pose.items() if k != "separation"}) if map_pose is not None else None

        def couple_and_filter(vol, kp, job, stream=None, first_frame=0, net=None, depth=None):
            """The most probable pose and the pose samples (from the raw volumes), the skeleton coupling and the filter of one batch,
            in that order: (filter dict, skeleton dict, job, pose dict, pose-sample dict, scene-field dict).  ``first_frame``: the
            batch's first frame in the sequence.  ``net``, ``depth`` (with ``scene_field``): the module replica and the depth maps of
            the batch, for the scene field of the raw volumes and of every belief computed here."""
            fr = sk = None
            mp = ps = None
            sf = expect = None
            if scene_field is not None:
                field = net.scene_field(depth)

                def expect(v):
                    return net.scene_expectations(v, depth=depth, field=field, radii2=scene_field["radii2"])
                sf = {"volumes": expect(vol)}
            if psp is not None:
                ps = psp.sample(vol, samples=pose_sample["samples"], seed=pose_sample["seed"], first_frame=first_frame, joints=kp,
                                stream=stream)
                if sf is not None:
                    sf["pose_samples"] = scene_field_lookup(field, sf["volumes"]["free"], ps["index"], radii2=scene_field["radii2"])
            if mpose is not None:                                        # alternatives: the pose with the same bits, and the runner-up
                mp = mpose.solve(vol, joints=kp, stream=stream) if separation is None else \
                    mpose.alternatives(vol, separation=separation, joints=kp, stream=stream)
            if sp is not None:
                sk = sp.couple(vol, joints=kp, stream=stream, return_beliefs=vf is not None or vp is not None or sf is not None
                               or (render_coupled and job is not None))
                if sf is not None:
                    sf["coupled"] = expect(sk["beliefs"])
                    if not (vf is not None or vp is not None or (render_coupled and job is not None)):
                        sk = {k: v for k, v in sk.items() if k != "beliefs"}
                if vf is not None or vp is not None:
                    vol = sk["beliefs"]
                if render_coupled and job is not None:
                    job = job[:-1] + (sk["beliefs"],)
            if vf is not None:
                want_beliefs = render_filtered and job is not None
                if vs is not None:     # the same dict; the smoother keeps copies of its own, so the beliefs are dropped unless drawn
                    fr = vs.push(vol, joints=kp, stream=stream)
                else:
                    fr = vf.step(vol, joints=kp, return_beliefs=want_beliefs or sf is not None, stream=stream)
                if sf is not None:
                    sf["filtered"] = expect(fr["beliefs"])
                fr = {k: v for k, v in fr.items() if k != "beliefs" or want_beliefs}
                if "beliefs" in fr:
                    job = job[:-1] + (fr["beliefs"],)
            if vp is not None:             # on the raw volumes, or the coupled beliefs: never on the filter's
                vp.push(vol, joints=kp, stream=stream)
            if sf is not None:         # the mask is the module's cached buffer, overwritten by the next batch: not kept
                sf = {k: {n: t for n, t in v.items() if n != "free"} for k, v in sf.items()}
            return fr, sk, job, mp, ps, sf

        rendering = render_dir is not None or render_video is not None
        if rendering:
            if render_every < 1:
                raise ValueError(f"--render_every must be >= 1, got {render_every}")
            if render_format not in ("png", "jpg") or render_view not in ("render", "overlay", "both"):
                raise ValueError(f"bad render_format {render_format!r} or render_view {render_view!r}")
            if png_encoder not in ("host", "device"):
                raise ValueError(f"png_encoder must be host or device, got {png_encoder!r}")
            if render_dir is not None:
                os.makedirs(render_dir, exist_ok=True)
            self.render_options = {"format": render_format, "png_encoder": png_encoder, "video": render_video, "fps": render_fps, "view": render_view,
                                   "quality": render_quality, "renderer": {} if render_size is None else {"out_size": tuple(render_size)},
                                   "volumes": bool(render_volumes), "volume_joints": volume_joints}

        def drain(keep):
            while len(pending) > keep:
                kp, st, done, job, sc, con, md, fr, sk, mp, ps, sf = pending.pop(0)
                if done is not None:
                    done.synchronize()
                kp_host = kp.cpu().numpy()
                preds.extend(np.asarray(k, dtype=np.float32) for k in kp_host)
                if st is not None:
                    frame_stats.extend(joint_statistics_to_numpy(st))
                if sc is not None:
                    frame_scene.extend(scene_check_to_numpy(sc))
                if con is not None:
                    frame_constraint.extend(scene_constraint_to_numpy(con[0]))
                    if con[1] is not None:
                        frame_scene_constrained.extend(scene_check_to_numpy(con[1]))
                if md is not None:
                    frame_modes.extend(joint_modes_to_numpy(md))
                if fr is not None:
                    frame_filter.extend(volume_filter_to_numpy(fr))
                if sk is not None:
                    frame_skeleton.extend(skeleton_couple_to_numpy(sk))
                if mp is not None:
                    frame_map.extend(skeleton_pose_to_numpy(mp) if separation is None else skeleton_alternatives_to_numpy(mp))
                if ps is not None:
                    frame_pose_samples.extend(skeleton_samples_to_numpy(ps))
                if sf is not None:
                    per = {k: scene_field_to_numpy(v) for k, v in sf.items()}
                    frame_scene_field.extend({k: per[k][b] for k in per} for b in range(len(kp_host)))
                if job is not None:
                    self._render(job, kp_host)         # the joints of this batch are final here, with any number of streams

        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            ahead = [pool.submit(load, p) for p in batches[0][0]] if batches else []
            for i, (imgs, deps) in enumerate(batches):
                frames = [f.result() for f in ahead]
                if i + 1 < len(batches):
                    ahead = [pool.submit(load, p) for p in batches[i + 1][0]]
                img = self._images(frames)
                depth = self._depths(deps)
                job = None
                if rendering:
                    pick = [k for k in range(len(imgs)) if (i * batch_size + k) % render_every == 0]
                    if pick:
                        job = (render_dir, pick, [os.path.split(imgs[k])[1] for k in pick], self._frames_u8([frames[k] for k in pick]),
                               depth[pick])
                if self.pipe is None:
                    kp, _, vol, _ = self.net(img, self.net.grid_coord_proj_batch, self.net.coord_volumes, depth_map_batch=depth)
                    job = job + (vol,) if job is not None else None       # drained before the next forward overwrites the volumes
                    con = None
                    if constrain:
                        c = self.net.constrain_to_scene(vol, kp, depth)
                        con = (c, self._scene().check(depth, c["joints"]) if scene else None)
                    fr, sk, job, mp, ps, sf = couple_and_filter(vol, kp, job, first_frame=i * batch_size, net=self.net,
                                                                depth=depth)                           # before the next forward
                    # overwrites the volumes
                    pending.append((kp, self.net.joint_statistics(vol, kp) if stats else None, None, job,
                                    self._scene().check(depth, kp) if scene else None, con,
                                    self.net.joint_modes(vol, k=modes) if modes else None, fr, sk, mp, ps, sf))
                else:
                    net, stream = self.pipe.next_slot()
                    (kp, _, vol, _), done = self.pipe(img, self.net.grid_coord_proj_batch, self.net.coord_volumes, depth_map_batch=depth)
                    job = job + (vol,) if job is not None else None       # the slot's buffers: handed back only after drain()
                    st = sc = con = md = fr = sk = mp = ps = sf = None
                    if stats or scene or constrain or modes or vf is not None or sp is not None or vp is not None or mpose is not None \
                            or psp is not None or scene_field is not None:
                        # on the stream the batch ran on, with that replica's workspace; `done` moves behind it, so drain() hands the
                        # buffers back only after the statistics are complete
                        with torch.cuda.stream(stream):
                            if stats:
                                st = net.joint_statistics(vol, kp)
                            if scene:
                                sc = self._scene(stream.cuda_stream).check(depth, kp)
                            if constrain:
                                c = net.constrain_to_scene(vol, kp, depth)
                                con = (c, self._scene(stream.cuda_stream).check(depth, c["joints"]) if scene else None)
                            if modes:
                                md = net.joint_modes(vol, k=modes)
                            # one filter for all slots: its own event chain makes this stream wait for the step of the batch before;
                            # one skeleton prior too: it carries no state and keeps one workspace per stream
                            fr, sk, job, mp, ps, sf = couple_and_filter(vol, kp, job, stream, first_frame=i * batch_size, net=net,
                                                                        depth=depth)
                            done = torch.cuda.Event()
                            done.record(stream)
                    pending.append((kp, st, done, job, sc, con, md, fr, sk, mp, ps, sf))
                drain(len(self.pipe) - 1 if self.pipe is not None else 0)
            try:
                drain(0)
            finally:
                if self.video is not None:
                    self.video.close()
                    self.video = None
        frame_samples = None
        if sample is not None:                  # before finish(): the draws read the stored filtered beliefs, finish() releases them
            from sceneego_amd.op import volume_samples_to_numpy
            frame_samples = volume_samples_to_numpy(vs.sample(**sample))
        frame_smooth = volume_smoother_to_numpy(vs.finish()) if vs is not None else None
        if vp is not None and path_separation is not None:
            from sceneego_amd.op import volume_path_alternatives_to_numpy
            frame_path = volume_path_alternatives_to_numpy(vp.alternatives(separation=path_separation))
        else:
            frame_path = volume_path_to_numpy(vp.finish()) if vp is not None else None
        if not (stats or scene or constrain or modes or vf is not None or sp is not None or vp is not None or mpose is not None
                or psp is not None or scene_field is not None):
            return preds
        return (preds,) + ((frame_stats,) if stats else ()) + ((frame_scene,) if scene else ()) \
            + ((frame_constraint,) if constrain else ()) + ((frame_scene_constrained,) if constrain and scene else ()) \
            + ((frame_modes,) if modes else ()) + ((frame_filter,) if vf is not None else ()) \
            + ((frame_skeleton,) if sp is not None else ()) + ((frame_smooth,) if vs is not None else ()) \
            + ((frame_path,) if vp is not None else ()) + ((frame_map,) if mpose is not None else ()) \
            + ((frame_samples,) if sample is not None else ()) + ((frame_pose_samples,) if psp is not None else ()) \
            + ((frame_scene_field,) if scene_field is not None else ())


def _size(text):
    try:
        h, w = (int(v) for v in text.lower().split("x"))
        if h <= 0 or w <= 0:
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError(f"HxW expected, e.g. 720x960; got {text!r}")
    return h, w


def _quality(text):
    q = int(text)
    if not 1 <= q <= 100:
        raise argparse.ArgumentTypeError(f"1..100 expected, got {text!r}")
    return q


def _fps(text):
    v = float(text)
    if not v > 0:
        raise argparse.ArgumentTypeError(f"a positive rate expected, got {text!r}")
    return int(v) if v == int(v) else v


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default=os.path.join(ROOT, "experiments", "sceneego", "test", "sceneego.yaml"))
    ap.add_argument("--root_dir", required=True, help="directory holding the sequence directories")
    ap.add_argument("--seq_name", required=True)
    ap.add_argument("--estimated_depth_name", default=None, help="<seq>/<name>/img_%%06d.jpg.exr (default: rendered/depths)")
    ap.add_argument("--weights", default=None, help="checkpoint path, or 'synthetic' (default: config.test.model_path)")
    ap.add_argument("--depth_decode", default="device", choices=("device", "host"))
    ap.add_argument("--image_decode", default="device", choices=("device", "host"))
    ap.add_argument("--streams", type=int, default=1, help="forwards in flight (PipelinedForward when > 1)")
    ap.add_argument("--workers", type=int, default=8, help=f"JPEG read / parse (host decode: decode) threads (at most {MAX_WORKERS})")
    ap.add_argument("--output", default=None, help="pickle of the predicted [15,3] joints of every frame")
    ap.add_argument("--render_dir", default=None, help="write <img_name>.render.png and <img_name>.overlay.png of the picked frames here")
    ap.add_argument("--render_every", type=int, default=1, help="with --render_dir: render every N-th frame (default: every frame)")
    ap.add_argument("--stats_output", default=None, help="pickle of the per-frame joint statistics (list of dicts of numpy arrays: "
                    "cov, sigma, entropy, peak_prob, peak_index, peak_coord)")
    ap.add_argument("--scene_output", default=None, help="pickle of the per-frame scene checks (list of dicts of numpy arrays: "
                    "nearest_dist, clearance, bone_clearance, penetration_depth, penetrating, contact, ...); prints their summary")
    ap.add_argument("--constrain_output", default=None, help="pickle of the per-frame scene constraints (list of dicts of numpy arrays: "
                    "joints, constrained, free_mass, moved, free_peak_prob, free_peak_index, free_peak_coord); with --scene_output the "
                    "scene check also runs on the constrained joints and both summaries are printed")
    ap.add_argument("--modes_output", default=None, help="pickle of the per-frame joint modes (list of dicts of numpy arrays: coord, "
                    "peak_coord, peak_prob, mass, index, count, total, valid)")
    ap.add_argument("--modes_k", type=int, default=4, help="with --modes_output: modes kept per joint, 1..16")
    ap.add_argument("--track_output", default=None, help="with --modes_output: pickle in the format of --output holding one mode per "
                    "joint and frame, picked over the sequence (sceneego_amd/track.py: a convention, not calibrated)")
    ap.add_argument("--track_sigma", type=float, default=0.1, help="with --track_output: metres a joint is assumed to move per frame")
    ap.add_argument("--filter_output", default=None, help="pickle in the format of --output holding the joints of a grid Bayes filter "
                    "over the sequence's volumes (sceneego_amd/volume_filter.py: a convention, not calibrated)")
    ap.add_argument("--filter_info_output", default=None, help="pickle of the per-frame filter dicts (list of dicts of numpy arrays: "
                    "joints, evidence, restarted, shift)")
    ap.add_argument("--filter_sigma", type=float, default=0.1, help="the filter's motion model: metres a joint is assumed to move per frame")
    ap.add_argument("--filter_radius", type=int, default=None, help="voxels the Gaussian step is truncated at, 0..16 "
                    "(default: min(16, G - 1, ceil(3 sigma / voxel edge)))")
    ap.add_argument("--filter_floor", type=float, default=1e-3, help="the filter's uniform floor in [0, 1]: the chance of a jump")
    ap.add_argument("--fit_frames", type=int, default=None, help="fit --filter_sigma and --filter_floor to the volumes of the first F "
                    "consecutive frames before the main pass (sceneego_amd/motion_fit.py: EM at the fixed --filter_radius; a fit to the "
                    "network's own volumes, not a validation against ground truth); --filter_output, --smooth_output and --path_output "
                    "then run on the fitted values")
    ap.add_argument("--fit_iterations", type=int, default=None, help="with --fit_frames: at most this many EM iterations (default 8)")
    ap.add_argument("--fit_output", default=None, help="with --fit_frames: JSON file of the fit (sigma, floor, radius, log_likelihood, "
                    "history, mean_sq_step, pairs, converged, saturated, truncation_binding, sigma_per_joint, floor_per_joint)")
    ap.add_argument("--smooth_output", default=None, help="pickle in the format of --output holding the joints of the forward-backward "
                    "smoother over the sequence's volumes (sceneego_amd/volume_smoother.py; --filter_sigma, --filter_radius, "
                    "--filter_floor: the filter's convention, not calibrated); implies the filter")
    ap.add_argument("--smooth_info_output", default=None, help="pickle of the per-frame smoother dicts (list of dicts of numpy arrays: "
                    "joints, smoothed, agreement, filtered_joints, shift_filtered, shift)")
    ap.add_argument("--smooth_max_gb", type=float, default=None, help="with --smooth_output: the most device memory the stored volumes "
                    "and beliefs may take, in GiB (default: half of what is free at the first batch)")
    ap.add_argument("--sample_output", default=None, help="pickle of the per-frame dicts of trajectory samples drawn from the smoother's "
                    "posterior (VolumeSmoother.sample: index, coord, kind, valid [S,15,...], mean, spread, shift); implies the smoother "
                    "on --filter_sigma / --filter_radius / --filter_floor and draws before it finishes; a convention, not calibrated")
    ap.add_argument("--samples", type=int, default=None, help="with --sample_output: trajectories per joint (default 16)")
    ap.add_argument("--sample_seed", type=int, default=None, help="with --sample_output: the seed, 0..2^64-1 (default 0)")
    ap.add_argument("--pose_samples_output", default=None, help="pickle of the per-frame dicts of whole poses drawn from the posterior of "
                    "the skeleton model (SkeletonPrior.sample: index, coord, kind, valid [S,15,...], bone_error [S,14], mean, spread, "
                    "sampled, shift); implies the skeleton model options --bone_lengths / --bone_frames, --skeleton_tau, "
                    "--skeleton_floor, and the fitted values with --skeleton_fit_frames; samples of the model's posterior, not calibrated")
    ap.add_argument("--scene_field_output", default=None, help="pickle of the per-frame dicts of the volumes against the scene distance "
                    "field of the frame's depth map (volumes, and coupled / filtered / pose_samples where those options are on: "
                    "contact_prob, contact_free_prob, blocked_prob, expected_distance, expected_free_distance, mass, radii2; distances are "
                    "quantised to voxel centres, the radii are conventions, not calibrated)")
    ap.add_argument("--contact_radii", default=None, help="with --scene_field_output: 1..8 ascending contact radii in voxel spacings, "
                    "e.g. 1,2,3 (the default)")
    ap.add_argument("--pose_samples", type=int, default=None, help="with --pose_samples_output: poses per frame (default 16)")
    ap.add_argument("--pose_sample_seed", type=int, default=None, help="with --pose_samples_output: the seed, 0..2^64-1 (default 0)")
    ap.add_argument("--path_output", default=None, help="pickle in the format of --output holding the joints of the most probable "
                    "trajectory of every joint through the sequence's volumes (sceneego_amd/volume_viterbi.py; --filter_sigma, "
                    "--filter_radius, --filter_floor: the filter's convention, not calibrated); with --skeleton_output it runs on the "
                    "coupled beliefs")
    ap.add_argument("--path_info_output", default=None, help="pickle of the per-frame path dicts (list of dicts of numpy arrays: "
                    "joints, index, coord, jumped, segment_start, log_score, moved, shift)")
    ap.add_argument("--path_alternatives_output", default=None, help="pickle of the per-frame path dicts with the runner-up: the keys "
                    "of --path_info_output, then the margin by which every frame of the path was decided, the best trajectory that "
                    "is somewhere else in that frame and the runner-up trajectory of each segment (VolumeViterbi.alternatives: the "
                    "backward max-product pass; 47.2 MB per frame at 15 x 64^3 stay on the device); implies the --path_* options")
    ap.add_argument("--path_separation", type=int, default=None, help="with --path_alternatives_output: an alternative lies further than "
                    "this many voxels (Chebyshev) from the path voxel in its frame (default 2)")
    ap.add_argument("--path_refine", type=int, default=None, help="with --path_output: the path voxel is refined to the centroid of the "
                    "volume over this many voxels around it, 0..3 (default 1; 0: the voxel centre, and no volumes are stored)")
    ap.add_argument("--path_max_gb", type=float, default=None, help="with --path_output: the most device memory the stored "
                    "back-pointers and volumes may take, in GiB (default: half of what is free at the first batch)")
    ap.add_argument("--skeleton_output", default=None, help="pickle in the format of --output holding the joints coupled over the "
                    "kinematic tree inside every frame (sceneego_amd/skeleton_prior.py: a convention, not calibrated)")
    ap.add_argument("--skeleton_info_output", default=None, help="pickle of the per-frame skeleton dicts (list of dicts of numpy arrays: "
                    "joints, evidence, coupled, bone_error, shift, bone_error_before)")
    ap.add_argument("--map_output", default=None, help="pickle in the format of --output holding the most probable pose of every frame "
                    "under the bone-length model of --skeleton_output (sceneego_amd/skeleton_pose.py: max-product over the kinematic "
                    "tree on the raw volumes; --bone_lengths, --bone_frames, --skeleton_tau, --skeleton_floor as there; a convention, not "
                    "calibrated)")
    ap.add_argument("--map_info_output", default=None, help="pickle of the per-frame pose dicts (list of dicts of numpy arrays: joints, "
                    "index, coord, jumped, solved, log_score, bone_error, shift, bone_error_before)")
    ap.add_argument("--map_alternatives_output", default=None, help="pickle of the per-frame dicts of SkeletonPose.alternatives (the pose "
                    "dicts of --map_info_output and margin, alt_log_score, alt_index, alt_coord, alt_pose_index, alt_pose_jumped, "
                    "alt_pose_joints, max_marginal_peak_index, pose_is_peak, runner_up, runner_up_joints, runner_up_margin, "
                    "runner_up_bone_error): how close the second-best pose was; implies the --map_* model options")
    ap.add_argument("--map_separation", type=int, default=None, help="with --map_alternatives_output: an alternative places its anchor "
                    "joint more than this many voxels (Chebyshev, default 2) from the joint's voxel in the most probable pose")
    ap.add_argument("--map_refine", type=int, default=None, help="with --map_output: each pose voxel is refined to the centroid of its "
                    "joint's volume over a window of this many voxels around it (0..3, default 1; 0: the voxel centre)")
    ap.add_argument("--bone_lengths", default=None, help="a .npy of 14 bone lengths in metres (edges 1..14 of the kinematic tree) or 15 "
                    "(entry 0 ignored); default: estimated from a first pass over --bone_frames frames")
    ap.add_argument("--bone_frames", type=int, default=64, help="without --bone_lengths: at most this many evenly spaced frames feed "
                    "the bone-length estimate")
    ap.add_argument("--skeleton_fit_frames", type=int, default=None, help="fit the bone lengths, --skeleton_tau and --skeleton_floor to "
                    "the volumes of F evenly spaced frames before the main pass (sceneego_amd/skeleton_fit.py: EM from --bone_lengths or "
                    "the median estimate; a fit to the volumes, not calibrated against ground truth); --skeleton_output and --map_output "
                    "then run on the fitted values")
    ap.add_argument("--skeleton_fit_iterations", type=int, default=None, help="with --skeleton_fit_frames: at most this many EM "
                    "iterations (default 8)")
    ap.add_argument("--skeleton_fit_output", default=None, help="with --skeleton_fit_frames: JSON file of the fit (bone_lengths, tau, "
                    "floor, radius, log_likelihood, history, ...)")
    ap.add_argument("--skeleton_tau", type=float, default=0.03, help="the width of the bone-length shell in metres")
    ap.add_argument("--skeleton_floor", type=float, default=1e-3, help="the skeleton prior's uniform floor in [0, 1]: the chance that "
                    "the bone prior is wrong for an edge")
    ap.add_argument("--render_format", default="png", choices=("png", "jpg"),
                    help="with --render_dir: png (PIL on the host) or jpg (quality-90 4:4:4 JPEG files encoded on the device)")
    ap.add_argument("--png_encoder", default="host", choices=("host", "device"),
                    help="with --render_dir and --render_format png: host (PIL) or device (lossless, sceneego_amd/png_encode.py: the "
                         "picked frames of a batch are encoded where they were rendered, only the files' bytes cross to the host)")
    ap.add_argument("--render_video", default=None, help="write the picked frames as one Motion-JPEG AVI (4:2:0, encoded on the device)")
    ap.add_argument("--render_fps", type=_fps, default=25, help="with --render_video: frames per second of the file")
    ap.add_argument("--render_view", default="render", choices=("render", "overlay", "both"),
                    help="with --render_video: the third-person view, the fisheye overlay, or both side by side (equal heights only)")
    ap.add_argument("--render_quality", type=_quality, default=90, help="with --render_video: JPEG quality, 1..100")
    ap.add_argument("--render_size", type=_size, default=None, help="HxW of the third-person view (default: 720x960)")
    ap.add_argument("--render_volumes", default="false",
                    help="true (with --render_dir / --render_video): also write <img_name>.volumes.render.* and .volumes.overlay.* (the "
                         "joint probability volumes drawn over the pair); the video shows the volume views.  filtered: the same with the "
                         "beliefs of the grid Bayes filter (--filter_sigma, --filter_radius, --filter_floor) instead of the raw volumes; "
                         "coupled: with the skeleton-coupled beliefs (--skeleton_tau, --skeleton_floor)")
    ap.add_argument("--volume_joints", default=None, help="with --render_volumes true: the joints to draw, e.g. 9,10,13,14 (default: all)")
    return ap


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.render_volumes.lower() not in ("true", "false", "filtered", "coupled"):
        raise SystemExit("--render_volumes must be true, false, filtered or coupled")
    args.render_filtered = args.render_volumes.lower() == "filtered"
    args.render_coupled = args.render_volumes.lower() == "coupled"
    args.render_volumes = args.render_volumes.lower() in ("true", "filtered", "coupled")
    if args.render_volumes and args.render_dir is None and args.render_video is None:
        raise SystemExit("--render_volumes true / filtered needs --render_dir or --render_video")
    if args.volume_joints is not None and not args.render_volumes:
        raise SystemExit("--volume_joints needs --render_volumes true or filtered")
    if not args.filter_sigma >= 0 or args.filter_sigma == float("inf"):
        raise SystemExit("--filter_sigma must be a finite number >= 0")
    if not 0.0 <= args.filter_floor <= 1.0:
        raise SystemExit("--filter_floor must lie in [0, 1]")
    if args.filter_radius is not None and not 0 <= args.filter_radius <= 16:
        raise SystemExit("--filter_radius must be in 0..16")
    args.filter = None
    if args.filter_output is not None or args.filter_info_output is not None or args.render_filtered:
        args.filter = {"sigma": args.filter_sigma, "radius": args.filter_radius, "floor": args.filter_floor}
    args.smooth = None
    if args.smooth_output is not None or args.smooth_info_output is not None or args.sample_output is not None:
        if args.smooth_max_gb is not None and not args.smooth_max_gb >= 0:
            raise SystemExit("--smooth_max_gb must be >= 0")
        args.smooth = {"max_bytes": None if args.smooth_max_gb is None else int(args.smooth_max_gb * 2 ** 30)}
        args.filter = {"sigma": args.filter_sigma, "radius": args.filter_radius, "floor": args.filter_floor}
    elif args.smooth_max_gb is not None:
        raise SystemExit("--smooth_max_gb needs --smooth_output")
    args.sample = None
    if args.sample_output is not None:
        samples, seed = 16 if args.samples is None else args.samples, 0 if args.sample_seed is None else args.sample_seed
        if samples < 1:
            raise SystemExit("--samples must be >= 1")
        if not 0 <= seed < 2 ** 64:
            raise SystemExit("--sample_seed must be in 0..2^64-1")
        args.sample = {"samples": samples, "seed": seed}
    elif args.samples is not None or args.sample_seed is not None:
        raise SystemExit("--samples and --sample_seed need --sample_output")
    args.path = None
    if args.path_output is not None or args.path_info_output is not None or args.path_alternatives_output is not None:
        if args.path_max_gb is not None and not args.path_max_gb >= 0:
            raise SystemExit("--path_max_gb must be >= 0")
        if args.path_refine is not None and not 0 <= args.path_refine <= 3:
            raise SystemExit("--path_refine must be in 0..3")
        args.path = {"sigma": args.filter_sigma, "radius": args.filter_radius, "floor": args.filter_floor,
                     "refine": 1 if args.path_refine is None else args.path_refine,
                     "max_bytes": None if args.path_max_gb is None else int(args.path_max_gb * 2 ** 30)}
        if args.path_alternatives_output is not None:
            if args.path_separation is not None and args.path_separation < 0:
                raise SystemExit("--path_separation must be >= 0")
            args.path["separation"] = 2 if args.path_separation is None else args.path_separation
        elif args.path_separation is not None:
            raise SystemExit("--path_separation needs --path_alternatives_output")
    elif args.path_max_gb is not None or args.path_refine is not None or args.path_separation is not None:
        raise SystemExit("--path_max_gb, --path_refine and --path_separation need --path_output")
    args.fit = None
    if args.fit_frames is not None:
        if args.fit_frames < 2:
            raise SystemExit("--fit_frames must be >= 2: the fit needs a pair of consecutive frames")
        if args.fit_iterations is not None and args.fit_iterations < 1:
            raise SystemExit("--fit_iterations must be >= 1")
        args.fit = {"frames": args.fit_frames, "iterations": 8 if args.fit_iterations is None else args.fit_iterations}
    elif args.fit_iterations is not None or args.fit_output is not None:
        raise SystemExit("--fit_iterations and --fit_output need --fit_frames")
    args.skeleton_fit = None
    if args.skeleton_fit_frames is not None:
        if args.skeleton_fit_frames < 1:
            raise SystemExit("--skeleton_fit_frames must be >= 1")
        if args.skeleton_fit_iterations is not None and args.skeleton_fit_iterations < 1:
            raise SystemExit("--skeleton_fit_iterations must be >= 1")
        args.skeleton_fit = {"frames": args.skeleton_fit_frames,
                             "iterations": 8 if args.skeleton_fit_iterations is None else args.skeleton_fit_iterations}
    elif args.skeleton_fit_iterations is not None or args.skeleton_fit_output is not None:
        raise SystemExit("--skeleton_fit_iterations and --skeleton_fit_output need --skeleton_fit_frames")
    if not (args.skeleton_tau > 0 and args.skeleton_tau != float("inf")):
        raise SystemExit("--skeleton_tau must be a finite number > 0")
    if not 0.0 <= args.skeleton_floor <= 1.0:
        raise SystemExit("--skeleton_floor must lie in [0, 1]")
    if args.bone_frames < 1:
        raise SystemExit("--bone_frames must be >= 1")
    args.pose_sample = None
    if args.pose_samples_output is not None:
        samples = 16 if args.pose_samples is None else args.pose_samples
        seed = 0 if args.pose_sample_seed is None else args.pose_sample_seed
        if samples < 1:
            raise SystemExit("--pose_samples must be >= 1")
        if not 0 <= seed < 2 ** 64:
            raise SystemExit("--pose_sample_seed must be in 0..2^64-1")
        args.pose_sample = {"samples": samples, "seed": seed}
    elif args.pose_samples is not None or args.pose_sample_seed is not None:
        raise SystemExit("--pose_samples and --pose_sample_seed need --pose_samples_output")
    args.skeleton = args.skeleton_output is not None or args.skeleton_info_output is not None or args.render_coupled
    args.map = args.map_output is not None or args.map_info_output is not None or args.map_alternatives_output is not None
    if args.map_refine is not None and not args.map:
        raise SystemExit("--map_refine needs --map_output")
    if args.map_separation is not None and args.map_alternatives_output is None:
        raise SystemExit("--map_separation needs --map_alternatives_output")
    if args.map_separation is not None and args.map_separation < 0:
        raise SystemExit("--map_separation must be >= 0")
    if args.map_refine is not None and not 0 <= args.map_refine <= 3:
        raise SystemExit("--map_refine must be in 0..3")
    if args.track_output is not None and args.modes_output is None:
        raise SystemExit("--track_output needs --modes_output")
    if not 1 <= args.modes_k <= 16:
        raise SystemExit("--modes_k must be in 1..16")
    if not args.track_sigma > 0:
        raise SystemExit("--track_sigma must be positive")
    from sceneego_amd.render import parse_joint_list
    try:
        args.volume_joints = parse_joint_list(args.volume_joints)
    except ValueError as e:
        raise SystemExit(str(e))
    return args


def main(argv=None):
    from sceneego_amd import load_config
    from sceneego_amd import metrics as M
    args = parse_args(argv)
    config = load_config(args.config)
    images, poses, depths = frame_list(args.root_dir, args.seq_name, args.estimated_depth_name)
    if not images:
        raise SystemExit("no frames: every pose is None or every image is missing")
    print(f"dataset length: {len(images)}")
    runner = SequenceRunner(config, weights=args.weights, streams=args.streams, depth_decode=args.depth_decode,
                            workers=args.workers, image_decode=args.image_decode)
    skeleton = map_pose = skeleton_fitted = pose_sample = None
    if args.skeleton or args.map or args.skeleton_fit is not None or args.pose_sample is not None:
        from sceneego_amd.skeleton_prior import estimate_bone_lengths
        if args.bone_lengths is not None:
            lengths = np.load(args.bone_lengths)
        else:
            # a first pass over at most --bone_frames evenly spaced frames: the per-bone median of the raw joints' distances
            pick = sorted({int(round(v)) for v in np.linspace(0, len(images) - 1, min(args.bone_frames, len(images)))})
            raw = runner.run([images[k] for k in pick], [depths[k] for k in pick], config.test.batch_size)
            lengths = estimate_bone_lengths(np.stack(raw))
            print(f"bone lengths estimated from {len(pick)} frames: " + " ".join(f"{v:.4f}" for v in lengths[1:]))
        tau, floor = args.skeleton_tau, args.skeleton_floor
        if args.skeleton_fit is not None:
            # a first pass over --skeleton_fit_frames evenly spaced frames: EM for the bone lengths, tau and floor on a fixed support
            from sceneego_amd.op import skeleton_fit_to_json
            from sceneego_amd.skeleton_prior import MAX_RADIUS, default_radius
            pick = sorted({int(round(v)) for v in np.linspace(0, len(images) - 1, min(args.skeleton_fit["frames"], len(images)))})
            start = {"bone_lengths": np.asarray(lengths, dtype=np.float64), "tau": tau, "floor": floor}
            try:
                sfit = runner.fit_skeleton([images[k] for k in pick], [depths[k] for k in pick], config.test.batch_size, start,
                                           iterations=args.skeleton_fit["iterations"])
            except ValueError as e:
                raise SystemExit(str(e))
            lengths, tau, floor = sfit["bone_lengths"], float(sfit["tau"]), float(sfit["floor"])
            skeleton_fitted = {"bone_lengths": np.asarray(lengths[1:], dtype=np.float64), "tau": tau, "floor": floor}
            began = np.asarray(start["bone_lengths"], dtype=np.float64).reshape(-1)[-(len(lengths) - 1):]
            print("skeleton model fitted to {} frames ({} valid, {} iterations; a fit to the volumes, not calibrated against ground truth): "
                  "tau {:.4f} -> {:.4f} m, floor {:.3g} -> {:.3g}, log-likelihood {:.6g} -> {:.6g}{}{}".format(
                      len(pick), sfit["frames_used"], len(sfit["log_likelihood"]) - 1, args.skeleton_tau, tau, args.skeleton_floor, floor,
                      sfit["log_likelihood"][0], sfit["log_likelihood"][-1], ", a bound is active" if sfit["saturated"] else "",
                      ", the support cuts a fitted shell: fit again from the fitted values" if sfit["truncation_binding"].any() else ""))
            print("bone lengths at the start:  " + " ".join(f"{v:.4f}" for v in began))
            print("bone lengths fitted:        " + " ".join(f"{v:.4f}" for v in lengths[1:]))
            if args.skeleton_fit_output is not None:
                os.makedirs(os.path.dirname(os.path.abspath(args.skeleton_fit_output)), exist_ok=True)
                with open(args.skeleton_fit_output, "w") as f:
                    json.dump(skeleton_fit_to_json(sfit, frames=len(pick), start={"bone_lengths": began, "tau": args.skeleton_tau,
                                                                                   "floor": args.skeleton_floor}), f, indent=1)
            h = runner.net.cuboid_side / runner.net.volume_size
            reach, most = default_radius(lengths[1:], tau, h), min(MAX_RADIUS, runner.net.volume_size - 1)
            if reach > most:
                raise SystemExit(f"the shells reach {reach} voxels of {h:.5f} m; at most min({MAX_RADIUS}, grid - 1) = {most} are supported")
        if args.skeleton:
            skeleton = {"bone_lengths": lengths, "tau": tau, "floor": floor}
        if args.pose_sample is not None:
            pose_sample = {"bone_lengths": lengths, "tau": tau, "floor": floor, **args.pose_sample}
        if args.map:
            map_pose = {"bone_lengths": lengths, "tau": tau, "floor": floor, "refine": 1 if args.map_refine is None else args.map_refine}
            if args.map_alternatives_output is not None:
                map_pose["separation"] = 2 if args.map_separation is None else args.map_separation
    fitted = None
    if args.fit is not None:
        # a first pass over the first --fit_frames consecutive frames: EM for sigma and floor at the fixed radius
        from sceneego_amd.op import motion_fit_to_json
        n = min(args.fit["frames"], len(images))
        if n < 2:
            raise SystemExit("--fit_frames: the sequence has fewer than 2 frames")
        start = {"sigma": args.filter_sigma, "radius": args.filter_radius, "floor": args.filter_floor}
        fit = runner.fit_motion(images[:n], depths[:n], config.test.batch_size, start, iterations=args.fit["iterations"])
        fitted = {"sigma": float(fit["sigma"]), "radius": int(fit["radius"]), "floor": float(fit["floor"])}
        print("motion model fitted to {} frames ({} pairs, {} iterations; a fit to the volumes, not calibrated against ground truth): "
              "sigma {:.4f} -> {:.4f} m, floor {:.3g} -> {:.3g}, radius {}, log-likelihood {:.6g} -> {:.6g}{}{}".format(
                  n, fit["pairs"], len(fit["log_likelihood"]) - 1, args.filter_sigma, fitted["sigma"], args.filter_floor,
                  fitted["floor"], fitted["radius"], fit["log_likelihood"][0], fit["log_likelihood"][-1],
                  ", sigma saturated" if fit["saturated"] else "",
                  ", the radius cuts the step: refit with a larger --filter_radius" if fit["truncation_binding"] else ""))
        if args.fit_output is not None:
            os.makedirs(os.path.dirname(os.path.abspath(args.fit_output)), exist_ok=True)
            with open(args.fit_output, "w") as f:
                json.dump(motion_fit_to_json(fit, frames=n, start=start), f, indent=1)
        for model in (args.filter, args.path):
            if model is not None:
                model.update(fitted)
    scene_field = None
    if args.scene_field_output is not None:
        radii2 = None
        if args.contact_radii is not None:
            try:
                spacings = [float(v) for v in args.contact_radii.split(",")]
            except ValueError:
                raise SystemExit("--contact_radii must be a comma-separated list of radii in voxel spacings, e.g. 1,2,3")
            if not 1 <= len(spacings) <= 8 or spacings != sorted(spacings) or spacings[0] < 0:
                raise SystemExit("--contact_radii: 1..8 ascending non-negative radii expected")
            radii2 = [int(np.floor(v * v)) for v in spacings]       # squared distances on the grid are integers
        scene_field = {"radii2": radii2}
    elif args.contact_radii is not None:
        raise SystemExit("--contact_radii needs --scene_field_output")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want_stats = args.stats_output is not None
    want_scene = args.scene_output is not None
    want_constraint = args.constrain_output is not None
    want_modes = args.modes_output is not None
    want_filter = args.filter is not None
    preds = runner.run(images, depths, config.test.batch_size, stats=want_stats, render_dir=args.render_dir,
                       render_every=args.render_every, scene=want_scene, render_format=args.render_format,
                       render_video=args.render_video, render_fps=args.render_fps, render_view=args.render_view,
                       render_quality=args.render_quality, render_size=args.render_size, render_volumes=args.render_volumes,
                       volume_joints=args.volume_joints, constrain=want_constraint, modes=args.modes_k if want_modes else 0,
                       filter=args.filter, render_filtered=args.render_filtered, skeleton=skeleton, render_coupled=args.render_coupled,
                       smooth=args.smooth, path=args.path, map_pose=map_pose, sample=args.sample,
                       pose_sample=pose_sample, scene_field=scene_field, png_encoder=args.png_encoder)
    if want_stats or want_scene or want_constraint or want_modes or want_filter or skeleton is not None or args.path is not None \
            or map_pose is not None or pose_sample is not None or scene_field is not None:
        preds, *extra = preds
        frame_stats = extra.pop(0) if want_stats else None
        frame_scene = extra.pop(0) if want_scene else None
        frame_constraint = extra.pop(0) if want_constraint else None
        frame_scene_constrained = extra.pop(0) if want_constraint and want_scene else None
        frame_modes = extra.pop(0) if want_modes else None
        frame_filter = extra.pop(0) if want_filter else None
        frame_skeleton = extra.pop(0) if skeleton is not None else None
        frame_smooth = extra.pop(0) if args.smooth is not None else None
        frame_path = extra.pop(0) if args.path is not None else None
        frame_map = extra.pop(0) if map_pose is not None else None
        frame_samples = extra.pop(0) if args.sample is not None else None
        frame_pose_samples = extra.pop(0) if pose_sample is not None else None
        frame_scene_field = extra.pop(0) if scene_field is not None else None
        if fitted is not None:                                # the info pickles record the fitted values the operators ran on
            for frames in (frame_filter, frame_smooth, frame_path):
                for fr in frames or ():
                    fr.update(fitted)
        if skeleton_fitted is not None:
            for frames in (frame_skeleton, frame_map, frame_pose_samples):
                for fr in frames or ():
                    fr.update(skeleton_fitted)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pred = np.stack(preds).astype(np.float64)
    gt = np.stack([np.asarray(p, dtype=np.float64) for p in poses])
    mpjpe, pampjpe = M.mpjpe(pred, gt), M.pa_mpjpe(pred, gt)
    print("mpjpe: {}".format(mpjpe))
    print("pa mpjpe: {}".format(pampjpe))
    print(f"frames/s: {len(preds) / dt:.2f} ({len(preds)} frames in {dt:.3f} s, depth decode on the {args.depth_decode}, image decode on the {args.image_decode})")
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "wb") as f:
            pickle.dump(preds, f)
    result = {"frames": len(preds), "mpjpe": mpjpe, "pa_mpjpe": pampjpe, "fps": len(preds) / dt, "predictions": preds}
    if fitted is not None:
        result["fit"] = fit
    if skeleton_fitted is not None:
        result["skeleton_fit"] = sfit
    if want_stats:
        os.makedirs(os.path.dirname(os.path.abspath(args.stats_output)), exist_ok=True)
        with open(args.stats_output, "wb") as f:
            pickle.dump(frame_stats, f)
        result["stats"] = frame_stats
    if want_scene:
        os.makedirs(os.path.dirname(os.path.abspath(args.scene_output)), exist_ok=True)
        with open(args.scene_output, "wb") as f:
            pickle.dump(frame_scene, f)
        result["scene"] = frame_scene
        result["scene_summary"] = M.scene_summary(frame_scene)
        print(M.format_scene_summary(result["scene_summary"]))
    if want_constraint:
        os.makedirs(os.path.dirname(os.path.abspath(args.constrain_output)), exist_ok=True)
        with open(args.constrain_output, "wb") as f:
            pickle.dump(frame_constraint, f)
        result["constraint"] = frame_constraint
        if want_scene:
            result["scene_constrained"] = frame_scene_constrained
            result["scene_summary_constrained"] = M.scene_summary(frame_scene_constrained)
            print("constrained joints: " + M.format_scene_summary(result["scene_summary_constrained"]))
    if want_modes:
        os.makedirs(os.path.dirname(os.path.abspath(args.modes_output)), exist_ok=True)
        with open(args.modes_output, "wb") as f:
            pickle.dump(frame_modes, f)
        result["modes"] = frame_modes
        if args.track_output is not None:
            from sceneego_amd.track import select_modes
            joints, choice = select_modes(frame_modes, sigma=args.track_sigma, fallback=np.stack(preds))
            tracked = [np.asarray(j, dtype=np.float32) for j in joints]
            os.makedirs(os.path.dirname(os.path.abspath(args.track_output)), exist_ok=True)
            with open(args.track_output, "wb") as f:
                pickle.dump(tracked, f)
            result["tracked"], result["track_choice"] = tracked, choice
            result["tracked_mpjpe"] = M.mpjpe(joints.astype(np.float64), gt)
            print("tracked modes (a convention, not calibrated): mpjpe: {}, mode 0 in {:.1%} of the joints, fallback in {:.1%}".format(
                result["tracked_mpjpe"], float((choice == 0).mean()), float((choice < 0).mean())))
    if want_filter:
        filtered = [np.asarray(fr["joints"], dtype=np.float32) for fr in frame_filter]
        for path, obj in ((args.filter_output, filtered), (args.filter_info_output, frame_filter)):
            if path is not None:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "wb") as f:
                    pickle.dump(obj, f)
        result["filtered"], result["filter"] = filtered, frame_filter
        result["filtered_mpjpe"] = M.mpjpe(np.stack(filtered).astype(np.float64), gt)
        print("filtered volumes (a convention, not calibrated): mpjpe: {}, mean shift {:.4f} m, {} restarts after the first frame".format(
            result["filtered_mpjpe"], float(np.mean([fr["shift"] for fr in frame_filter])),
            int(sum(fr["restarted"].sum() for fr in frame_filter[1:]))))
    if args.smooth is not None:
        smoothed = [np.asarray(fr["joints"], dtype=np.float32) for fr in frame_smooth]
        for path, obj in ((args.smooth_output, smoothed), (args.smooth_info_output, frame_smooth)):
            if path is not None:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "wb") as f:
                    pickle.dump(obj, f)
        result["smoothed"], result["smoother"] = smoothed, frame_smooth
        result["smoothed_mpjpe"] = M.mpjpe(np.stack(smoothed).astype(np.float64), gt)
        print("smoothed volumes (a convention, not calibrated): mpjpe: {} (soft-argmax {}, filtered {}), mean shift from the filtered "
              "joints {:.4f} m, {} of {} joint-frames smoothed".format(
                  result["smoothed_mpjpe"], mpjpe, result["filtered_mpjpe"], float(np.mean([fr["shift_filtered"] for fr in frame_smooth])),
                  int(sum(fr["smoothed"].sum() for fr in frame_smooth)), int(sum(fr["smoothed"].size for fr in frame_smooth))))
    if args.sample is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.sample_output)), exist_ok=True)
        with open(args.sample_output, "wb") as f:
            pickle.dump(frame_samples, f)
        result["samples"] = frame_samples
        result.update(M.best_of_samples(frame_samples, np.stack(smoothed).astype(np.float64), gt))
        print("trajectory samples (the model's posterior given the volumes read as likelihoods, not calibrated): {} per joint, seed {}: "
              "mean spread {:.4f} m, best-of-{} mpjpe: {} (smoothed {}), {} of {} draws valid".format(
                  args.sample["samples"], args.sample["seed"], result["mean_sample_spread"], args.sample["samples"],
                  result["best_of_n_mpjpe"], result["smoothed_mpjpe"], result["valid_draws"], result["draws"]))
    if skeleton is not None:
        coupled = [np.asarray(fr["joints"], dtype=np.float32) for fr in frame_skeleton]
        for path, obj in ((args.skeleton_output, coupled), (args.skeleton_info_output, frame_skeleton)):
            if path is not None:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "wb") as f:
                    pickle.dump(obj, f)
        result["coupled"], result["skeleton"], result["bone_lengths"] = coupled, frame_skeleton, np.asarray(lengths, dtype=np.float64)
        result["coupled_mpjpe"] = M.mpjpe(np.stack(coupled).astype(np.float64), gt)
        print("skeleton-coupled joints (a convention, not calibrated): mpjpe: {}, mean shift {:.4f} m, mean bone error {:.4f} -> {:.4f} m, "
              "{} frames fell back".format(result["coupled_mpjpe"], float(np.mean([fr["shift"] for fr in frame_skeleton])),
                                           float(np.mean([fr["bone_error_before"] for fr in frame_skeleton])),
                                           float(np.mean([fr["bone_error"] for fr in frame_skeleton])),
                                           int(sum(not fr["coupled"] for fr in frame_skeleton))))
    if args.path is not None:
        on_path = [np.asarray(fr["joints"], dtype=np.float32) for fr in frame_path]
        path_alternatives = frame_path if "separation" in args.path else None
        if path_alternatives is not None:                                # the path dicts are the leading entries
            from sceneego_amd.op import PATH_ALTERNATIVE_KEYS
            frame_path = [{k: v for k, v in fr.items() if k not in PATH_ALTERNATIVE_KEYS} for fr in path_alternatives]
        for path, obj in ((args.path_output, on_path), (args.path_info_output, frame_path),
                          (args.path_alternatives_output, path_alternatives)):
            if path is not None:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "wb") as f:
                    pickle.dump(obj, f)
        result["path"], result["path_info"] = on_path, frame_path
        result["path_mpjpe"] = M.mpjpe(np.stack(on_path).astype(np.float64), gt)
        others = "".join(f", {name} {result[key]}" for name, key in (("filtered", "filtered_mpjpe"), ("smoothed", "smoothed_mpjpe"),
                                                                      ("coupled", "coupled_mpjpe")) if key in result)
        print("most probable path (a convention, not calibrated): mpjpe: {} (soft-argmax {}{}), mean shift {:.4f} m, {} jumps and {} "
              "segment starts after the first frame in {} joint-frames".format(
                  result["path_mpjpe"], mpjpe, others, float(np.nanmean([fr["shift"] for fr in frame_path])),
                  int(sum(fr["jumped"].sum() for fr in frame_path)), int(sum(fr["segment_start"].sum() for fr in frame_path[1:])),
                  int(sum(fr["index"].size for fr in frame_path))))
        if path_alternatives is not None:
            margins = np.array([fr["runner_up_margin"] for fr in path_alternatives], dtype=np.float64)
            per_frame = np.array([fr["margin"] for fr in path_alternatives], dtype=np.float64)
            result["path_alternatives"] = path_alternatives
            result["path_runner_up_margin"] = float(np.mean(margins[np.isfinite(margins)])) if np.isfinite(margins).any() else float("nan")
            result["path_runner_up_close"] = float(np.mean(per_frame < np.log(2.0)))
            print("runner-up trajectories (log score ratios under the motion model's conventions, not probabilities): mean runner-up "
                  "margin {:.3f}, {:.1%} of the joint-frames decided by less than ln 2, {} not complete".format(
                      result["path_runner_up_margin"], result["path_runner_up_close"],
                      int(sum((~fr["complete"]).sum() for fr in path_alternatives))))
    if map_pose is not None:
        posed = [np.asarray(fr["joints"], dtype=np.float32) for fr in frame_map]
        frame_alternatives = frame_map if "separation" in map_pose else None
        if frame_alternatives is not None:                               # the pose dicts are the leading entries
            from sceneego_amd.op import POSE_KEYS
            frame_map = [{k: fr[k] for k in POSE_KEYS + ("shift", "bone_error_before")} for fr in frame_alternatives]
        for path, obj in ((args.map_output, posed), (args.map_info_output, frame_map), (args.map_alternatives_output, frame_alternatives)):
            if path is not None:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "wb") as f:
                    pickle.dump(obj, f)
        result["map"], result["map_info"], result["bone_lengths"] = posed, frame_map, np.asarray(lengths, dtype=np.float64)
        result["map_mpjpe"] = M.mpjpe(np.stack(posed).astype(np.float64), gt)
        others = "".join(f", {name} {result[key]}" for name, key in (("coupled", "coupled_mpjpe"), ("path", "path_mpjpe")) if key in result)
        bones = ", coupled {:.4f} m".format(float(np.mean([fr["bone_error"] for fr in frame_skeleton]))) if skeleton is not None else ""
        print("most probable pose (a convention, not calibrated): mpjpe: {} (soft-argmax {}{}), mean shift {:.4f} m, mean bone error "
              "{:.4f} -> {:.4f} m{}, {} jumps in {} joint-frames, {} frames not solved".format(
                  result["map_mpjpe"], mpjpe, others, float(np.nanmean([fr["shift"] for fr in frame_map])),
                  float(np.mean([fr["bone_error_before"] for fr in frame_map])), float(np.nanmean([fr["bone_error"] for fr in frame_map])),
                  bones, int(sum(fr["jumped"].sum() for fr in frame_map)), int(sum(fr["index"].size for fr in frame_map)),
                  int(sum(not fr["solved"] for fr in frame_map))))
        if frame_alternatives is not None:
            margins = np.array([fr["runner_up_margin"] for fr in frame_alternatives], dtype=np.float64)
            result["map_alternatives"] = frame_alternatives
            result["map_runner_up_margin"] = float(np.mean(margins[np.isfinite(margins)])) if np.isfinite(margins).any() else float("nan")
            result["map_runner_up_close"] = float(np.mean(margins < np.log(2.0)))
            print("runner-up pose (separation {} voxels; a convention, not calibrated): mean runner-up margin {:.4f}, {:.1%} of {} frames "
                  "below ln 2, {} frames not complete".format(map_pose["separation"], result["map_runner_up_margin"],
                                                              result["map_runner_up_close"], len(margins),
                                                              int(sum(not fr["complete"] for fr in frame_alternatives))))
    if pose_sample is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.pose_samples_output)), exist_ok=True)
        with open(args.pose_samples_output, "wb") as f:
            pickle.dump(frame_pose_samples, f)
        result["pose_samples"], result["bone_lengths"] = frame_pose_samples, np.asarray(lengths, dtype=np.float64)
        # nested: --sample_output puts the trajectory sampler's figures under the same names at the top level
        ps = result["pose_samples_summary"] = {**M.best_of_samples(frame_pose_samples, pred, gt),
                                               **M.best_pose_of_samples(frame_pose_samples, pred, gt)}
        from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS
        bone = np.asarray(lengths, dtype=np.float64).reshape(-1)[-(len(KINEMATIC_PARENTS) - 1):]
        raw_bone = np.abs(np.linalg.norm(pred[:, 1:] - pred[:, list(KINEMATIC_PARENTS[1:])], axis=-1) - bone)
        sample_bone = np.concatenate([np.asarray(fr["bone_error"], dtype=np.float64).reshape(-1) for fr in frame_pose_samples])
        ps["mean_bone_error"] = float(np.nanmean(sample_bone)) if np.isfinite(sample_bone).any() else float("nan")
        ps["estimate_bone_error"] = float(raw_bone.mean())
        print("pose samples (the skeleton model's posterior given the volumes read as likelihoods, not calibrated; the spread is no error "
              "bar): {} per frame, seed {}: mean spread {:.4f} m, mean bone error {:.4f} m (soft-argmax joints {:.4f} m), best-of-{} mpjpe "
              "per joint: {}, per whole pose: {} (soft-argmax {}), {} of {} draws valid, {} frames without a whole pose".format(
                  pose_sample["samples"], pose_sample["seed"], ps["mean_sample_spread"], ps["mean_bone_error"],
                  ps["estimate_bone_error"], pose_sample["samples"], ps["best_of_n_mpjpe"], ps["best_pose_of_n_mpjpe"], mpjpe,
                  ps["valid_draws"], ps["draws"], ps["frames_without_pose"]))
    if scene_field is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.scene_field_output)), exist_ok=True)
        with open(args.scene_field_output, "wb") as f:
            pickle.dump(frame_scene_field, f)
        result["scene_field"] = frame_scene_field
        result["scene_field_summary"] = M.scene_field_summary(
            [fr["volumes"] for fr in frame_scene_field],
            sample_frames=[fr["pose_samples"] for fr in frame_scene_field] if pose_sample is not None else None)
        print(M.format_scene_field_summary(result["scene_field_summary"]))
    return result


if __name__ == "__main__":
    main()
