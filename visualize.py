#!/usr/bin/env python3
"""Counterpart of the reference's ``visualize.py`` (``visualize.py:12-38``) on MI355X, without a display: one frame, its depth map
and its predicted pose -> a rendered image of the scene point cloud with the skeleton, the skeleton drawn into the fisheye frame,
and the point cloud as a PLY file.

    python visualize.py --img_path data/demo/imgs/img_001000.jpg --depth_path data/demo/depths/img_001000.jpg.exr \\
                        --pose_path data/demo/out/img_001000.jpg.pkl [--output render.png] [--overlay overlay.png] [--ply scene.ply]
                        [--azimuth 35 --elevation 25 --distance 3.5 --fov 50 --size 720x960 --splat 2] [--format png|jpg]
                        [--volumes_path img_001000.jpg.volumes.npy [--volume_joints 9,10,13,14] [--cuboid_side 2]]

The reference opens an open3d window (``draw_geometries([scene, predicted_pose_mesh])``); this script renders the same two
geometries on the device (``sceneego_amd/render.py``, ``csrc/render.hip``) and writes files.  It reads what ``demo.py`` reads and
writes: the frame (a baseline JPEG is decoded on the device where that path takes the file, otherwise by PIL), the depth map
(``.exr`` / ``.npy`` / ``.npz``) and the pickle of float32 [15, 3] joints.  An empty string for ``--output`` / ``--overlay`` /
``--ply`` skips that file.  ``--format jpg`` writes the two images as quality-90 4:4:4 JPEG files encoded on the device
(``sceneego_amd/jpeg_encode.py``); their default names become ``render.jpg`` and ``overlay.jpg``.  ``--volumes_path`` takes the
float32 [15, G, G, G] file ``demo.py --save_volumes true`` writes and draws the joint probability volumes over both images
(``SceneRenderer.render_volumes`` / ``overlay_volumes``).
"""
import argparse
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CALIBRATION = os.path.join(ROOT, "sceneego_amd", "calibration", "fisheye.calibration_05_08.json")


def _size(text):
    try:
        h, w = (int(v) for v in text.lower().split("x"))
        if h <= 0 or w <= 0:
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError(f"--size wants HxW, e.g. 720x960; got {text!r}")
    return h, w


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--img_path", type=str, required=True)
    ap.add_argument("--depth_path", type=str, required=True)
    ap.add_argument("--pose_path", type=str, required=True)
    ap.add_argument("--output", type=str, default=None,
                    help="third-person view of the point cloud and the skeleton (default: render.png, or render.jpg with --format jpg)")
    ap.add_argument("--overlay", type=str, default=None,
                    help="the skeleton drawn into the fisheye frame (default: overlay.png, or overlay.jpg with --format jpg)")
    ap.add_argument("--format", type=str, default="png", choices=("png", "jpg"),
                    help="png (PIL on the host) or jpg (quality-90 4:4:4 JPEG encoded on the device)")
    ap.add_argument("--png_encoder", type=str, default="host", choices=("host", "device"),
                    help="with --format png: host (PIL) or device (lossless, sceneego_amd/png_encode.py: the same pixels)")
    ap.add_argument("--ply", type=str, default="scene.ply", help="the coloured point cloud (binary PLY)")
    ap.add_argument("--azimuth", type=float, default=35.0, help="degrees around the cuboid centre (0, 0, 1)")
    ap.add_argument("--elevation", type=float, default=25.0, help="degrees towards the head camera")
    ap.add_argument("--distance", type=float, default=3.5, help="metres from the cuboid centre")
    ap.add_argument("--fov", type=float, default=50.0, help="vertical field of view, degrees")
    ap.add_argument("--size", type=_size, default=(720, 960), help="HxW of the rendered view")
    ap.add_argument("--splat", type=int, default=2, choices=(1, 2, 3, 4), help="footprint of a point, pixels")
    ap.add_argument("--calibration", type=str, default=CALIBRATION)
    ap.add_argument("--volumes_path", type=str, default=None,
                    help="float32 [15,G,G,G] .npy of demo.py --save_volumes true: draw the joint probability volumes over both images")
    ap.add_argument("--volume_joints", type=str, default=None, help="with --volumes_path: the joints to draw, e.g. 9,10,13,14 (default: all)")
    ap.add_argument("--cuboid_side", type=float, default=2.0, help="with --volumes_path: side of the volume's cuboid, metres")
    args = ap.parse_args(argv)
    if args.volume_joints is not None and args.volumes_path is None:
        ap.error("--volume_joints needs --volumes_path")
    from sceneego_amd.render import parse_joint_list
    try:
        args.volume_joints = parse_joint_list(args.volume_joints)
    except ValueError as e:
        ap.error(str(e))
    if args.output is None:
        args.output = "render." + args.format
    if args.overlay is None:
        args.overlay = "overlay." + args.format
    return args


def load_frame(img_path, device):
    """uint8 [1, H, W, 3] (B, G, R) on the device: decoded there when the JPEG path takes the file, else by PIL."""
    import torch

    from sceneego_amd.jpeg_device import JpegFile, decode_jpeg_batch
    from sceneego_amd.preprocess import load_image_bgr
    jpeg = JpegFile(img_path) if img_path.lower().endswith((".jpg", ".jpeg")) else None
    if jpeg is not None and jpeg.device:
        return decode_jpeg_batch([jpeg], device)
    return torch.from_numpy(load_image_bgr(img_path))[None].to(device)


def visualize(args):
    import torch

    from sceneego_amd.preprocess import load_depth
    from sceneego_amd.render import SceneRenderer, orbit_view, save_jpeg, save_png, write_ply
    if not torch.cuda.is_available():
        raise RuntimeError("visualize.py needs an MI355X (HIP device); the renderer has no CPU fallback")
    device = torch.device("cuda")
    with open(args.pose_path, "rb") as f:
        pose = pickle.load(f)
    frame = load_frame(args.img_path, device)
    depth = torch.from_numpy(load_depth(args.depth_path))[None].to(device)
    renderer = SceneRenderer(args.calibration, frame_size=tuple(frame.shape[1:3]), out_size=args.size, fov_y_deg=args.fov,
                             splat=args.splat, device=device)
    save = save_jpeg if getattr(args, "format", "png") == "jpg" else save_png
    if getattr(args, "format", "png") == "png" and getattr(args, "png_encoder", "host") == "device":
        from sceneego_amd.png_encode import save_png_device as save
    volumes = None
    if getattr(args, "volumes_path", None):
        import numpy as np
        volumes = torch.from_numpy(np.ascontiguousarray(np.load(args.volumes_path), dtype=np.float32)).to(device)
        which, side = getattr(args, "volume_joints", None), getattr(args, "cuboid_side", 2.0)
    written = []
    if args.output:
        view = orbit_view(args.azimuth, args.elevation, args.distance)
        if volumes is None:
            save(args.output, renderer.render(depth, frame, pose, view=view)[0])
        else:
            save(args.output, renderer.render_volumes(depth, frame, pose, volumes, side, view=view, joint_mask=which)[0])
        written.append(args.output)
    if args.overlay:
        if volumes is None:
            save(args.overlay, renderer.overlay(frame, pose, depth=depth)[0])
        else:
            save(args.overlay, renderer.overlay_volumes(frame, pose, volumes, side, depth=depth, joint_mask=which)[0])
        written.append(args.overlay)
    if args.ply:
        write_ply(args.ply, *renderer.scene_points(depth, frame))
        written.append(args.ply)
    return written


def main(argv=None):
    for path in visualize(parse_args(argv)):
        print(path)


if __name__ == "__main__":
    main()
