"""ctypes binding of ``libsceneego_hip.so`` (C ABI declared in ``include/sceneego_hip.h``).

PyTorch is only the allocator and stream provider here: every call passes ``tensor.data_ptr()`` and the
current HIP stream.  There is deliberately NO fallback: if the shared library is missing, or a tensor
is not on a HIP device, the call raises.
"""
from __future__ import annotations

import ctypes
import numbers
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# tools/ may point at the development build (csrc/build.sh --devtools -> libsceneego_hip_dev.so)
LIB_PATH = os.environ.get("SCENEEGO_HIP_LIB") or os.path.join(_HERE, "libsceneego_hip.so")
ABI_VERSION = 43

EPI_RELU = 1
EPI_RES_PRE_RELU = 2
EPI_RES_POST_RELU = 4
EPI_OUT_PLANAR = 8
IN_OCTET = 32       # se_conv3d_f32, 2-D Winograd 3x3x3 shapes: octet-planar input [B][C/8][D][D][D][8]
OUT_OCTET = 64      # ... octet-planar output
RES_OCTET = 128     # ... octet-planar skip tensor
IN_QUAD = 1024      # se_conv3d_f32, launches whose variant (with these flags) is 3: quad-planar input [B][C/4][D][D][D][4]
OUT_QUAD = 2048     # ... quad-planar output
RES_QUAD = 4096     # ... quad-planar skip tensor
IN_PLANAR3 = 16     # se_conv3d_f32, k = 7: triplet-planar input [B][ceil(cin/3)][D][D][D][3]

_vp, _i, _f, _d, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong
_u = ctypes.c_uint

# name -> (restype, argtypes); must list every symbol of include/sceneego_hip.h (tests/test_abi.py checks)
SIGNATURES = {
    "se_abi_version": (_i, []),
    "se_voxelize_f64": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _vp]),
    "se_voxelize_strided_f64": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _i, _i, _vp]),
    "se_voxelize_full_f64": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _d, _vp]),
    "se_unproject_gather_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_unproject_gather_planar3_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_voxelize_planar3_f64": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _i, _i, _vp]),
    "se_unproject_gather_planar1_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_voxelize_planar1_f64": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _i, _i, _vp]),
    "se_intersection_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "se_bias_act_nchw_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "se_deconv2d_k4s2_assemble_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_bias_relu_maxpool3x3s2_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "se_conv2d_1x1_tile_f32": (_i, [_i, _i, _i, _i]),
    "se_conv2d_1x1_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_conv2d_1x1_small_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_conv2d_1x1_small_s2_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_conv2d_1x1_s2_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_conv2d_3x3_tile_f32": (_i, [_i, _i, _i, _i, _i]),
    "se_conv2d_3x3_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_conv2d_3x3_s2_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_conv3d_pack_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_conv3d_packed_elems": (_ll, [_i, _i, _i, _i]),
    "se_conv3d_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _ll, _vp]),
    "se_conv3d_pool_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _ll, _vp]),
    "se_conv3d_skip16_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_pointwise_chain3_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "se_deconv3d_k2s2_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_maxpool3d_2_f32": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "se_maxpool3d_2_octin_f32": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "se_softargmax3d_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "se_softargmax3d_scratch_elems": (_ll, [_i]),
    "se_softargmax3d_finish_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "se_joint_stats_scratch_elems": (_ll, [_i]),
    "se_joint_stats_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "se_pointwise_chain3_softargmax_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "se_conv3d_pack_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_conv3d_packed_elems_bf16": (_ll, [_i, _i, _i, _i]),
    "se_conv3d_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_pointwise_chain3_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "se_pointwise_chain3_softargmax_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "se_deconv3d_k2s2_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_maxpool3d_2_bf16": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "se_unproject_gather_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_voxelize_strided_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _i, _i, _vp]),
    "se_preprocess_image_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "se_bias_act_nchw_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "se_conv3d_f32_algo": (_i, [_i, _i, _i, _i]),
    "se_conv3d_f32_variant": (_i, [_i, _i, _i, _i, _i, _i]),
    "se_conv3d_k7_fft_packed_elems": (_ll, [_i, _i]),
    "se_conv3d_k7_fft_pack_f32": (_i, [_vp, _vp, _vp, _f, _vp, _i, _i, _vp]),
    "se_conv3d_k7_fft_workspace_elems": (_ll, [_i, _i, _i]),
    "se_conv3d_k7_fft_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _ll, _vp]),
    "se_conv3d_split3_packed_elems": (_ll, [_i, _i]),
    "se_conv3d_split3_pack": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "se_conv3d_k3_split3_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_conv3d_split6_packed_elems": (_ll, [_i, _i, _i, _i]),
    "se_conv3d_split6_pack": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "se_deconv2d_k4s2_s6_domain": (_i, [_i, _i, _i, _i, _i]),
    "se_deconv2d_k4s2_s6_packed_elems": (_ll, [_i, _i]),
    "se_deconv2d_k4s2_s6_pack": (_i, [_vp, _vp, _i, _i, _vp]),
    "se_deconv2d_k4s2_s6_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_conv3d_w6_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _ll, _vp]),
    "se_conv3d_f32_split6": (_i, [_i, _i, _i, _i, _i, _i]),
    "se_conv3d_k3_split6_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "se_split6_planes_f32": (_i, [_vp, _vp, _ll, _vp]),
    "se_exr_piz_scratch_bytes": (_ll, [_vp, _i, _vp, _i]),
    "se_exr_piz_decode_f32": (_i, [_vp, _ll, _vp, _i, _vp, _i, _vp, _i, _i, _f, _vp, _ll, _vp, _vp]),
    "se_exr_zip_scratch_bytes": (_ll, [_vp, _i, _vp, _i]),
    "se_exr_zip_decode_f32": (_i, [_vp, _ll, _vp, _i, _vp, _i, _vp, _i, _i, _f, _vp, _ll, _vp, _vp]),
    "se_jpeg_scratch_bytes": (_ll, [_vp, _i, _vp, _i, _vp]),
    "se_jpeg_decode_bgr_u8": (_i, [_vp, _ll, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _ll, _vp, _i, _vp]),
    "se_jpeg_encode_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_jpeg_encode_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _ll, _vp, _vp, _vp, _ll, _vp]),
    "se_png_encode_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_png_encode_bound": (_ll, [_i, _i, _i]),
    "se_png_encode_u8": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _ll, _vp]),
    "se_render_splat_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _d, _d, _d, _i, _d, _d, _d, _vp]),
    "se_render_resolve_f64": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "se_render_overlay_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _d, _d, _vp, _vp, _vp]),
    "se_render_volume_palette": (None, [_vp]),
    "se_render_volume_packed_bytes": (_ll, [_i, _i]),
    "se_render_volume_pack_f32": (_i, [_vp, _vp, _ll, _i, _i, _vp]),
    "se_render_volume_view_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, ctypes.c_uint, _d, _d, _vp]),
    "se_render_volume_overlay_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _d, ctypes.c_uint, _d, _d, _vp]),
    "se_scene_probe_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_scene_probe_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _d, _d, _vp]),
    "se_scene_free_mask_u8": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _d, _vp]),
    "se_softargmax3d_masked_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "se_softargmax3d_masked_scratch_elems": (_ll, [_i]),
    "se_scene_sites_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _d, _d, _vp]),
    "se_scene_distance_scratch_bytes": (_ll, [_i, _i]),
    "se_scene_distance_i32": (_i, [_vp, _vp, _vp, _vp, _ll, _i, _i, _vp]),
    "se_scene_expect_scratch_elems": (_ll, [_i]),
    "se_scene_expect_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "se_joint_modes_scratch_bytes": (_ll, [_i, _i, _i]),
    "se_joint_modes_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp]),
    "se_volume_filter_scratch_bytes": (_ll, [_i, _i, _i]),
    "se_volume_filter_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "se_volume_smooth_scratch_bytes": (_ll, [_i, _i, _i]),
    "se_volume_smooth_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "se_volume_transition_stats_scratch_bytes": (_ll, [_i, _i, _i]),
    "se_volume_transition_stats_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "se_volume_sample_scratch_bytes": (_ll, [_i, _i, _i]),
    "se_volume_sample_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _i, _ll, _ll, _u, _u, _vp, _vp]),
    "se_volume_viterbi_scratch_bytes": (_ll, [_i, _i, _i]),
    "se_volume_viterbi_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "se_volume_viterbi_path_i32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "se_volume_viterbi_refine_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_volume_viterbi_keep_f32": (_i, [_vp] * 12 + [_ll, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "se_volume_viterbi_back_scratch_bytes": (_ll, [_i, _i, _i]),
    "se_volume_viterbi_back_f32": (_i, [_vp] * 21 + [_ll, _i, _i, _i, _i, _i, _f, _i, _i, _vp]),
    "se_volume_viterbi_branch_i32": (_i, [_vp] * 7 + [_i, _i, _i, _i, _i, _vp]),
    "se_shell_correlate_scratch_bytes": (_ll, [_i, _i]),
    "se_shell_correlate_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _f, _f, _vp]),
    "se_skeleton_couple_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_skeleton_couple_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp]),
    "se_shell_moments_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_shell_moments_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _vp]),
    "se_skeleton_edge_stats_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_skeleton_edge_stats_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp]),
    "se_skeleton_upward_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_skeleton_upward_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp]),
    "se_skeleton_sample_scratch_bytes": (_ll, [_i, _i, _i]),
    "se_skeleton_sample_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _i, _ll, _ll, _u, _u, _vp]),
    "se_shell_maxcorr_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _f, _vp]),
    "se_shell_argmax_i32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "se_skeleton_pose_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_skeleton_pose_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp]),
    "se_skeleton_alternatives_scratch_bytes": (_ll, [_i, _i, _i, _i]),
    "se_skeleton_alternatives_f32": (_i, [_vp, _vp, _vp, _i] + [_vp] * 16 + [_ll, _i, _i, _i, _i, _i, _f, _vp]),
}
# present only in development builds (csrc/build.sh --devtools): A/B kernel selection and cycle-stamp diagnostics (tools/)
DEVTOOLS_SIGNATURES = {
    "se_debug_set_variant": (None, [_i]),
    "se_debug_set_stamp_buffer": (None, [_vp]),
}

_lib = None


class HipExtensionError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load the shared library once; raise loudly when it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or sceneego_amd/csrc/build.sh). The SceneEgo hot path has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in DEVTOOLS_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    got = lib.se_abi_version()
    if got != ABI_VERSION:
        raise HipExtensionError(f"libsceneego_hip.so ABI {got} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def source_fingerprint() -> str:
    """sha256 over the kernel sources (csrc/*.hip, *.h, build.sh and the C-ABI header), names included, in sorted order.
    rocprofv3 counter records under profiles/ carry it, so a record taken on other kernels is recognised as stale (bench.py)."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".sh")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "sceneego_hip.h"))
    for p in files:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def built_fingerprint() -> str | None:
    """source_fingerprint() of the sources the loaded shared library was built from (written by csrc/build.sh next to the .so),
    or None when the stamp is missing."""
    try:
        with open(os.path.splitext(LIB_PATH)[0] + ".srchash") as f:
            return f.read().strip() or None
    except OSError:
        return None


def require_hip(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipExtensionError("SceneEgo HIP operators need tensors on a HIP device (got %s)" % t.device)
    load()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(code: int, what: str) -> None:
    if code != 0:
        raise HipExtensionError(f"{what} failed with code {code}" + (" (bad argument)" if code == -1 else " (hipError_t)"))


def _chk_f32(*ts):
    for t in ts:
        if t is not None:
            assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())


# ---------------------------------------------------------------------------------------------
def _check_args(what, named, optional=(), device=None):
    """Every entry (name, tensor, dtype, size) of ``named``, and every entry of ``optional`` whose tensor is not None, is a contiguous
    tensor of that dtype on one HIP device (``device``, or the first entry's), else HipExtensionError naming the operator and the
    argument: the kernels trust what they are given, so this runs before anything is launched.  ``size``: None (any), an int (the
    number of elements) or a shape, in which None stands for any extent.  Returns the device."""
    for name, t, dtype, size in tuple(named) + tuple(e for e in optional if e[1] is not None):
        if not isinstance(t, torch.Tensor):
            raise HipExtensionError(f"{what}: {name} is not a tensor")
        if not t.is_cuda:
            raise HipExtensionError(f"{what}: {name} is on {t.device}: the operator needs tensors on a HIP device (there is no CPU fallback)")
        if t.dtype != dtype or not t.is_contiguous():
            raise HipExtensionError(f"{what}: {name} is {t.dtype} (contiguous: {t.is_contiguous()}), expected contiguous {dtype}")
        if isinstance(size, tuple):
            if t.dim() != len(size) or any(want is not None and have != want for have, want in zip(t.shape, size)):
                raise HipExtensionError(f"{what}: {name} has shape {tuple(t.shape)}, expected {size}")
        elif size is not None and t.numel() != size:
            raise HipExtensionError(f"{what}: {name} has {t.numel()} elements, expected {size}")
        if device is None:
            device = t.device
        if t.device != device:
            raise HipExtensionError(f"{what}: {name} is on {t.device}, expected {device}")
    return device


def _scratch(what, scratch, need, dtype, device):
    """The optional workspace of an operator: allocated per call when None, else (type and device checked by _check_args) big enough."""
    if scratch is None:
        return torch.empty(need, device=device, dtype=dtype)
    if scratch.numel() < need:
        raise HipExtensionError(f"{what}: scratch has {scratch.numel()} elements of {dtype}, needs {need}")
    return scratch


def _overlap(a, b) -> bool:
    """The storage of two contiguous tensors overlaps."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def voxelize(depth, ray_tab, occ, batch, depth_h, depth_w, up, pad_x, volume_size, cuboid_side):
    require_hip(depth, ray_tab, occ)
    _chk_f32(depth, occ)
    assert ray_tab.dtype == torch.float64 and ray_tab.is_contiguous()
    _check(load().se_voxelize_f64(_ptr(depth), _ptr(ray_tab), _ptr(occ), batch, depth_h, depth_w, up, pad_x,
                                  volume_size, float(cuboid_side), _stream()), "se_voxelize_f64")


def voxelize_strided(depth, ray_tab, buf, batch, depth_h, depth_w, up, pad_x, volume_size, cuboid_side, stride_c, c_offset):
    require_hip(depth, ray_tab, buf)
    _chk_f32(depth)
    assert ray_tab.dtype == torch.float64 and ray_tab.is_contiguous() and buf.is_contiguous()
    assert buf.dtype in (torch.bfloat16, torch.float32)
    if buf.dtype == torch.bfloat16:     # octet-planar [B][stride_c / 8][N][8]
        _check(load().se_voxelize_strided_bf16(_ptr(depth), _ptr(ray_tab), _ptr(buf), batch, depth_h, depth_w, up, pad_x,
                                               volume_size, float(cuboid_side), stride_c // 8, c_offset, _stream()),
               "se_voxelize_strided_bf16")
        return
    _check(load().se_voxelize_strided_f64(_ptr(depth), _ptr(ray_tab), _ptr(buf), batch, depth_h, depth_w, up, pad_x,
                                          volume_size, float(cuboid_side), stride_c, c_offset, _stream()),
           "se_voxelize_strided_f64")


def voxelize_planar3(depth, ray_tab, buf, batch, depth_h, depth_w, up, pad_x, volume_size, cuboid_side, triplets_total, channel):
    """Scatter the occupancy into slot `channel` of a triplet-planar float32 buffer (cleared by unproject_gather_planar3)."""
    require_hip(depth, ray_tab, buf)
    _chk_f32(depth, buf)
    assert ray_tab.dtype == torch.float64 and ray_tab.is_contiguous()
    assert buf.numel() == batch * triplets_total * volume_size ** 3 * 3
    _check(load().se_voxelize_planar3_f64(_ptr(depth), _ptr(ray_tab), _ptr(buf), batch, depth_h, depth_w, up, pad_x,
                                          volume_size, float(cuboid_side), triplets_total, channel, _stream()),
           "se_voxelize_planar3_f64")


def voxelize_planar1(depth, ray_tab, buf, batch, depth_h, depth_w, up, pad_x, volume_size, cuboid_side, planes_total, channel):
    """Scatter the occupancy into plane `channel` of a planar float32 buffer [B, planes_total, G^3] (cleared by unproject_gather_planar1)."""
    require_hip(depth, ray_tab, buf)
    _chk_f32(depth, buf)
    assert ray_tab.dtype == torch.float64 and ray_tab.is_contiguous()
    assert buf.numel() == batch * planes_total * volume_size ** 3
    _check(load().se_voxelize_planar1_f64(_ptr(depth), _ptr(ray_tab), _ptr(buf), batch, depth_h, depth_w, up, pad_x,
                                          volume_size, float(cuboid_side), planes_total, channel, _stream()),
           "se_voxelize_planar1_f64")


def voxelize_full(depth, ray_tab, occ, batch, depth_h, depth_w, volume_size, cuboid_side):
    require_hip(depth, ray_tab, occ)
    _chk_f32(depth, occ)
    assert ray_tab.dtype == torch.float64 and ray_tab.is_contiguous()
    _check(load().se_voxelize_full_f64(_ptr(depth), _ptr(ray_tab), _ptr(occ), batch, depth_h, depth_w,
                                       volume_size, float(cuboid_side), _stream()), "se_voxelize_full_f64")


def preprocess_image_u8(img_u8, out, crop_x, mean3, std3):
    """img_u8 [B,H,W,3] uint8 BGR on the device -> out [B,3,H/4,(W-2*crop_x)/4] float32 (normalised, reference arithmetic)."""
    require_hip(img_u8, out)
    assert img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.shape[-1] == 3
    _chk_f32(out)
    B, H, W, _ = img_u8.shape
    m = (ctypes.c_double * 3)(*[float(x) for x in mean3])
    sd = (ctypes.c_double * 3)(*[float(x) for x in std3])
    _check(load().se_preprocess_image_u8(_ptr(img_u8), _ptr(out), B, H, W, crop_x, m, sd, _stream()), "se_preprocess_image_u8")
    return out



def _exr_scratch_bytes(codec, chunk_desc, channel_desc) -> int:
    import numpy as np
    assert chunk_desc.dtype == np.int64 and chunk_desc.flags.c_contiguous and chunk_desc.shape[1:] == (16,)
    assert channel_desc.dtype == np.int32 and channel_desc.flags.c_contiguous and channel_desc.shape[1:] == (8,)
    name = f"se_exr_{codec}_scratch_bytes"
    n = getattr(load(), name)(chunk_desc.ctypes.data_as(_vp), chunk_desc.shape[0], channel_desc.ctypes.data_as(_vp), channel_desc.shape[0])
    if n < 0:
        raise HipExtensionError(f"{name} failed with code {n} (bad argument)")
    return int(n)


def _exr_decode(codec, payload_ptr, payload_bytes, desc_ptr, n_chunks, chan_ptr, n_files, out, clamp, scratch, status):
    require_hip(out, scratch, status)
    _chk_f32(out)
    assert out.dim() == 3 and out.shape[0] == n_files and status.dtype == torch.int32 and status.shape == (n_chunks, 2)
    assert scratch.dtype == torch.uint8 and status.is_contiguous()
    name = f"se_exr_{codec}_decode_f32"
    _check(getattr(load(), name)(_vp(payload_ptr), int(payload_bytes), _vp(desc_ptr), n_chunks, _vp(chan_ptr), n_files, _ptr(out),
                                 out.shape[1], out.shape[2], float(clamp), _ptr(scratch), scratch.numel(), _ptr(status), _stream()), name)


def exr_piz_scratch_bytes(chunk_desc, channel_desc) -> int:
    """chunk_desc int64 [n, 16] and channel_desc int32 [files, 8] (HOST numpy arrays, include/sceneego_hip.h): fills the scratch
    offset / record capacity columns of chunk_desc in place and returns the scratch bytes of se_exr_piz_decode_f32."""
    return _exr_scratch_bytes("piz", chunk_desc, channel_desc)


def exr_piz_decode(payload_ptr, payload_bytes, desc_ptr, n_chunks, chan_ptr, n_files, out, clamp, scratch, status):
    """PIZ chunks -> out float32 [n_files, H_out, W_out] on the current stream.  payload_ptr / desc_ptr / chan_ptr: device addresses
    (ints) inside a buffer the caller keeps alive; status int32 [n_chunks, 2]."""
    _exr_decode("piz", payload_ptr, payload_bytes, desc_ptr, n_chunks, chan_ptr, n_files, out, clamp, scratch, status)


def exr_zip_scratch_bytes(chunk_desc, channel_desc) -> int:
    """As exr_piz_scratch_bytes (the columns are scratch offset / bytes), for se_exr_zip_decode_f32."""
    return _exr_scratch_bytes("zip", chunk_desc, channel_desc)


def exr_zip_decode(payload_ptr, payload_bytes, desc_ptr, n_chunks, chan_ptr, n_files, out, clamp, scratch, status):
    """As exr_piz_decode, for ZIP / ZIPS / NONE chunks."""
    _exr_decode("zip", payload_ptr, payload_bytes, desc_ptr, n_chunks, chan_ptr, n_files, out, clamp, scratch, status)


def jpeg_scratch_bytes(img_desc, seg_desc, layout) -> int:
    """img_desc int32 [n, 64], seg_desc int64 [m, 8] and layout int64 [>= 4] (HOST numpy arrays, include/sceneego_hip.h): fills the
    derived columns and the layout in place and returns the scratch bytes of se_jpeg_decode_bgr_u8."""
    import numpy as np
    assert img_desc.dtype == np.int32 and img_desc.flags.c_contiguous and img_desc.shape[1:] == (64,)
    assert seg_desc.dtype == np.int64 and seg_desc.flags.c_contiguous and seg_desc.shape[1:] == (8,)
    assert layout.dtype == np.int64 and layout.flags.c_contiguous and layout.size >= 4
    n = load().se_jpeg_scratch_bytes(img_desc.ctypes.data_as(_vp), img_desc.shape[0], seg_desc.ctypes.data_as(_vp),
                                     seg_desc.shape[0], layout.ctypes.data_as(_vp))
    if n < 0:
        raise HipExtensionError(f"se_jpeg_scratch_bytes failed with code {n} (bad argument)")
    return int(n)


def jpeg_decode(payload_ptr, payload_bytes, img_ptr, n_images, seg_ptr, n_segs, tables_ptr, quant_ptr, layout, out, scratch, status,
                rounds=-1):
    """JPEG segments -> out uint8 [B, H, W, 3] (B, G, R) on the current stream.  *_ptr: device addresses (ints) inside a buffer the
    caller keeps alive; layout: the host int64 array se_jpeg_scratch_bytes filled; status int32 [n_segs, 2]."""
    require_hip(out, scratch, status)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 4 and out.shape[3] == 3
    assert scratch.dtype == torch.uint8 and status.dtype == torch.int32 and status.shape == (n_segs, 2) and status.is_contiguous()
    _check(load().se_jpeg_decode_bgr_u8(_vp(payload_ptr), int(payload_bytes), _vp(img_ptr), n_images, _vp(seg_ptr), n_segs,
                                        _vp(tables_ptr), _vp(quant_ptr), layout.ctypes.data_as(_vp), _ptr(out), out.shape[0],
                                        out.shape[1], out.shape[2], _ptr(scratch), scratch.numel(), _ptr(status), int(rounds),
                                        _stream()), "se_jpeg_decode_bgr_u8")


def unproject_gather(feat, idx, w, out, batch, texels, channels, voxels, out_stride_c, out_c_offset):
    require_hip(feat, idx, w, out)
    _chk_f32(feat, w)
    assert idx.dtype == torch.int32 and idx.is_contiguous() and out.is_contiguous()
    assert out.dtype in (torch.bfloat16, torch.float32)
    if out.dtype == torch.bfloat16:     # octet-planar [B][out_stride_c / 8][voxels][8]
        _check(load().se_unproject_gather_bf16(_ptr(feat), _ptr(idx), _ptr(w), _ptr(out), batch, texels, channels,
                                               voxels, out_stride_c // 8, out_c_offset, _stream()), "se_unproject_gather_bf16")
        return
    _check(load().se_unproject_gather_f32(_ptr(feat), _ptr(idx), _ptr(w), _ptr(out), batch, texels, channels,
                                          voxels, out_stride_c, out_c_offset, _stream()), "se_unproject_gather_f32")


def unproject_gather_planar3(feat, idx, w, out, batch, texels, channels, voxels, triplets_total):
    require_hip(feat, idx, w, out)
    _chk_f32(feat, w, out)
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    assert out.numel() == batch * triplets_total * voxels * 3
    _check(load().se_unproject_gather_planar3_f32(_ptr(feat), _ptr(idx), _ptr(w), _ptr(out), batch, texels, channels,
                                                  voxels, triplets_total, _stream()), "se_unproject_gather_planar3_f32")


def unproject_gather_planar1(feat, idx, w, out, batch, texels, channels, voxels, planes_total):
    require_hip(feat, idx, w, out)
    _chk_f32(feat, w, out)
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    assert out.numel() == batch * planes_total * voxels
    _check(load().se_unproject_gather_planar1_f32(_ptr(feat), _ptr(idx), _ptr(w), _ptr(out), batch, texels, channels,
                                                  voxels, planes_total, _stream()), "se_unproject_gather_planar1_f32")


def intersection(buf, occ, batch, voxels, channels, stride_c):
    require_hip(buf, occ)
    _chk_f32(buf, occ)
    _check(load().se_intersection_f32(_ptr(buf), _ptr(occ), batch, voxels, channels, stride_c, _stream()),
           "se_intersection_f32")


def bias_act_nchw(x, bias, residual, relu):
    """In place on ``x`` [N,C,H,W] (contiguous): x = relu?(x + bias[c] (+ residual)).  float32: any map size; bfloat16: H * W % 8 == 0."""
    require_hip(x, bias)
    n, c, hh, ww = x.shape
    if x.dtype == torch.bfloat16:
        assert bias.dtype == torch.bfloat16 and x.is_contiguous() and (residual is None or (residual.dtype == x.dtype and residual.is_contiguous()))
        _check(load().se_bias_act_nchw_bf16(_ptr(x), _ptr(bias), _ptr(residual), _ptr(x), n, c, hh * ww, 1 if relu else 0,
                                            _stream()), "se_bias_act_nchw_bf16")
        return x
    _chk_f32(x, bias, residual)
    _check(load().se_bias_act_nchw_f32(_ptr(x), _ptr(bias), _ptr(residual), _ptr(x), n, c, hh * ww, 1 if relu else 0,
                                       _stream()), "se_bias_act_nchw_f32")
    return x


def bias_relu_maxpool(x, bias):
    """``x`` [B, C, 2 ho, 2 wo] float32 (raw stem convolution) -> max_pool2d(relu(x + bias), 3, stride 2, padding 1) [B, C, ho, wo] in one
    pass (se_bias_relu_maxpool3x3s2_f32); wo % 4 == 0."""
    require_hip(x, bias)
    _chk_f32(x, bias)
    B, C, H, W = x.shape
    assert H % 2 == 0 and W % 8 == 0 and bias.numel() == C
    out = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=torch.float32)
    _check(load().se_bias_relu_maxpool3x3s2_f32(_ptr(x), _ptr(bias), _ptr(out), B, C, H // 2, W // 2, _stream()), "se_bias_relu_maxpool3x3s2_f32")
    return out


_TILE_MEMO = {}


def _tile_memo(fn_name, *args) -> int:
    """The library's tile answers depend on the arguments and the current device's CU count only: one ctypes call per distinct question."""
    key = (fn_name, torch.cuda.current_device() if torch.cuda.is_available() else -1) + args
    t = _TILE_MEMO.get(key)
    if t is None:
        t = _TILE_MEMO[key] = int(getattr(load(), fn_name)(*args))
    return t


def conv2d_1x1_tile(batch, cin, cout, hw) -> int:
    """Channel-tile width the packed weights of a 1x1 convolution need (128 / 64), 0 when se_conv2d_1x1_f32 does not cover the shape."""
    return _tile_memo("se_conv2d_1x1_tile_f32", int(batch), int(cin), int(cout), int(hw))


def conv2d_1x1_pack(w2d, tile):
    """Folded [cout, cin] matrix -> [cout / tile, cin / 16, tile, 16] (the layout se_conv2d_1x1_f32 streams per (channel tile, k step))."""
    cout, cin = w2d.shape
    return w2d.reshape(cout // tile, tile, cin // 16, 16).permute(0, 2, 1, 3).contiguous()


def conv2d_1x1(x, wpack, bias, residual, relu, in_bias=None):
    """``x`` [B, cin, H, W] NCHW float32 -> relu?(W x' + bias (+ residual)) [B, cout, H, W] in one launch (se_conv2d_1x1_f32);
    ``in_bias`` [cin]: x' = relu(x + in_bias) (the producing convolution's bias + ReLU applied on the way in), else x' = x."""
    require_hip(x, wpack, bias)
    _chk_f32(x, wpack, bias, residual, in_bias)
    B, cin, H, W = x.shape
    cout = wpack.shape[0] * wpack.shape[2]
    assert wpack.dim() == 4 and wpack.shape[1] * 16 == cin and wpack.shape[2] == conv2d_1x1_tile(B, cin, cout, H * W)
    assert in_bias is None or in_bias.numel() == cin
    out = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
    _check(load().se_conv2d_1x1_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(residual), _ptr(in_bias), _ptr(out), B, cin, cout, H * W,
                                    1 if relu else 0, _stream()), "se_conv2d_1x1_f32")
    return out


def conv2d_1x1_small_ok(batch, cin, cout, hw) -> bool:
    """Shapes se_conv2d_1x1_small_f32 covers."""
    return cin % 64 == 0 and cout % 16 == 0 and hw % 16 == 0 and (batch * hw) % 64 == 0 and batch > 0


def conv2d_1x1_small(x, wpack16, bias, residual, relu, in_bias=None):
    """conv2d_1x1's result from the small-M kernel (se_conv2d_1x1_small_f32: 64 pixels x 16 channels per workgroup, k split over four / two
    wave groups); ``wpack16`` = ``conv2d_1x1_pack(w2d, 16)``."""
    require_hip(x, wpack16, bias)
    _chk_f32(x, wpack16, bias, residual, in_bias)
    B, cin, H, W = x.shape
    cout = wpack16.shape[0] * 16
    assert wpack16.dim() == 4 and wpack16.shape[1] * 16 == cin and wpack16.shape[2] == 16 and conv2d_1x1_small_ok(B, cin, cout, H * W)
    assert in_bias is None or in_bias.numel() == cin
    out = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
    _check(load().se_conv2d_1x1_small_f32(_ptr(x), _ptr(wpack16), _ptr(bias), _ptr(residual), _ptr(in_bias), _ptr(out), B, cin, cout, H * W,
                                          1 if relu else 0, _stream()), "se_conv2d_1x1_small_f32")
    return out


def conv2d_1x1_s2(x, wpack, bias, relu=False):
    """``x`` [B, cin, 2 ho, 2 wo] -> relu?(W x[:, :, ::2, ::2] + bias) [B, cout, ho, wo]: the stride-2 1x1 convolution (se_conv2d_1x1_s2_f32;
    ``wpack`` packed for ``conv2d_1x1_tile(B, cin, cout, ho * wo)``) - or, with a 16-channel packing, its small-M form
    (se_conv2d_1x1_small_s2_f32)."""
    require_hip(x, wpack, bias)
    _chk_f32(x, wpack, bias)
    B, cin, H, W = x.shape
    assert H % 2 == 0 and W % 2 == 0
    ho, wo = H // 2, W // 2
    cout = wpack.shape[0] * wpack.shape[2]
    out = torch.empty((B, cout, ho, wo), device=x.device, dtype=torch.float32)
    assert wpack.dim() == 4 and wpack.shape[1] * 16 == cin
    if wpack.shape[2] == 16:
        assert conv2d_1x1_small_ok(B, cin, cout, ho * wo)
        _check(load().se_conv2d_1x1_small_s2_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(out), B, cin, cout, ho, wo, 1 if relu else 0, _stream()),
               "se_conv2d_1x1_small_s2_f32")
        return out
    assert wpack.shape[2] == conv2d_1x1_tile(B, cin, cout, ho * wo)
    _check(load().se_conv2d_1x1_s2_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(out), B, cin, cout, ho, wo, 1 if relu else 0, _stream()),
           "se_conv2d_1x1_s2_f32")
    return out


def conv2d_3x3_tile(batch, cin, cout, h, w) -> int:
    """Channel-tile width the packed weights of a 3x3 stride-1 convolution need (32 / 16), 0 when se_conv2d_3x3_f32 does not cover the shape."""
    return _tile_memo("se_conv2d_3x3_tile_f32", int(batch), int(cin), int(cout), int(h), int(w))


def conv2d_3x3_pack(w4d, tile):
    """Folded [cout, cin, 3, 3] tensor -> [cout / tile, cin / 16, 9, tile, 16] (what se_conv2d_3x3_f32 streams per (channel tile, k step))."""
    cout, cin = w4d.shape[:2]
    return w4d.reshape(cout // tile, tile, cin // 16, 16, 9).permute(0, 2, 4, 1, 3).contiguous()


def conv2d_3x3(x, wpack, bias, relu):
    """``x`` [B, cin, H, W] NCHW float32 -> relu?(conv3x3(x) (+ bias)) [B, cout, H, W], stride 1, padding 1 (se_conv2d_3x3_f32);
    ``bias`` None: the raw sums (the consumer applies the bias - conv2d_1x1's ``in_bias``)."""
    require_hip(x, wpack)
    _chk_f32(x, wpack, bias)
    B, cin, H, W = x.shape
    cout = wpack.shape[0] * wpack.shape[3]
    assert wpack.dim() == 5 and wpack.shape[1] * 16 == cin and wpack.shape[2] == 9 and wpack.shape[3] == conv2d_3x3_tile(B, cin, cout, H, W)
    out = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
    _check(load().se_conv2d_3x3_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(out), B, cin, cout, H, W, 1 if relu else 0, _stream()),
           "se_conv2d_3x3_f32")
    return out


def conv2d_3x3_s2_ok(cin, cout, ho, wo) -> bool:
    """Shapes se_conv2d_3x3_s2_f32 covers (output map ho x wo)."""
    tile_ok = (ho % 4 == 0) if wo % 16 == 0 else (wo % 8 == 0 and ho % 8 == 0)
    return cin % 32 == 0 and cout % 16 == 0 and ho > 0 and wo > 0 and tile_ok and cin * ho * wo * 4 < (1 << 31) // 4


def conv2d_3x3_s2(x, wpack, bias, relu):
    """``x`` [B, cin, 2 ho, 2 wo] -> relu?(conv3x3 stride 2 padding 1 (x) (+ bias)) [B, cout, ho, wo] (se_conv2d_3x3_s2_f32); ``wpack`` =
    ``conv2d_3x3_pack(w, 16)``."""
    require_hip(x, wpack)
    _chk_f32(x, wpack, bias)
    B, cin, H, W = x.shape
    assert H % 2 == 0 and W % 2 == 0
    cout = wpack.shape[0] * wpack.shape[3]
    assert wpack.dim() == 5 and wpack.shape[1] * 16 == cin and wpack.shape[2] == 9 and wpack.shape[3] == 16
    out = torch.empty((B, cout, H // 2, W // 2), device=x.device, dtype=torch.float32)
    _check(load().se_conv2d_3x3_s2_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(out), B, cin, cout, H // 2, W // 2, 1 if relu else 0, _stream()),
           "se_conv2d_3x3_s2_f32")
    return out


def deconv2d_k4s2_assemble(z, bias, batch, cout, h, w, relu=True, split6=None):
    """``z`` [B,16,cout,h,w] (per-tap GEMM results of a ConvTranspose2d(4, 2, 1), tap = 4 ky + kx) -> relu?(y + bias) [B,cout,2h,2w].

    With ``split6`` (``deconv2d_k4s2_s6_pack`` of the layer's folded weight) the first argument is the layer's INPUT [B,cin,h,w] and one
    launch does product and assembly together (se_deconv2d_k4s2_s6_f32: six bf16 products per float32 product)."""
    require_hip(z, bias)
    if split6 is not None:
        return deconv2d_k4s2_s6(z, split6, bias, cout, relu=relu)
    _chk_f32(z, bias)
    assert z.is_contiguous() and z.numel() == batch * 16 * cout * h * w
    out = torch.empty((batch, cout, 2 * h, 2 * w), device=z.device, dtype=torch.float32)
    _check(load().se_deconv2d_k4s2_assemble_f32(_ptr(z), _ptr(bias), _ptr(out), batch, cout, h, w, 1 if relu else 0, _stream()),
           "se_deconv2d_k4s2_assemble_f32")
    return out


def deconv2d_k4s2_s6_ok(batch, cin, cout, h, w) -> bool:
    """Shapes se_deconv2d_k4s2_s6_f32 covers (cin % 32, cout % 64, w % 16, h % 8, 32-bit byte offsets into the input)."""
    return bool(load().se_deconv2d_k4s2_s6_domain(batch, cin, cout, h, w))


def deconv2d_k4s2_s6_pack(w):
    """Folded ConvTranspose2d(4, 2, 1) weight ``w`` [cin, cout, 4, 4] (float32, on the device) -> its three bf16 planes in the order
    se_deconv2d_k4s2_s6_f32 walks them, [cin / 32, cout / 16, 2, 8, 3, 64, 8]; None for a shape that has none."""
    require_hip(w)
    _chk_f32(w)
    cin, cout = int(w.shape[0]), int(w.shape[1])
    assert w.dim() == 4 and tuple(w.shape[2:]) == (4, 4)
    n = int(load().se_deconv2d_k4s2_s6_packed_elems(cin, cout))
    if n <= 0:
        return None
    out = torch.empty((cin // 32, cout // 16, 2, 8, 3, 64, 8), device=w.device, dtype=torch.bfloat16)
    assert out.numel() == n
    _check(load().se_deconv2d_k4s2_s6_pack(_ptr(w), _ptr(out), cin, cout, _stream()), "se_deconv2d_k4s2_s6_pack")
    return out


def deconv2d_k4s2_s6(x, wsplit, bias, cout, relu=True):
    """``x`` [B,cin,h,w] -> relu?(ConvTranspose2d(4, 2, 1)(x) + bias) [B,cout,2h,2w] in one launch; HipExtensionError (bad argument)
    outside the kernel's domain - the entry point checks, nothing is launched then."""
    require_hip(x, wsplit, bias)
    assert x.dim() == 4 and x.is_contiguous() and wsplit.dtype == torch.bfloat16 and wsplit.is_contiguous()
    _chk_f32(bias)
    B, cin, h, w = x.shape
    assert wsplit.numel() == (cin // 32) * (cout // 16) * 2 * 8 * 3 * 512 and bias.numel() == cout
    out = torch.empty((B, cout, 2 * h, 2 * w), device=x.device, dtype=torch.float32)
    _check(load().se_deconv2d_k4s2_s6_f32(_ptr(x), x.element_size(), _ptr(wsplit), _ptr(bias), _ptr(out), B, cin, cout, h, w,
                                          1 if relu else 0, _stream()), "se_deconv2d_k4s2_s6_f32")
    return out


def conv3d_packed_elems(cout, cin_pad, ksize, transposed, bf16=False) -> int:
    fn = load().se_conv3d_packed_elems_bf16 if bf16 else load().se_conv3d_packed_elems
    n = int(fn(cout, cin_pad, ksize, 1 if transposed else 0))
    if n <= 0:
        raise HipExtensionError(f"unsupported conv shape cout={cout} cin_pad={cin_pad} k={ksize}")
    return n


def conv3d_variant(batch, dim, cin, cout, ksize, flags=0) -> int:
    """The kernel a launch of ``batch`` samples with these layout flags (IN_OCTET / IN_QUAD ...) runs on: conv3d_algo()'s value, except
    3 = the F(4,3) x F(4,3) member of the 2-D Winograd family (same fused forms as 2; its planar layout is QUAD-planar: it takes a
    quad-planar input or a channels-last one with < 32 channels; any octet-planar flag keeps the launch on 2) and 0 for a 2-D Winograd
    shape with <= 4096 voxels in the batch (16^3 at batch 1) called without planar forms, which the in-workgroup split-K kernel serves
    better; the V2V program keeps such a level channels-last."""
    return int(load().se_conv3d_f32_variant(batch, dim, cin, cout, ksize, flags))


def conv3d_algo(dim, cin, cout, ksize) -> int:
    """Kernel family se_conv3d_f32 selects for this float32 shape (include/sceneego_hip.h: 0 direct, 1 / 2 Winograd 1-D / 2-D)."""
    return int(load().se_conv3d_f32_algo(dim, cin, cout, ksize))


def conv3d_pack(w, b, gamma, beta, mean, var, eps, wpack, bpack, cout, cin, cin_pad, ksize, transposed):
    """Fold BatchNorm into the convolution and write the packed weights and bias (float32 format: csrc/conv3d_pack.h, written by
    csrc/conv3d_pack.hip; bfloat16: csrc/conv3d_bf16.hip)."""
    require_hip(w, wpack, bpack)
    _chk_f32(w, b, gamma, beta, mean, var, bpack)
    if wpack.dtype == torch.bfloat16:
        _check(load().se_conv3d_pack_bf16(_ptr(w), _ptr(b), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), float(eps),
                                          _ptr(wpack), _ptr(bpack), cout, cin, cin_pad, ksize, 1 if transposed else 0,
                                          _stream()), "se_conv3d_pack_bf16")
        return
    _chk_f32(wpack)
    _check(load().se_conv3d_pack_f32(_ptr(w), _ptr(b), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), float(eps),
                                     _ptr(wpack), _ptr(bpack), cout, cin, cin_pad, ksize, 1 if transposed else 0,
                                     _stream()), "se_conv3d_pack_f32")


# Optional per-launch timing (bench.py's roofline leg): HIP events recorded on the launch stream around every
# conv launch, keyed by shape.  None = off (the default; nothing is recorded in normal operation).
_prof = None
last_launch_detail = []     # (key, flags or None, ms) of every launch of the last profiled pass, in issue order (bench.py: per-launch kernel variant)
last_launch_order = []      # launch keys of the last profiled pass, in issue order (tools/pmc_r03.py labels rocprofv3 dispatches with it)


def start_profile():
    global _prof
    _prof = []


def stop_profile():
    """-> {key: [ms, ...]} ; caller must have synchronised the device."""
    global _prof, last_launch_order, last_launch_detail
    rec, _prof = _prof, None
    out = {}
    detail = []
    for r in rec or []:
        key, e0, e1 = r[0], r[1], r[2]
        ms = e0.elapsed_time(e1)
        out.setdefault(key, []).append(ms)
        if key[0] != "stage":
            detail.append((key, r[3] if len(r) > 3 else None, ms))
    last_launch_order = [d[0] for d in detail]
    last_launch_detail = detail
    return out


class stage:
    """HIP events around one STAGE of the forward (backbone / gather / voxelise / v2v / softargmax) when profiling is on
    (bench.py's separate untimed pass); a no-op otherwise.  Keys are ("stage", name)."""

    def __init__(self, name):
        self.key = ("stage", name)

    def __enter__(self):
        if _prof is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _prof is not None and exc[0] is None:
            self.e1.record()
            _prof.append((self.key, self.e0, self.e1))
        return False


class _timed:
    """HIP events around one launch when profiling is on (bench.py); a no-op otherwise."""

    def __init__(self, key, flags=None):
        self.key = key
        self.flags = flags

    def __enter__(self):
        if _prof is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _prof is not None and exc[0] is None:
            self.e1.record()
            _prof.append((self.key, self.e0, self.e1, self.flags))
        return False


def _tag(t):
    return "" if t.dtype == torch.float32 else "_bf16"


def conv3d(inp, wpack, bpack, residual, out, batch, dim, cin, cin_pad, cout, ksize, flags, workspace=None, pool_out=None):
    """``pool_out`` (float32, 2-D Winograd 3x3x3 shapes only): channels-last [B, D/2, D/2, D/2, cout] tensor that also receives
    max_pool3d(out, 2, 2) from the kernel's epilogue (se_conv3d_pool_f32).
    ``workspace`` serves ONE stream at a time: the split-K levels (4^3, 2^3) and - when given - the chunk-half split of the 7^3 Winograd
    layer at batch 1 pass partial sums through it (a second stream needs its own: V2VProgram.workspace_side).  With a workspace the 7^3
    Winograd layer sums a frame in a different float32 order at batch 1 than at batch > 1; the frequency-domain front
    layer (conv3d_k7_fft, the production path since round 6) is batch-invariant bit for bit."""
    require_hip(inp, out)
    with _timed(("conv3d" + _tag(inp), ksize, cin_pad, cout, dim), flags):
        if inp.dtype == torch.bfloat16:
            assert wpack.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
            assert inp.shape[-1] == (8 if ksize == 7 else cin_pad)       # the 7^3 layer reads octet-planar input
            assert residual is None or residual.dtype == torch.bfloat16
            _check(load().se_conv3d_bf16(_ptr(inp), _ptr(wpack), _ptr(bpack), _ptr(residual), _ptr(out), batch, dim,
                                         cin_pad, cout, ksize, flags, _stream()), "se_conv3d_bf16")
        elif pool_out is not None:
            require_hip(pool_out)
            assert pool_out.dtype == torch.float32 and pool_out.numel() == batch * (dim // 2) ** 3 * cout and pool_out.is_contiguous()
            _check(load().se_conv3d_pool_f32(_ptr(inp), _ptr(wpack), _ptr(bpack), _ptr(residual), _ptr(out), _ptr(pool_out), batch,
                                             dim, cin, cin_pad, cout, ksize, flags, _ptr(workspace),
                                             0 if workspace is None else workspace.numel(), _stream()), "se_conv3d_pool_f32")
        elif getattr(wpack, "split6", None) is not None:
            # the layer has split planes (conv3d_split6_pack hangs them on its packed float32 tensor): the plan may choose a split form
            _check(load().se_conv3d_w6_f32(_ptr(inp), _ptr(wpack), _ptr(wpack.split6), _ptr(bpack), _ptr(residual), _ptr(out), batch, dim,
                                           cin, cin_pad, cout, ksize, flags, _ptr(workspace),
                                           0 if workspace is None else workspace.numel(), _stream()), "se_conv3d_w6_f32")
        else:
            _check(load().se_conv3d_f32(_ptr(inp), _ptr(wpack), _ptr(bpack), _ptr(residual), _ptr(out), batch, dim, cin,
                                        cin_pad, cout, ksize, flags, _ptr(workspace),
                                        0 if workspace is None else workspace.numel(), _stream()), "se_conv3d_f32")


def conv3d_k7_fft_supported(dim, cin, cout) -> bool:
    """Shapes the frequency-domain form of the 7x7x7 layer covers (se_conv3d_k7_fft_f32)."""
    return dim >= 16 and dim % 16 == 0 and int(load().se_conv3d_k7_fft_packed_elems(cin, cout)) > 0


def conv3d_k7_fft_pack(w, gamma, var, eps, cout, cin):
    """Conv3d weight [cout][cin][7][7][7] (+ the BatchNorm3d scale) -> its spectra in MFMA fragment order (se_conv3d_k7_fft_pack_f32)."""
    require_hip(w)
    _chk_f32(w, gamma, var)
    n = int(load().se_conv3d_k7_fft_packed_elems(cin, cout))
    if n <= 0:
        raise HipExtensionError(f"frequency-domain 7x7x7 convolution does not cover cin={cin} cout={cout}")
    out = torch.empty(n, device=w.device, dtype=torch.float32)
    _check(load().se_conv3d_k7_fft_pack_f32(_ptr(w), _ptr(gamma), _ptr(var), float(eps), _ptr(out), cout, cin, _stream()),
           "se_conv3d_k7_fft_pack_f32")
    return out


def conv3d_k7_fft_workspace_elems(batch, dim, cin) -> int:
    return int(load().se_conv3d_k7_fft_workspace_elems(batch, dim, cin))


def conv3d_k7_fft(inp, hfrag, bpack, out, batch, dim, cin, cout, flags, workspace):
    """``inp`` planar [B, cin, D, D, D]; ``out`` channels-last [B, D, D, D, 16] or (OUT_QUAD) quad-planar [B, 4, D, D, D, 4];
    ``workspace``: float32 scratch for the spectra of >= 1 sample (conv3d_k7_fft_workspace_elems); one stream at a time."""
    require_hip(inp, hfrag, bpack, out, workspace)
    _chk_f32(inp, hfrag, bpack, out, workspace)
    assert inp.numel() == batch * cin * dim ** 3 and out.numel() == batch * cout * dim ** 3
    with _timed(("conv3d_fft", 7, cin, cout, dim), flags):
        _check(load().se_conv3d_k7_fft_f32(_ptr(inp), _ptr(hfrag), _ptr(bpack), _ptr(out), batch, dim, cin, cout, flags,
                                           _ptr(workspace), workspace.numel(), _stream()), "se_conv3d_k7_fft_f32")


def conv3d_split3_pack(w_folded, cout, cin, cin_pad):
    """EXPERIMENTAL: float32 [cout][cin][3][3][3] weights (BatchNorm scale folded in) -> the split-bf16 kernel's packed (hi, lo) halves."""
    require_hip(w_folded)
    _chk_f32(w_folded)
    n = int(load().se_conv3d_split3_packed_elems(cout, cin_pad))
    if n <= 0:
        raise HipExtensionError(f"split-bf16 convolution does not cover cout={cout} cin_pad={cin_pad}")
    out = torch.empty(n, device=w_folded.device, dtype=torch.bfloat16)
    _check(load().se_conv3d_split3_pack(_ptr(w_folded), _ptr(out), cout, cin, cin_pad, _stream()), "se_conv3d_split3_pack")
    return out


def conv3d_k3_split3(inp, wsplit, bpack, residual, out, batch, dim, cin_pad, cout, flags):
    """EXPERIMENTAL: 3x3x3 convolution on float32 tensors (channels-last, or octet-planar per IN_/OUT_/RES_OCTET) with split-bf16
    arithmetic (se_conv3d_k3_split3_f32)."""
    require_hip(inp, out, wsplit, bpack)
    _chk_f32(inp, out, bpack, residual)
    assert wsplit.dtype == torch.bfloat16
    with _timed(("conv3d_split3", 3, cin_pad, cout, dim)):
        _check(load().se_conv3d_k3_split3_f32(_ptr(inp), _ptr(wsplit), _ptr(bpack), _ptr(residual), _ptr(out), batch, dim, cin_pad, cout,
                                              flags, _stream()), "se_conv3d_k3_split3_f32")


def conv3d_split6_pack(wpack, cout, cin_pad, ksize, transposed=False):
    """The split planes of a layer (csrc/split6.h: every folded float32 weight as three bf16 parts, A-fragment order) from its packed
    float32 buffer ``wpack``, or None for a shape that has none (cin_pad % 32 != 0).  The planes are also hung on ``wpack`` as
    ``wpack.split6``: conv3d() then lets the library's plan choose a six-product form for the launches of that layer."""
    require_hip(wpack)
    _chk_f32(wpack)
    n = int(load().se_conv3d_split6_packed_elems(cout, cin_pad, ksize, 1 if transposed else 0))
    if n <= 0:
        return None
    out = torch.empty(n, device=wpack.device, dtype=torch.bfloat16)
    _check(load().se_conv3d_split6_pack(_ptr(wpack), _ptr(out), cout, cin_pad, ksize, 1 if transposed else 0, _stream()),
           "se_conv3d_split6_pack")
    wpack.split6 = out
    return out


def conv3d_split6(batch, dim, cin, cout, ksize, flags=0) -> bool:
    """True when conv3d() runs this float32 launch (cin_pad == cin) of a layer with split planes on a six-product bf16 form."""
    return bool(load().se_conv3d_f32_split6(batch, dim, cin, cout, ksize, flags))


def conv3d_k3_split6(inp, wsplit6, bpack, residual, out, batch, dim, cin, cin_pad, cout, flags):
    """The split form of the 3x3x3 kernel of the 8^3-sized levels on its whole domain (se_conv3d_k3_split6_f32), channels-last."""
    require_hip(inp, out, wsplit6, bpack)
    _chk_f32(inp, out, bpack, residual)
    assert wsplit6.dtype == torch.bfloat16 and inp.numel() == batch * dim ** 3 * cin_pad and out.numel() == batch * dim ** 3 * cout
    assert wsplit6.numel() == int(load().se_conv3d_split6_packed_elems(cout, cin_pad, 3, 0))
    assert residual is None or residual.numel() == out.numel()
    with _timed(("conv3d_split6", 3, cin_pad, cout, dim), flags):
        _check(load().se_conv3d_k3_split6_f32(_ptr(inp), _ptr(wsplit6), _ptr(bpack), _ptr(residual), _ptr(out), batch, dim, cin, cin_pad,
                                              cout, flags, _stream()), "se_conv3d_k3_split6_f32")


def split6_planes(x):
    """Test entry point: the device's 3-way bf16 split of a float32 tensor (even element count) -> planes [3, n] bfloat16."""
    require_hip(x)
    _chk_f32(x)
    planes = torch.empty((3, x.numel()), device=x.device, dtype=torch.bfloat16)
    _check(load().se_split6_planes_f32(_ptr(x), _ptr(planes), x.numel(), _stream()), "se_split6_planes_f32")
    return planes


def conv3d_skip16(inp, wpack, bpack_sum, skip_in, skip_w, out, batch, dim, cin, cout, flags):
    """3x3x3 convolution (2-D Winograd kernels, planar in / out) + the block's 1x1x1 skip convolution over the 16-channel ``skip_in``
    (channels-last, or quad-planar with RES_QUAD on the quad family) in one launch (se_conv3d_skip16_f32); ``bpack_sum`` = sum of both
    folded biases."""
    require_hip(inp, out, skip_in, skip_w, bpack_sum)
    _chk_f32(inp, out, skip_in, skip_w, bpack_sum)
    # skip_in: channels-last [B, D, D, D, 16], or with RES_QUAD quad-planar [B, 4, D, D, D, 4]
    assert skip_in.numel() == batch * dim ** 3 * 16
    assert tuple(skip_w.shape) == (cout, 16) and skip_w.is_contiguous() and skip_in.is_contiguous()
    with _timed(("conv3d", 3, cin, cout, dim), flags | 256):        # 256 = SE_EPI_SKIPCONV16 (the entry point sets it)
        _check(load().se_conv3d_skip16_f32(_ptr(inp), _ptr(wpack), _ptr(bpack_sum), _ptr(skip_in), _ptr(skip_w), _ptr(out), batch,
                                           dim, cin, cout, flags, _stream()), "se_conv3d_skip16_f32")


def pointwise_chain3(inp, pc1, pc2, pc3, out, batch, dim, softargmax=None, in_quad=False):
    """back_layers.1 -> back_layers.2 -> output_layer in one launch; pc* are packed 1x1x1 convs (32->32, 32->32, 32->J).
    ``softargmax`` = (coord [dim^3, 3], scratch): float32 only - the launch also writes pass 1 of the soft-argmax (softmax mode) into
    ``scratch``; finish with softargmax3d_finish.  ``in_quad`` (that form only): ``inp`` is quad-planar [B][8][dim^3][4]."""
    require_hip(inp, out)
    assert out.dtype == torch.float32
    assert not in_quad or softargmax is not None
    if softargmax is not None:
        coord, scratch = softargmax
        require_hip(coord, scratch)
        _chk_f32(coord, scratch)
        assert scratch.numel() >= softargmax3d_scratch_elems(batch * pc3.cout) and coord.numel() == 3 * dim ** 3
        if inp.dtype == torch.bfloat16:
            assert not in_quad
            with _timed(("tail_bf16", 1, 32, pc3.cout, dim)):
                _check(load().se_pointwise_chain3_softargmax_bf16(_ptr(inp), _ptr(pc1.w), _ptr(pc1.b), _ptr(pc2.w), _ptr(pc2.b), _ptr(pc3.w),
                                                                  _ptr(pc3.b), _ptr(out), _ptr(coord), _ptr(scratch), batch, dim, pc3.cout,
                                                                  _stream()), "se_pointwise_chain3_softargmax_bf16")
            return
        _chk_f32(inp)
        with _timed(("tail", 1, 32, pc3.cout, dim)):
            _check(load().se_pointwise_chain3_softargmax_f32(_ptr(inp), _ptr(pc1.w), _ptr(pc1.b), _ptr(pc2.w), _ptr(pc2.b), _ptr(pc3.w),
                                                             _ptr(pc3.b), _ptr(out), _ptr(coord), _ptr(scratch), batch, dim, pc3.cout,
                                                             IN_QUAD if in_quad else 0, _stream()), "se_pointwise_chain3_softargmax_f32")
        return
    fn = load().se_pointwise_chain3_bf16 if inp.dtype == torch.bfloat16 else load().se_pointwise_chain3_f32
    with _timed(("tail" + _tag(inp), 1, 32, pc3.cout, dim)):
        _check(fn(_ptr(inp), _ptr(pc1.w), _ptr(pc1.b), _ptr(pc2.w), _ptr(pc2.b), _ptr(pc3.w),
                  _ptr(pc3.b), _ptr(out), batch, dim, pc3.cout, _stream()), "se_pointwise_chain3")


def deconv3d_k2s2(inp, wpack, bpack, residual, out, batch, dim, cin, cout, flags):
    """``flags`` may carry OUT_QUAD (float32, 64 -> 32 and 128 -> 64, dim % 16 == 0): ``out`` is then quad-planar [B][cout/4][2D][2D][2D][4]."""
    require_hip(inp, out)
    fn = load().se_deconv3d_k2s2_bf16 if inp.dtype == torch.bfloat16 else load().se_deconv3d_k2s2_f32
    assert out.dtype == inp.dtype and wpack.dtype == inp.dtype and (residual is None or residual.dtype == inp.dtype)
    with _timed(("deconv" + _tag(inp), 2, cin, cout, dim)):
        _check(fn(_ptr(inp), _ptr(wpack), _ptr(bpack), _ptr(residual), _ptr(out), batch, dim,
                  cin, cout, flags, _stream()), "se_deconv3d_k2s2")


def maxpool3d_2(inp, out, batch, dim, channels, in_octet=False):
    require_hip(inp, out)
    fn = load().se_maxpool3d_2_bf16 if inp.dtype == torch.bfloat16 else load().se_maxpool3d_2_f32
    if in_octet:
        assert inp.dtype == torch.float32
        fn = load().se_maxpool3d_2_octin_f32
    assert out.dtype == inp.dtype
    with _timed(("maxpool" + _tag(inp), 2, channels, channels, dim)):
        _check(fn(_ptr(inp), _ptr(out), batch, dim, channels, _stream()), "se_maxpool3d_2")


def softargmax3d_scratch_elems(rows) -> int:
    return int(load().se_softargmax3d_scratch_elems(rows))


def softargmax3d_finish(vol, scratch, out_vol, joints, rows, voxels, mode):
    """Pass 2 of the soft-argmax from partial records written by pointwise_chain3(..., softargmax=...)."""
    require_hip(vol, scratch, out_vol, joints)
    _chk_f32(vol, scratch, out_vol, joints)
    _check(load().se_softargmax3d_finish_f32(_ptr(vol), _ptr(scratch), _ptr(out_vol), _ptr(joints), rows, voxels, mode, _stream()),
           "se_softargmax3d_finish_f32")


def softargmax3d(vol, coord, out_vol, joints, rows, voxels, mode, scratch=None):
    require_hip(vol, coord, out_vol, joints)
    _chk_f32(vol, coord, out_vol, joints)
    if scratch is None:
        scratch = torch.empty(softargmax3d_scratch_elems(rows), device=vol.device, dtype=torch.float32)
    _check(load().se_softargmax3d_f32(_ptr(vol), _ptr(coord), _ptr(out_vol), _ptr(joints), _ptr(scratch), rows,
                                      voxels, mode, _stream()), "se_softargmax3d_f32")


def joint_stats_scratch_elems(rows) -> int:
    return int(load().se_joint_stats_scratch_elems(rows))


JOINT_STATS_SLOTS = 12     # cxx cyy czz cxy cxz cyz entropy peak_p peak_x peak_y peak_z sigma (include/sceneego_hip.h)


def joint_stats(prob, coord, joints, stats, peak_index, rows, voxels, scratch=None):
    """se_joint_stats_f32: per-row covariance about ``joints``, entropy and peak of the softmaxed volumes ``prob`` [rows, voxels]
    into ``stats`` [rows, 12] float32 and ``peak_index`` [rows] int32.  Every argument is checked here and a bad one raises
    HipExtensionError before anything is launched: the kernel reads with 16-byte loads and trusts the sizes it is given."""
    what = "joint_stats"
    if rows <= 0 or voxels <= 0 or voxels % 4:
        raise HipExtensionError(f"{what}: rows = {rows}, voxels = {voxels}: both must be positive and voxels a multiple of 4")
    dev = _check_args(what, (("prob", prob, torch.float32, rows * voxels), ("coord", coord, torch.float32, voxels * 3),
                             ("joints", joints, torch.float32, rows * 3), ("stats", stats, torch.float32, rows * JOINT_STATS_SLOTS),
                             ("peak_index", peak_index, torch.int32, rows)), (("scratch", scratch, torch.float32, None),))
    scratch = _scratch(what, scratch, joint_stats_scratch_elems(rows), torch.float32, dev)
    _check(load().se_joint_stats_f32(_ptr(prob), _ptr(coord), _ptr(joints), _ptr(stats), _ptr(peak_index), _ptr(scratch), rows,
                                     voxels, _stream()), "se_joint_stats_f32")


# ---------------------------------------------------------------------------------------------
# Headless renderer (csrc/render.hip; sceneego_amd/render.py drives it)
RENDER_JOINTS = 15
RENDER_R_JOINT, RENDER_R_BONE = 0.03, 0.0075                       # metres
RENDER_JOINT_RGB, RENDER_BONE_RGB = (0.1, 0.1, 0.7), (0.1, 0.9, 0.1)  # reference utils/skeleton.py:52


def render_splat(depth, ray_tab, image, view, zbuf, f, cx, cy, splat=2, min_z=0.1, max_depth=100.0, near=0.05):
    """se_render_splat_f64: depth [B,dh,dw] float32, ray_tab [H,W,3] float64, image [B,H,W,3] uint8 (B, G, R), view [12] float64 ->
    zbuf [B,Hout,Wout] int64 (the uint64 keys; cleared inside).  Shapes and devices are checked here, before anything is launched."""
    what = "render_splat"
    _check_args(what, (("depth", depth, torch.float32, (None, None, None)), ("ray_tab", ray_tab, torch.float64, (None, None, 3)),
                       ("zbuf", zbuf, torch.int64, (None, None, None))))
    B, dh, dw = depth.shape
    H, W, _ = ray_tab.shape
    _check_args(what, (("image", image, torch.uint8, (B, H, W, 3)), ("view", view, torch.float64, (12,)),
                       ("zbuf", zbuf, torch.int64, (B, None, None))), device=depth.device)
    _check(load().se_render_splat_f64(_ptr(depth), _ptr(ray_tab), _ptr(image), _ptr(view), _ptr(zbuf), B, dh, dw, H, W, zbuf.shape[1],
                                      zbuf.shape[2], float(f), float(cx), float(cy), int(splat), float(min_z), float(max_depth),
                                      float(near), _stream()), "se_render_splat_f64")
    return zbuf


def _rgb3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def render_resolve(rays, joints, zbuf, out, r_joint=RENDER_R_JOINT, r_bone=RENDER_R_BONE, near=0.05, joint_rgb=RENDER_JOINT_RGB,
                   bone_rgb=RENDER_BONE_RGB, background=(255, 255, 255)):
    """se_render_resolve_f64: rays [Hout,Wout,3] float64, joints [B,15,3] float64 (frame of the rays), zbuf [B,Hout,Wout] int64 ->
    out [B,Hout,Wout,3] uint8 (R, G, B)."""
    what = "render_resolve"
    _check_args(what, (("zbuf", zbuf, torch.int64, (None, None, None)),))
    B, Ho, Wo = zbuf.shape
    _check_args(what, (("rays", rays, torch.float64, (Ho, Wo, 3)), ("joints", joints, torch.float64, (B, RENDER_JOINTS, 3)),
                       ("out", out, torch.uint8, (B, Ho, Wo, 3))), device=zbuf.device)
    bg = (ctypes.c_ubyte * 3)(*[int(x) for x in background])
    _check(load().se_render_resolve_f64(_ptr(rays), _ptr(joints), _ptr(zbuf), _ptr(out), B, Ho, Wo, float(r_joint), float(r_bone),
                                        float(near), _rgb3(joint_rgb), _rgb3(bone_rgb), bg, _stream()), "se_render_resolve_f64")
    return out


def render_overlay(rays, joints, frame, out, depth=None, r_joint=RENDER_R_JOINT, r_bone=RENDER_R_BONE, near=0.05,
                   joint_rgb=RENDER_JOINT_RGB, bone_rgb=RENDER_BONE_RGB):
    """se_render_overlay_f64: rays [H,W,3] float64 (the camera's unit rays), joints [B,15,3] float64 (camera frame), frame [B,H,W,3]
    uint8 (B, G, R), depth None or [B,dh,dw] float32 -> out [B,H,W,3] uint8 (R, G, B)."""
    what = "render_overlay"
    _check_args(what, (("frame", frame, torch.uint8, (None, None, None, 3)),))
    B, H, W, _ = frame.shape
    _check_args(what, (("rays", rays, torch.float64, (H, W, 3)), ("joints", joints, torch.float64, (B, RENDER_JOINTS, 3)),
                       ("out", out, torch.uint8, (B, H, W, 3))), (("depth", depth, torch.float32, (B, None, None)),), device=frame.device)
    dh, dw = depth.shape[1:] if depth is not None else (0, 0)
    _check(load().se_render_overlay_f64(_ptr(rays), _ptr(joints), _ptr(frame), _ptr(depth), _ptr(out), B, H, W, dh, dw, float(r_joint),
                                        float(r_bone), float(near), _rgb3(joint_rgb), _rgb3(bone_rgb), _stream()),
           "se_render_overlay_f64")
    return out


# Volume renderer (csrc/render_volume.hip; SceneRenderer.render_volumes / overlay_volumes drive it)
RENDER_VOLUME_SLOTS = 16           # floats per cell of the packed copy: 15 joints and a zero
RENDER_VOLUME_ALL = (1 << RENDER_JOINTS) - 1


def render_volume_palette():
    """The 15 per-joint colours (R, G, B) of include/sceneego_hip.h, read from the library (host only: no device needed)."""
    buf = (ctypes.c_ubyte * (3 * RENDER_JOINTS))()
    load().se_render_volume_palette(ctypes.cast(buf, ctypes.c_void_p))
    return tuple(tuple(int(buf[3 * j + k]) for k in range(3)) for j in range(RENDER_JOINTS))


def render_volume_packed_elems(batch, grid):
    """float32 elements of the packed copy of ``batch`` frames of ``grid``^3 cells."""
    n = int(load().se_render_volume_packed_bytes(int(batch), int(grid)))
    if n < 0:
        raise HipExtensionError(f"render_volume: batch = {batch}, grid = {grid}: batch must be 1..65535 and grid 2..1024")
    return n // 4


def render_volume_pack(volumes, packed):
    """se_render_volume_pack_f32: volumes [B,15,G,G,G] float32 -> packed, float32 with at least B * G^3 * 16 elements."""
    what = "render_volume_pack"
    _check_args(what, (("volumes", volumes, torch.float32, (None, RENDER_JOINTS, None, None, None)),))
    B, G = volumes.shape[0], volumes.shape[2]
    if not volumes.shape[2] == volumes.shape[3] == volumes.shape[4]:
        raise HipExtensionError(f"{what}: volumes [B,15,G,G,G] expected, got {tuple(volumes.shape)}")
    _render_packed(what, packed, B, G, volumes.device)
    _check(load().se_render_volume_pack_f32(_ptr(volumes), _ptr(packed), packed.numel() * 4, B, G, _stream()), "se_render_volume_pack_f32")
    return packed


def _render_packed(what, packed, B, grid, device):
    """``packed`` is the float32 buffer render_volume_pack fills: at least render_volume_packed_elems(B, grid) elements."""
    need = render_volume_packed_elems(B, grid)
    _check_args(what, (("packed", packed, torch.float32, None),), device=device)
    if packed.numel() < need:
        raise HipExtensionError(f"{what}: packed has {packed.numel()} elements, needs at least {need}")


def render_volume_view(packed, scale, rays, view, zbuf, out, grid, cuboid_side, base=None, near=0.05, joint_mask=RENDER_VOLUME_ALL,
                       gain=1.0, opacity=0.8):
    """se_render_volume_view_f64: packed (render_volume_pack), scale [B,15] float64, rays [Hout,Wout,3] float64 (pinhole table), view
    12 floats on the host, zbuf None (no occlusion) or [B,Hout,Wout] int64 -> out [B,Hout,Wout,3] uint8 (R, G, B), drawn over
    ``base`` (default: over ``out`` itself, in place)."""
    base = out if base is None else base
    what = "render_volume_view"
    _check_args(what, (("out", out, torch.uint8, (None, None, None, 3)),))
    B, Ho, Wo, _ = out.shape
    _render_packed(what, packed, B, grid, out.device)
    _check_args(what, (("scale", scale, torch.float64, (B, RENDER_JOINTS)), ("rays", rays, torch.float64, (Ho, Wo, 3)),
                       ("base", base, torch.uint8, (B, Ho, Wo, 3))), (("zbuf", zbuf, torch.int64, (B, Ho, Wo)),), device=out.device)
    v = (ctypes.c_double * 12)(*[float(x) for x in view])
    _check(load().se_render_volume_view_f64(_ptr(packed), _ptr(scale), _ptr(rays), ctypes.cast(v, ctypes.c_void_p), _ptr(zbuf),
                                            _ptr(base), _ptr(out), B, Ho, Wo, int(grid), float(cuboid_side), float(near),
                                            int(joint_mask), float(gain), float(opacity), _stream()), "se_render_volume_view_f64")
    return out


def render_volume_overlay(packed, scale, rays, out, grid, cuboid_side, base=None, depth=None, near=0.05,
                          joint_mask=RENDER_VOLUME_ALL, gain=1.0, opacity=0.8):
    """se_render_volume_overlay_f64: packed, scale [B,15] float64, rays [H,W,3] float64 (the camera's unit rays), depth None (no
    occlusion) or [B,dh,dw] float32 -> out [B,H,W,3] uint8 (R, G, B), drawn over ``base`` (default: ``out`` itself, in place)."""
    base = out if base is None else base
    what = "render_volume_overlay"
    _check_args(what, (("out", out, torch.uint8, (None, None, None, 3)),))
    B, H, W, _ = out.shape
    _render_packed(what, packed, B, grid, out.device)
    _check_args(what, (("scale", scale, torch.float64, (B, RENDER_JOINTS)), ("rays", rays, torch.float64, (H, W, 3)),
                       ("base", base, torch.uint8, (B, H, W, 3))), (("depth", depth, torch.float32, (B, None, None)),), device=out.device)
    dh, dw = depth.shape[1:] if depth is not None else (0, 0)
    _check(load().se_render_volume_overlay_f64(_ptr(packed), _ptr(scale), _ptr(rays), _ptr(depth), _ptr(base), _ptr(out), B, H, W, dh, dw,
                                               int(grid), float(cuboid_side), float(near), int(joint_mask), float(gain), float(opacity),
                                               _stream()), "se_render_volume_overlay_f64")
    return out


# Scene probe (csrc/scene_probe.hip; sceneego_amd/scene_check.py drives it)
SCENE_PROBE_MAX = 64
SCENE_PROBE_SLOTS = 8      # nearest_q, nearest point x y z, c.c, sight_dot, surface, 0 (include/sceneego_hip.h)
# Skeleton.lines of the reference (utils/skeleton.py:20-21), the table csrc/render.hip holds as c_bones
SKELETON_LINES = ((0, 1), (0, 4), (1, 2), (2, 3), (4, 5), (5, 6), (1, 7), (4, 11), (7, 8), (8, 9), (9, 10), (11, 12), (12, 13), (13, 14),
                  (7, 11))
# Skeleton.kinematic_parents of the reference (utils/skeleton.py): the tree csrc/skeleton_prior.hip couples the joints over.  Its
# fourteen edges are the first fourteen SKELETON_LINES; the fifteenth, hip to hip (7, 11), closes a loop and is not part of the tree.
KINEMATIC_PARENTS = (0, 0, 1, 2, 0, 4, 5, 1, 7, 8, 9, 4, 11, 12, 13)


def scene_probe_scratch_bytes(batch, height, width, probes) -> int:
    n = int(load().se_scene_probe_scratch_bytes(int(batch), int(height), int(width), int(probes)))
    if n < 0:
        raise HipExtensionError(f"scene_probe: no launch for batch {batch}, {height}x{width} rays, {probes} probes")
    return n


def scene_probe(depth, ray_tab, probes, out, index, scratch=None, min_z=0.1, max_depth=100.0):
    """se_scene_probe_f64: depth [B,dh,dw] float32, ray_tab [H,W,3] float64, probes [B,P,3] float64 (1 <= P <= 64) -> out [B,P,8]
    float64, index [B,P,2] int32 (the header states every slot).  ``scratch``: an optional uint8 workspace of at least
    ``scene_probe_scratch_bytes(B, H, W, P)`` bytes (allocated per call otherwise).  Returns (out, index)."""
    what = "scene_probe"
    _check_args(what, (("depth", depth, torch.float32, (None, None, None)), ("ray_tab", ray_tab, torch.float64, (None, None, 3)),
                       ("probes", probes, torch.float64, (None, None, 3))))
    B, dh, dw = depth.shape
    H, W = ray_tab.shape[:2]
    P = probes.shape[1]
    if not 1 <= P <= SCENE_PROBE_MAX:
        raise HipExtensionError(f"{what}: {P} probes per frame, 1..{SCENE_PROBE_MAX} supported")
    _check_args(what, (("probes", probes, torch.float64, (B, P, 3)), ("out", out, torch.float64, (B, P, SCENE_PROBE_SLOTS)),
                       ("index", index, torch.int32, (B, P, 2))), (("scratch", scratch, torch.uint8, None),), device=depth.device)
    scratch = _scratch(what, scratch, scene_probe_scratch_bytes(B, H, W, P), torch.uint8, depth.device)
    _check(load().se_scene_probe_f64(_ptr(depth), _ptr(ray_tab), _ptr(probes), _ptr(out), _ptr(index), _ptr(scratch), scratch.numel(),
                                     B, dh, dw, H, W, P, float(min_z), float(max_depth), _stream()), "se_scene_probe_f64")
    return out, index


# ----------------------------------------------------------------------------------------------------------------------------------
# Scene-constrained joints (csrc/scene_constraint.hip; sceneego_amd/op.py and VoxelNetwork_depth.constrain_to_scene drive them)
MASKED_SLOTS = 8           # free_mass, sum f p c (x y z), free_peak_p, free peak coordinate x y z (include/sceneego_hip.h)


def scene_free_mask(depth, pix, rng, free, height, width, margin, max_depth):
    """se_scene_free_mask_u8: depth [B,dh,dw] float32, the sight table pix [voxels] int32 / rng [voxels] float32 of a ``height`` x
    ``width`` frame -> free [B,voxels] uint8 (1 free, 0 blocked; the header states the rule).  Every argument is checked here and a
    bad one raises HipExtensionError before anything is launched.  Returns ``free``."""
    what = "scene_free_mask"
    _check_args(what, (("depth", depth, torch.float32, (None, None, None)), ("pix", pix, torch.int32, (None,))))
    B, dh, dw = (int(v) for v in depth.shape)
    voxels = int(pix.numel())
    height, width = int(height), int(width)
    _check_args(what, (("rng", rng, torch.float32, voxels), ("free", free, torch.uint8, B * voxels)), device=depth.device)
    if B <= 0 or B > 65535 or dh <= 0 or dw <= 0 or height <= 0 or width <= 0 or height * width > 0x7fff0000:
        raise HipExtensionError(f"{what}: batch {B}, depth {dh}x{dw}, frame {height}x{width} not supported")
    if voxels <= 0 or voxels % 4:
        raise HipExtensionError(f"{what}: voxels = {voxels} must be a positive multiple of 4")
    margin, max_depth = float(margin), float(max_depth)
    if margin != margin or not max_depth > 0.0:
        raise HipExtensionError(f"{what}: margin {margin} must not be NaN and max_depth {max_depth} must be positive")
    _check(load().se_scene_free_mask_u8(_ptr(depth), _ptr(pix), _ptr(rng), _ptr(free), B, dh, dw, height, width, voxels, margin,
                                        max_depth, _stream()), "se_scene_free_mask_u8")
    return free


def softargmax3d_masked_scratch_elems(rows) -> int:
    return int(load().se_softargmax3d_masked_scratch_elems(int(rows)))


def softargmax3d_masked(prob, coord, free, out, peak_index, rows, rows_per_frame, voxels, scratch=None):
    """se_softargmax3d_masked_f32: the soft-argmax sums and the peak of ``prob`` [rows, voxels] over the voxels that ``free``
    [rows / rows_per_frame, voxels] uint8 marks free, into ``out`` [rows, 8] float32 and ``peak_index`` [rows] int32.  Every argument
    is checked here and a bad one raises HipExtensionError before anything is launched: the kernel reads with 16-byte loads and trusts
    the sizes it is given."""
    what = "softargmax3d_masked"
    rows, rows_per_frame, voxels = int(rows), int(rows_per_frame), int(voxels)
    if rows <= 0 or rows > 65535 or rows_per_frame <= 0 or rows % rows_per_frame or voxels <= 0 or voxels % 4:
        raise HipExtensionError(f"{what}: rows = {rows} (1..65535, a multiple of rows_per_frame = {rows_per_frame}), voxels = {voxels} "
                                "(a positive multiple of 4) expected")
    dev = _check_args(what, (("prob", prob, torch.float32, rows * voxels), ("coord", coord, torch.float32, voxels * 3),
                             ("free", free, torch.uint8, rows // rows_per_frame * voxels),
                             ("out", out, torch.float32, rows * MASKED_SLOTS), ("peak_index", peak_index, torch.int32, rows)),
                      (("scratch", scratch, torch.float32, None),))
    scratch = _scratch(what, scratch, softargmax3d_masked_scratch_elems(rows), torch.float32, dev)
    _check(load().se_softargmax3d_masked_f32(_ptr(prob), _ptr(coord), _ptr(free), _ptr(out), _ptr(peak_index), _ptr(scratch), rows,
                                             rows_per_frame, voxels, _stream()), "se_softargmax3d_masked_f32")
    return out, peak_index


# ----------------------------------------------------------------------------------------------------------------------------------
# Scene distance field (csrc/scene_field.hip; sceneego_amd/scene_field.py, op.py and VoxelNetwork_depth.scene_expectations drive them)
EXPECT_SLOTS = 24          # mass, blocked, sum p sqrt(d2), the same over free voxels, 8 contact sums, 8 free contact sums, 4 zeros
EXPECT_MAX_RADII = 8
SCENE_NO_SITE = 0x7fffffff  # d2 of a voxel in a frame without a site (nearest = -1 there)
SCENE_DISTANCE_MAX_GRID = 128


def scene_sites(depth, ray_tab, sites, grid, side, min_z=0.1, max_depth=100.0):
    """se_scene_sites_u8: depth [B,dh,dw] float32, ray_tab [H,W,3] float64 -> sites uint8 with B * grid^3 elements (cleared inside),
    1 where a scene point of the frame rounds to the voxel (the header states the rule).  Every argument is checked here and a bad
    one raises HipExtensionError before anything is launched.  Returns ``sites``."""
    what = "scene_sites"
    _check_args(what, (("depth", depth, torch.float32, (None, None, None)), ("ray_tab", ray_tab, torch.float64, (None, None, 3))))
    B, dh, dw = (int(v) for v in depth.shape)
    H, W = int(ray_tab.shape[0]), int(ray_tab.shape[1])
    grid, side, min_z, max_depth = int(grid), float(side), float(min_z), float(max_depth)
    if B <= 0 or B > 65535 or dh <= 0 or dw <= 0 or H <= 0 or W <= 0 or H * W > 0x7fff0000 or not 2 <= grid <= 1024:
        raise HipExtensionError(f"{what}: batch {B}, depth {dh}x{dw}, frame {H}x{W}, grid {grid} not supported")
    if not (0.0 < side < float("inf")) or not min_z >= 0.0 or not max_depth > 0.0:
        raise HipExtensionError(f"{what}: side {side} must be positive and finite, min_z {min_z} >= 0 and max_depth {max_depth} > 0")
    _check_args(what, (("sites", sites, torch.uint8, B * grid ** 3),), device=depth.device)
    _check(load().se_scene_sites_u8(_ptr(depth), _ptr(ray_tab), _ptr(sites), B, dh, dw, H, W, grid, side, min_z, max_depth, _stream()),
           "se_scene_sites_u8")
    return sites


def scene_distance_scratch_bytes(batch, grid) -> int:
    n = int(load().se_scene_distance_scratch_bytes(int(batch), int(grid)))
    if n < 0:
        raise HipExtensionError(f"scene_distance: batch = {batch} (1..65535), grid = {grid} (2..{SCENE_DISTANCE_MAX_GRID}) not supported")
    return n


def scene_distance(sites, d2, nearest, batch, grid, scratch=None):
    """se_scene_distance_i32: sites uint8 [batch * grid^3] (any non-zero byte is a site) -> d2, nearest int32 of the same size: the
    exact squared distance to the nearest site in voxel index units and that site's flat index, the lowest among equals
    (0x7fffffff / -1 in a frame without a site).  ``scratch``: an optional uint8 workspace of at least
    ``scene_distance_scratch_bytes(batch, grid)`` bytes (allocated per call otherwise).  Returns (d2, nearest)."""
    what = "scene_distance"
    batch, grid = int(batch), int(grid)
    need = scene_distance_scratch_bytes(batch, grid)
    n = batch * grid ** 3
    dev = _check_args(what, (("sites", sites, torch.uint8, n), ("d2", d2, torch.int32, n), ("nearest", nearest, torch.int32, n)),
                      (("scratch", scratch, torch.uint8, None),))
    scratch = _scratch(what, scratch, need, torch.uint8, dev)
    if scratch.data_ptr() % 8:
        raise HipExtensionError(f"{what}: scratch must be 8-byte aligned")
    _check(load().se_scene_distance_i32(_ptr(sites), _ptr(d2), _ptr(nearest), _ptr(scratch), scratch.numel(), batch, grid, _stream()),
           "se_scene_distance_i32")
    return d2, nearest


def scene_expect_scratch_elems(rows) -> int:
    return int(load().se_scene_expect_scratch_elems(int(rows)))


def scene_expect(prob, d2, free, radii2, out, rows, rows_per_frame, voxels, scratch=None):
    """se_scene_expect_f32: ``prob`` [rows, voxels] float32 against the field ``d2`` int32 and the free mask ``free`` uint8, both
    [rows / rows_per_frame, voxels], with the squared contact radii ``radii2`` int32 [K] (1 <= K <= 8) on the device, into ``out``
    [rows, 24] float32 (the header states every slot; nothing is divided).  Every argument is checked here and a bad one raises
    HipExtensionError before anything is launched: the kernel reads with 16-byte loads and trusts the sizes it is given."""
    what = "scene_expect"
    rows, rows_per_frame, voxels = int(rows), int(rows_per_frame), int(voxels)
    if rows <= 0 or rows > 65535 or rows_per_frame <= 0 or rows % rows_per_frame or voxels <= 0 or voxels % 4:
        raise HipExtensionError(f"{what}: rows = {rows} (1..65535, a multiple of rows_per_frame = {rows_per_frame}), voxels = {voxels} "
                                "(a positive multiple of 4) expected")
    frames = rows // rows_per_frame
    dev = _check_args(what, (("prob", prob, torch.float32, rows * voxels), ("d2", d2, torch.int32, frames * voxels),
                             ("free", free, torch.uint8, frames * voxels), ("radii2", radii2, torch.int32, (None,)),
                             ("out", out, torch.float32, rows * EXPECT_SLOTS)), (("scratch", scratch, torch.float32, None),))
    K = int(radii2.numel())
    if not 1 <= K <= EXPECT_MAX_RADII:
        raise HipExtensionError(f"{what}: {K} radii, 1..{EXPECT_MAX_RADII} supported")
    if prob.data_ptr() % 16 or d2.data_ptr() % 16 or free.data_ptr() % 4 or radii2.data_ptr() % 4:
        raise HipExtensionError(f"{what}: prob and d2 must be 16-byte aligned, free and radii2 4-byte aligned")
    scratch = _scratch(what, scratch, scene_expect_scratch_elems(rows), torch.float32, dev)
    _check(load().se_scene_expect_f32(_ptr(prob), _ptr(d2), _ptr(free), _ptr(radii2), _ptr(out), _ptr(scratch), rows, rows_per_frame,
                                      voxels, K, _stream()), "se_scene_expect_f32")
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# Multi-hypothesis joints (csrc/joint_modes.hip; sceneego_amd/op.py and VoxelNetwork_depth.joint_modes drive it)
MODES_SLOTS = 8            # p_peak, mass, mom_x mom_y mom_z, peak coordinate x y z (include/sceneego_hip.h)
MODES_MAX_K, MODES_MAX_RADIUS = 16, 3


def joint_modes_scratch_bytes(rows, grid, k) -> int:
    return int(load().se_joint_modes_scratch_bytes(int(rows), int(grid), int(k)))


def joint_modes(prob, coord, modes, index, count, total, rows, voxels, grid, k, radius, min_prob, scratch=None):
    """se_joint_modes_f32: the ``k`` strongest local maxima of every row of ``prob`` [rows, voxels] (voxels = grid^3) into ``modes``
    [rows, k, 8] float32, ``index`` [rows, k] int32, ``count`` / ``total`` [rows] int32 (the header states the definition).
    ``scratch``: an optional uint8 workspace of at least ``joint_modes_scratch_bytes(rows, grid, k)`` bytes.  Every argument is checked
    here and a bad one raises HipExtensionError before anything is launched: the kernel trusts the sizes it is given."""
    what = "joint_modes"
    rows, voxels, grid, k, radius, min_prob = int(rows), int(voxels), int(grid), int(k), int(radius), float(min_prob)
    if rows <= 0 or rows > 65535 or grid < 2 or voxels != grid ** 3 or voxels % 4:
        raise HipExtensionError(f"{what}: rows = {rows} (1..65535), grid = {grid} (>= 2), voxels = {voxels} (grid^3, a multiple of 4) "
                                "expected")
    if not 1 <= k <= MODES_MAX_K or not 0 <= radius <= MODES_MAX_RADIUS:
        raise HipExtensionError(f"{what}: k = {k} (1..{MODES_MAX_K}) and radius = {radius} (0..{MODES_MAX_RADIUS}) expected")
    if not min_prob >= 0.0:
        raise HipExtensionError(f"{what}: min_prob = {min_prob} must be >= 0 and not NaN")
    dev = _check_args(what, (("prob", prob, torch.float32, rows * voxels), ("coord", coord, torch.float32, voxels * 3),
                             ("modes", modes, torch.float32, rows * k * MODES_SLOTS), ("index", index, torch.int32, rows * k),
                             ("count", count, torch.int32, rows), ("total", total, torch.int32, rows)),
                      (("scratch", scratch, torch.uint8, None),))
    need = joint_modes_scratch_bytes(rows, grid, k)
    if need <= 0:
        raise HipExtensionError(f"{what}: grid = {grid} is not supported")
    scratch = _scratch(what, scratch, need, torch.uint8, dev)
    _check(load().se_joint_modes_f32(_ptr(prob), _ptr(coord), _ptr(modes), _ptr(index), _ptr(count), _ptr(total), _ptr(scratch),
                                     scratch.numel(), rows, voxels, grid, k, radius, min_prob, _stream()), "se_joint_modes_f32")
    return modes, index, count, total


# ----------------------------------------------------------------------------------------------------------------------------------
# Grid Bayes filter over the joint volumes of a sequence (csrc/volume_filter.hip; sceneego_amd/volume_filter.py drives it)
FILTER_MAX_GRID, FILTER_MAX_RADIUS = 128, 16
FILTER_CHAIN = 80          # sequential float32 additions on the longest path of Z and of the joint sums (csrc/volume_filter.hip: L)


def _grid_args(what, frames, rows, voxels, grid, radius=None, floor=None):
    """The arguments every operator over [frames, rows, grid^3] volumes takes, as ints and a float, range-checked against the one set
    of limits of csrc/volume_grid.h.  ``radius`` None: the operator has neither taps nor a floor (both come back as None)."""
    frames, rows, voxels, grid = int(frames), int(rows), int(voxels), int(grid)
    if radius is not None:
        radius, floor = int(radius), float(floor)
    if frames < 1 or rows <= 0 or rows > 65535 or not 2 <= grid <= FILTER_MAX_GRID or voxels != grid ** 3:
        raise HipExtensionError(f"{what}: frames = {frames} (>= 1), rows = {rows} (1..65535), grid = {grid} (2..{FILTER_MAX_GRID}), "
                                f"voxels = {voxels} (grid^3) expected")
    if radius is None:
        return frames, rows, voxels, grid, None, None
    if not 0 <= radius <= min(FILTER_MAX_RADIUS, grid - 1):
        raise HipExtensionError(f"{what}: radius = {radius} (0..{min(FILTER_MAX_RADIUS, grid - 1)}) expected")
    if not 0.0 <= floor <= 1.0:
        raise HipExtensionError(f"{what}: floor = {floor} must lie in [0, 1]")
    return frames, rows, voxels, grid, radius, floor


def _grid_scratch(what, scratch, need, rows, grid, radius, dev):
    """The workspace of a grid-sequence call: ``need`` is what the library asks for, 0 when it does not take the shape."""
    if need <= 0:
        raise HipExtensionError(f"{what}: rows = {rows}, grid = {grid}, radius = {radius} is not supported")
    return _scratch(what, scratch, need, torch.uint8, dev)


def volume_filter_scratch_bytes(rows, grid, radius) -> int:
    return int(load().se_volume_filter_scratch_bytes(int(rows), int(grid), int(radius)))


def volume_filter(prob, coord, taps, state, belief_out, joints, evidence, restarted, frames, rows, voxels, grid, radius, floor,
                  have_prior=None, scratch=None):
    """se_volume_filter_f32: ``frames`` consecutive steps of the grid Bayes filter on ``prob`` [frames, rows, voxels] (voxels =
    grid^3) from the belief in ``state`` [rows, voxels], which is updated in place (the header states the definition).  ``taps``
    [2 radius + 1] float32 on the device; ``have_prior`` None (no row has a prior) or int32 [rows]; ``belief_out`` None or [frames,
    rows, voxels]; ``joints`` [frames, rows, 3], ``evidence`` [frames, rows] float32 and ``restarted`` [frames, rows] int32 are written.
    ``scratch``: an optional uint8 workspace of at least ``volume_filter_scratch_bytes(rows, grid, radius)`` bytes.  Every argument
    is checked here and a bad one raises HipExtensionError before anything is launched: the kernels trust the sizes they are given."""
    what = "volume_filter"
    frames, rows, voxels, grid, radius, floor = _grid_args(what, frames, rows, voxels, grid, radius, floor)
    dev = _check_args(what, (("prob", prob, torch.float32, frames * rows * voxels), ("coord", coord, torch.float32, voxels * 3),
                             ("taps", taps, torch.float32, 2 * radius + 1), ("state", state, torch.float32, rows * voxels),
                             ("joints", joints, torch.float32, frames * rows * 3), ("evidence", evidence, torch.float32, frames * rows),
                             ("restarted", restarted, torch.int32, frames * rows)),
                      (("belief_out", belief_out, torch.float32, frames * rows * voxels), ("have_prior", have_prior, torch.int32, rows),
                       ("scratch", scratch, torch.uint8, None)))
    if belief_out is not None and (_overlap(belief_out, prob) or _overlap(belief_out, state)):
        raise HipExtensionError(f"{what}: belief_out must not alias prob or state")
    scratch = _grid_scratch(what, scratch, volume_filter_scratch_bytes(rows, grid, radius), rows, grid, radius, dev)
    _check(load().se_volume_filter_f32(_ptr(prob), _ptr(coord), _ptr(taps), _ptr(state), _ptr(belief_out), _ptr(joints),
                                       _ptr(evidence), _ptr(restarted), _ptr(scratch), scratch.numel(), frames, rows, voxels, grid,
                                       radius, floor, _ptr(have_prior), _stream()), "se_volume_filter_f32")
    return joints, evidence, restarted


# The filter's backward pass (csrc/volume_filter.hip: se_volume_smooth_f32; sceneego_amd/volume_smoother.py drives it)
SMOOTH_CHAIN = 80          # sequential float32 additions on the longest path of s, S and the joint sums: the filter's fold (L)


def volume_smooth_scratch_bytes(rows, grid, radius) -> int:
    return int(load().se_volume_smooth_scratch_bytes(int(rows), int(grid), int(radius)))


def volume_smooth(prob, belief, restarted, coord, taps, state, smoothed_out, joints, agreement, smoothed, frames, rows, voxels, grid,
                  radius, floor, have_link=None, scratch=None):
    """se_volume_smooth_f32: the backward pass over ``frames`` consecutive frames, last to first, on the volumes ``prob`` and the
    filtered beliefs ``belief`` [frames, rows, voxels] with the filter's ``restarted`` [frames, rows] int32 (the header states the
    definition).  ``state`` [rows, voxels] carries the backward belief from call to call and is updated in place; ``have_link`` None
    (the call ends the track) or int32 [rows]: where the last frame is linked to the frame behind it.  ``taps``: the filter's, on the
    device (the call reverses them).  ``smoothed_out`` None, ``belief`` itself (in place) or a tensor disjoint from it; ``joints``
    [frames, rows, 3], ``agreement`` [frames, rows] float32 and ``smoothed`` [frames, rows] int32 are written.  ``scratch``: an optional
    uint8 workspace of at least ``volume_smooth_scratch_bytes(rows, grid, radius)`` bytes.  Every argument is checked here and a bad
    one raises HipExtensionError before anything is launched: the kernels trust the sizes they are given."""
    what = "volume_smooth"
    frames, rows, voxels, grid, radius, floor = _grid_args(what, frames, rows, voxels, grid, radius, floor)
    total = frames * rows * voxels
    dev = _check_args(what, (("prob", prob, torch.float32, total), ("belief", belief, torch.float32, total),
                             ("restarted", restarted, torch.int32, frames * rows), ("coord", coord, torch.float32, voxels * 3),
                             ("taps", taps, torch.float32, 2 * radius + 1), ("state", state, torch.float32, rows * voxels),
                             ("joints", joints, torch.float32, frames * rows * 3), ("agreement", agreement, torch.float32, frames * rows),
                             ("smoothed", smoothed, torch.int32, frames * rows)),
                      (("smoothed_out", smoothed_out, torch.float32, total), ("have_link", have_link, torch.int32, rows),
                       ("scratch", scratch, torch.uint8, None)))
    if _overlap(state, prob) or _overlap(state, belief):
        raise HipExtensionError(f"{what}: state must not alias prob or belief")
    if smoothed_out is not None:
        if smoothed_out.data_ptr() != belief.data_ptr() and _overlap(smoothed_out, belief):
            raise HipExtensionError(f"{what}: smoothed_out must be belief itself (in place) or disjoint from it")
        if _overlap(smoothed_out, prob) or _overlap(smoothed_out, state):
            raise HipExtensionError(f"{what}: smoothed_out must not alias prob or state")
    scratch = _grid_scratch(what, scratch, volume_smooth_scratch_bytes(rows, grid, radius), rows, grid, radius, dev)
    _check(load().se_volume_smooth_f32(_ptr(prob), _ptr(belief), _ptr(restarted), _ptr(coord), _ptr(taps), _ptr(state),
                                       _ptr(smoothed_out), _ptr(joints), _ptr(agreement), _ptr(smoothed), _ptr(scratch),
                                       scratch.numel(), frames, rows, voxels, grid, radius, floor, _ptr(have_link), _stream()),
           "se_volume_smooth_f32")
    return joints, agreement, smoothed


# The E-step sums of a fit of the filter's motion model (csrc/volume_filter.hip: se_volume_transition_stats_f32;
# sceneego_amd/motion_fit.py drives it)
STATS_CHAIN = 80           # sequential float32 additions on the longest path of each of the six sums: the filter's fold (L)
STATS_SLOTS = 6            # S, s, A0, A2, Bsum, Rsum


def volume_transition_stats_scratch_bytes(rows, grid, radius) -> int:
    return int(load().se_volume_transition_stats_scratch_bytes(int(rows), int(grid), int(radius)))


def volume_transition_stats(prob, belief, restarted, taps, state, stats, linked, frames, rows, voxels, grid, radius, floor,
                            have_link=None, scratch=None):
    """se_volume_transition_stats_f32: the smoother's backward walk over ``frames`` consecutive frames, last to first, on the volumes
    ``prob`` and the filtered beliefs ``belief`` [frames, rows, voxels] with the filter's ``restarted`` [frames, rows] int32, writing
    per frame and row the six sums ``stats`` [frames, rows, 6] float32 (S, s, A0, A2, Bsum, Rsum: the header states the definition;
    NaN where the frame is not linked) and ``linked`` [frames, rows] int32.  ``state`` [rows, voxels] carries the backward belief from
    call to call and is updated in place; ``have_link`` None (the call ends the track) or int32 [rows].  ``taps``: the filter's, on
    the device.  ``scratch``: an optional uint8 workspace of at least ``volume_transition_stats_scratch_bytes(rows, grid, radius)``
    bytes.  Every argument is checked here and a bad one raises HipExtensionError before anything is launched: the kernels trust
    the sizes they are given."""
    what = "volume_transition_stats"
    frames, rows, voxels, grid, radius, floor = _grid_args(what, frames, rows, voxels, grid, radius, floor)
    total = frames * rows * voxels
    dev = _check_args(what, (("prob", prob, torch.float32, total), ("belief", belief, torch.float32, total),
                             ("restarted", restarted, torch.int32, frames * rows), ("taps", taps, torch.float32, 2 * radius + 1),
                             ("state", state, torch.float32, rows * voxels), ("stats", stats, torch.float32, frames * rows * STATS_SLOTS),
                             ("linked", linked, torch.int32, frames * rows)),
                      (("have_link", have_link, torch.int32, rows), ("scratch", scratch, torch.uint8, None)))
    if _overlap(state, prob) or _overlap(state, belief):
        raise HipExtensionError(f"{what}: state must not alias prob or belief")
    scratch = _grid_scratch(what, scratch, volume_transition_stats_scratch_bytes(rows, grid, radius), rows, grid, radius, dev)
    _check(load().se_volume_transition_stats_f32(_ptr(prob), _ptr(belief), _ptr(restarted), _ptr(taps), _ptr(state), _ptr(stats),
                                                 _ptr(linked), _ptr(scratch), scratch.numel(), frames, rows, voxels, grid, radius,
                                                 floor, _ptr(have_link), _stream()), "se_volume_transition_stats_f32")
    return stats, linked


# Trajectory samples on the filter's model (csrc/volume_sample.hip: se_volume_sample_f32; VolumeSmoother.sample drives it)
SAMPLE_STEP, SAMPLE_JUMP, SAMPLE_FRESH = 0, 1, 2      # `kind`: the branch a frame's draw took


def volume_sample_scratch_bytes(frames, rows, grid) -> int:
    return int(load().se_volume_sample_scratch_bytes(int(frames), int(rows), int(grid)))


def volume_sample(belief, restarted, taps, next_voxel, index, kind, frames, rows, voxels, grid, radius, floor, samples, first_sample=0,
                  first_frame=0, seed=0, have_link=None, scratch=None):
    """se_volume_sample_f32: ``samples`` trajectories per row through ``frames`` consecutive frames, drawn last to first from the
    filtered beliefs ``belief`` [frames, rows, voxels] with the filter's ``restarted`` [frames, rows] int32 (the header states the
    definition).  ``next_voxel`` [samples, rows] int32 carries the voxel of the frame behind the call from call to call and is updated
    in place; ``have_link`` None (the call ends the track) or int32 [rows].  ``index`` and ``kind`` [samples, frames, rows] int32 are
    written.  ``first_sample`` and ``first_frame``: the global index of the call's first sample and frame (the random numbers depend
    on the global indices alone); ``seed``: 0..2^64-1.  ``taps``: the filter's, on the device.  ``scratch``: an optional uint8
    workspace of at least ``volume_sample_scratch_bytes(frames, rows, grid)`` bytes.  Every argument is checked here and a bad one
    raises HipExtensionError before anything is launched: the kernels trust the sizes they are given."""
    what = "volume_sample"
    frames, rows, voxels, grid, radius, floor = _grid_args(what, frames, rows, voxels, grid, radius, floor)
    samples, first_sample, first_frame, seed = int(samples), int(first_sample), int(first_frame), int(seed)
    if samples < 1 or first_sample < 0 or first_frame < 0 or first_sample + samples > 2 ** 32 or first_frame + frames > 2 ** 32:
        raise HipExtensionError(f"{what}: samples = {samples} (>= 1), first_sample = {first_sample} and first_frame = {first_frame} "
                                "(>= 0, the last index below 2^32) expected")
    if not 0 <= seed < 2 ** 64:
        raise HipExtensionError(f"{what}: seed = {seed} (0..2^64-1) expected")
    dev = _check_args(what, (("belief", belief, torch.float32, frames * rows * voxels),
                             ("restarted", restarted, torch.int32, frames * rows), ("taps", taps, torch.float32, 2 * radius + 1),
                             ("next_voxel", next_voxel, torch.int32, samples * rows),
                             ("index", index, torch.int32, samples * frames * rows), ("kind", kind, torch.int32, samples * frames * rows)),
                      (("have_link", have_link, torch.int32, rows), ("scratch", scratch, torch.uint8, None)))
    if _overlap(index, kind) or _overlap(next_voxel, index) or _overlap(next_voxel, kind):
        raise HipExtensionError(f"{what}: next_voxel, index and kind must not alias")
    scratch = _grid_scratch(what, scratch, volume_sample_scratch_bytes(frames, rows, grid), rows, grid, radius, dev)
    _check(load().se_volume_sample_f32(_ptr(belief), _ptr(restarted), _ptr(taps), _ptr(next_voxel), _ptr(index), _ptr(kind),
                                       _ptr(scratch), scratch.numel(), frames, rows, voxels, grid, radius, floor, samples,
                                       first_sample, first_frame, seed & 0xFFFFFFFF, seed >> 32, _ptr(have_link), _stream()),
           "se_volume_sample_f32")
    return index, kind


# The max-product pass on the filter's model (csrc/volume_viterbi.hip; sceneego_amd/volume_viterbi.py drives it)
VITERBI_JUMP = 1 << 30     # the jump bit of a back-pointer; the predecessor's flat index is the rest
VITERBI_MAX_REFINE = 3


def volume_viterbi_scratch_bytes(rows, grid, radius) -> int:
    return int(load().se_volume_viterbi_scratch_bytes(int(rows), int(grid), int(radius)))


def volume_viterbi(prob, taps, state, peak_state, best_state, back_out, peak, best, exponent, restarted, frames, rows, voxels, grid,
                   radius, floor, have_prior=None, scratch=None):
    """se_volume_viterbi_f32: ``frames`` consecutive steps of the max-product recursion on ``prob`` [frames, rows, voxels] (voxels =
    grid^3) from the scaled scores in ``state`` [rows, voxels] with their ``peak_state`` [rows] int32 and ``best_state`` [rows]
    float32, all three updated in place (the header states the definition).  ``taps`` [2 radius + 1] float32 on the device;
    ``have_prior`` None (no row has a prior) or int32 [rows].  ``back_out`` [frames, rows, voxels] int32, ``peak``, ``exponent``,
    ``restarted`` [frames, rows] int32 and ``best`` [frames, rows] float32 are written.  ``scratch``: an optional uint8 workspace of at
    least ``volume_viterbi_scratch_bytes(rows, grid, radius)`` bytes.  Every argument is checked here and a bad one raises
    HipExtensionError before anything is launched: the kernels trust the sizes they are given."""
    what = "volume_viterbi"
    frames, rows, voxels, grid, radius, floor = _grid_args(what, frames, rows, voxels, grid, radius, floor)
    total = frames * rows * voxels
    dev = _check_args(what, (("prob", prob, torch.float32, total), ("taps", taps, torch.float32, 2 * radius + 1),
                             ("state", state, torch.float32, rows * voxels), ("peak_state", peak_state, torch.int32, rows),
                             ("best_state", best_state, torch.float32, rows), ("back_out", back_out, torch.int32, total),
                             ("peak", peak, torch.int32, frames * rows), ("best", best, torch.float32, frames * rows),
                             ("exponent", exponent, torch.int32, frames * rows), ("restarted", restarted, torch.int32, frames * rows)),
                      (("have_prior", have_prior, torch.int32, rows), ("scratch", scratch, torch.uint8, None)))
    if _overlap(state, prob) or _overlap(back_out, prob) or _overlap(back_out, state):
        raise HipExtensionError(f"{what}: prob, state and back_out must not alias one another")
    scratch = _grid_scratch(what, scratch, volume_viterbi_scratch_bytes(rows, grid, radius), rows, grid, radius, dev)
    _check(load().se_volume_viterbi_f32(_ptr(prob), _ptr(taps), _ptr(state), _ptr(peak_state), _ptr(best_state), _ptr(back_out),
                                        _ptr(peak), _ptr(best), _ptr(exponent), _ptr(restarted), _ptr(scratch), scratch.numel(),
                                        frames, rows, voxels, grid, radius, floor, _ptr(have_prior), _stream()),
           "se_volume_viterbi_f32")
    return peak, best, exponent, restarted


def volume_viterbi_keep(prob, taps, state, peak_state, best_state, back_out, peak, best, exponent, restarted, scores_out, frames, rows,
                        voxels, grid, radius, floor, have_prior=None, scratch=None):
    """se_volume_viterbi_keep_f32: ``volume_viterbi`` with one more output, ``scores_out`` [frames, rows, voxels] float32 (every frame's
    scores as ``state`` holds them after its fold pass); every other output has the bits ``volume_viterbi`` gives.  Arguments are
    checked before anything is launched."""
    what = "volume_viterbi_keep"
    frames, rows, voxels, grid, radius, floor = _grid_args(what, frames, rows, voxels, grid, radius, floor)
    total = frames * rows * voxels
    dev = _check_args(what, (("prob", prob, torch.float32, total), ("taps", taps, torch.float32, 2 * radius + 1),
                             ("state", state, torch.float32, rows * voxels), ("peak_state", peak_state, torch.int32, rows),
                             ("best_state", best_state, torch.float32, rows), ("back_out", back_out, torch.int32, total),
                             ("peak", peak, torch.int32, frames * rows), ("best", best, torch.float32, frames * rows),
                             ("exponent", exponent, torch.int32, frames * rows), ("restarted", restarted, torch.int32, frames * rows),
                             ("scores_out", scores_out, torch.float32, total)),
                      (("have_prior", have_prior, torch.int32, rows), ("scratch", scratch, torch.uint8, None)))
    big = (("prob", prob), ("state", state), ("back_out", back_out), ("scores_out", scores_out))
    if any(_overlap(a, b) for i, (_, a) in enumerate(big) for _, b in big[i + 1:]):
        raise HipExtensionError(f"{what}: prob, state, back_out and scores_out must not alias one another")
    scratch = _grid_scratch(what, scratch, volume_viterbi_scratch_bytes(rows, grid, radius), rows, grid, radius, dev)
    _check(load().se_volume_viterbi_keep_f32(_ptr(prob), _ptr(taps), _ptr(state), _ptr(peak_state), _ptr(best_state), _ptr(back_out),
                                             _ptr(peak), _ptr(best), _ptr(exponent), _ptr(restarted), _ptr(scores_out), _ptr(scratch),
                                             scratch.numel(), frames, rows, voxels, grid, radius, floor, _ptr(have_prior), _stream()),
           "se_volume_viterbi_keep_f32")
    return peak, best, exponent, restarted


def volume_viterbi_back_scratch_bytes(rows, grid, radius) -> int:
    return int(load().se_volume_viterbi_back_scratch_bytes(int(rows), int(grid), int(radius)))


BACK_OUTPUTS = (("mm_best", torch.float32), ("mm_peak", torch.int32), ("path_value", torch.float32), ("alt_value", torch.float32),
                ("alt_index", torch.int32), ("complete", torch.int32), ("r_best", torch.float32), ("r_exponent", torch.int32))


def volume_viterbi_back(prob, scores, exponent, restarted, index, taps, carry, out, frames, rows, voxels, grid, radius, floor,
                        separation, have_next, succ=None, max_marginals=None, scratch=None):
    """se_volume_viterbi_back_f32: the backward max-product pass over one stored chunk, last frame to first (the header states the
    definition).  ``prob``, ``scores`` [frames, rows, voxels] float32; ``exponent``, ``restarted``, ``index`` [frames, rows] int32;
    ``carry``: a dict of the backward state carried from chunk to chunk on the device, ``r`` [rows, voxels] float32, ``link`` [rows]
    int32, ``best`` [rows] float32, ``complete`` [rows] int32 (read only with ``have_next`` = 1, always written); ``out``: a dict of
    the [frames, rows] outputs named in ``BACK_OUTPUTS``.  ``succ`` None or [frames, rows, voxels] int32: it may be the memory of
    ``scores`` (``scores.view(torch.int32)``); ``max_marginals`` None or [frames, rows, voxels] float32.  Every argument is checked
    here and a bad one raises HipExtensionError before anything is launched."""
    what = "volume_viterbi_back"
    frames, rows, voxels, grid, radius, floor = _grid_args(what, frames, rows, voxels, grid, radius, floor)
    if isinstance(separation, bool) or not isinstance(separation, numbers.Integral) or separation < 0:
        raise HipExtensionError(f"{what}: separation = {separation!r} (an integer >= 0) expected")
    if not isinstance(have_next, (bool, int)) or int(have_next) not in (0, 1):
        raise HipExtensionError(f"{what}: have_next = {have_next!r} must be 0 or 1")
    if not isinstance(carry, dict) or tuple(sorted(carry)) != ("best", "complete", "link", "r"):
        raise HipExtensionError(f"{what}: carry must be a dict with the keys r, link, best, complete")
    if not isinstance(out, dict) or any(name not in out for name, _ in BACK_OUTPUTS):
        raise HipExtensionError(f"{what}: out must be a dict with the keys " + ", ".join(name for name, _ in BACK_OUTPUTS))
    total = frames * rows * voxels
    named = (("prob", prob, torch.float32, total), ("scores", scores, torch.float32, total),
             ("exponent", exponent, torch.int32, frames * rows), ("restarted", restarted, torch.int32, frames * rows),
             ("index", index, torch.int32, frames * rows), ("taps", taps, torch.float32, 2 * radius + 1),
             ("carry r", carry["r"], torch.float32, rows * voxels), ("carry link", carry["link"], torch.int32, rows),
             ("carry best", carry["best"], torch.float32, rows), ("carry complete", carry["complete"], torch.int32, rows))
    named += tuple((name, out[name], dtype, frames * rows) for name, dtype in BACK_OUTPUTS)
    dev = _check_args(what, named, (("succ", succ, torch.int32, total), ("max_marginals", max_marginals, torch.float32, total),
                                    ("scratch", scratch, torch.uint8, None)))
    if _overlap(carry["r"], prob) or _overlap(carry["r"], scores) or _overlap(prob, scores):
        raise HipExtensionError(f"{what}: prob, scores and the carried r must not alias one another")
    if succ is not None and (_overlap(succ, prob) or _overlap(succ, carry["r"])
                             or (_overlap(succ, scores) and succ.data_ptr() != scores.data_ptr())):
        raise HipExtensionError(f"{what}: succ may be the memory of scores, voxel for voxel, and must not overlap anything else")
    if max_marginals is not None and any(_overlap(max_marginals, t) for t in (prob, scores, carry["r"]) + (() if succ is None else (succ,))):
        raise HipExtensionError(f"{what}: max_marginals must not alias prob, scores, succ or the carried r")
    scratch = _grid_scratch(what, scratch, volume_viterbi_back_scratch_bytes(rows, grid, radius), rows, grid, radius, dev)
    _check(load().se_volume_viterbi_back_f32(
        _ptr(prob), _ptr(scores), _ptr(exponent), _ptr(restarted), _ptr(index), _ptr(taps), _ptr(carry["r"]), _ptr(carry["link"]),
        _ptr(carry["best"]), _ptr(carry["complete"]), *(_ptr(out[name]) for name, _ in BACK_OUTPUTS), _ptr(succ), _ptr(max_marginals),
        _ptr(scratch), scratch.numel(), frames, rows, voxels, grid, radius, floor, int(separation), int(have_next), _stream()),
        "se_volume_viterbi_back_f32")
    return out


def volume_viterbi_branch(back, succ, restarted, anchor, cursor, index, jumped, frames, rows, voxels, direction, have_carry):
    """se_volume_viterbi_branch_i32: the branch walk over one stored chunk from the anchors ``anchor`` [frames, rows] int32 (a voxel at
    a segment's anchor frame, -1 elsewhere): ``direction`` -1 back through ``back`` (chunks last first; writes every frame of
    ``index`` and ``jumped``), then +1 on through ``succ`` (chunks first to last; writes the frames it reaches).  ``cursor`` [rows]
    int32 is read with ``have_carry`` = 1 and written.  Arguments are checked before anything is launched."""
    what = "volume_viterbi_branch"
    frames, rows, voxels = int(frames), int(rows), int(voxels)
    if frames < 1 or rows <= 0 or rows > 65535 or not 1 <= voxels <= FILTER_MAX_GRID ** 3:
        raise HipExtensionError(f"{what}: frames = {frames} (>= 1), rows = {rows} (1..65535), voxels = {voxels} (1..{FILTER_MAX_GRID}^3) "
                                "expected")
    if isinstance(direction, bool) or direction not in (-1, 1):
        raise HipExtensionError(f"{what}: direction = {direction!r} must be -1 or 1")
    if not isinstance(have_carry, (bool, int)) or int(have_carry) not in (0, 1):
        raise HipExtensionError(f"{what}: have_carry = {have_carry!r} must be 0 or 1")
    _check_args(what, (("back", back, torch.int32, frames * rows * voxels), ("succ", succ, torch.int32, frames * rows * voxels),
                       ("restarted", restarted, torch.int32, frames * rows), ("anchor", anchor, torch.int32, frames * rows),
                       ("cursor", cursor, torch.int32, rows), ("index", index, torch.int32, frames * rows),
                       ("jumped", jumped, torch.int32, frames * rows)))
    _check(load().se_volume_viterbi_branch_i32(_ptr(back), _ptr(succ), _ptr(restarted), _ptr(anchor), _ptr(cursor), _ptr(index),
                                               _ptr(jumped), frames, rows, voxels, int(direction), int(have_carry), _stream()),
           "se_volume_viterbi_branch_i32")
    return index, jumped


def volume_viterbi_path(back, peak, restarted, cursor, index, jumped, frames, rows, voxels, have_next):
    """se_volume_viterbi_path_i32: the back-walk over one stored chunk (``back`` [frames, rows, voxels], ``peak`` and ``restarted``
    [frames, rows], all int32), last frame to first; ``cursor`` [rows] int32 is read when ``have_next`` (a later chunk was walked
    before) and written; ``index`` and ``jumped`` [frames, rows] int32 are written.  Arguments are checked before anything is launched."""
    what = "volume_viterbi_path"
    frames, rows, voxels = int(frames), int(rows), int(voxels)
    if frames < 1 or rows <= 0 or rows > 65535 or not 1 <= voxels <= FILTER_MAX_GRID ** 3:
        raise HipExtensionError(f"{what}: frames = {frames} (>= 1), rows = {rows} (1..65535), voxels = {voxels} (1..{FILTER_MAX_GRID}^3) "
                                "expected")
    if not isinstance(have_next, (bool, int)) or int(have_next) not in (0, 1):
        raise HipExtensionError(f"{what}: have_next = {have_next!r} must be 0 or 1")
    _check_args(what, (("back", back, torch.int32, frames * rows * voxels), ("peak", peak, torch.int32, frames * rows),
                       ("restarted", restarted, torch.int32, frames * rows), ("cursor", cursor, torch.int32, rows),
                       ("index", index, torch.int32, frames * rows), ("jumped", jumped, torch.int32, frames * rows)))
    _check(load().se_volume_viterbi_path_i32(_ptr(back), _ptr(peak), _ptr(restarted), _ptr(cursor), _ptr(index), _ptr(jumped), frames,
                                             rows, voxels, int(have_next), _stream()), "se_volume_viterbi_path_i32")
    return index, jumped


def volume_viterbi_refine(prob, coord, index, joints, frames, rows, voxels, grid, refine):
    """se_volume_viterbi_refine_f32: ``joints`` [frames, rows, 3] float32 from the path ``index`` [frames, rows] int32: the centroid of
    ``prob`` [frames, rows, voxels] over the window of ``refine`` voxels (0..3) around each path voxel, or the voxel centre
    (``refine`` = 0: ``prob`` may be None).  Arguments are checked before anything is launched."""
    what = "volume_viterbi_refine"
    frames, rows, voxels, grid = _grid_args(what, frames, rows, voxels, grid)[:4]
    if isinstance(refine, bool) or int(refine) != refine or not 0 <= int(refine) <= VITERBI_MAX_REFINE:
        raise HipExtensionError(f"{what}: refine = {refine!r} (an integer in 0..{VITERBI_MAX_REFINE}) expected")
    refine = int(refine)
    named = (("coord", coord, torch.float32, voxels * 3), ("index", index, torch.int32, frames * rows),
             ("joints", joints, torch.float32, frames * rows * 3))
    prob_entry = ("prob", prob, torch.float32, frames * rows * voxels)
    _check_args(what, named + ((prob_entry,) if refine > 0 else ()), () if refine > 0 else (prob_entry,))
    _check(load().se_volume_viterbi_refine_f32(_ptr(prob), _ptr(coord), _ptr(index), _ptr(joints), frames, rows, voxels, grid, refine,
                                               _stream()), "se_volume_viterbi_refine_f32")
    return joints


# ----------------------------------------------------------------------------------------------------------------------------------
# Skeleton-coupled joints (csrc/skeleton_prior.hip; sceneego_amd/skeleton_prior.py drives it)
SKELETON_MAX_JOINTS, SKELETON_MAX_GRID, SKELETON_MAX_RADIUS = 32, 128, 24
SKELETON_SUM_CHAIN = 142   # sequential float32 additions on the longest path of a row sum s, t, Z (csrc/skeleton_prior.hip: L)


def SHELL_CHAIN(radius) -> int:
    """T(R) = (2R+1)^2 + 2R: the roundings on the longest path of one output of the shell correlation (csrc/skeleton_prior.hip: one
    chain of fused multiply-adds per di-plane, the planes added in sequence).  Never more than the block's non-zero taps."""
    radius = int(radius)
    return (2 * radius + 1) ** 2 + 2 * radius


def _skeleton_shape(what, grid, radius):
    if not 2 <= grid <= SKELETON_MAX_GRID:
        raise HipExtensionError(f"{what}: grid = {grid} (2..{SKELETON_MAX_GRID}) expected")
    if not 0 <= radius <= min(SKELETON_MAX_RADIUS, grid - 1):
        raise HipExtensionError(f"{what}: radius = {radius} (0..{min(SKELETON_MAX_RADIUS, grid - 1)}) expected")


def _tree_args(what, parents, frames, voxels, grid, radius, floor):
    """The arguments of the two passes over the kinematic tree: ``parents`` as a list of ints that obeys the parent rule, its length J,
    and the rest as ints and a float, range-checked."""
    try:
        parents = [int(v) for v in parents]
    except (TypeError, ValueError):
        raise HipExtensionError(f"{what}: parents must be a sequence of integers") from None
    J = len(parents)
    frames, voxels, grid, radius, floor = int(frames), int(voxels), int(grid), int(radius), float(floor)
    if not 1 <= J <= SKELETON_MAX_JOINTS or parents[0] != 0 or any(not 0 <= parents[j] < j for j in range(1, J)):
        raise HipExtensionError(f"{what}: parents = {parents}: 1..{SKELETON_MAX_JOINTS} joints with parents[0] = 0 and "
                                "0 <= parents[j] < j expected")
    if frames < 1:
        raise HipExtensionError(f"{what}: frames = {frames} (>= 1) expected")
    _skeleton_shape(what, grid, radius)
    if voxels != grid ** 3:
        raise HipExtensionError(f"{what}: voxels = {voxels} is not grid^3 = {grid ** 3}")
    if not 0.0 <= floor <= 1.0:
        raise HipExtensionError(f"{what}: floor = {floor} must lie in [0, 1]")
    return parents, J, frames, voxels, grid, radius, floor


def shell_correlate_scratch_bytes(tap_rows, radius) -> int:
    return int(load().se_shell_correlate_scratch_bytes(int(tap_rows), int(radius)))


def shell_correlate(a, taps, tap_row, s, out, rows, grid, radius, scale_mul=1.0, add=0.0, scratch=None):
    """se_shell_correlate_f32: ``out[r] = scale_mul * corr(a[r], taps[tap_row[r]]) / s[r] + add`` for the ``rows`` volumes ``a``
    [rows, grid^3]; ``taps`` [tap_rows, (2 radius + 1)^3] float32, ``tap_row`` [rows] int32 and ``s`` [rows] float32 on the device (the
    header states the correlation).  ``scratch``: an optional uint8 workspace of at least ``shell_correlate_scratch_bytes(tap_rows,
    radius)`` bytes.  Every argument is checked here and a bad one raises HipExtensionError before anything is launched."""
    what = "shell_correlate"
    rows, grid, radius, scale_mul, add = int(rows), int(grid), int(radius), float(scale_mul), float(add)
    if not 1 <= rows <= 65535:
        raise HipExtensionError(f"{what}: rows = {rows} (1..65535) expected")
    _skeleton_shape(what, grid, radius)
    voxels, block = grid ** 3, (2 * radius + 1) ** 3
    dev = _check_args(what, (("a", a, torch.float32, rows * voxels), ("taps", taps, torch.float32, (None, block)),
                             ("tap_row", tap_row, torch.int32, rows), ("s", s, torch.float32, rows),
                             ("out", out, torch.float32, rows * voxels)), (("scratch", scratch, torch.uint8, None),))
    tap_rows = int(taps.shape[0])
    if not 1 <= tap_rows <= 65535:
        raise HipExtensionError(f"{what}: taps holds {tap_rows} blocks, 1..65535 expected")
    if _overlap(out, a):
        raise HipExtensionError(f"{what}: out must not alias a")
    scratch = _scratch(what, scratch, shell_correlate_scratch_bytes(tap_rows, radius), torch.uint8, dev)
    _check(load().se_shell_correlate_f32(_ptr(a), _ptr(taps), _ptr(tap_row), _ptr(s), _ptr(out), _ptr(scratch), scratch.numel(), rows,
                                         tap_rows, grid, radius, scale_mul, add, _stream()), "se_shell_correlate_f32")
    return out


def skeleton_couple_scratch_bytes(frames, joints, grid, radius) -> int:
    return int(load().se_skeleton_couple_scratch_bytes(int(frames), int(joints), int(grid), int(radius)))


def skeleton_couple(prob, coord, taps, parents, beliefs, joints, evidence, coupled, frames, voxels, grid, radius, floor, scratch=None):
    """se_skeleton_couple_f32: belief propagation over the tree ``parents`` (a sequence of J ints, parents[0] = 0, parents[j] < j) on
    ``prob`` [frames, J, voxels] (voxels = grid^3) with the shell taps ``taps`` [J, (2 radius + 1)^3] on the device (the header states
    the definition).  ``beliefs`` None or [frames, J, voxels]; ``joints`` [frames, J, 3], ``evidence`` [frames, J] float32 and
    ``coupled`` [frames] int32 are written.  ``scratch``: an optional uint8 workspace of at least ``skeleton_couple_scratch_bytes(
    frames, J, grid, radius)`` bytes.  Every argument is checked here and a bad one raises HipExtensionError before anything is
    launched: the kernels trust the sizes they are given."""
    what = "skeleton_couple"
    parents, J, frames, voxels, grid, radius, floor = _tree_args(what, parents, frames, voxels, grid, radius, floor)
    dev = _check_args(what, (("prob", prob, torch.float32, frames * J * voxels), ("coord", coord, torch.float32, voxels * 3),
                             ("taps", taps, torch.float32, J * (2 * radius + 1) ** 3),
                             ("joints", joints, torch.float32, frames * J * 3), ("evidence", evidence, torch.float32, frames * J),
                             ("coupled", coupled, torch.int32, frames)),
                      (("beliefs", beliefs, torch.float32, frames * J * voxels), ("scratch", scratch, torch.uint8, None)))
    if beliefs is not None and _overlap(beliefs, prob):
        raise HipExtensionError(f"{what}: beliefs must not alias prob")
    scratch = _scratch(what, scratch, skeleton_couple_scratch_bytes(frames, J, grid, radius), torch.uint8, dev)
    par = (ctypes.c_int * J)(*parents)
    _check(load().se_skeleton_couple_f32(_ptr(prob), _ptr(coord), _ptr(taps), ctypes.cast(par, ctypes.c_void_p), _ptr(beliefs),
                                         _ptr(joints), _ptr(evidence), _ptr(coupled), _ptr(scratch), scratch.numel(), frames, J,
                                         voxels, grid, radius, floor, _stream()), "se_skeleton_couple_f32")
    return joints, evidence, coupled


# The E-step sums of a fit of the skeleton model (csrc/skeleton_prior.hip: se_skeleton_edge_stats_f32, se_shell_moments_f32;
# sceneego_amd/skeleton_fit.py drives them)
EDGE_STATS_SLOTS = 4       # S0, S1, S2, SJ


def MOMENT_CHAIN(grid) -> int:
    """SE_SK_MOMENT_CHAIN(G): the roundings on the longest path of the reduction behind the correlation values of one moment (4 for
    the lane's four outputs, 6 + 2 for the workgroup, ceil(records / 64) + 6 for the fold of the row's G ceil(G/16) ceil(G/64) records)."""
    grid = int(grid)
    return 18 + (grid * ((grid + 15) // 16) * ((grid + 63) // 64) + 63) // 64


def shell_moments_scratch_bytes(rows, tap_rows, grid, radius) -> int:
    return int(load().se_shell_moments_scratch_bytes(int(rows), int(tap_rows), int(grid), int(radius)))


def shell_moments(e, a, taps, taps_r, taps_r2, tap_row, out, rows, grid, radius, scratch=None):
    """se_shell_moments_f32: ``out[r] = (S0, S1, S2)``, S_m = sum_x e[r](x) corr(a[r], w_m[tap_row[r]])(x), for the ``rows`` pairs of
    volumes ``e``, ``a`` [rows, grid^3]; the three tap blocks [tap_rows, (2 radius + 1)^3] float32 and ``tap_row`` [rows] int32 on the
    device; ``out`` [rows, 3] float32 (the header states the sums).  ``scratch``: an optional uint8 workspace of at least
    ``shell_moments_scratch_bytes(rows, tap_rows, grid, radius)`` bytes.  Every argument is checked here and a bad one raises
    HipExtensionError before anything is launched."""
    what = "shell_moments"
    rows, grid, radius = int(rows), int(grid), int(radius)
    if not 1 <= rows <= 65535:
        raise HipExtensionError(f"{what}: rows = {rows} (1..65535) expected")
    _skeleton_shape(what, grid, radius)
    voxels, block = grid ** 3, (2 * radius + 1) ** 3
    dev = _check_args(what, (("e", e, torch.float32, rows * voxels), ("a", a, torch.float32, rows * voxels),
                             ("taps", taps, torch.float32, (None, block)), ("tap_row", tap_row, torch.int32, rows),
                             ("out", out, torch.float32, rows * 3)), (("scratch", scratch, torch.uint8, None),))
    tap_rows = int(taps.shape[0])
    if not 1 <= tap_rows <= 65535:
        raise HipExtensionError(f"{what}: taps holds {tap_rows} blocks, 1..65535 expected")
    _check_args(what, (("taps_r", taps_r, torch.float32, tap_rows * block), ("taps_r2", taps_r2, torch.float32, tap_rows * block)),
                device=dev)
    scratch = _scratch(what, scratch, shell_moments_scratch_bytes(rows, tap_rows, grid, radius), torch.uint8, dev)
    _check(load().se_shell_moments_f32(_ptr(e), _ptr(a), _ptr(taps), _ptr(taps_r), _ptr(taps_r2), _ptr(tap_row), _ptr(out),
                                       _ptr(scratch), scratch.numel(), rows, tap_rows, grid, radius, _stream()), "se_shell_moments_f32")
    return out


def skeleton_edge_stats_scratch_bytes(frames, joints, grid, radius) -> int:
    return int(load().se_skeleton_edge_stats_scratch_bytes(int(frames), int(joints), int(grid), int(radius)))


def skeleton_edge_stats(prob, taps, taps_r, taps_r2, parents, stats, norms, valid, frames, voxels, grid, radius, floor, scratch=None):
    """se_skeleton_edge_stats_f32: ``skeleton_couple``'s two passes over the tree ``parents`` on ``prob`` [frames, J, voxels] with the
    three tap blocks [J, (2 radius + 1)^3] on the device, for the edge statistics in place of the beliefs (the header states them):
    ``stats`` [frames, J, 4] (S0, S1, S2, SJ), ``norms`` [frames, J, 3] (s, t, Z) float32 and ``valid`` [frames] int32 are written.
    ``scratch``: an optional uint8 workspace of at least ``skeleton_edge_stats_scratch_bytes(frames, J, grid, radius)`` bytes.  Every
    argument is checked here and a bad one raises HipExtensionError before anything is launched."""
    what = "skeleton_edge_stats"
    parents, J, frames, voxels, grid, radius, floor = _tree_args(what, parents, frames, voxels, grid, radius, floor)
    block = (2 * radius + 1) ** 3
    dev = _check_args(what, (("prob", prob, torch.float32, frames * J * voxels), ("taps", taps, torch.float32, J * block),
                             ("taps_r", taps_r, torch.float32, J * block), ("taps_r2", taps_r2, torch.float32, J * block),
                             ("stats", stats, torch.float32, frames * J * EDGE_STATS_SLOTS),
                             ("norms", norms, torch.float32, frames * J * 3), ("valid", valid, torch.int32, frames)),
                      (("scratch", scratch, torch.uint8, None),))
    scratch = _scratch(what, scratch, skeleton_edge_stats_scratch_bytes(frames, J, grid, radius), torch.uint8, dev)
    par = (ctypes.c_int * J)(*parents)
    _check(load().se_skeleton_edge_stats_f32(_ptr(prob), _ptr(taps), _ptr(taps_r), _ptr(taps_r2), ctypes.cast(par, ctypes.c_void_p),
                                             _ptr(stats), _ptr(norms), _ptr(valid), _ptr(scratch), scratch.numel(), frames, J, voxels,
                                             grid, radius, floor, _stream()), "se_skeleton_edge_stats_f32")
    return stats, norms, valid


# Pose samples from the skeleton posterior (csrc/skeleton_sample.hip: se_skeleton_upward_f32, se_skeleton_sample_f32;
# SkeletonPrior.sample drives them).  `kind` takes SAMPLE_STEP / SAMPLE_JUMP / SAMPLE_FRESH, as the trajectory sampler's.
def skeleton_upward_scratch_bytes(frames, joints, grid, radius) -> int:
    return int(load().se_skeleton_upward_scratch_bytes(int(frames), int(joints), int(grid), int(radius)))


def skeleton_upward(prob, taps, parents, upward, sums, valid, frames, voxels, grid, radius, floor, scratch=None):
    """se_skeleton_upward_f32: the upward pass of ``skeleton_couple`` over the tree ``parents`` on ``prob`` [frames, J, voxels] with the
    shell taps ``taps`` [J, (2 radius + 1)^3] on the device, and the root's product (the header states it).  ``upward`` [frames, J,
    voxels] float32 (the A_j), ``sums`` [frames, J] float32 (s_j, also for j = 0) and ``valid`` [frames] int32 are written.
    ``scratch``: an optional uint8 workspace of at least ``skeleton_upward_scratch_bytes(frames, J, grid, radius)`` bytes.  Every
    argument is checked here and a bad one raises HipExtensionError before anything is launched."""
    what = "skeleton_upward"
    parents, J, frames, voxels, grid, radius, floor = _tree_args(what, parents, frames, voxels, grid, radius, floor)
    dev = _check_args(what, (("prob", prob, torch.float32, frames * J * voxels),
                             ("taps", taps, torch.float32, J * (2 * radius + 1) ** 3),
                             ("upward", upward, torch.float32, frames * J * voxels), ("sums", sums, torch.float32, frames * J),
                             ("valid", valid, torch.int32, frames)), (("scratch", scratch, torch.uint8, None),))
    if _overlap(upward, prob):
        raise HipExtensionError(f"{what}: upward must not alias prob")
    scratch = _scratch(what, scratch, skeleton_upward_scratch_bytes(frames, J, grid, radius), torch.uint8, dev)
    par = (ctypes.c_int * J)(*parents)
    _check(load().se_skeleton_upward_f32(_ptr(prob), _ptr(taps), ctypes.cast(par, ctypes.c_void_p), _ptr(upward), _ptr(sums),
                                         _ptr(valid), _ptr(scratch), scratch.numel(), frames, J, voxels, grid, radius, floor,
                                         _stream()), "se_skeleton_upward_f32")
    return upward, sums, valid


def skeleton_sample_scratch_bytes(frames, joints, grid) -> int:
    return int(load().se_skeleton_sample_scratch_bytes(int(frames), int(joints), int(grid)))


def _sample_args(what, samples, count, first_sample, first_frame, seed):
    """The arguments of a sampler's call as ints: ``samples`` >= 1, the offsets of the first sample and of the first of ``count``
    frames not negative with the last index below 2^32 (the counter words of the generator are 32 bits), ``seed`` in 0..2^64-1."""
    samples, first_sample, first_frame, seed = int(samples), int(first_sample), int(first_frame), int(seed)
    if samples < 1 or first_sample < 0 or first_frame < 0 or first_sample + samples > 2 ** 32 or first_frame + count > 2 ** 32:
        raise HipExtensionError(f"{what}: samples = {samples} (>= 1), first_sample = {first_sample} and first_frame = {first_frame} "
                                "(>= 0, the last index below 2^32) expected")
    if not 0 <= seed < 2 ** 64:
        raise HipExtensionError(f"{what}: seed = {seed} (0..2^64-1) expected")
    return samples, first_sample, first_frame, seed


def skeleton_sample(upward, valid, taps, parents, index, kind, frames, voxels, grid, radius, floor, samples, first_sample=0,
                    first_frame=0, seed=0, scratch=None):
    """se_skeleton_sample_f32: ``samples`` poses per frame, drawn joint by joint down the tree ``parents`` from ``upward`` [frames, J,
    voxels] (``skeleton_upward``'s) with the shell taps ``taps`` on the device (the header states the definition).  ``valid`` None
    (every frame is valid) or int32 [frames].  ``index`` and ``kind`` [samples, frames, J] int32 are written.  ``first_sample`` and
    ``first_frame``: the global index of the call's first sample and frame (the random numbers depend on the global indices alone);
    ``seed``: 0..2^64-1, split into the two key words.  ``scratch``: an optional uint8 workspace of at least
    ``skeleton_sample_scratch_bytes(frames, J, grid)`` bytes, 8-byte aligned.  Every argument is checked here and a bad one raises
    HipExtensionError before anything is launched: the kernels trust the sizes they are given."""
    what = "skeleton_sample"
    parents, J, frames, voxels, grid, radius, floor = _tree_args(what, parents, frames, voxels, grid, radius, floor)
    samples, first_sample, first_frame, seed = _sample_args(what, samples, frames, first_sample, first_frame, seed)
    dev = _check_args(what, (("upward", upward, torch.float32, frames * J * voxels),
                             ("taps", taps, torch.float32, J * (2 * radius + 1) ** 3),
                             ("index", index, torch.int32, samples * frames * J), ("kind", kind, torch.int32, samples * frames * J)),
                      (("valid", valid, torch.int32, frames), ("scratch", scratch, torch.uint8, None)))
    if _overlap(index, kind) or _overlap(index, upward) or _overlap(kind, upward):
        raise HipExtensionError(f"{what}: index, kind and upward must not alias")
    scratch = _scratch(what, scratch, skeleton_sample_scratch_bytes(frames, J, grid), torch.uint8, dev)
    if scratch.data_ptr() % 8:
        raise HipExtensionError(f"{what}: scratch must be 8-byte aligned")
    par = (ctypes.c_int * J)(*parents)
    _check(load().se_skeleton_sample_f32(_ptr(upward), _ptr(valid), _ptr(taps), ctypes.cast(par, ctypes.c_void_p), _ptr(index),
                                         _ptr(kind), _ptr(scratch), scratch.numel(), frames, J, voxels, grid, radius, floor, samples,
                                         first_sample, first_frame, seed & 0xFFFFFFFF, seed >> 32, _stream()),
           "se_skeleton_sample_f32")
    return index, kind


# ----------------------------------------------------------------------------------------------------------------------------------
# Most probable pose (csrc/skeleton_pose.hip; sceneego_amd/skeleton_pose.py drives it)
def _shell_rows(what, rows, grid, radius, taps):
    if not 1 <= rows <= 65535:
        raise HipExtensionError(f"{what}: rows = {rows} (1..65535) expected")
    _skeleton_shape(what, grid, radius)
    tap_rows = int(taps.shape[0]) if isinstance(taps, torch.Tensor) and taps.dim() == 2 else 0
    if not 1 <= tap_rows <= 65535:
        raise HipExtensionError(f"{what}: taps must be a [1..65535, {(2 * radius + 1) ** 3}] tensor")
    return tap_rows


def shell_maxcorr(a, taps, tap_row, out, rows, grid, radius, scale_mul=1.0, scratch=None):
    """se_shell_maxcorr_f32: ``out[r](x) = scale_mul * max over the non-zero taps d of a[r](x + d) taps[tap_row[r]](d)`` for the ``rows``
    volumes ``a`` [rows, grid^3] (the header states it); ``taps`` [tap_rows, (2 radius + 1)^3] float32 and ``tap_row`` [rows] int32 on
    the device.  ``scratch``: an optional uint8 workspace of at least ``shell_correlate_scratch_bytes(tap_rows, radius)`` bytes.  Every
    argument is checked here and a bad one raises HipExtensionError before anything is launched."""
    what = "shell_maxcorr"
    rows, grid, radius, scale_mul = int(rows), int(grid), int(radius), float(scale_mul)
    tap_rows = _shell_rows(what, rows, grid, radius, taps)
    voxels, block = grid ** 3, (2 * radius + 1) ** 3
    dev = _check_args(what, (("a", a, torch.float32, rows * voxels), ("taps", taps, torch.float32, (None, block)),
                             ("tap_row", tap_row, torch.int32, rows), ("out", out, torch.float32, rows * voxels)),
                      (("scratch", scratch, torch.uint8, None),))
    if _overlap(out, a):
        raise HipExtensionError(f"{what}: out must not alias a")
    scratch = _scratch(what, scratch, shell_correlate_scratch_bytes(tap_rows, radius), torch.uint8, dev)
    _check(load().se_shell_maxcorr_f32(_ptr(a), _ptr(taps), _ptr(tap_row), _ptr(out), _ptr(scratch), scratch.numel(), rows, tap_rows,
                                       grid, radius, scale_mul, _stream()), "se_shell_maxcorr_f32")
    return out


def shell_argmax(a, taps, tap_row, query, out_tap, out_value, rows, grid, radius):
    """se_shell_argmax_i32: per row of ``a`` [rows, grid^3] and per voxel of ``query`` [queries] int32 the lowest tap index that attains
    the maximum ``shell_maxcorr`` takes there (-1: none) into ``out_tap`` [rows, queries] int32 and that maximum into ``out_value``
    [rows, queries] float32.  Every argument is checked here and a bad one raises HipExtensionError before anything is launched."""
    what = "shell_argmax"
    rows, grid, radius = int(rows), int(grid), int(radius)
    tap_rows = _shell_rows(what, rows, grid, radius, taps)
    queries = int(query.numel()) if isinstance(query, torch.Tensor) else 0
    if queries < 1:
        raise HipExtensionError(f"{what}: query must hold at least one voxel")
    voxels, block = grid ** 3, (2 * radius + 1) ** 3
    _check_args(what, (("a", a, torch.float32, rows * voxels), ("taps", taps, torch.float32, (None, block)),
                       ("tap_row", tap_row, torch.int32, rows), ("query", query, torch.int32, queries),
                       ("out_tap", out_tap, torch.int32, rows * queries), ("out_value", out_value, torch.float32, rows * queries)))
    _check(load().se_shell_argmax_i32(_ptr(a), _ptr(taps), _ptr(tap_row), _ptr(query), _ptr(out_tap), _ptr(out_value), rows, queries,
                                      tap_rows, grid, radius, _stream()), "se_shell_argmax_i32")
    return out_tap, out_value


def skeleton_pose_scratch_bytes(frames, joints, grid, radius) -> int:
    return int(load().se_skeleton_pose_scratch_bytes(int(frames), int(joints), int(grid), int(radius)))


def skeleton_pose(prob, taps, parents, index, jumped, exponent, best_root, solved, frames, voxels, grid, radius, floor, scratch=None):
    """se_skeleton_pose_f32: the max-product pass over the tree ``parents`` (as for ``skeleton_couple``) on ``prob`` [frames, J, voxels]
    with the shell taps ``taps`` [J, (2 radius + 1)^3] on the device (the header states the definition).  ``index``, ``jumped`` and
    ``exponent`` [frames, J] int32, ``best_root`` [frames] float32 and ``solved`` [frames] int32 are written.  ``scratch``: an optional
    uint8 workspace of at least ``skeleton_pose_scratch_bytes(frames, J, grid, radius)`` bytes.  Every argument is checked here and a
    bad one raises HipExtensionError before anything is launched: the kernels trust the sizes they are given."""
    what = "skeleton_pose"
    parents, J, frames, voxels, grid, radius, floor = _tree_args(what, parents, frames, voxels, grid, radius, floor)
    dev = _check_args(what, (("prob", prob, torch.float32, frames * J * voxels), ("taps", taps, torch.float32, J * (2 * radius + 1) ** 3),
                             ("index", index, torch.int32, frames * J), ("jumped", jumped, torch.int32, frames * J),
                             ("exponent", exponent, torch.int32, frames * J), ("best_root", best_root, torch.float32, frames),
                             ("solved", solved, torch.int32, frames)), (("scratch", scratch, torch.uint8, None),))
    scratch = _scratch(what, scratch, skeleton_pose_scratch_bytes(frames, J, grid, radius), torch.uint8, dev)
    par = (ctypes.c_int * J)(*parents)
    _check(load().se_skeleton_pose_f32(_ptr(prob), _ptr(taps), ctypes.cast(par, ctypes.c_void_p), _ptr(index), _ptr(jumped),
                                       _ptr(exponent), _ptr(best_root), _ptr(solved), _ptr(scratch), scratch.numel(), frames, J, voxels,
                                       grid, radius, floor, _stream()), "se_skeleton_pose_f32")
    return index, jumped, exponent, best_root, solved


ALTERNATIVES_OUTPUTS = ("index", "jumped", "exponent", "best_root", "solved", "down_exponent", "mm_best", "pose_value", "alt_value",
                        "mm_peak", "alt_index", "alt_pose", "alt_jumped", "complete")


def skeleton_alternatives_scratch_bytes(frames, joints, grid, radius) -> int:
    return int(load().se_skeleton_alternatives_scratch_bytes(int(frames), int(joints), int(grid), int(radius)))


def skeleton_alternatives(prob, taps, parents, separation, index, jumped, exponent, best_root, solved, down_exponent, mm_best, pose_value,
                          alt_value, mm_peak, alt_index, alt_pose, alt_jumped, complete, frames, voxels, grid, radius, floor,
                          max_marginals=None, scratch=None):
    """se_skeleton_alternatives_f32: the upward pass of ``skeleton_pose`` and the downward max-product pass behind it (the header
    states the definition), with the window half-width ``separation`` (an int >= 0).  Written: ``index``, ``jumped``, ``exponent``
    [frames, J] int32, ``best_root`` [frames] float32 and ``solved`` [frames] int32 as by ``skeleton_pose``; ``down_exponent``,
    ``mm_peak``, ``alt_index`` [frames, J] int32; ``mm_best``, ``pose_value``, ``alt_value`` [frames, J] float32; ``alt_pose``,
    ``alt_jumped`` [frames, J, J] int32; ``complete`` [frames] int32; ``max_marginals`` None or [frames, J, voxels] float32.
    ``scratch``: an optional uint8 workspace of at least ``skeleton_alternatives_scratch_bytes(frames, J, grid, radius)`` bytes.  Every
    argument is checked here and a bad one raises HipExtensionError before anything is launched."""
    what = "skeleton_alternatives"
    parents, J, frames, voxels, grid, radius, floor = _tree_args(what, parents, frames, voxels, grid, radius, floor)
    if isinstance(separation, bool) or not isinstance(separation, numbers.Integral) or separation < 0:
        raise HipExtensionError(f"{what}: separation = {separation!r} (an integer >= 0) expected")
    i32, f32, FJ = torch.int32, torch.float32, frames * J
    dev = _check_args(what, (("prob", prob, f32, FJ * voxels), ("taps", taps, f32, J * (2 * radius + 1) ** 3),
                             ("index", index, i32, FJ), ("jumped", jumped, i32, FJ), ("exponent", exponent, i32, FJ),
                             ("best_root", best_root, f32, frames), ("solved", solved, i32, frames),
                             ("down_exponent", down_exponent, i32, FJ), ("mm_best", mm_best, f32, FJ), ("pose_value", pose_value, f32, FJ),
                             ("alt_value", alt_value, f32, FJ), ("mm_peak", mm_peak, i32, FJ), ("alt_index", alt_index, i32, FJ),
                             ("alt_pose", alt_pose, i32, FJ * J), ("alt_jumped", alt_jumped, i32, FJ * J),
                             ("complete", complete, i32, frames)),
                      (("max_marginals", max_marginals, f32, FJ * voxels), ("scratch", scratch, torch.uint8, None)))
    if max_marginals is not None and _overlap(max_marginals, prob):
        raise HipExtensionError(f"{what}: max_marginals must not alias prob")
    scratch = _scratch(what, scratch, skeleton_alternatives_scratch_bytes(frames, J, grid, radius), torch.uint8, dev)
    par = (ctypes.c_int * J)(*parents)
    _check(load().se_skeleton_alternatives_f32(_ptr(prob), _ptr(taps), ctypes.cast(par, ctypes.c_void_p), int(separation), _ptr(index),
                                               _ptr(jumped), _ptr(exponent), _ptr(best_root), _ptr(solved), _ptr(down_exponent),
                                               _ptr(mm_best), _ptr(pose_value), _ptr(alt_value), _ptr(mm_peak), _ptr(alt_index),
                                               _ptr(alt_pose), _ptr(alt_jumped), _ptr(complete), _ptr(max_marginals), _ptr(scratch),
                                               scratch.numel(), frames, J, voxels, grid, radius, floor, _stream()),
           "se_skeleton_alternatives_f32")
    return index, jumped, exponent, best_root, solved


# ----------------------------------------------------------------------------------------------------------------------------------
# Baseline JPEG encoder (csrc/jpeg_enc.hip; sceneego_amd/jpeg_encode.py drives it)
def jpeg_encode_scratch_bytes(batch, height, width, subsampling) -> int:
    """se_jpeg_encode_scratch_bytes: device workspace of one encode call; ``subsampling`` is 444 or 420."""
    n = load().se_jpeg_encode_scratch_bytes(int(batch), int(height), int(width), int(subsampling))
    if n < 0:
        raise HipExtensionError(f"se_jpeg_encode_scratch_bytes: bad shape (batch {batch}, {height}x{width}, subsampling {subsampling})")
    return int(n)


def jpeg_encode(frames, quant_luma, quant_chroma, subsampling, restart_rows, out, length, status, scratch, bgr=False):
    """se_jpeg_encode_u8: frames uint8 [B,H,W,3] -> out uint8 [B,capacity] (the scan of every frame), length int32 [B], status int32
    [B,2]; ``quant_*``: numpy uint16 [64], natural order.  Runs on the current stream."""
    import numpy as np
    what = "jpeg_encode"
    _check_args(what, (("frames", frames, torch.uint8, (None, None, None, 3)),))
    B, H, W = frames.shape[:3]
    _check_args(what, (("out", out, torch.uint8, (B, None)), ("length", length, torch.int32, B), ("status", status, torch.int32, (B, 2)),
                       ("scratch", scratch, torch.uint8, None)), device=frames.device)
    ql = np.ascontiguousarray(quant_luma, dtype=np.uint16).reshape(64)
    qc = np.ascontiguousarray(quant_chroma, dtype=np.uint16).reshape(64)
    _check(load().se_jpeg_encode_u8(_ptr(frames), B, H, W, 1 if bgr else 0, ql.ctypes.data, qc.ctypes.data, int(subsampling),
                                    int(restart_rows), _ptr(out), out.shape[1], _ptr(length), _ptr(status), _ptr(scratch),
                                    scratch.numel(), _stream()), "se_jpeg_encode_u8")


# ----------------------------------------------------------------------------------------------------------------------------------
# Lossless PNG encoder (csrc/png_enc.hip; sceneego_amd/png_encode.py drives it)
def png_encode_scratch_bytes(batch, height, width, channels) -> int:
    """se_png_encode_scratch_bytes: device workspace of one encode call; ``channels`` is 3 (RGB) or 1 (gray)."""
    n = load().se_png_encode_scratch_bytes(int(batch), int(height), int(width), int(channels))
    if n < 0:
        raise HipExtensionError(f"se_png_encode_scratch_bytes: bad shape (batch {batch}, {height}x{width}, channels {channels})")
    return int(n)


def png_encode_bound(height, width, channels) -> int:
    """se_png_encode_bound: bytes no zlib stream of a frame of this shape exceeds; the capacity ``png_encode`` asks for."""
    n = load().se_png_encode_bound(int(height), int(width), int(channels))
    if n < 0:
        raise HipExtensionError(f"se_png_encode_bound: bad shape ({height}x{width}, channels {channels})")
    return int(n)


def png_encode(frames, out, length, status, scratch):
    """se_png_encode_u8: frames uint8 [B,H,W,3] or [B,H,W] -> out uint8 [B,capacity] (the zlib stream of every frame), length int32
    [B], status int32 [B,2].  Runs on the current stream."""
    what = "png_encode"
    _check_args(what, (("frames", frames, torch.uint8, None),))
    if frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
        raise HipExtensionError(f"{what}: frames has shape {tuple(frames.shape)}, expected [B,H,W,3] or [B,H,W]")
    B, H, W = frames.shape[:3]
    _check_args(what, (("out", out, torch.uint8, (B, None)), ("length", length, torch.int32, B), ("status", status, torch.int32, (B, 2)),
                       ("scratch", scratch, torch.uint8, None)), device=frames.device)
    _check(load().se_png_encode_u8(_ptr(frames), _ptr(out), _ptr(length), _ptr(status), _ptr(scratch), scratch.numel(), B, H, W,
                                   3 if frames.dim() == 4 else 1, out.shape[1], _stream()), "se_png_encode_u8")
