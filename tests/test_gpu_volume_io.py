"""GPU: the kernels that build the V2V input and read its output - voxeliser, 4-tap gather, intersection, soft-argmax - through the C
ABI, against the float64 numpy models of tests/volume_io_model.py on the inputs of tests/volume_io_cases.py (small shapes that take the
paths the workload's own shape never takes; tests/test_volume_io_host.py shows on the CPU that the cases can tell a wrong kernel
from a right one).  Every output buffer is filled with a poison value before each call.

Every bound here is exact (bit for bit) or derived in the comment next to it; none is measured.  u = 2^-24 is the unit roundoff of
float32."""
import functools
import math

import numpy as np
import pytest
import torch

import volume_io_cases as C
import volume_io_model as M
from sceneego_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
POISON = -7.25                      # exact in float32 and bfloat16


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------------------------ voxeliser
@functools.lru_cache(maxsize=None)
def voxel_want(name):
    c = C.voxel_case(name) if name in C.VOXEL_CASES else C.voxel_full_case(name)
    return c, M.voxelize_model(c["depth"], c["ray"], c["up"], c["pad_x"], c["G"], c["side"])


def _vox_args(c):
    return dev(c["depth"]), dev(c["ray"]), c["B"], c["dh"], c["dw"], c["up"], c["pad_x"], c["G"], c["side"]


@pytest.mark.parametrize("name", list(C.VOXEL_CASES))
def test_voxelize_dense_bit_exact(name):
    c, occ = voxel_want(name)
    depth, ray, B, dh, dw, up, pad, G, side = _vox_args(c)
    out = torch.full((B, G, G, G), POISON, device=DEV)
    _lib.voxelize(depth, ray, out, B, dh, dw, up, pad, G, side)
    got = out.cpu().numpy()
    assert same_bits(got, M.place_dense(occ)), f"{int((got != occ).sum())} voxels differ"


@pytest.mark.parametrize("name", list(C.VOXEL_FULL_CASES))
def test_voxelize_full_bit_exact(name):
    c, occ = voxel_want(name)
    B, G = c["B"], c["G"]
    out = torch.full((B, G, G, G), POISON, device=DEV)
    _lib.voxelize_full(dev(c["depth"]), dev(c["ray"]), out, B, c["dh"], c["dw"], G, c["side"])
    got = out.cpu().numpy()
    assert same_bits(got, M.place_dense(occ)), f"{int((got != occ).sum())} voxels differ"


@pytest.mark.parametrize("stride_c,c_offset", [(12, 4), (16, 8), (8, 0)])
@pytest.mark.parametrize("name", list(C.VOXEL_CASES))
def test_voxelize_strided_clears_its_four_channels_and_nothing_else(name, stride_c, c_offset):
    c, occ = voxel_want(name)
    depth, ray, B, dh, dw, up, pad, G, side = _vox_args(c)
    start = np.full((B, G ** 3, stride_c), POISON, dtype=np.float32)
    buf = dev(start)
    _lib.voxelize_strided(depth, ray, buf, B, dh, dw, up, pad, G, side, stride_c, c_offset)
    assert same_bits(buf.cpu().numpy(), M.place_strided(start, occ, c_offset))


@pytest.mark.parametrize("triplets_total,channel", [(4, 10), (2, 5), (3, 0)])
@pytest.mark.parametrize("name", list(C.VOXEL_CASES))
def test_voxelize_planar3_scatters_only(name, triplets_total, channel):
    c, occ = voxel_want(name)
    depth, ray, B, dh, dw, up, pad, G, side = _vox_args(c)
    start = np.full((B, triplets_total, G ** 3, 3), POISON, dtype=np.float32)
    buf = dev(start)
    _lib.voxelize_planar3(depth, ray, buf, B, dh, dw, up, pad, G, side, triplets_total, channel)
    assert same_bits(buf.cpu().numpy(), M.place_planar3(start, occ, channel))


@pytest.mark.parametrize("planes_total,channel", [(5, 3), (1, 0), (4, 3)])
@pytest.mark.parametrize("name", list(C.VOXEL_CASES))
def test_voxelize_planar1_scatters_only(name, planes_total, channel):
    c, occ = voxel_want(name)
    depth, ray, B, dh, dw, up, pad, G, side = _vox_args(c)
    start = np.full((B, planes_total, G ** 3), POISON, dtype=np.float32)
    buf = dev(start)
    _lib.voxelize_planar1(depth, ray, buf, B, dh, dw, up, pad, G, side, planes_total, channel)
    assert same_bits(buf.cpu().numpy(), M.place_planar1(start, occ, channel))


@pytest.mark.parametrize("octs_total,c_offset", [(3, 16), (3, 8), (1, 0)])
@pytest.mark.parametrize("name", list(C.VOXEL_CASES))
def test_voxelize_bf16_clears_its_octet_and_nothing_else(name, octs_total, c_offset):
    c, occ = voxel_want(name)
    depth, ray, B, dh, dw, up, pad, G, side = _vox_args(c)
    buf = torch.full((B, octs_total, G ** 3, 8), POISON, device=DEV, dtype=torch.bfloat16)
    start = buf.view(torch.int16).cpu().numpy().view(np.uint16)
    _lib.voxelize_strided(depth, ray, buf, B, dh, dw, up, pad, G, side, octs_total * 8, c_offset)
    got = buf.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, M.place_octet_bf16(start, occ, c_offset))


# ------------------------------------------------------------------------------------------------------------------ gather
def gather_inputs(B, texels, channels, voxels):
    idx, w = C.gather_table(voxels, texels)
    return C.gather_feat(B, texels, channels), idx, w


def run_gather_cl(feat, idx, w, stride_c, c_offset):
    B, texels, channels = feat.shape
    voxels = idx.shape[0]
    out = torch.full((B, voxels, stride_c), POISON, device=DEV)
    _lib.unproject_gather(dev(feat), dev(idx), dev(w), out, B, texels, channels, voxels, stride_c, c_offset)
    return out.cpu().numpy()


def check_gather(got, feat, idx, w):
    """|got - want64| <= 4 u S + 2^-149: four float32 multiply-adds (fused or not) into a sum of four terms - each term passes through at
    most four roundings, each relative to a partial sum of magnitude <= S = sum |feat * w|; 2^-149 covers an underflowing product."""
    want, S = M.gather_model(feat, idx, w)
    err = np.abs(got.astype(np.float64) - want)
    bound = 4 * U * S + 2.0 ** -149
    worst = float((err / bound).max())
    print(f"gather error / bound = {worst:.3e}")
    assert worst <= 1.0
    assert (got[:, (idx < 0).all(axis=1)] == 0).all()                 # no live tap: exactly zero


@pytest.mark.parametrize("B,texels,channels,voxels,stride_c,c_offset", C.GATHER_CL_CASES)
def test_gather_channels_last_vs_float64(B, texels, channels, voxels, stride_c, c_offset):
    feat, idx, w = gather_inputs(B, texels, channels, voxels)
    got = run_gather_cl(feat, idx, w, stride_c, c_offset)
    check_gather(got[:, :, c_offset:c_offset + channels], feat, idx, w)
    rest = np.ones(stride_c, dtype=bool)
    rest[c_offset:c_offset + channels] = False
    assert (got[:, :, rest] == np.float32(POISON)).all()              # channels outside the written range keep the poison


@pytest.mark.parametrize("B,texels,channels,voxels,triplets_total,planes_total", C.GATHER_PLANAR_CASES)
def test_gather_planar_forms_bit_equal_channels_last_and_zero_their_spare_slots(B, texels, channels, voxels, triplets_total, planes_total):
    feat, idx, w = gather_inputs(B, texels, channels, voxels)
    cl = run_gather_cl(feat, idx, w, channels, 0)
    check_gather(cl, feat, idx, w)
    args = (dev(feat), dev(idx), dev(w))
    p3 = torch.full((B, triplets_total, voxels, 3), POISON, device=DEV)
    _lib.unproject_gather_planar3(*args, p3, B, texels, channels, voxels, triplets_total)
    # The spare slots of the last triplet the channels reach are exactly (+)zero.  Triplets beyond it (triplets_total > ceil(channels / 3))
    # are left alone: that is the entry point's stated contract (include/sceneego_hip.h) and tests/test_gpu_kernels.py holds it at 64^3.
    T = (channels + 2) // 3
    got3 = p3.cpu().numpy()
    assert same_bits(got3[:, :T], M.to_planar3(cl, T, 0.0))
    assert (got3[:, T:] == np.float32(POISON)).all()
    p1 = torch.full((B, planes_total, voxels), POISON, device=DEV)
    _lib.unproject_gather_planar1(*args, p1, B, texels, channels, voxels, planes_total)
    assert same_bits(p1.cpu().numpy(), M.to_planar1(cl, planes_total, 0.0))


@pytest.mark.parametrize("B,texels,channels,voxels,octs_total,c_offset", C.GATHER_BF16_CASES)
def test_gather_bf16_is_the_float32_value_rounded_once(B, texels, channels, voxels, octs_total, c_offset):
    feat, idx, w = gather_inputs(B, texels, channels, voxels)
    cl = run_gather_cl(feat, idx, w, channels, 0)
    check_gather(cl, feat, idx, w)
    out = torch.full((B, octs_total, voxels, 8), POISON, device=DEV, dtype=torch.bfloat16)
    want = out.view(torch.int16).cpu().numpy().view(np.uint16).copy()
    _lib.unproject_gather(dev(feat), dev(idx), dev(w), out, B, texels, channels, voxels, octs_total * 8, c_offset)
    o0, n = c_offset // 8, channels // 8
    want[:, o0:o0 + n] = M.bf16_round(cl).reshape(B, voxels, n, 8).transpose(0, 2, 1, 3)
    assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), want)


# ------------------------------------------------------------------------------------------------------------------ intersection
@pytest.mark.parametrize("B,voxels,channels,stride_c", C.INTERSECTION_CASES)
def test_intersection_is_one_float32_multiply_and_leaves_the_tail(B, voxels, channels, stride_c):
    from sceneego_amd import synth
    start = synth.normal(60 + B, "viog/ibuf/%d" % voxels, (B, voxels, stride_c))
    occ = synth.uniform(61 + B, "viog/iocc/%d" % voxels, (B, voxels), -2.0, 2.0)
    occ.reshape(-1)[::5] = 0.0
    occ.reshape(-1)[1::7] = 1.0
    buf = dev(start)
    _lib.intersection(buf, dev(occ), B, voxels, channels, stride_c)
    assert same_bits(buf.cpu().numpy(), M.intersection_model(start, occ, channels))


# ------------------------------------------------------------------------------------------------------------------ soft-argmax
def run_softargmax(logits, coord, mode):
    rows, N = logits.shape
    vol, c = dev(logits), dev(coord)
    out = torch.full((rows, N), POISON, device=DEV)
    joints = torch.full((rows, 3), POISON, device=DEV)
    scratch = torch.full((_lib.softargmax3d_scratch_elems(rows),), float("nan"), device=DEV)
    _lib.softargmax3d(vol, c, out, joints, rows, N, mode, scratch)
    torch.cuda.synchronize()
    return {"vol": out.cpu().numpy(), "joints": joints.cpu().numpy(), "scratch": scratch, "logits_dev": vol}


def check_softargmax(got, logits, coord, mode, tag, rows_to_check=None):
    """Float32 summation bounds from the shape of the sums (csrc/softargmax.hip), first order in u, + 1 for the higher orders.

    A term e_i * c_i of a joint's numerator passes through: its product (1 rounding), the sum of the four products of an iteration (3),
    n_it = ceil(chunk / 1024) serial additions of a lane, 8 levels of the workgroup tree, the product with the chunk's weight (1), at most
    4 serial additions of the fold and 6 levels of its butterfly: T = n_it + 23 roundings, each relative to a partial sum of magnitude
    <= A = sum p |c|.  The denominator L likewise (T roundings at most), which moves the joint J by T u |J|; 1 / L and the product with it: 2 u |J|.
    The weights themselves: e_i = expf(x_i - m) and f = expf(m - M) are two calls of <= 1 ulp = 2 u each (the HIP math library's stated
    accuracy of expf), and their arguments are rounded differences, off by u |x_i - m| and u |m - M|, which moves exp by the same
    relative amount: together u (M - x_i), since x_i <= m <= M.  Weighted like the sums, that is u Dc = u sum p |c| (M - x) in the
    numerator and u D |J| through the denominator (both from the float64 model; they are properties of the logits).  Hence
        |dJ| <= u ((T + 4 + 2 + 1) (A + |J|) + Dc + |J| D)                mode 1
        |dJ| <= u (T + 1) (A + |J|)                                        mode 0 (no exp, no division)
    A probability p_i = expf(x_i - M) * (1 / L): argument u (M - x_i) with p_i (M - x_i) <= peak / e, expf 2 u, the product u, 1 / L u,
    and L's own error (T + 4 + D) u:  |dp_i| <= u peak (T + D + 9 + 1) + 2^-126 (a flushed subnormal).  Mode 0 volumes are relu, exact.
    At 64^3 and 15 rows (T = 24, D of a few units, A + |J| <= 4 m) the joint bound is ~1e-5 m: far inside the 3e-4 m that
    tests/test_gpu_kernels.py holds at that shape; asserted below for every case as well."""
    rows, N = logits.shape
    m = M.softargmax_model(logits, coord, mode)
    sel = np.arange(rows) if rows_to_check is None else np.asarray(rows_to_check)
    T = math.ceil(C.sa_chunk(rows, N) / 1024) + 23
    J, A = m["joints"][sel], m["A"][sel]
    if mode == 1:
        jb = U * ((T + 7) * (A + np.abs(J)) + m["Dc"][sel] + np.abs(J) * m["D"][sel][:, None]) + 2.0 ** -126
        vb = (U * m["peak"][sel] * (T + m["D"][sel] + 10) + 2.0 ** -126)[:, None]
    else:
        jb = U * (T + 1) * (A + np.abs(J)) + 2.0 ** -126
        vb = np.zeros((len(sel), 1))
    assert np.isfinite(got["joints"][sel]).all() and np.isfinite(got["vol"][sel]).all(), tag
    jr = float((np.abs(got["joints"][sel].astype(np.float64) - J) / jb).max())
    verr = np.abs(got["vol"][sel].astype(np.float64) - m["vol"][sel])
    vr = float((verr / np.maximum(vb, 2.0 ** -149)).max()) if mode == 1 else float(verr.max())
    print(f"{tag}: joint error / bound = {jr:.3e}, volume error / bound = {vr:.3e}, largest joint bound = {float(jb.max()):.3e}")
    assert jr <= 1.0, f"{tag}: a joint misses its float32 summation bound by {jr:.3f}x"
    if mode == 1:
        assert vr <= 1.0, f"{tag}: a probability misses its bound by {vr:.3f}x"
        assert float(jb.max()) < 3e-4
    else:
        assert same_bits(got["vol"][sel], np.maximum(logits[sel], np.float32(0)))
    return m


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("rows,voxels", C.SA_RANDOM_CASES)
def test_softargmax_random_logits_vs_float64(rows, voxels, mode):
    lg, coord = C.sa_random(rows, voxels), C.sa_coord(voxels)
    check_softargmax(run_softargmax(lg, coord, mode), lg, coord, mode, f"rows {rows} voxels {voxels} mode {mode}")


@pytest.mark.parametrize("rows,voxels", C.SA_SPIKE_CASES)
def test_softargmax_spike_returns_its_voxel(rows, voxels):
    """One logit of +80 over a non-positive background: every other term is below e^-80 of the spike's, whose own weight is
    expf(0) = 1 exactly, so the joint is the spike's coordinate and its probability 1, to 2^-22 relative, wherever in its chunk,
    its quad and its row the spike sits."""
    lg, pos = C.sa_spike(rows, voxels)
    coord = C.sa_coord(voxels)
    got = run_softargmax(lg, coord, 1)
    want = coord[pos].astype(np.float64)
    assert (np.abs(got["joints"].astype(np.float64) - want) <= 2.0 ** -22 * np.abs(want)).all()
    r = np.arange(rows)
    assert (np.abs(got["vol"][r, pos].astype(np.float64) - 1.0) <= 2.0 ** -22).all()
    rest = got["vol"].copy()
    rest[r, pos] = 0
    assert float(rest.max()) <= 1e-30 and float(rest.min()) >= 0.0


@pytest.mark.parametrize("rows,voxels", C.SA_NEGINF_CASES)
def test_softargmax_neg_inf_logits_have_probability_zero_and_leave_the_row_finite(rows, voxels):
    """-inf logits scattered, filling one whole chunk of the split row, and all of a row but one voxel: finite rows (as
    torch.softmax), exactly 0 at the -inf voxels, joints inside the bound of the random family.
    (Before the fix of softargmax_partial_kernel a chunk of nothing but -inf gave expf(-inf - -inf) = NaN and NaN * 0 poisoned the row.)"""
    lg, coord = C.sa_neginf(rows, voxels), C.sa_coord(voxels)
    got = run_softargmax(lg, coord, 1)
    assert np.isfinite(torch.softmax(torch.from_numpy(lg), dim=1).numpy()).all()
    check_softargmax(got, lg, coord, 1, f"-inf rows {rows} voxels {voxels}")
    assert (got["vol"][np.isneginf(lg)] == 0).all()


def test_softargmax_all_neg_inf_row_and_nan_rows_are_nan_as_in_torch():
    lg, nan_rows = C.sa_nan_rows()
    coord = C.sa_coord(lg.shape[1])
    got = run_softargmax(lg, coord, 1)
    want = torch.softmax(torch.from_numpy(lg), dim=1).numpy()
    assert np.array_equal(np.isnan(got["vol"]), np.isnan(want))
    bad = list(nan_rows)
    assert np.isnan(got["vol"][bad]).all() and np.isnan(got["joints"][bad]).all()
    ok = [r for r in range(lg.shape[0]) if r not in nan_rows]
    check_softargmax(got, lg, coord, 1, "rows beside NaN rows", rows_to_check=ok)
    assert (got["vol"][12, 0:4] == 0).all()


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("rows,voxels", [(15, 1000), (120, 1000), (60, 13824)])
def test_softargmax_finish_alone_reproduces_the_two_pass_result(rows, voxels, mode):
    """se_softargmax3d_finish_f32 on the partial records se_softargmax3d_f32 wrote: bit-identical joints and volumes."""
    lg, coord = C.sa_random(rows, voxels), C.sa_coord(voxels)
    first = run_softargmax(lg, coord, mode)
    out = torch.full((rows, voxels), POISON, device=DEV)
    joints = torch.full((rows, 3), POISON, device=DEV)
    _lib.softargmax3d_finish(first["logits_dev"], first["scratch"], out, joints, rows, voxels, mode)
    assert same_bits(out.cpu().numpy(), first["vol"]) and same_bits(joints.cpu().numpy(), first["joints"])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_anything_is_launched():
    """SE_ERR_BAD_ARG (-1) of the entry points; null pointers throughout: a refused call launches nothing."""
    lib = _lib.load()
    N = None
    # se_unproject_gather_f32(feat, idx, w, out, batch, texels, channels, voxels, out_stride_c, out_c_offset, stream)
    assert lib.se_unproject_gather_f32(N, N, N, N, 1, 4, 8, 16, 12, 8, N) == -1          # out_c_offset + channels > out_stride_c
    assert lib.se_unproject_gather_f32(N, N, N, N, 1, 4, 4, 16, 12, 2, N) == -1          # misaligned offset
    assert lib.se_unproject_gather_f32(N, N, N, N, 1, 4, 4, 16, 10, 0, N) == -1          # misaligned stride
    assert lib.se_unproject_gather_f32(N, N, N, N, 1, 4, 6, 16, 12, 0, N) == -1          # channels % 4
    # se_unproject_gather_planar{3,1}_f32(feat, idx, w, out, batch, texels, channels, voxels, total, stream): channels in {16, 32, 64} only
    for ch in (8, 24, 48, 128):
        assert lib.se_unproject_gather_planar3_f32(N, N, N, N, 1, 4, ch, 16, 64, N) == -1
        assert lib.se_unproject_gather_planar1_f32(N, N, N, N, 1, 4, ch, 16, 192, N) == -1
    assert lib.se_unproject_gather_planar3_f32(N, N, N, N, 1, 4, 32, 16, 10, N) == -1    # 3 * triplets_total < channels
    assert lib.se_unproject_gather_planar1_f32(N, N, N, N, 1, 4, 32, 16, 31, N) == -1    # planes_total < channels
    # se_voxelize_planar{3,1}_f64(depth, ray, buf, batch, dh, dw, up, pad_x, G, side, total, channel, stream)
    assert lib.se_voxelize_planar3_f64(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 2, 6, N) == -1    # channel >= 3 * triplets_total
    assert lib.se_voxelize_planar3_f64(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 2, -1, N) == -1
    assert lib.se_voxelize_planar1_f64(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 3, 3, N) == -1    # channel >= planes_total
    # se_voxelize_strided_f64(..., side, stride_c, c_offset, stream)
    assert lib.se_voxelize_strided_f64(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 8, 8, N) == -1    # c_offset + 4 > stride_c
    assert lib.se_voxelize_strided_f64(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 8, 2, N) == -1    # misaligned offset
    assert lib.se_voxelize_strided_f64(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 10, 4, N) == -1   # misaligned stride
    # se_voxelize_strided_bf16(..., side, octs_total, c_offset, stream)
    assert lib.se_voxelize_strided_bf16(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 2, 4, N) == -1   # c_offset % 8
    assert lib.se_voxelize_strided_bf16(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 2, 16, N) == -1  # octet beyond octs_total
    assert lib.se_voxelize_strided_bf16(N, N, N, 1, 4, 4, 4, 0, 4, 2.0, 0, 0, N) == -1
    # se_unproject_gather_bf16(feat, idx, w, out, batch, texels, channels, voxels, octs_total, out_c_offset, stream)
    assert lib.se_unproject_gather_bf16(N, N, N, N, 1, 4, 12, 16, 4, 0, N) == -1         # channels % 8
    assert lib.se_unproject_gather_bf16(N, N, N, N, 1, 4, 8, 16, 4, 4, N) == -1          # offset % 8
    assert lib.se_unproject_gather_bf16(N, N, N, N, 1, 4, 16, 16, 2, 8, N) == -1         # offset + channels > 8 * octs_total
    # se_intersection_f32(buf, occ, batch, voxels, channels, stride_c, stream)
    assert lib.se_intersection_f32(N, N, 1, 16, 8, 12, N) == -1                          # 2 * channels > stride_c
    assert lib.se_intersection_f32(N, N, 1, 16, 6, 16, N) == -1                          # channels % 4
    # se_softargmax3d_f32(vol, coord, out_vol, joints, scratch, rows, voxels, mode, stream) and its pass 2 alone
    assert lib.se_softargmax3d_f32(N, N, N, N, N, 1, 6, 1, N) == -1                      # voxels % 4
    assert lib.se_softargmax3d_f32(N, N, N, N, N, 1, 8, 2, N) == -1                      # mode 2
    assert lib.se_softargmax3d_f32(N, N, N, N, N, 0, 8, 1, N) == -1
    assert lib.se_softargmax3d_finish_f32(N, N, N, N, 1, 6, 1, N) == -1
    assert lib.se_softargmax3d_finish_f32(N, N, N, N, 1, 8, 2, N) == -1
