/*
 * sceneego_hip.h — C ABI of libsceneego_hip.so (gfx950 / MI355X).
 *
 * The SceneEgo reference (jianwang-mpi/SceneEgo) is pure Python and has no FFI / plugin registry:
 * its depth-aware voxel pose path dispatches ATen operators (and numpy for the voxeliser).  This
 * library is what stands in for those operator calls; each entry point below names the reference
 * call site (file:line, relative to the reference repo) it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes; no torch / HIP types in the signatures (`stream` is a hipStream_t
 *     passed as void*, NULL = default stream);
 *   - every pointer is DEVICE memory owned by the caller; nothing is allocated, freed or
 *     synchronised inside; launches are asynchronous on `stream` and hipGraph-capturable;
 *   - return value: 0 on success, otherwise the hipError_t of the failed call, or
 *     SE_ERR_BAD_ARG (-1) for an unsupported shape/argument (nothing is launched then);
 *   - activations are float32, channels-last: volumes are [B][Z][Y][X][C] ("NDHWC"; the reference's
 *     meshgrid order i,j,k of voxel_net_depth.py:117-121 is our Z,Y,X, flat voxel n = (i*G + j)*G + k),
 *     images are [B][H][W][C].
 *
 * Parity surface: every *_f32 / *_f64 entry point computes in the reference's arithmetic type and is covered by the
 * parity tests.  NOT part of the parity surface (opt-in, reduced precision, never selected by se_conv3d_f32 and never
 * part of bench.py's `value`): the *_bf16 entry points (bfloat16 storage, BASELINE configs[2]) and the three
 * se_conv3d_split3_* / se_conv3d_k3_split3_f32 entry points (EXPERIMENTAL: float32 tensors, 16-bit-mantissa products).
 */
#ifndef SCENEEGO_HIP_H
#define SCENEEGO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SE_ERR_BAD_ARG (-1)

/* epilogue flags of se_conv3d_f32 / se_deconv3d_k2s2_f32 */
#define SE_EPI_RELU          1   /* y = max(y, 0)                                                    */
#define SE_EPI_RES_PRE_RELU  2   /* y += residual BEFORE the ReLU  (Res3DBlock: relu(res + skip))     */
#define SE_EPI_RES_POST_RELU 4   /* y += residual AFTER the ReLU   (decoder: upsample(x) + skip_x)    */
#define SE_EPI_OUT_PLANAR    8   /* write [B][Cout][voxels] (NCDHW) instead of NDHWC                  */
#define SE_IN_PLANAR3        16  /* se_conv3d_f32, k = 7, cout = 16, dim % 8 == 0, no residual only: `in` is
                                  * triplet-planar [B][ceil(cin/3)][D][D][D][3] (channel c at triplet c/3,
                                  * slot c%3; slots >= cin must be finite) - see se_unproject_gather_planar3_f32 */
#define SE_IN_OCTET          32  /* se_conv3d_f32, k = 3 shapes with se_conv3d_f32_algo() == 2 only: `in` is octet-planar          */
#define SE_OUT_OCTET         64  /* [B][C/8][D][D][D][8] (channel c at octet c/8, slot c%8) / `out` is written that way /          */
#define SE_RES_OCTET         128 /* the skip tensor `residual` is read that way                                                 */
#define SE_EPI_SKIPCONV16    256 /* set by se_conv3d_skip16_f32 only (not a caller flag of se_conv3d_f32)                       */
#define SE_IN_QUAD           1024 /* se_conv3d_f32, k = 3 launches with se_conv3d_f32_variant(..., these flags) == 3 only: `in` is QUAD-planar   */
#define SE_OUT_QUAD          2048 /* [B][C/4][D][D][D][4] (channel c at quad c/4, slot c%4) / `out` is written that way /                     */
#define SE_RES_QUAD          4096 /* the skip tensor `residual` is read that way.  Quad- and octet-planar flags do not mix in one launch.    */
#define SE_LAYOUT_OCTET_BITS (SE_IN_OCTET | SE_OUT_OCTET | SE_RES_OCTET)
#define SE_LAYOUT_QUAD_BITS  (SE_IN_QUAD | SE_OUT_QUAD | SE_RES_QUAD)

/* ABI version; bumped on any signature change. */
int se_abi_version(void);

/* Occupancy voxeliser.  Replaces VoxelNetwork_depth.depth_map_to_voxel_numpy +
 * point_cloud_to_voxel_numpy (network/voxel_net_depth.py:194-222; per-sample host loop :252-255).
 *   depth    [B][depth_h][depth_w] float32 metres
 *   ray_tab  [up][up][3] float64: unit ray of padded-image pixel (x'+pad_x, y), indexed [y][x']
 *   occ      [B][G][G][G] float32, written as {0,1} (cleared inside)
 * Per pixel (y, x') of the `up` x `up` nearest-resized depth (src row floor(y*depth_h/up), src col
 * floor(x'*depth_w/up)): p = ray*d in float64; q = rint(((p.x+side/2)*G)/side, ((p.y+side/2)*G)/side,
 * (p.z*G)/side) (half-to-even, unfused); if 0<=q<=G-1 on all axes occ[qx][qy][qz] = 1.  If pad_x > 0
 * the zero-padded columns contribute the point (0,0,0).  Bit-exact with the reference.          */
int se_voxelize_f64(const float* depth, const double* ray_tab, float* occ,
                    int batch, int depth_h, int depth_w, int up, int pad_x,
                    int volume_size, double cuboid_side, void* stream);

/* Same, writing straight into the V2V input buffer buf [B][G^3][stride_c]: channels [c_offset, c_offset+4) of every voxel
 * are cleared, then channel c_offset receives the occupancy (replaces torch.stack/unsqueeze/cat,
 * network/voxel_net_depth.py:256-262, for the with_scene && !with_intersection case).                   */
int se_voxelize_strided_f64(const float* depth, const double* ray_tab, float* buf,
                            int batch, int depth_h, int depth_w, int up, int pad_x,
                            int volume_size, double cuboid_side, int stride_c, int c_offset, void* stream);

/* Same for a full-width depth map without resize/pad: dataset/real_depth_utils.py:29-60
 * (`voxel_output=True` path).  ray_tab [depth_h][depth_w][3] float64 indexed [y][x].            */
int se_voxelize_full_f64(const float* depth, const double* ray_tab, float* occ,
                         int batch, int depth_h, int depth_w,
                         int volume_size, double cuboid_side, void* stream);

/* Table-driven bilinear voxel gather.  Replaces nn.Upsample(1024^2) + ConstantPad2d(128) +
 * F.grid_sample (network/voxel_net_depth.py:60-61,238,243; utils/op.py:194-214) without the
 * 1024x1280 intermediate.
 *   feat [B][texels][channels] float32 (NHWC feature map, texels = H*W)
 *   idx  [voxels][4] int32 texel index per tap (-1 = zero tap), w [voxels][4] float32 tap weights
 *   out  [B][voxels][out_stride_c]; channels [out_c_offset, out_c_offset+channels) are written.
 * channels % 4 == 0, out_stride_c % 4 == 0, out_c_offset % 4 == 0.                                */
int se_unproject_gather_f32(const float* feat, const int* idx, const float* w, float* out,
                            int batch, int texels, int channels, int voxels,
                            int out_stride_c, int out_c_offset, void* stream);

/* with_intersection=True input assembly (network/voxel_net_depth.py:258-260): given vol channels
 * [0,c) already in `buf` [B][voxels][stride_c] and occ [B][voxels], writes buf[..., c:2c] = vol*occ. */
int se_intersection_f32(float* buf, const float* occ, int batch, int voxels, int channels,
                        int stride_c, void* stream);

/* Fused bias (+ residual) (+ ReLU) epilogue for the backbone's MIOpen 2D convolutions (BatchNorm folded into weight
 * and bias): replaces the bn / `out += residual` / relu element-wise passes of Bottleneck.forward
 * (network/pose_resnet.py:72-90).  x, residual (or NULL), out: [batch][channels][hw] float32, out may alias x. */
int se_bias_act_nchw_f32(const float* x, const float* bias, const float* residual, float* out,
                         int batch, int channels, int hw, int relu, void* stream);

/* Stem tail of the backbone in one pass: `bn1` (folded into conv1's weights: + bias), `relu` and `maxpool` (3x3, stride 2, padding 1),
 * network/pose_resnet.py:229-232, on the raw result of conv1: out = relu(max over the window (x) + bias[c]).
 * x [batch][channels][2 ho][2 wo], out [batch][channels][ho][wo] float32; wo % 4 == 0. */
int se_bias_relu_maxpool3x3s2_f32(const float* x, const float* bias, float* out, int batch, int channels, int ho, int wo, void* stream);

/* 1x1 convolution (stride 1) of the backbone as ONE float32 MFMA GEMM with its whole epilogue: replaces conv1 / conv3 / the stride-1
 * downsample of Bottleneck.forward with their BatchNorm (folded into w and bias), `out += residual` and the ReLU
 * (network/pose_resnet.py:72-90) - MIOpen's convolution plus the se_bias_act_nchw_f32 pass behind it (round 6; csrc/conv2d_1x1.hip).
 *   x [batch][cin][hw], residual (or NULL) / out [batch][cout][hw] float32 NCHW;  bias [cout]
 *   wpack = the folded [cout][cin] matrix as [cout / BC][cin / 16][BC][16] with BC = se_conv2d_1x1_tile_f32(batch, cin, cout, hw)
 *   (128 when cout % 128 == 0, else 64; 0 = shape not covered: cin % 16, cout % 64, hw % 16, batch * hw % 64 must be 0).
 *   in_bias (or NULL) [cin]: x is the RAW result of the producing convolution and its bias + ReLU are applied on the way in,
 *   x' = max(x + in_bias[c], 0) - conv2's `bn2` + `relu` (pose_resnet.py:79-81) folded into conv3's launch.
 * float32 in, float32 accumulate: differs from the MIOpen result by summation order only. */
int se_conv2d_1x1_tile_f32(int batch, int cin, int cout, int hw);
int se_conv2d_1x1_f32(const float* x, const float* wpack, const float* bias, const float* residual, const float* in_bias, float* out,
                      int batch, int cin, int cout, int hw, int relu, void* stream);

/* The same operator for the launches of batch 1-2 that would leave most CUs without a workgroup (64 - 1024 pixels against megabytes of
 * weights): 64 pixels x 16 channels per workgroup, the k steps over four / two wave groups.  wpack16 = [cout / 16][cin / 16][16][16];
 * cin % 64 == 0, cout % 16 == 0, hw % 16 == 0, batch * hw % 64 == 0 (SE_ERR_BAD_ARG otherwise).  Arguments as se_conv2d_1x1_f32. */
int se_conv2d_1x1_small_f32(const float* x, const float* wpack16, const float* bias, const float* residual, const float* in_bias, float* out,
                            int batch, int cin, int cout, int hw, int relu, void* stream);
/* ... stride 2: x [batch][cin][2 ho][2 wo] -> out [batch][cout][ho][wo]; the conditions above on (cin, cout, ho * wo), wo % 4 == 0. */
int se_conv2d_1x1_small_s2_f32(const float* x, const float* wpack16, const float* bias, float* out, int batch, int cin, int cout, int ho,
                               int wo, int relu, void* stream);

/* ... and its stride-2 form, the `downsample` convolution of a stage's first Bottleneck (network/pose_resnet.py:140-146):
 * x [batch][cin][2 ho][2 wo] -> out [batch][cout][ho][wo] = W x[:, :, ::2, ::2] + bias (+ ReLU); wpack / covered shapes as
 * se_conv2d_1x1_tile_f32(batch, cin, cout, ho * wo) says, wo % 4 == 0. */
int se_conv2d_1x1_s2_f32(const float* x, const float* wpack, const float* bias, float* out, int batch, int cin, int cout, int ho, int wo,
                         int relu, void* stream);

/* 3x3 convolution (stride 1, padding 1) of the backbone's deep stages as a direct float32 MFMA product: replaces conv2 (`conv3x3`,
 * network/pose_resnet.py:22-25) of the Bottlenecks of layer3 / layer4 with its folded BatchNorm (round 6; csrc/conv2d_3x3.hip).
 *   x [batch][cin][h][w], out [batch][cout][h][w] float32 NCHW; bias [cout] or NULL (the raw sums: the consumer adds it, see in_bias above)
 *   wpack = the folded [cout][cin][3][3] tensor as [cout / BC][cin / 16][9][BC][16] with BC = se_conv2d_3x3_tile_f32(batch, cin, cout, h, w)
 *   (32 or 16; 0 = shape not covered: cin % 32, cout % 32 must be 0 and the map 8k x 8m or 4k x 16m).
 * float32 in, float32 accumulate: differs from the MIOpen result by summation order only. */
int se_conv2d_3x3_tile_f32(int batch, int cin, int cout, int h, int w);
int se_conv2d_3x3_f32(const float* x, const float* wpack, const float* bias, float* out, int batch, int cin, int cout, int h, int w,
                      int relu, void* stream);

/* ... and its stride-2 form (conv2 of a stage's first Bottleneck): x [batch][cin][2 ho][2 wo] -> out [batch][cout][ho][wo], padding 1;
 * wpack = [cout / 16][cin / 16][9][16][16] (channel tile 16); cin % 32 == 0, cout % 16 == 0, output map 8k x 8m or 4k x 16m. */
int se_conv2d_3x3_s2_f32(const float* x, const float* wpack, const float* bias, float* out, int batch, int cin, int cout, int ho, int wo,
                         int relu, void* stream);

/* Output side of the 2-D pose head's transposed convolutions - ConvTranspose2d(k=4, s=2, p=1) + BatchNorm2d + ReLU,
 * network/pose_resnet.py:205-224 (built), :238 (run) - when the layer is computed as ONE GEMM over the un-shifted input:
 *   z    [batch][4 ky][4 kx][cout][h][w] = W_tap [cout x cin] @ x[b] [cin x h*w] for each of the 16 taps (any GEMM library;
 *        the host side uses rocBLAS through torch.matmul), BatchNorm scale folded into W
 *   out  [batch][cout][2h][2w] = bias[co] + the four taps that reach each output pixel (zero outside the map), ReLU if `relu`. */
int se_deconv2d_k4s2_assemble_f32(const float* z, const float* bias, float* out, int batch, int cout, int h, int w,
                                  int relu, void* stream);

/* Weight preparation: folds an eval-mode BatchNorm3d into the convolution and re-orders the weights
 * into the MFMA fragment order the conv kernels read (v_mfma_f32_16x16x4_f32 A-operand blocks).
 * Replaces nothing at run time in the reference — it is what makes Conv3d+BatchNorm3d(+ReLU)
 * (network/v2v.py:12-14,24-30,35-38,61-63) one kernel.
 *   w      Conv3d weight [cout][cin][k][k][k], or (transposed != 0) ConvTranspose3d weight [cin][cout][2][2][2]
 *   b      conv bias [cout] or NULL
 *   gamma,beta,mean,var  BatchNorm3d weight/bias/running_mean/running_var [cout], or all NULL (no BN)
 *   wpack  out, se_conv3d_packed_elems(...) floats;  bpack out, cout_pad floats (cout rounded up to 16)
 * cin_pad >= cin is the channel count of the activation tensor the conv will read (multiple of 16;
 * extra channels get zero weights).  The buffer's sections (A, B, E, F, G, H, I: one per kernel family that reads
 * the layer), their sizes and the value of every element: csrc/conv3d_pack.h; the kernels that write it:
 * csrc/conv3d_pack.hip.  se_conv3d_packed_elems is the sum of the sections the layer has.           */
int se_conv3d_pack_f32(const float* w, const float* b, const float* gamma, const float* beta,
                       const float* mean, const float* var, float eps,
                       float* wpack, float* bpack,
                       int cout, int cin, int cin_pad, int ksize, int transposed, void* stream);
long long se_conv3d_packed_elems(int cout, int cin_pad, int ksize, int transposed);

/* Conv3d (k = 1, 3 or 7, stride 1, zero padding (k-1)/2) + folded BN + epilogue.
 * Replaces Basic3DBlock / Res3DBlock convs and output_layer (network/v2v.py:8-43,161).
 *   in  [B][D][D][D][cin_pad]   out [B][D][D][D][cout] (or planar, SE_EPI_OUT_PLANAR)
 *       (flags & SE_IN_PLANAR3, k = 7 only: in is [B][ceil(cin/3)][D][D][D][3]; cin_pad then only names the packed weights)
 *   residual: same shape as out (NDHWC) or NULL.  cin = real input channels (<= cin_pad, the channel stride
 *   of `in`; channels [cin, cin_pad) must hold finite values, they meet zero weights); cin_pad % 16 == 0;
 *   cout % 16 == 0 unless planar.  Volumes with dim % 8 == 0 and dim >= 16 run the LDS-tiled kernels, everything
 *   else the direct kernel; results are identical in both up to float32 summation order.
 *   workspace (optional, may be NULL): `workspace_elems` floats of scratch; when given, small volumes
 *   (too few voxels to fill 256 CUs) split the 27 taps over extra workgroups and reduce the partial sums
 *   from the workspace in a fixed order (deterministic), and the 7^3 front layer of a launch with fewer than two
 *   tiles per CU (batch 1 at 64^3) splits every tile's 3-channel chunks between two workgroups - the second halves'
 *   sums pass through the first B * D^3 * 16 floats of the workspace and are added by a second kernel of the same
 *   call.  32 Mi floats cover every V2V level up to B = 64.  A workspace serves one stream at a time. */
int se_conv3d_f32(const float* in, const float* wpack, const float* bpack, const float* residual,
                  float* out, int batch, int dim, int cin, int cin_pad, int cout, int ksize, int flags,
                  float* workspace, long long workspace_elems, void* stream);

/* se_conv3d_f32 that also writes max_pool3d(out, kernel 2, stride 2) from the kernel's epilogue: `pool_out` is channels-last
 * [B][D/2][D/2][D/2][cout] float32.  Stands in for a Res3DBlock's last convolution followed by encoder_pool (reference
 * network/v2v.py:104-119) without re-reading the block output.  Only shapes with se_conv3d_f32_algo() == 2 (the 2-D Winograd
 * kernel) and cin_pad == cin; SE_ERR_BAD_ARG otherwise.  `out` is written as by se_conv3d_f32 (either layout). */
int se_conv3d_pool_f32(const float* in, const float* wpack, const float* bpack, const float* residual,
                       float* out, float* pool_out, int batch, int dim, int cin, int cin_pad, int cout, int ksize, int flags,
                       float* workspace, long long workspace_elems, void* stream);

/* 3x3x3 convolution + folded BN with the Res3DBlock's 1x1x1 skip convolution computed in the same launch (reference
 * network/v2v.py:21-43: res_branch's second convolution and skip_con of a block whose channel count changes):
 *     out = act( conv3(in; wpack) + skip_w . skip_in + bpack )
 * `skip_in` is the block input, 16 channels, channels-last [B][D][D][D][16] - or, with SE_RES_QUAD beside SE_IN_QUAD | SE_OUT_QUAD,
 * quad-planar [B][4][D][D][D][4] (what se_conv3d_k7_fft_f32 writes with SE_OUT_QUAD); `skip_w` its BN-folded weights [cout][16];
 * `bpack` must hold the SUM of both folded biases.  2-D Winograd shapes (se_conv3d_f32_algo() == 2) with octet-planar `in`
 * and `out` only (flags must carry SE_IN_OCTET | SE_OUT_OCTET, or SE_IN_QUAD | SE_OUT_QUAD where se_conv3d_f32_variant(..., those
 * flags) == 3; SE_EPI_RELU optional); SE_ERR_BAD_ARG otherwise.  Saves the
 * 1x1x1 launch, its output tensor and the skip-tensor read of the 3x3x3 convolution. */
int se_conv3d_skip16_f32(const float* in, const float* wpack, const float* bpack, const float* skip_in, const float* skip_w,
                         float* out, int batch, int dim, int cin, int cout, int flags, void* stream);

/* Fused V2V tail: two 1x1x1 32->32 convs (+BN+ReLU) and the 1x1x1 32->cout3 output layer in one pass
 * (network/v2v.py:155-161 back_layers.1/.2 + output_layer :161,169).  in [B][D]^3[32]; out planar [B][cout3][D^3];
 * wpackN / bpackN come from se_conv3d_pack_f32 (ksize 1, cin_pad 32); cout3 <= 16.                           */
int se_pointwise_chain3_f32(const float* in, const float* wpack1, const float* bpack1,
                            const float* wpack2, const float* bpack2, const float* wpack3, const float* bpack3,
                            float* out, int batch, int dim, int cout3, void* stream);

/* se_pointwise_chain3_f32 with pass 1 of se_softargmax3d_f32 (mode 1: softmax) folded in: the logits are written to `out` as
 * before and, while still in registers, reduced to the per-chunk partial records in `scratch`
 * (se_softargmax3d_scratch_elems(batch * cout3) floats).  `coord` = [dim^3][3] voxel-centre coordinates.  Finish with
 * se_softargmax3d_finish_f32(out, scratch, ...).  Replaces the back_layers / output_layer chain of network/v2v.py:155-161
 * together with the first half of utils/op.py:83-96.  flags: 0, or SE_IN_QUAD: `in` is quad-planar [B][8][dim^3][4] (what
 * back_layers.0's last convolution writes with SE_OUT_QUAD). */
int se_pointwise_chain3_softargmax_f32(const float* in, const float* wpack1, const float* bpack1, const float* wpack2,
                                       const float* bpack2, const float* wpack3, const float* bpack3, float* out,
                                       const float* coord, float* scratch, int batch, int dim, int cout3, int flags, void* stream);

/* ConvTranspose3d(k=2, s=2) + folded BN + ReLU (+ skip).  Replaces Upsample3DBlock and the decoder
 * adds (network/v2v.py:55-67,124-137).  in [B][D]^3[cin] -> out [B][2D]^3[cout]; residual [B][2D]^3[cout] (channels-last).
 * flags: SE_EPI_RELU, SE_EPI_RES_PRE_RELU / SE_EPI_RES_POST_RELU, and SE_OUT_QUAD (cin -> cout = 64 -> 32 or 128 -> 64, D % 16 == 0
 * only, else SE_ERR_BAD_ARG): `out` is written quad-planar [B][cout/4][2D][2D][2D][4], the input layout of the 3x3x3 kernel behind it;
 * SE_RES_QUAD (with SE_OUT_QUAD and SE_EPI_RES_POST_RELU only): `residual` is quad-planar [B][cout/4][2D][2D][2D][4] too. */
int se_deconv3d_k2s2_f32(const float* in, const float* wpack, const float* bpack, const float* residual,
                         float* out, int batch, int dim, int cin, int cout, int flags, void* stream);

/* F.max_pool3d(kernel 2, stride 2) (network/v2v.py:46-52).  in [B][D]^3[C] -> out [B][D/2]^3[C]. */
int se_maxpool3d_2_f32(const float* in, float* out, int batch, int dim, int channels, void* stream);
/* Same with an octet-planar input [B][channels/8][dim^3][8] (the output of an SE_OUT_OCTET convolution); out is channels-last. */
int se_maxpool3d_2_octin_f32(const float* in, float* out, int batch, int dim, int channels, void* stream);

/* 3D soft-argmax.  Replaces op.integrate_tensor_3d_with_coordinates (utils/op.py:83-96).
 *   vol    [rows][voxels] float32 (rows = B*joints, planar logits, already multiplied by volume_multiplier)
 *   coord  [voxels][3] float32 voxel-centre coordinates
 *   out_vol[rows][voxels] softmax(vol) (mode 1) or relu(vol) (mode 0)
 *   joints [rows][3] = sum_n out_vol[n] * coord[n]
 *   scratch: se_softargmax3d_scratch_elems(rows) floats of workspace.
 * Mode 1 treats non-finite logits as torch.softmax does: a -inf logit has probability exactly 0 and leaves the rest of its row
 * finite (also where it fills a whole chunk of the split row); a row of nothing but -inf, or one that holds a NaN, is NaN
 * throughout, joints included.                                                                      */
int se_softargmax3d_f32(const float* vol, const float* coord, float* out_vol, float* joints,
                        float* scratch, int rows, int voxels, int mode, void* stream);

/* Pass 2 of se_softargmax3d_f32 alone (softmaxed volumes + joints from the partial records in `scratch`). */
int se_softargmax3d_finish_f32(const float* vol, const float* scratch, float* out_vol, float* joints, int rows, int voxels,
                               int mode, void* stream);
long long se_softargmax3d_scratch_elems(int rows);

/* Per-joint statistics of the softmaxed volumes (no counterpart in the reference, which returns the volumes and leaves it at that).
 *   prob   [rows][voxels] float32 probabilities, as se_softargmax3d_f32 / se_softargmax3d_finish_f32 write them in mode 1
 *   coord  [voxels][3] float32 voxel-centre coordinates
 *   joints [rows][3] the soft-argmax joints
 *   stats  [rows][12]: 0..5  cxx cyy czz cxy cxz cyz, c_ab = sum_n p_n (c_na - j_a)(c_nb - j_b): the second central moment ABOUT
 *                            `joints` (m^2)
 *                      6     entropy -sum_n p_n ln p_n (nats; p_n == 0 contributes 0)
 *                      7     peak_p = max_n p_n
 *                      8..10 coord[peak_index]
 *                      11    sigma = sqrtf((cxx + cyy) + czz) (m)
 *   peak_index [rows] int32: the LOWEST flat index with p_n == peak_p
 *   scratch: se_joint_stats_scratch_elems(rows) floats of workspace.
 * A row that holds a NaN probability gets 12 NaNs and peak_index -1; other rows are unaffected.  Two launches on `stream`
 * (se_sa_splits(rows) chunks per row as the soft-argmax, then one wave per row), no atomics: bitwise identical from run to run.
 * Allocates nothing (legal inside hipGraph capture).  rows <= 0, rows > 65535, voxels <= 0, voxels & 3, a null pointer or a
 * prob / coord that is not 16-byte aligned -> SE_ERR_BAD_ARG.                                                                 */
int se_joint_stats_f32(const float* prob, const float* coord, const float* joints, float* stats, int* peak_index,
                       float* scratch, int rows, int voxels, void* stream);
long long se_joint_stats_scratch_elems(int rows);

/* Producers of the triplet-planar float32 V2V input [B][triplets_total][voxels][3] (SE_IN_PLANAR3; the 7^3 front layer
 * fetches its halo columns from ~5x fewer cache lines than from the channels-last record).  Same arithmetic, bit for bit, as
 * se_unproject_gather_f32 / se_voxelize_strided_f64.  The gather writes channels [0, channels) (channels = 16, 32 or 64) and
 * ZEROES the remaining slots of its last triplet; se_voxelize_planar3_f64 then only scatters 1.0 into slot `channel`
 * (it does not clear: call it after the gather, with channel in that cleared range, e.g. 32 for 32 feature channels).  */
int se_unproject_gather_planar3_f32(const float* feat, const int* idx, const float* w, float* out,
                                    int batch, int texels, int channels, int voxels, int triplets_total, void* stream);
int se_voxelize_planar3_f64(const float* depth, const double* ray_tab, float* buf, int batch, int depth_h, int depth_w,
                            int up, int pad_x, int volume_size, double cuboid_side,
                            int triplets_total, int channel, void* stream);

/* Producers of the fully PLANAR float32 V2V input [B][planes_total][voxels] (round 6: what se_conv3d_k7_fft_f32 reads).  Same
 * arithmetic, bit for bit, as se_unproject_gather_f32 / se_voxelize_strided_f64.  The gather writes planes [0, channels) (channels = 16,
 * 32 or 64) and ZEROES planes [channels, planes_total); se_voxelize_planar1_f64 then only scatters 1.0 into plane `channel` (call it
 * after the gather, with `channel` in that cleared range: 32 for 32 feature channels).  Reference call sites as for the planar3 pair. */
int se_unproject_gather_planar1_f32(const float* feat, const int* idx, const float* w, float* out,
                                    int batch, int texels, int channels, int voxels, int planes_total, void* stream);
int se_voxelize_planar1_f64(const float* depth, const double* ray_tab, float* buf, int batch, int depth_h, int depth_w,
                            int up, int pad_x, int volume_size, double cuboid_side,
                            int planes_total, int channel, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The 7x7x7 front layer in the frequency domain (round 6; csrc/conv3d_fft7.hip).  Same reference call site as se_conv3d_f32 with
 * ksize 7: Basic3DBlock(33 | 32 -> 16, 7) = Conv3d(k 7, pad 3) + BatchNorm3d + ReLU, network/v2v.py:8-18 (built :147, run :166).
 * Three launches per chunk of samples: a 24^3 real-to-complex DFT of every (16^3-output tile, input channel), one complex GEMM over the
 * channels per frequency on the matrix cores, the inverse DFT of every (tile, output channel) with bias and ReLU.  float32 throughout;
 * results differ from the direct convolution by float32 rounding of the transforms (~1e-6 of max|y|).
 *   in   PLANAR float32 [B][cin][D][D][D]  (se_unproject_gather_planar1_f32 / se_voxelize_planar1_f64 write it)
 *   out  channels-last [B][D][D][D][16], or with SE_OUT_QUAD quad-planar [B][4][D][D][D][4]; flags: SE_EPI_RELU, SE_OUT_QUAD only
 *   hfrag  se_conv3d_k7_fft_packed_elems(cin, cout) floats from se_conv3d_k7_fft_pack_f32: the weight spectra (BatchNorm scale folded
 *          in: gamma / var / eps as for se_conv3d_pack_f32, NULL = no BatchNorm) in MFMA fragment order;  bpack: the folded bias that
 *          se_conv3d_pack_f32 writes (16 floats)
 *   workspace  the spectra of one chunk of samples: se_conv3d_k7_fft_workspace_elems(n, dim, cin) floats hold n samples (0.19 GB per
 *          sample at 64^3); the call walks the batch in chunks of as many samples as the workspace holds (>= 1, else SE_ERR_BAD_ARG).
 *          A workspace serves one stream at a time.
 * Shapes: cin = 33 (features + occupancy) or 32 (`with_scene: False`), cout = 16, dim % 16 == 0; the *_elems functions return -1 and the calls SE_ERR_BAD_ARG for anything else
 * (se_conv3d_f32 serves those). */
long long se_conv3d_k7_fft_packed_elems(int cin, int cout);
int se_conv3d_k7_fft_pack_f32(const float* w, const float* gamma, const float* var, float eps, float* hfrag, int cout, int cin,
                              void* stream);
long long se_conv3d_k7_fft_workspace_elems(int batch, int dim, int cin);
int se_conv3d_k7_fft_f32(const float* in, const float* hfrag, const float* bpack, float* out, int batch, int dim, int cin, int cout,
                         int flags, float* workspace, long long workspace_elems, void* stream);

/* ------------------------------------------------------------------------------------------------
 * bf16-storage V2V (BASELINE config 3): activations and weights bfloat16 in HBM, float32 accumulation on
 * v_mfma_f32_16x16x32_bf16, float32 bias / BN shift, one round-to-nearest-even to bfloat16 per layer output.
 * Same reference call sites as the _f32 entry points above; `se_bf16` is the raw 16-bit pattern.
 * Volumes are channels-last [B][D][D][D][C] with C % 8 == 0 (a lane moves 8 channels = 16 bytes).
 * ------------------------------------------------------------------------------------------------ */
typedef unsigned short se_bf16;

/* Weight preparation (BN folded, MFMA A-fragment order [cout tile][k step][lane][8]).  A k step covers 4 groups of
 * (tap, 8 channels); the group order is [channel chunk of `chunk_octets` x 8 channels][tap][octet] with every chunk
 * padded to whole k steps.  chunk_octets: 2 for 3^3 convs (cin_pad % 16 == 0); 4 (cin_pad % 32 == 0) or 2 for 1^3 and
 * transposed convs; 1 for the 7^3 front layer (cin_pad = 40 / 72), whose taps are stored in the bank-conflict-free
 * pair order of the LDS kernel.
 * transposed != 0: ConvTranspose3d k2s2 weight [cin][cout][2][2][2], the 8 output parities take the place of taps.
 * cout % 32 == 0, or cout <= 16 (one tile).  wpack: se_conv3d_packed_elems_bf16(...) elements; bpack: float32,
 * cout rounded up to 16.                                                                                        */
int se_conv3d_pack_bf16(const float* w, const float* b, const float* gamma, const float* beta,
                        const float* mean, const float* var, float eps,
                        se_bf16* wpack, float* bpack,
                        int cout, int cin, int cin_pad, int ksize, int transposed, void* stream);
long long se_conv3d_packed_elems_bf16(int cout, int cin_pad, int ksize, int transposed);

/* EXPERIMENTAL (round 3; never on the float32 headline path - VoxelNetwork_depth.set_v2v_dtype("split_bf16") selects it): Conv3d
 * k = 3 + folded BN + epilogue on float32 channels-last tensors with SPLIT-bf16 arithmetic: every operand x = hi + lo
 * (hi = bf16(x), lo = bf16(x - hi)), a product = hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with float32 accumulation.
 * Replaces the same reference calls as se_conv3d_f32 with ksize 3 (network/v2v.py:21-43) for the shapes dim % 16 == 0,
 * cin_pad % 8 == 0, cout % 32 == 0.
 * se_conv3d_split3_pack: w = float32 [cout][cin][3][3][3] with the BatchNorm scale already folded in -> wsplit
 * (se_conv3d_split3_packed_elems bf16 elements; -1 for an unsupported shape): both halves in MFMA fragment order.
 * se_conv3d_k3_split3_f32: bpack = the folded float32 bias (as se_conv3d_pack_f32 writes it); flags: SE_EPI_RELU,
 * SE_EPI_RES_PRE_RELU / SE_EPI_RES_POST_RELU, SE_IN_OCTET / SE_OUT_OCTET / SE_RES_OCTET (octet-planar tensors, as for
 * se_conv3d_f32's 2-D Winograd shapes).  SE_ERR_BAD_ARG for anything else (nothing launched).                                 */
long long se_conv3d_split3_packed_elems(int cout, int cin_pad);
int se_conv3d_split3_pack(const float* w, se_bf16* wsplit, int cout, int cin, int cin_pad, void* stream);
int se_conv3d_k3_split3_f32(const float* in, const se_bf16* wsplit, const float* bpack, const float* residual, float* out,
                            int batch, int dim, int cin_pad, int cout, int flags, void* stream);

/* Six-product split forms of the float32 program (csrc/split6.h): float32 tensors in and out, every float32 product x * w taken as
 * six bf16 products of a 3-way split of both operands (x = a + b + c, w = p + q + r, round to nearest even; ap, aq, bp, ar, cp, bq)
 * on v_mfma_f32_16x16x32_bf16 with float32 accumulation: the dropped products total <= 2^-23 |x| |w|.  Part of the float32 parity
 * surface: the plan of se_conv3d_w6_f32 chooses such a form where one exists and measured faster than its float32 form.
 * se_conv3d_split6_pack: wpack = the layer's packed float32 buffer (se_conv3d_pack_f32, same cout / cin_pad / ksize / transposed;
 *   section A is read) -> wsplit, se_conv3d_split6_packed_elems bf16 elements (-1: no split planes for the shape; they exist
 *   for cin_pad % 32 == 0): the three planes of every folded weight in A-fragment order (csrc/conv3d_pack.h).  Biases stay float32.
 * se_conv3d_w6_f32: se_conv3d_f32 with the layer's split planes (NULL: exactly se_conv3d_f32).
 * se_conv3d_f32_split6: 1 when se_conv3d_w6_f32 with split planes runs such a call (cin_pad == cin) on a split form, else 0.
 * se_conv3d_k3_split6_f32: the split form of the 3^3 kernel of the 8^3-sized levels on its whole domain (dim 8 or 16,
 *   cin % 32 == 0, cin_pad % 32 == 0, cout % 32 == 0, batch * dim^3 <= 8192; flags SE_EPI_RELU, SE_EPI_RES_PRE_RELU / _POST_RELU),
 *   whatever se_conv3d_w6_f32 would choose; SE_ERR_BAD_ARG otherwise (nothing launched).
 * se_split6_planes_f32 (test entry point): the device split of n (even) float32 values -> planes [3][n].                       */
long long se_conv3d_split6_packed_elems(int cout, int cin_pad, int ksize, int transposed);
int se_conv3d_split6_pack(const float* wpack, se_bf16* wsplit, int cout, int cin_pad, int ksize, int transposed, void* stream);

/* The 2-D pose head's ConvTranspose2d(k=4, s=2, p=1) + BatchNorm2d + ReLU (se_deconv2d_k4s2_assemble_f32 above) as ONE launch,
 * product and assembly together: a four-phase implicit GEMM with every float32 product taken as six bf16 products on
 * v_mfma_f32_16x16x32_bf16 (csrc/split6.h; float32 accuracy), bias and ReLU in the epilogue.
 *   x      [batch][cin][h][w] float32 (x_elem_bytes = 4; any other element size: SE_ERR_BAD_ARG)
 *   wsplit se_deconv2d_k4s2_s6_pack of the folded ConvTranspose2d weight w [cin][cout][4][4]: three bf16 planes that sum to w exactly,
 *          in the order the kernel walks them, [cin / 32][cout / 16][a 2][fragment 8][plane 3][lane 64][8]: fragment 4 dy + f is
 *          kernel row ky = 3 - a - 2 dy and column kx = 3, 1, 2, 0 for f = 0 .. 3; lane l, element j is input channel
 *          32 chunk + 8 (l >> 4) + j and output channel 16 tile + (l & 15); se_deconv2d_k4s2_s6_packed_elems elements (-1: none)
 *   out    [batch][cout][2h][2w] = bias[co] + the four taps that reach each output pixel (zero outside the map), ReLU if `relu`
 * Domain (se_deconv2d_k4s2_s6_domain returns 1; else the launch returns SE_ERR_BAD_ARG and nothing is launched): cin % 32 == 0,
 * cout % 64 == 0, w % 16 == 0, h % 8 == 0, the input below 2^31 bytes.  No atomics, fixed summation order: launches repeat bit for
 * bit and a sample's result does not depend on the batch it is in. */
int se_deconv2d_k4s2_s6_domain(int batch, int cin, int cout, int h, int w);
long long se_deconv2d_k4s2_s6_packed_elems(int cin, int cout);
int se_deconv2d_k4s2_s6_pack(const float* w, se_bf16* wsplit, int cin, int cout, void* stream);
int se_deconv2d_k4s2_s6_f32(const void* x, int x_elem_bytes, const se_bf16* wsplit, const float* bias, float* out, int batch, int cin,
                            int cout, int h, int w, int relu, void* stream);
int se_conv3d_w6_f32(const float* in, const float* wpack, const se_bf16* wsplit6, const float* bpack, const float* residual,
                     float* out, int batch, int dim, int cin, int cin_pad, int cout, int ksize, int flags,
                     float* workspace, long long workspace_elems, void* stream);
int se_conv3d_f32_split6(int batch, int dim, int cin, int cout, int ksize, int flags);
int se_conv3d_k3_split6_f32(const float* in, const se_bf16* wsplit6, const float* bpack, const float* residual, float* out,
                            int batch, int dim, int cin, int cin_pad, int cout, int flags, void* stream);
int se_split6_planes_f32(const float* x, se_bf16* planes, long long n, void* stream);

/* Conv3d k = 1, 3 or 7 + folded BN + epilogue (flags as se_conv3d_f32; SE_EPI_OUT_PLANAR is not supported: the
 * float32 planar logits come from se_pointwise_chain3_bf16).  in [B][D]^3[cin_pad] -> out [B][D]^3[cout].
 * k = 7 (the front layer) reads its input OCTET-PLANAR: in [B][cin_pad/8][D]^3[8] — the layer walks the input one
 * 8-channel octet at a time, and a channels-last record of 80 B would be fetched five times for 16 B each.      */
int se_conv3d_bf16(const se_bf16* in, const se_bf16* wpack, const float* bpack, const se_bf16* residual,
                   se_bf16* out, int batch, int dim, int cin_pad, int cout, int ksize, int flags, void* stream);

/* V2V tail as se_pointwise_chain3_f32: bfloat16 in [B][D]^3[32], float32 planar logits out [B][cout3][D^3]. */
int se_pointwise_chain3_bf16(const se_bf16* in, const se_bf16* wpack1, const float* bpack1,
                             const se_bf16* wpack2, const float* bpack2, const se_bf16* wpack3, const float* bpack3,
                             float* out, int batch, int dim, int cout3, void* stream);

/* se_pointwise_chain3_bf16 with pass 1 of se_softargmax3d_f32 (mode 1: softmax) folded in, as se_pointwise_chain3_softargmax_f32 does for
 * the float32 program (round 6): the float32 logits are written to `out` and, while in registers, reduced to the per-chunk partial records
 * in `scratch` (se_softargmax3d_scratch_elems(batch * cout3) floats); finish with se_softargmax3d_finish_f32.  network/v2v.py:155-161 +
 * the first half of utils/op.py:83-96. */
int se_pointwise_chain3_softargmax_bf16(const se_bf16* in, const se_bf16* wpack1, const float* bpack1, const se_bf16* wpack2,
                                        const float* bpack2, const se_bf16* wpack3, const float* bpack3, float* out,
                                        const float* coord, float* scratch, int batch, int dim, int cout3, void* stream);

int se_deconv3d_k2s2_bf16(const se_bf16* in, const se_bf16* wpack, const float* bpack, const se_bf16* residual,
                          se_bf16* out, int batch, int dim, int cin, int cout, int flags, void* stream);
int se_maxpool3d_2_bf16(const se_bf16* in, se_bf16* out, int batch, int dim, int channels, void* stream);

/* Producers of the bfloat16 V2V input, octet-planar buf [B][octs_total][voxels][8]: as se_unproject_gather_f32 /
 * se_voxelize_strided_f64.  The gather writes `channels` (% 8) channels starting at channel out_c_offset (% 8); the
 * voxeliser clears octet c_offset / 8 and writes the occupancy (1.0 = 0x3F80) into channel c_offset (% 8 == 0).
 * (with_intersection / scene_volumes inputs are assembled in float32 by the _f32 entry points and converted once.) */
int se_unproject_gather_bf16(const float* feat, const int* idx, const float* w, se_bf16* out,
                             int batch, int texels, int channels, int voxels, int octs_total, int out_c_offset,
                             void* stream);
int se_voxelize_strided_bf16(const float* depth, const double* ray_tab, se_bf16* buf, int batch, int depth_h,
                             int depth_w, int up, int pad_x, int volume_size, double cuboid_side,
                             int octs_total, int c_offset, void* stream);

/* Image pre-processing of the demo path on the device (dataset/demo_dataset.py:72-82, utils/data_transforms.py:38-72):
 * img BGR uint8 [B][height][width][3] -> crop crop_x columns each side -> exact 1/4 bilinear resize (= rounded mean of the
 * central 2x2 of every 4x4 block, cv2.resize INTER_LINEAR at scale 1/4) -> /255, -mean3[c], /std3[c] in float64 ->
 * out float32 [B][3][height/4][(width-2*crop_x)/4].  mean3 / std3: HOST pointers to 3 doubles (read at launch).   */
int se_preprocess_image_u8(const unsigned char* img, float* out, int batch, int height, int width, int crop_x,
                           const double* mean3, const double* std3, void* stream);

/* se_bias_act_nchw_f32 for a bfloat16 backbone (x, bias, residual, out bfloat16; float32 arithmetic; hw % 8 == 0). */
int se_bias_act_nchw_bf16(const se_bf16* x, const se_bf16* bias, const se_bf16* residual, se_bf16* out,
                          int batch, int channels, int hw, int relu, void* stream);

/* Which kernel family se_conv3d_f32 selects for a float32 convolution of this shape (bench.py prices the roofline with it):
 *   0 direct implicit GEMM (every product on the matrix cores),
 *   1 1-D Winograd F(4,3) along z (1/2 of the direct products), 2 2-D Winograd F(4,3) x F(2,3) along z, y (1/3),
 *   7 1-D Winograd along z for the 7x7x7 front layer: F(6,7) (12/42 of the direct products) when dim % 16 == 0, else F(4,7) (10/28).
 * Pure function of the arguments; no device access. */
int se_conv3d_f32_algo(int dim, int cin, int cout, int ksize);
/* Which kernel a launch of `batch` samples with these flags really runs on: se_conv3d_f32_algo()'s value, except
 *   3 = the F(4,3) x F(4,3) ping-pong kernel (a member of the 2-D Winograd family with the same fused forms; it executes 1/4 of the
 *       direct convolution's MFMAs, algo 2 executes 1/3).  Its planar layout is QUAD-planar (SE_IN_QUAD / SE_OUT_QUAD / SE_RES_QUAD):
 *       it takes a quad-planar input or a channels-last one with fewer than 32 channels; a channels-last input with >= 32 channels
 *       and every launch with an octet-planar flag stay on algo 2 (whose planar layout is octet-planar);
 *   0 for a 2-D Winograd shape with <= 4096 voxels in the batch when `flags` asks for none of the planar forms (such a call
 *       runs on the in-workgroup split-K kernel).
 * `flags`: the SE_IN_* / SE_OUT_* / SE_RES_* layout bits of the launch (others ignored).  A caller that wants planar hand-overs asks
 * with the quad bits first: 3 = use them; otherwise the octet bits (2 = use those).  bench.py prices every launch with it. */
int se_conv3d_f32_variant(int batch, int dim, int cin, int cout, int ksize, int flags);

/* PIZ-compressed scanline OpenEXR chunks -> float32 on the device (stands in for cv2.imread of the depth maps,
 * dataset/test_dataset.py:173-178, and for sceneego_amd/exr.py read_depth_exr; bit-identical to the latter).
 *   chunk_desc  int64 [n_chunks][16], one row per chunk: 0 byte offset of the chunk's block (after y and size) in `payload`,
 *               1 block bytes, 2 file index (row of channel_desc, sample of out), 3 first row (y - ymin), 4 rows, 5 stored
 *               uncompressed (size == expected bytes), 6 minNonZero, 7 maxNonZero, 8 offset of the Huffman data in the block,
 *               9 its bytes, 10 im, 11 iM, 12 nBits, 13 scratch offset and 14 record capacity (both written by
 *               se_exr_piz_scratch_bytes), 15 unused
 *   channel_desc int32 [n_files][8]: 0 width, 1 height, 2 pixel type of the selected channel (0 UINT, 1 HALF, 2 FLOAT), 3 16-bit
 *               words per pixel of the channels stored before it, 4 its words per pixel (1 or 2), 5 words per pixel of all
 *               channels, 6-7 unused
 * se_exr_piz_scratch_bytes: HOST pointers; lays out the per-chunk scratch slices (fills columns 13, 14 of chunk_desc) and returns
 *   the scratch bytes se_exr_piz_decode_f32 needs, or SE_ERR_BAD_ARG.
 * se_exr_piz_decode_f32: device pointers; out float32 [n_files][out_h][out_w] gets, for every chunk, the output rows whose nearest
 *   source row (min(floor(y * (height / out_h)), height - 1), same for columns) lies in the chunk; values above `clamp` are set to
 *   it when clamp > 0 (NaN kept).  status int32 [n_chunks][2]: {code, words decoded}; code 0 ok, 1 descriptor out of range,
 *   2 code-length table past the Huffman bytes, 3 table larger than its scratch, 4 nBits past the bytes, 5 no code matches,
 *   6 stream ended after `words decoded` symbols, 7 run past the end of the output.  A chunk with a non-zero code writes nothing
 *   to `out`.  Kernels se_exr_piz_huffman_kernel, se_exr_piz_wavelet_kernel; every read stays inside payload_bytes / the chunk's
 *   block, every write inside its scratch slice and its rows of `out`. */
long long se_exr_piz_scratch_bytes(long long* chunk_desc, int n_chunks, const int* channel_desc, int n_files);
int se_exr_piz_decode_f32(const void* payload, long long payload_bytes, const long long* chunk_desc, int n_chunks,
                          const int* channel_desc, int n_files, float* out, int out_h, int out_w, float clamp,
                          void* scratch, long long scratch_bytes, int* status, void* stream);

/* ZIP (16 lines per chunk), ZIPS (1 line) and uncompressed (NONE) scanline OpenEXR chunks -> float32 on the device (the same call
 * sites; bit-identical to sceneego_amd/exr.py read_depth_exr).
 *   chunk_desc  int64 [n_chunks][16], one row per chunk: 0 byte offset of the chunk's block (after y and size) in `payload`,
 *               1 block bytes, 2 file index (row of channel_desc, sample of out), 3 first row (y - ymin), 4 rows, 5 stored
 *               uncompressed (block bytes == bytes_per_line * rows, and every NONE chunk; only its first bytes_per_line * rows
 *               bytes are read), 6-12 unused, 13 scratch offset and 14 scratch bytes (both written by se_exr_zip_scratch_bytes),
 *               15 unused.  A chunk that is not stored holds one zlib stream (RFC 1950 / 1951).
 *   channel_desc int32 [n_files][8]: as for se_exr_piz_decode_f32 (bytes_per_line = 2 * column 5 * width).
 * se_exr_zip_scratch_bytes: HOST pointers; lays out the per-chunk scratch slices (fills columns 13, 14 of chunk_desc: each slice
 *   16-byte aligned, bytes_per_line * rows bytes for a compressed chunk, none for a stored one) and returns the scratch bytes
 *   se_exr_zip_decode_f32 needs, or SE_ERR_BAD_ARG.
 * se_exr_zip_decode_f32: device pointers; `out` as for se_exr_piz_decode_f32 (nearest resize, clamp).  A stream is accepted exactly
 *   when zlib.decompress accepts it and it inflates to bytes_per_line * rows bytes (exr.py would read a longer or shorter stream;
 *   here it is a bad stream).  status int32 [n_chunks][2]: {code, bytes inflated when the decode stopped}; codes distinct from the
 *   PIZ ones so that one status vector covers a mixed batch: 0 ok, 1 descriptor out of range, 8 bad zlib header (CM, CINFO,
 *   FCHECK, FDICT), 9 block type 3, 10 stored block LEN != ~NLEN, 11 bad code-length set (over-subscribed, incomplete, no
 *   end-of-block, HLIT > 286 or HDIST > 30), 12 invalid symbol or code-length repeat, 13 distance too far back, 14 stream ended
 *   before the final block and its Adler-32, 15 decompressed size != bytes_per_line * rows, 16 Adler-32 mismatch.  A chunk with a
 *   non-zero code writes nothing to `out`.  Kernels se_exr_zip_inflate_kernel (one wavefront per chunk), se_exr_zip_recon_kernel
 *   (predictor, de-interleave, conversion, resize); every read stays inside payload_bytes / the chunk's block, every write inside
 *   its scratch slice and its rows of `out`. */
long long se_exr_zip_scratch_bytes(long long* chunk_desc, int n_chunks, const int* channel_desc, int n_files);
int se_exr_zip_decode_f32(const void* payload, long long payload_bytes, const long long* chunk_desc, int n_chunks,
                          const int* channel_desc, int n_files, float* out, int out_h, int out_w, float clamp,
                          void* scratch, long long scratch_bytes, int* status, void* stream);

/* Baseline JPEG frames -> uint8 B, G, R on the device (stands in for sceneego_amd/preprocess.py load_image_bgr, PIL on libjpeg-turbo;
 * bit-identical to it on files of plain blocks, see status 4 below).  sceneego_amd/jpeg_device.py parses, validates and unstuffs on the host.
 *   img_desc  int32 [n_images][64]: 0 width, 1 height, 2 components (1 or 3), 3 MCUs per row, 4 MCU rows, 5 blocks per MCU (<= 10),
 *             6 first segment, 7 segments, 8 output slot (sample of out), 9 hmax, 10 vmax, 12-14 h per component (frame order),
 *             15-17 v, 18-20 quantisation slot (== component), 21-23 DC table slot (0-3), 24-26 AC table slot (4-7), 27-29 plane
 *             width (8 * h * MCUs per row), 30-32 plane height (8 * v * MCU rows), 33-35 first block of the component in the MCU,
 *             36 first global block and 37-39 plane byte offsets (both written by se_jpeg_scratch_bytes), 40-49 component of every
 *             block of the MCU, 50 restart interval (informational); gray images use one block per MCU of 8x8 pixels.
 *   seg_desc  int64 [n_segs][8], one row per restart segment, ordered by image then segment: 0 byte offset of its unstuffed
 *             entropy-coded data in `payload` (4-byte aligned; the slot holds ((len + 3) & ~3) + 8 bytes, zero after len),
 *             1 len, 2 image (row of img_desc), 3 first MCU, 4 MCUs, 5 first lane, 6 lanes, 7 first global block (5-7 written by
 *             se_jpeg_scratch_bytes).
 *   tables    [n_images][8] records of 1536 bytes (slots 0-3 DC, 4-7 AC): uint16 lookahead[512] (9 bits; length << 8 | symbol, 0
 *             for a longer code), int32 maxcode[18] (-1 for none), int32 valoffset[18] at byte 1096, uint8 values[256] at byte 1168.
 *   quant     int32 [n_images][4][64], natural order, each value already cast to int16 as libjpeg's ISLOW_MULT_TYPE.
 * se_jpeg_scratch_bytes: HOST pointers; fills the derived columns and layout int64[4] = {blocks, lanes, plane bytes, longest
 *   per-(segment, component) block run}, returns the scratch bytes se_jpeg_decode_bgr_u8 needs, or SE_ERR_BAD_ARG.
 * se_jpeg_decode_bgr_u8: device pointers except `layout` (host, from se_jpeg_scratch_bytes); out uint8 [n_out][out_h][out_w][3]
 *   (B, G, R) gets every image at its output slot.  `rounds`: inter-workgroup synchronisation launches (< 0: the default, 3); 0
 *   leaves every unsynchronised workgroup to the sequential repair kernel, with the same result.  status int32 [n_segs][2]:
 *   {code, value}; 0 ok, 1 descriptor out of range, 2 no code matches (value: bit offset in the segment), 3 stream ended (value:
 *   blocks completed of mcus * blocks per MCU), 4 a block outside the plain domain (value: one such block, counted from the
 *   segment's first; se_jpeg_idct_kernel sets it only where the entry still holds 0, and not for a block of the MCU padding that
 *   holds no sample of its component).  A block is plain when every dequantised
 *   coefficient and every pass-1 workspace value of the ISLOW IDCT fits int16 and every pass-2 value after its descale, before the
 *   +128, lies in [-512, 511]: there jidctint.c's C code, which the kernel follows, equals libjpeg-turbo's SIMD IDCT, and the
 *   bit-identity with PIL holds only there; the caller decodes a file with any non-zero status on the host (jpeg_device.py does).
 *   Kernels se_jpeg_sync_intra_kernel, se_jpeg_sync_inter_kernel,
 *   se_jpeg_sync_repair_kernel, se_jpeg_scan_kernel, se_jpeg_scan_top_kernel, se_jpeg_write_kernel, se_jpeg_dc_kernel,
 *   se_jpeg_idct_kernel, se_jpeg_color_kernel; every read stays inside payload_bytes and the segment's slot, every write inside
 *   the scratch layout and out. */
long long se_jpeg_scratch_bytes(int* img_desc, int n_images, long long* seg_desc, int n_segs, long long* layout);
int se_jpeg_decode_bgr_u8(const void* payload, long long payload_bytes, const int* img_desc, int n_images, const long long* seg_desc,
                          int n_segs, const void* tables, const int* quant, const long long* layout, unsigned char* out, int n_out,
                          int out_h, int out_w, void* scratch, long long scratch_bytes, int* status, int rounds, void* stream);

/* Headless renderer (stands in for the reference's visualize.py: utils/depth2pointcloud.py get_point_cloud_single_image +
 * utils/skeleton.py joints_2_mesh, drawn by open3d).  All arithmetic is float64, unfused, in the order written here
 * (tests/render_model.py restates it).  joint_rgb, bone_rgb (3 floats in [0, 1], R G B) and background (3 bytes, R G B) are HOST
 * pointers, read during the call; every other pointer is device memory.  batch <= 65535; splat 1..4; near >= 0.
 *
 * se_render_splat_f64: point cloud -> z-buffer of a pinhole view.  One thread per frame pixel (y, x):
 *   depth    [B][depth_h][depth_w] float32 metres        ray_tab [height][width][3] float64: the calibrated camera's ray of (x, y)
 *   image    [B][height][width][3] uint8 (B, G, R)        view    [12] float64: row-major R[3][3], then t[3]
 *   zbuf     [B][out_h][out_w] uint64, cleared to all-ones ("no point") inside, then written
 *   1. d = depth[b][(y * depth_h) / height][(x * depth_w) / width] (integer division);  2. dropped unless d > 0 && d <= max_depth
 *   (a NaN fails);  3. p = ray * d per component, dropped unless p.z > min_z;  4. q_i = ((R[i][0] p.x + R[i][1] p.y) + R[i][2] p.z)
 *   + t[i], dropped unless q.z > near;  5. u = (f q.x) / q.z + cx, v = (f q.y) / q.z + cy, dropped unless u >= -4 && u < out_w + 4
 *   && v >= -4 && v < out_h + 4 (tested on the doubles), iu = (int)floor(u), iv = (int)floor(v);  6. key = (uint64)(bits of
 *   (float)q.z) << 32 | R << 16 | G << 8 | B;  7. for dy, dx in [0, splat): px = iu - (splat - 1) / 2 + dx, py likewise; inside the
 *   image: zbuf[b][py][px] = min(zbuf[b][py][px], key), a 64-bit atomic minimum.  Positive floats order like their bits, so the
 *   result is the nearest point and, at equal depth, the lowest colour word, whatever the launch order: bitwise reproducible.
 *
 * se_render_resolve_f64 / se_render_overlay_f64: the skeleton ray-cast along a per-pixel ray table, one thread per pixel.
 *   rays     [h][w][3] float64, direction through the origin: ((px + 0.5 - cx) / f, (py + 0.5 - cy) / f, 1) for the pinhole view
 *            (the hit parameter s is then view z), the calibrated camera's unit rays for the overlay (s is distance, as in a depth map)
 *   joints   [B][15][3] float64 in the frame of `rays`; bones: Skeleton.lines (utils/skeleton.py:20-21)
 *   With a = d.d for the ray direction d: sphere of centre c, radius r_joint: b = d.c, disc = b b - a (c.c - r r), roots
 *   (b -+ sqrt(disc)) / a when disc >= 0.  Capless cylinder from A to B, radius r_bone, skipped when |B - A| < 1e-9: v = B - A,
 *   e = d - (d.v / v.v) v, g = A - (A.v / v.v) v, qa = e.e (skipped unless > 0), qb = e.g, disc = qb qb - qa (g.g - r r), roots
 *   (qb -+ sqrt(disc)) / qa kept when the axial parameter (s d.v - A.v) / v.v lies in [0, 1].  Every dot product is
 *   (x x + y y) + z z.  The hit is the smallest root with s > near over spheres 0..14, then bones 0..14 (an equal later root does not
 *   replace an earlier one); a non-finite joint disables its sphere and its bones.  Normal n = s d - c (sphere), s e - g (cylinder);
 *   shade = 0.3 + 0.7 max(0, -(n.d) / (|n| |d|)); channel = (int)((255 base) shade + 0.5).
 *   resolve: out [B][out_h][out_w][3] uint8 (R, G, B) = the skeleton colour when there is a hit and zbuf is empty or
 *            s < (double)(float of zbuf >> 32) (strict: a tie goes to the scene), else the z-buffer's colour, else `background`.
 *   overlay: frame [B][height][width][3] uint8 (B, G, R) -> out, same shape, (R, G, B), with the skeleton over it; depth (may be
 *            NULL) [B][depth_h][depth_w] float32: the skeleton shows only where s < depth[b][(y depth_h) / height][(x depth_w) / width]. */
int se_render_splat_f64(const float* depth, const double* ray_tab, const unsigned char* image, const double* view,
                        unsigned long long* zbuf, int batch, int depth_h, int depth_w, int height, int width, int out_h, int out_w,
                        double f, double cx, double cy, int splat, double min_z, double max_depth, double near, void* stream);
int se_render_resolve_f64(const double* rays, const double* joints, const unsigned long long* zbuf, unsigned char* out, int batch,
                          int out_h, int out_w, double r_joint, double r_bone, double near, const float* joint_rgb,
                          const float* bone_rgb, const unsigned char* background, void* stream);
int se_render_overlay_f64(const double* rays, const double* joints, const unsigned char* frame, const float* depth,
                          unsigned char* out, int batch, int height, int width, int depth_h, int depth_w, double r_joint,
                          double r_bone, double near, const float* joint_rgb, const float* bone_rgb, void* stream);

/* Scene probe (no counterpart in the reference; sceneego_amd/scene_check.py drives it): up to 64 probe points per frame against
 * every scene point of the frame's depth map.  All arithmetic is float64, unfused, in the order written here; every dot product
 * is (x x + y y) + z z.  No square root and no division is computed: every value written is a correctly rounded sum or product,
 * or a copy, so the output has one right answer bit for bit (tests/scene_model.py restates it).
 *   depth    [B][depth_h][depth_w] float32 metres        ray_tab [height][width][3] float64: the calibrated camera's ray of (x, y)
 *   probes   [B][P][3] float64, 1 <= P <= 64             out     [B][P][8] float64        index [B][P][2] int32
 *   scratch  se_scene_probe_scratch_bytes(batch, height, width, P) bytes of device workspace, 8-byte aligned (-1: bad shape)
 * Pixel n = y * width + x (steps 1-3 of se_render_splat_f64): d = depth[b][(y * depth_h) / height][(x * depth_w) / width] (integer
 * division); the pixel has a SURFACE iff d > 0 && d <= max_depth (a NaN fails); s = ray * (double)d per component; it is a SCENE
 * POINT iff it has a surface and s.z > min_z.  A pixel whose ray has a non-finite component takes part in nothing.
 * Per probe c:  nearest point: e = s - c per component, q = e.e; nearest_q = the minimum of q over the scene points and
 * nearest_index the lowest n that attains it.  Line of sight: t = ray.c over all pixels with a finite ray, whatever their depth;
 * sight_dot = the maximum of t, sight_index the lowest n that attains it, surface = (double)d of that pixel if it has a surface,
 * else NaN.
 *   out row   {nearest_q, s[nearest_index].x, .y, .z, c.c, sight_dot, surface, 0.0}        index row {nearest_index, sight_index}
 * A frame without a scene point: nearest_q = +inf, NaN in out[1..3], nearest_index = -1 (the sight half is still filled; without
 * any finite ray sight_dot = -inf, sight_index = -1).  A probe with a non-finite component: 8 NaNs and {-1, -1}; other rows are
 * unaffected.  Probe coordinates are assumed small enough for t not to overflow.
 * Two launches (one workgroup per (2048-pixel tile, frame) writing (value, index) partials to scratch, then one wave per
 * (frame, probe)); lexicographic (value, index) reductions only, no floating-point atomics: independent of the launch order,
 * bitwise reproducible; nothing is allocated, so the call is legal under hipGraph capture.
 * SE_ERR_BAD_ARG: batch <= 0 or > 65535, n_probes outside 1..64, a non-positive size, a null pointer, scratch_bytes too small,
 * min_z < 0 or NaN, max_depth <= 0 or NaN. */
long long se_scene_probe_scratch_bytes(int batch, int height, int width, int probes);
int se_scene_probe_f64(const float* depth, const double* ray_tab, const double* probes, double* out, int* index, void* scratch,
                       long long scratch_bytes, int batch, int depth_h, int depth_w, int height, int width, int n_probes,
                       double min_z, double max_depth, void* stream);

/* Scene-constrained joints (no counterpart in the reference; sceneego_amd/op.py: build_sight_table, scene_free_mask,
 * constrained_joints; VoxelNetwork_depth.constrain_to_scene drives them): the soft-argmax taken over the part of the voxel grid that
 * lies in front of the depth surface.
 *
 * SIGHT TABLE, built once on the host per (grid, frame size).  For voxel n with the float32 centre c_n (build_coord_volume) and its
 * float32 projection (u, v) (grid_coord_proj):  x = floor((double)u + 0.5), y = floor((double)v + 0.5);
 *   pix[n] = y * width + x (int32) when u, v are finite and 0 <= x < width, 0 <= y < height, else -1;
 *   rng[n] = (float)sqrt(((double)cx cx + (double)cy cy) + (double)cz cz), the voxel's distance from the camera.
 *
 * FREE MASK, se_scene_free_mask_u8, per frame b and voxel n:
 *   depth [B][depth_h][depth_w] float32 metres     pix [voxels] int32     rng [voxels] float32     free_mask [B][voxels] uint8
 *   pix[n] < 0 (or >= height * width): free, there is no evidence against the voxel.  Otherwise y = pix[n] / width,
 *   x = pix[n] - y * width, d = depth[b][(y * depth_h) / height][(x * depth_w) / width] (the integer division of se_scene_probe_f64);
 *   the pixel has a SURFACE iff d > 0 && d <= max_depth (a NaN fails); the voxel is BLOCKED iff it has a surface and
 *   (double)d + margin < (double)rng[n]: one correctly rounded float64 sum and one comparison (equality counts as free).
 *   free_mask[b][n] = 1 free, 0 blocked.  One right answer, bit for bit (tests/scene_constraint_model.py restates it).
 * One launch, nothing allocated.  SE_ERR_BAD_ARG: a null pointer, batch outside 1..65535, a non-positive size, height * width above
 * 0x7fff0000, voxels & 3, a free_mask that is not 4-byte aligned, margin NaN, max_depth <= 0 or NaN.
 *
 * MASKED REDUCTION, se_softargmax3d_masked_f32, per row r = b * rows_per_frame + j:
 *   prob  [rows][voxels] float32 probabilities, as se_softargmax3d_f32 writes them in mode 1       coord [voxels][3] float32
 *   free_mask [rows / rows_per_frame][voxels] uint8 (any non-zero byte is free); f_n = free_mask[r / rows_per_frame][n]
 *   out [rows][8]: 0     free_mass = sum_n f_n p_n
 *                  1..3  sum_n f_n p_n c_n for x, y, z (NOT divided: the kernel does no division; the caller divides by slot 0)
 *                  4     free_peak_p = the largest p_n over the free voxels
 *                  5..7  coord[peak_index]
 *   peak_index [rows] int32: the LOWEST free index with p_n == free_peak_p
 *   scratch: se_softargmax3d_masked_scratch_elems(rows) floats of workspace.
 * A row without a free voxel: slots 0..4 are 0, slots 5..7 NaN, peak_index -1.  A row that holds a NaN probability (free or blocked)
 * gets 8 NaNs and peak_index -1; other rows are unaffected.  Two launches on `stream` (se_sa_splits(rows) chunks per row as the
 * soft-argmax, then one wave per row), a fixed reduction order and no atomics: bitwise identical from run to run.  Allocates nothing
 * (legal inside hipGraph capture).  rows <= 0, rows > 65535, rows_per_frame <= 0, rows % rows_per_frame, voxels <= 0, voxels & 3, a
 * null pointer, a prob / coord that is not 16-byte aligned or a free_mask that is not 4-byte aligned -> SE_ERR_BAD_ARG.              */
int se_scene_free_mask_u8(const float* depth, const int* pix, const float* rng, unsigned char* free_mask, int batch, int depth_h,
                          int depth_w, int height, int width, int voxels, double margin, double max_depth, void* stream);
int se_softargmax3d_masked_f32(const float* prob, const float* coord, const unsigned char* free_mask, float* out, int* peak_index,
                               float* scratch, int rows, int rows_per_frame, int voxels, void* stream);
long long se_softargmax3d_masked_scratch_elems(int rows);

/* Scene distance field (no counterpart in the reference; sceneego_amd/scene_field.py: SceneField; sceneego_amd/op.py: scene_sites,
 * scene_distance, scene_expect, scene_field_lookup; VoxelNetwork_depth.scene_field / scene_expectations drive them): the scene of a
 * depth map as a field on the network's own G^3 voxel grid - per voxel the exact squared distance, in voxel index units, to the
 * nearest voxel that holds scene, and that voxel's flat index - and any [rows][voxels] distribution reduced against it.  Flat index
 * n = (i G + j) G + k as everywhere.  tests/scene_field_model.py restates all three.
 *
 * SITES, se_scene_sites_u8:  depth [B][depth_h][depth_w] float32 metres     ray_tab [height][width][3] float64 (the table of
 *   se_scene_probe_f64)     sites [B][G^3] uint8, cleared inside (one memset node on `stream`, then one launch).
 *   The SCENE POINTS are exactly those of se_scene_probe_f64: pixel n = y * width + x, d = depth[b][(y * depth_h) / height]
 *   [(x * depth_w) / width] (integer division); the pixel has a surface iff d > 0 && d <= max_depth (a NaN fails); s = ray * (double)d
 *   per component; it is a scene point iff it has a surface and s.z > min_z.  A pixel whose ray has a non-finite component takes part
 *   in nothing.  Voxel centres follow build_coord_volume: their spacing is side / (G - 1).  In float64, unfused, in this order:
 *     qx = rint(((s.x + side / 2) * (G - 1)) / side)      qy likewise from s.y      qz = rint((s.z * (G - 1)) / side)
 *   with rint rounding half to even.  A point with 0 <= qx, qy, qz <= G - 1 (a NaN or an infinity fails) marks
 *   sites[b][(qx G + qy) G + qz] = 1; any other point marks nothing.  Every writer stores the same byte with an ordinary store: the
 *   result does not depend on the write order, and there are no atomics.  One right answer, bit for bit.
 *   SE_ERR_BAD_ARG: a null pointer, batch outside 1..65535, a non-positive size, height * width above 0x7fff0000, grid outside
 *   2..1024, side <= 0, infinite or NaN, min_z < 0 or NaN, max_depth <= 0 or NaN.
 *
 * DISTANCE, se_scene_distance_i32:  sites [B][G^3] uint8, any non-zero byte is a SITE; 2 <= G <= 128.
 *   d2 [B][G^3] int32 = min over the frame's sites m of |n - m|^2 = (i - i')^2 + (j - j')^2 + (k - k')^2, in integers (at most
 *   3 * 127^2 = 48 387);   nearest [B][G^3] int32 = the flat index of the site that minimises the key (|n - m|^2, m) taken
 *   lexicographically: among the sites at the least distance, the lowest index.  A frame without a site: d2 = 0x7fffffff and
 *   nearest = -1 at every voxel.  scratch: se_scene_distance_scratch_bytes(batch, grid) bytes of device workspace, 8-byte aligned
 *   (-1: bad shape).  Two launches: passes k and j of a separable transform per (frame, i) slab in LDS, pass i per (frame, j, 32 k)
 *   tile; each pass is the plain minimum of the key over the G candidates of a grid line, the candidate's d2 raised by the squared
 *   offset along the line.  Integers only, no atomics, nothing allocated (legal inside hipGraph capture): one right answer, bit for
 *   bit, the same from run to run.
 *   SE_ERR_BAD_ARG: a null pointer, batch outside 1..65535, grid outside 2..128, scratch_bytes too small, a scratch that is not
 *   8-byte aligned, a d2 / nearest that is not 4-byte aligned.
 *
 * EXPECTATION, se_scene_expect_f32, per row r = b * rows_per_frame + j:
 *   prob [rows][voxels] float32     d2 [rows / rows_per_frame][voxels] int32, as se_scene_distance_i32 writes it
 *   free_mask [rows / rows_per_frame][voxels] uint8, as se_scene_free_mask_u8 writes it (any non-zero byte is free, 0 is BLOCKED)
 *   radii2 [K] int32 on the device, 1 <= K <= 8, ascending by convention (the sums do not depend on their order)
 *   out [rows][24] float32, NOT divided (the kernel does no division):
 *     0          sum_n p_n
 *     1          sum_n p_n [blocked_n]
 *     2          sum_n p_n * sqrtf((float)d2_n) over the voxels with d2_n != 0x7fffffff (they have a nearest site); the product is
 *                rounded to float32, then added (unfused)
 *     3          slot 2 over the free voxels alone
 *     4 + k      sum_n p_n [d2_n <= radii2[k]], k < K (a voxel without a nearest site counts when radii2[k] is 0x7fffffff)
 *     12 + k     slot 4 + k over the free voxels alone
 *     the rest   0
 *   scratch: se_scene_expect_scratch_elems(rows) floats of workspace.
 * A row that holds a NaN probability (free or blocked) gets 24 NaNs; other rows are unaffected.  Two launches on `stream`
 * (se_sa_splits(rows) chunks per row as the soft-argmax, then one wave per row), a fixed reduction order and no atomics: bitwise
 * identical from run to run.  Allocates nothing (legal inside hipGraph capture).  rows <= 0, rows > 65535, rows_per_frame <= 0,
 * rows % rows_per_frame, voxels <= 0, voxels & 3, n_radii outside 1..8, a null pointer, a prob / d2 that is not 16-byte aligned or a
 * free_mask / radii2 that is not 4-byte aligned -> SE_ERR_BAD_ARG.                                                                  */
int se_scene_sites_u8(const float* depth, const double* ray_tab, unsigned char* sites, int batch, int depth_h, int depth_w, int height,
                      int width, int grid, double side, double min_z, double max_depth, void* stream);
long long se_scene_distance_scratch_bytes(int batch, int grid);
int se_scene_distance_i32(const unsigned char* sites, int* d2, int* nearest, void* scratch, long long scratch_bytes, int batch,
                          int grid, void* stream);
long long se_scene_expect_scratch_elems(int rows);
int se_scene_expect_f32(const float* prob, const int* d2, const unsigned char* free_mask, const int* radii2, float* out, float* scratch,
                        int rows, int rows_per_frame, int voxels, int n_radii, void* stream);

/* Multi-hypothesis joints (no counterpart in the reference; sceneego_amd/op.py: joint_modes; VoxelNetwork_depth.joint_modes drives
 * it): the K strongest local maxima (modes) of every softmaxed joint volume, each with the mass and the first moments of its
 * neighbourhood.  One right answer, bit for bit (tests/joint_modes_model.py restates it).
 *   prob   [rows][voxels] float32 probabilities, as se_softargmax3d_f32 writes them in mode 1; voxels = G^3, flat index
 *          n = (i G + j) G + k                                   coord  [voxels][3] float32 voxel-centre coordinates
 *   K in 1..16     radius in 0..3     min_prob >= 0
 * KEY        voxel n has the key (p_n, -n), compared lexicographically: a strict total order.
 * MODE       voxel n is a mode iff p_n > 0, p_n >= min_prob (equality counts) and its key is greater than the key of every
 *            neighbour: the up to 26 voxels with |di|, |dj|, |dk| <= 1 that lie inside the grid (nothing wraps from one row of the
 *            grid into the next).  Two equal adjacent voxels give one mode, the lower index; two equal voxels that are not adjacent
 *            are both modes; the zero tail of an underflowed softmax gives none.
 * SELECTION  the row's modes sorted by descending key (p descending, then index ascending); the first min(K, total) are selected.
 * WINDOW     of a selected mode at (i, j, k): every voxel m with |d| <= radius on each axis, clipped to the grid.
 *            mass = sum_m p_m, mom_a = sum_m p_m c_m,a (a = x, y, z): each sum accumulated in float64 in ASCENDING flat index m from
 *            the float32 values (the products are exact in float64) and rounded to float32 once at the end.  NOT divided: the kernel
 *            does no division; the caller divides by the mass.
 *   modes [rows][K][8] float32: 0 p_peak, 1 mass, 2..4 mom_x mom_y mom_z, 5..7 coord[index]
 *   index [rows][K] int32: the mode's flat index
 *   count [rows] int32: the number of selected modes, min(K, total)
 *   total [rows] int32: the number of modes in the row, uncapped (an exact integer)
 *   scratch: se_joint_modes_scratch_bytes(rows, G, K) bytes of workspace, 4-byte aligned (0 for rows <= 0 or a G / K out of range).
 * An unfilled record (slot >= count) has index -1, slots 0..4 equal to +0 and slots 5..7 NaN.  A row that holds a NaN probability
 * anywhere gets NaN in all its K x 8 slots, every index -1 and count = total = -1; other rows are unaffected.  Two launches on
 * `stream` (one workgroup per (row, tile of 4 i-planes x up to 256 / ceil(G / 4) j-rows) staged in LDS with a one-voxel halo, then
 * one wave per row), no atomics, selections under the total order and sums in a fixed order: bitwise identical from run to run.
 * Allocates nothing (legal inside hipGraph capture).  SE_ERR_BAD_ARG, with nothing launched: a null pointer, rows outside 1..65535,
 * G < 2, voxels != G^3, voxels & 3, K outside 1..16, radius outside 0..3, min_prob negative or NaN, a prob / coord that is not
 * 16-byte aligned, a scratch that is not 4-byte aligned or scratch_bytes below se_joint_modes_scratch_bytes(rows, G, K).           */
int se_joint_modes_f32(const float* prob, const float* coord, float* modes, int* index, int* count, int* total, void* scratch,
                       long long scratch_bytes, int rows, int voxels, int G, int K, int radius, float min_prob, void* stream);
long long se_joint_modes_scratch_bytes(int rows, int G, int K);

/* Grid Bayes filter over the joint volumes of a sequence (no counterpart in the reference; sceneego_amd/volume_filter.py:
 * VolumeFilter; VoxelNetwork_depth.volume_filter returns one).  A convention, not a calibrated model: the softmaxed volume is read as
 * the likelihood of the frame, a truncated Gaussian step as the motion model and a uniform floor as the chance of a jump.  The beliefs
 * have the shape and the meaning of the volumes.  tests/volume_filter_model.py restates the definition in float64.
 *   prob       [frames][rows][voxels] float32 probabilities, as se_softargmax3d_f32 writes them in mode 1; a row is one joint of one
 *              track, the frames are consecutive; voxels = G^3, flat index n = (i G + j) G + k
 *   coord      [voxels][3] float32 voxel-centre coordinates
 *   taps       [2 radius + 1] float32 on the DEVICE: w[d], d = -radius..radius, non-negative.  The caller computes them (float64
 *              exp(-(d h)^2 / (2 sigma^2)), h the voxel edge, normalised to sum 1, rounded to float32; sigma = 0 or radius = 0: {1}).
 *   state      [rows][voxels] float32.  In: the belief before the first frame of the call, read only for rows that have a prior.
 *              Out: the belief after the last frame.
 *   have_prior NULL (no row has a prior: the first call of a track) or int32 [rows] on the device: non-zero where `state` holds the
 *              row's prior.  It is read, never written; after any call every row has a prior.
 *   G in 2..128     radius in 0..min(16, G - 1)     floor in [0, 1]     rows in 1..65535     frames >= 1
 * PREDICT    q = blur3(b): the separable convolution with w along k, then j, then i, zero-padded (probability that leaves the grid is
 *            lost), then u = (1 - floor) q + floor / voxels.
 * UPDATE     a = p u,  Z = sum a,  b' = a / Z  (float32 division).
 * RESTART    a row restarts when it has no prior or when Z is not a finite number > 0.  Then b' = p, copied bit for bit whatever it
 *            holds: a row whose p holds a NaN restarts at this frame and again at the next.  Other rows are unaffected.
 *   belief_out NULL or [frames][rows][voxels] float32: b' of every frame
 *   joints     [frames][rows][3] float32: sum_n b'_n coord_n (computed as (sum a c) / Z; on a restart sum p c)
 *   evidence   [frames][rows] float32: Z, the predictive likelihood of the frame (1 / voxels is chance); NaN where the row had no
 *              prior; on a Z restart the offending value
 *   restarted  [frames][rows] int32: 1 where the row restarted
 *   scratch    se_volume_filter_scratch_bytes(rows, G, radius) bytes of workspace, 4-byte aligned (16-byte for the fast finish pass);
 *              0 for a shape out of range.  rows (G^3 + 8 G) floats.
 * The frames are processed in order inside the call: three launches per frame on `stream` (k- and j-blur of one i-plane per
 * workgroup in LDS; i-blur of one j-slab fused with the floor, the product and the partial sums; a finish pass that folds the partial
 * sums, decides the restart and writes b').  No atomics; every sum is taken in an order fixed by the shape alone, at most 80
 * sequential float32 additions on the longest path (volume_filter.hip states the order): bitwise identical from run to run and
 * independent of how the frames of a sequence are cut into calls.  Allocates nothing (legal inside hipGraph capture).
 * SE_ERR_BAD_ARG, with nothing launched: a null pointer other than belief_out / have_prior, a pointer that is not 4-byte aligned,
 * frames < 1, rows outside 1..65535, G outside 2..128, voxels != G^3, radius outside 0..min(16, G - 1), floor outside [0, 1] or NaN,
 * scratch_bytes below se_volume_filter_scratch_bytes(rows, G, radius).                                                              */
int se_volume_filter_f32(const float* prob, const float* coord, const float* taps, float* state, float* belief_out, float* joints,
                         float* evidence, int* restarted, void* scratch, long long scratch_bytes, int frames, int rows, int voxels,
                         int G, int radius, float floor, const int* have_prior, void* stream);
long long se_volume_filter_scratch_bytes(int rows, int G, int radius);

/* Forward-backward smoother over the joint volumes of a sequence: the backward pass that goes with se_volume_filter_f32
 * (sceneego_amd/volume_smoother.py: VolumeSmoother; VoxelNetwork_depth.volume_smoother returns one).  It adds no convention: motion
 * model, floor and restart rule are the filter's; only the frames a belief conditions on change (all of the track's, not 0..t).
 * tests/volume_smoother_model.py restates the definition in float64.
 *   prob       [frames][rows][voxels] float32: the volumes p_t the filter was given
 *   belief     [frames][rows][voxels] float32: the filter's belief_out b_t for the same frames
 *   restarted  [frames][rows] int32: the filter's output for the same frames
 *   coord, taps, G, radius, floor, rows, frames: as for se_volume_filter_f32.  blur3T below is blur3 with the taps REVERSED (w'[d] =
 *              w[-d]: the adjoint of blur3; the same for symmetric taps).  The call reverses them itself: pass the filter's taps.
 *   state      [rows][voxels] float32: the backward belief r.  In: r of the frame behind the call's last frame, read only for rows
 *              that have_link marks.  Out: r of the call's first frame.
 *   have_link  NULL (no row: the call ends the track) or int32 [rows] on the device: non-zero where the call's last frame is linked
 *              to the frame behind it, that is where that frame exists and its `restarted` is 0.
 * The frames of a call are processed from LAST to FIRST; a sequence is smoothed by calls over consecutive chunks in reverse order,
 * `state` carried from call to call.
 * LINK       frame t is linked to t + 1 unless t is the last frame of the track or restarted[t + 1][row] is set: a forward restart
 *            cuts the chain in both directions.
 * NO LINK    gamma_t = b_t and r_t = p_t, copied bit for bit; smoothed = 0, agreement NaN.
 * LINKED     u = (1 - floor) blur3T(r_{t+1}) + floor / voxels
 *            g = b_t u,  S = sum g,  gamma_t = g / S;   where S is not a finite number > 0: gamma_t = b_t (a copy), smoothed = 0
 *            a = p_t u,  s = sum a,  r_t = a / s;       where s is not a finite number > 0: r_t = p_t (a copy)
 *   smoothed_out NULL, or [frames][rows][voxels] float32: gamma_t of every frame.  It may be `belief` itself (in place); any other
 *              overlap with an input is the caller's error.
 *   joints     [frames][rows][3] float32: sum_n gamma_n coord_n (computed as (sum g c) / S; sum b c where gamma is the copy)
 *   agreement  [frames][rows] float32: S, how well the future's prediction for the frame agrees with the filtered belief (1 / voxels is
 *              chance); NaN where the row is not linked
 *   smoothed   [frames][rows] int32: 1 where gamma_t = g / S
 *   scratch    se_volume_smooth_scratch_bytes(rows, G, radius) bytes of workspace, 4-byte aligned (16-byte for the fast finish pass); 0
 *              for a shape out of range.  rows (2 G^3 + 8 G) floats and a few hundred bytes; the second G^3 array holds g and is
 *              reserved but left untouched by a call without smoothed_out.
 * One launch per call (the reversed taps) and three per frame on `stream`: the filter's k/j-blur kernel on r, an update kernel that
 * forms both products from one u, a finish pass.  No atomics; every sum is taken in the filter's fixed order, at most 80 sequential
 * float32 additions on the longest path: bitwise identical from run to run and independent of how the frames are cut into calls.
 * Allocates nothing.  SE_ERR_BAD_ARG, with nothing launched: a null pointer other than smoothed_out / have_link, a pointer that is not
 * 4-byte aligned, frames < 1, rows outside 1..65535, G outside 2..128, voxels != G^3, radius outside 0..min(16, G - 1), floor outside
 * [0, 1] or NaN, scratch_bytes below se_volume_smooth_scratch_bytes(rows, G, radius).                                               */
int se_volume_smooth_f32(const float* prob, const float* belief, const int* restarted, const float* coord, const float* taps,
                         float* state, float* smoothed_out, float* joints, float* agreement, int* smoothed, void* scratch,
                         long long scratch_bytes, int frames, int rows, int voxels, int G, int radius, float floor,
                         const int* have_link, void* stream);
long long se_volume_smooth_scratch_bytes(int rows, int G, int radius);

/* Transition statistics of the filter's motion model: the E-step sums of a Baum-Welch fit of (sigma, floor) to a sequence
 * (sceneego_amd/motion_fit.py: MotionModelFit; VoxelNetwork_depth.motion_fit returns one).  The transition (1 - floor) W_sigma +
 * floor / N is a two-component mixture whose Gaussian part is an exponential family in |d|^2, so the fit needs, per linked pair of
 * frames, the posterior mass of a step, of a jump and the posterior expected squared step.  This call is se_volume_smooth_f32's backward
 * walk with those sums in place of gamma; tests/motion_fit_model.py restates the definition in float64.
 *   prob, belief, restarted, taps, state, have_link, G, radius, floor, rows, frames: as for se_volume_smooth_f32, with the same link rule
 *   and the same order of the frames (last to first; a sequence by calls over consecutive chunks in reverse order).
 * With w' the taps reversed, m'[d] = (float)(d d) w'[d] (d = -radius..radius; one float32 rounding) and blur3(x; wk, wj, wi) the
 * zero-padded separable correlation along k, then j, then i with a tap vector per axis (blur3T(x) = blur3(x; w', w', w')):
 * LINKED     q0 = blur3(r_{t+1}; w', w', w')
 *            q2 = blur3(r_{t+1}; m', w', w') + blur3(r_{t+1}; w', m', w') + blur3(r_{t+1}; w', w', m')    the squared step, in voxels^2
 *            u = (1 - floor) q0 + floor / voxels,  a = p_t u,  s = sum a,  r_t = a / s;  where s is not a finite number > 0: r_t = p_t
 *            stats = { S = sum b_t u,  s,  A0 = sum b_t q0,  A2 = sum b_t q2,  Bsum = sum b_t,  Rsum = sum r_{t+1} }
 * NO LINK    r_t = p_t, copied bit for bit; the six stats are NaN.
 *   stats      [frames][rows][6] float32, in the order above.  With keep = 1 - floor and uniform = floor / voxels (float32, as the
 *              kernel forms them) the posterior of the pair (t, t + 1) holds step = keep A0 / S, jump = uniform Bsum Rsum / S
 *              (step + jump = 1 up to rounding) and sq = keep A2 / S, the expected squared step over the step component, in voxels^2.
 *              Bsum and Rsum are given so that the jump mass can be formed directly: at a small floor S - keep A0 cancels.
 *   linked     [frames][rows] int32: 1 where the frame was linked
 *   scratch    se_volume_transition_stats_scratch_bytes(rows, G, radius) bytes of workspace, 4-byte aligned (16-byte for the fast
 *              finish pass); 0 for a shape out of range.  rows (2 G^3 + 8 G) floats and a few hundred bytes.
 * q0 and u are formed exactly as se_volume_smooth_f32 forms them: `state` after the call and S equal that call's `state` and
 * `agreement` on the same inputs, bit for bit.  One launch per call (w' and m') and three per frame on `stream` (one for a frame in
 * which no row can be linked).  No atomics; every sum is taken in the filter's fixed order, at most 80 sequential float32 additions on
 * the longest path: bitwise identical from run to run and independent of how the frames are cut into calls.  Allocates nothing.
 * SE_ERR_BAD_ARG, with nothing launched: a null pointer other than have_link, a pointer that is not 4-byte aligned, frames < 1, rows
 * outside 1..65535, G outside 2..128, voxels != G^3, radius outside 0..min(16, G - 1), floor outside [0, 1] or NaN, scratch_bytes
 * below se_volume_transition_stats_scratch_bytes(rows, G, radius).                                                                  */
int se_volume_transition_stats_f32(const float* prob, const float* belief, const int* restarted, const float* taps, float* state,
                                   float* stats, int* linked, void* scratch, long long scratch_bytes, int frames, int rows,
                                   int voxels, int G, int radius, float floor, const int* have_link, void* stream);
long long se_volume_transition_stats_scratch_bytes(int rows, int G, int radius);

/* Trajectory samples: forward-filter backward-sampling on the model of se_volume_filter_f32 and se_volume_smooth_f32
 * (sceneego_amd/volume_smoother.py: VolumeSmoother.sample).  Joint draws from the posterior over whole trajectories of each row, given
 * the filtered beliefs.  It adds no convention: motion model, floor and link rule are the filter's and the smoother's.
 * tests/volume_sampler_model.py restates what follows in numpy float64 and index, kind and next are compared with it BIT FOR BIT: all
 * arithmetic is float64, one rounding per operation (no fused multiply-add), every sum SEQUENTIAL in ascending index.
 *   belief     [frames][rows][voxels] float32: the filter's belief_out b_t;  restarted [frames][rows] int32: the filter's output
 *   taps, G, radius, floor, rows, frames, voxels, flat index n = (i G + j) G + k: as for se_volume_filter_f32
 *   keep = (double)(1.0f - floor),  uniform = (double)(floor / (float)voxels)  (float32, as the filter forms them),  w[d] = (double)taps
 * TRANSITION from x at frame t to y at t + 1: (1 - floor) W(x -> y) + floor / N with W as blur3 has it, q(y) = sum_d w[d] b(y + d): the
 *            window of y is x = y + d with weight w[di] w[dj] w[dk], NO tap reversal, taps that leave the grid skipped.
 * CATEGORICAL DRAW over non-negative v_0..v_{n-1} with u in [0, 1): c_m = c_{m-1} + v_m, total = c_{n-1}; the first m with c_m > u total,
 *            or where rounding leaves none the last m with v_m > 0.  A value of 0 is never drawn.  A total that is not a finite number
 *            > 0: no draw.
 * GLOBAL DRAW from b_t with (u1, u2, u3): Rs[i][j] = sum_k b, P[i] = sum_j Rs[i][j], total_t = sum_i P[i]; i from P, j from Rs[i][.], k
 *            from b[i][j][.].  INVALID (index -1) when total_t is not a finite number > 0, a frame that holds a NaN for one.
 * WINDOW DRAW given y: r[di][dj] = sum_dk (double)b(y + d) w[dk],  q[di] = sum_dj r[di][dj] w[dj],  Wsum = sum_di q[di] w[di];
 *            step = keep Wsum, jump = uniform total_t, mass = step + jump.  A mass that is not a finite number > 0: the frame is drawn
 *            as an unlinked one.  Otherwise it is a jump iff u0 mass >= step: a global draw; else a step: di from q[di] w[di], dj from
 *            r[di][.] w[dj], dk from b(y + d) w[dk], with (u1, u2, u3).
 * CHAIN      per sample and row, last frame to first: a frame that is not linked takes a global draw (kind 2); a linked one the window
 *            draw (kind 0 a step, 1 a jump).  Frame t is linked to t + 1 unless t is the last frame of the track, restarted[t + 1] is
 *            set or the draw of t + 1 was invalid.
 * UNIFORMS   Philox4x32-10, key (seed_lo, seed_hi), counter (first_sample + sample, first_frame + frame, row, block).  A block's
 *            words give two uniforms, (double)((w0 << 32 | w1) >> 11) 2^-53 and the same of (w2, w3): block 0 u0, u1; block 1 u2, u3.
 *            The indices are GLOBAL: the result depends neither on how the frames are cut into calls nor on how the samples are split.
 *   next       [samples][rows] int32.  In: the voxel drawn for the frame behind the call's last frame, read only for rows that have_link
 *              marks (a value outside 0..voxels-1 links nothing).  Out: the voxel of the call's first frame, -1 when invalid.
 *   have_link  NULL or int32 [rows], as for se_volume_smooth_f32
 *   index      [samples][frames][rows] int32: x_t, -1 when invalid       kind  [samples][frames][rows] int32: 0, 1 or 2 (the branch taken)
 *   samples >= 1;  first_sample + samples and first_frame + frames at most 2^32, neither offset negative
 *   scratch    se_volume_sample_scratch_bytes(frames, rows, G) bytes, 8-byte aligned: Rs and P of every frame in float64,
 *              frames rows (G^2 + G) doubles; 0 for a shape out of range.  total_t is formed from P by the walk.
 * Two launches on `stream`: the sums of all frames of the call (one read of the beliefs), then the walk, one workgroup per (sample, row)
 * that loops over the frames from last to first inside the launch.  No atomics; bitwise identical from run to run.  Allocates nothing.
 * SE_ERR_BAD_ARG, with nothing launched: a null pointer other than have_link, a pointer that is not 4-byte aligned (scratch: 8-byte),
 * frames < 1, rows outside 1..65535, G outside 2..128, voxels != G^3, radius outside 0..min(16, G - 1), floor outside [0, 1] or NaN,
 * samples < 1, an offset out of range, scratch_bytes below se_volume_sample_scratch_bytes(frames, rows, G).                           */
int se_volume_sample_f32(const float* belief, const int* restarted, const float* taps, int* next, int* index, int* kind, void* scratch,
                         long long scratch_bytes, int frames, int rows, int voxels, int G, int radius, float floor, int samples,
                         long long first_sample, long long first_frame, unsigned int seed_lo, unsigned int seed_hi,
                         const int* have_link, void* stream);
long long se_volume_sample_scratch_bytes(int frames, int rows, int G);

/* Most probable joint trajectory: the max-product (Viterbi) pass that goes with se_volume_filter_f32 and se_volume_smooth_f32
 * (sceneego_amd/volume_viterbi.py: VolumeViterbi; VoxelNetwork_depth.volume_path returns one).  The filter and the smoother give per
 * frame the marginal of each joint; this gives the single most probable trajectory of each joint through the grid.
 * MODEL NOTE: it is the Viterbi recursion of the model whose transition score is max((1 - floor) W(d), floor / N), W the separable
 * product of the taps: within a factor of 2 of the filter's (1 - floor) W + floor / N, and separable.  No other convention is added.
 * tests/volume_viterbi_model.py restates the definition in numpy float32 and every output is compared with it BIT FOR BIT: all
 * arithmetic is float32, one rounding per operation (no fused multiply-add), in exactly the order below; float32 gradual underflow is
 * part of the definition (the library is built with denormals kept, hipcc's default for gfx950).
 *   prob, taps, G, radius, floor, rows, frames, voxels, flat index n = (i G + j) G + k: as for se_volume_filter_f32.
 *   keep = 1.0f - floor,  uniform = floor / (float)voxels   (floor rounded to float32 first)
 * STAGE      the maximum along one axis: best = 0.0f, offset 0; for d = -radius..radius ascending, skipping taps that leave the grid:
 *            cand = v[n + d] * w[d]; if cand > best, take it and d.  A NaN never wins (> is false), equal candidates keep the lowest
 *            d, all-zero keeps d = 0.
 * THREE STAGES along k, then j, then i, as in blur3, each on the values of the stage before: e3 = ((s w) w) w.  The winning offsets
 *            compose into the predecessor voxel y(x), x = (i, j, k):  i' = i + di(x);  j' = j + dj at (i', j, k);  k' = k + dk at
 *            (i', j', k).
 * STEP/JUMP  step = keep * e3(x),  jump = uniform * best_prev, best_prev the maximum of the previous frame's scaled scores at voxel
 *            peak_prev (lowest index among equals).  If jump > step: m = jump, predecessor peak_prev, jump bit set; otherwise m = step
 *            with predecessor y(x).
 * UPDATE     a = p(x) * m.  M = max a under the same rule (from 0.0f, strictly greater wins, ascending index: a NaN never wins, equals
 *            keep the lowest index), peak its index, e = ilogb(M), s = ldexpf(a, -e): an exact scaling but for underflow, best =
 *            ldexpf(M, -e) in [1, 2).  No division, no drift over long sequences.
 * RESTART    without a prior, or when M is not a finite number > 0: a = p, M, peak and e come from p, every back-pointer of the frame
 *            is -1 (segment start), restarted = 1.  If p has no finite positive maximum either: s = p unscaled, peak = -1, best = NaN,
 *            e = 0 and the next frame restarts.
 *   state      [rows][voxels] float32: the scaled scores s.  In: those before the call's first frame, read only for rows with a
 *              prior.  Out: those of the call's last frame.
 *   peak_state [rows] int32, best_state [rows] float32: peak and best that go with `state`, in / out like it
 *   have_prior NULL (no row has a prior: the first call of a track) or int32 [rows] on the device; a row has a prior where it is
 *              non-zero AND peak_state >= 0
 *   back_out   [frames][rows][voxels] int32: the predecessor's flat index, plus 1 << 30 for a jump, or -1
 *   peak, exponent, restarted [frames][rows] int32 and best [frames][rows] float32
 *   scratch    se_volume_viterbi_scratch_bytes(rows, G, radius) bytes, 4-byte aligned; 0 for a shape out of range.  rows (G^3 + 4 G)
 *              words and 2 rows G^3 bytes (the k and j offsets, int8).
 * Three launches per frame on `stream` (k and j stage of one i-plane per workgroup in LDS; i stage of one j-slab fused with the offset
 * composition, step or jump and the product; a fold of one (max, lowest index) record per workgroup) and one per call that scales the
 * state.  No atomics and no sums: every result is a product, a comparison or a selection under a total order, so the results are
 * bitwise identical from run to run and independent of how the frames are cut into calls.  Allocates nothing.
 * SE_ERR_BAD_ARG, with nothing launched: a null pointer other than have_prior, a pointer that is not 4-byte aligned, frames < 1, rows
 * outside 1..65535, G outside 2..128, voxels != G^3, radius outside 0..min(16, G - 1), floor outside [0, 1] or NaN, scratch_bytes below
 * se_volume_viterbi_scratch_bytes(rows, G, radius).
 *
 * se_volume_viterbi_path_i32: the back-walk over one stored chunk of `frames` frames, from its last frame to its first; a track is walked
 * by calls over its chunks LAST CHUNK FIRST.  x of the track's last frame is its peak; x_{t-1} = back_t[x_t] & (2^30 - 1); where frame
 * t starts a segment (restarted, back-pointer -1) x_{t-1} = peak_{t-1}.  A frame without a peak has index -1.
 *   cursor     [rows] int32, in / out: what the chunk's first frame points back to (< 0: the frame before it takes its own peak).  Read
 *              only with have_next = 1 (a later chunk was walked before); have_next = 0: the chunk's last frame ends the track.
 *   index      [frames][rows] int32: x_t          jumped  [frames][rows] int32: 1 where the path reached x_t by a jump
 * An index outside 0..voxels-1 found in `back` or `cursor` is never followed: the frame takes its own peak.  SE_ERR_BAD_ARG: a null or
 * misaligned pointer, frames < 1, rows outside 1..65535, voxels outside 1..128^3, have_next other than 0 / 1.
 *
 * se_volume_viterbi_refine_f32: joints [frames][rows][3] float32 from index [frames][rows]: the centroid of prob over the window
 * |delta| <= refine around x_t, clipped to the grid: float64 sums of p and p c in ascending flat index (as se_joint_modes_f32 does its
 * windows), NaN cells passed over, the quotient rounded once to float32.  Where the window sum is not a finite number > 0, or refine =
 * 0 (prob may then be NULL), the joint is the voxel centre; index -1 gives NaN.  refine in 0..3.  SE_ERR_BAD_ARG: a null or misaligned
 * pointer, frames < 1, rows outside 1..65535, G outside 2..128, voxels != G^3, refine outside 0..3.                                   */
int se_volume_viterbi_f32(const float* prob, const float* taps, float* state, int* peak_state, float* best_state, int* back_out,
                          int* peak, float* best, int* exponent, int* restarted, void* scratch, long long scratch_bytes, int frames,
                          int rows, int voxels, int G, int radius, float floor, const int* have_prior, void* stream);
long long se_volume_viterbi_scratch_bytes(int rows, int G, int radius);
int se_volume_viterbi_path_i32(const int* back, const int* peak, const int* restarted, int* cursor, int* index, int* jumped,
                               int frames, int rows, int voxels, int have_next, void* stream);
int se_volume_viterbi_refine_f32(const float* prob, const float* coord, const int* index, float* joints, int frames, int rows,
                                 int voxels, int G, int refine, void* stream);

/* Runner-up trajectories: the backward max-product pass over the sequence (VolumeViterbi(alternatives=True).alternatives()).  The
 * MAX-MARGINAL mm_t(x) is the score of the best whole trajectory that is at voxel x in frame t: mm_t = alpha_t beta_t with alpha the
 * forward scores above and beta_t(x) = max over z of tr(x -> z) p_{t+1}(z) beta_{t+1}(z).  From it follow, exactly and
 * deterministically, the margin by which each frame of the path was decided, the best trajectory that is somewhere else in a frame,
 * and the runner-up trajectory of a segment.  tests/volume_viterbi_alternatives_model.py restates what follows in numpy float32 and
 * every output is compared with it BIT FOR BIT; arithmetic, rounding and underflow as for se_volume_viterbi_f32.
 *
 * se_volume_viterbi_keep_f32: se_volume_viterbi_f32 with one more output, scores_out [frames][rows][voxels] float32: the frame's
 * scores as `state` holds them after the frame's fold pass, the raw a, or the copy of p on a restart; ldexpf(scores, -exponent) is
 * the scaled s of the frame.  Every other output has the bits se_volume_viterbi_f32 gives; scratch as there; scores_out NULL or
 * misaligned: SE_ERR_BAD_ARG.
 *
 * se_volume_viterbi_back_f32: the backward pass over one stored chunk of `frames` frames, from its last frame to its first; a track is
 * walked by calls over its chunks LAST CHUNK FIRST, the backward state carried in device memory between them.  Per frame t and row:
 * LINK       t is linked to t + 1 when t + 1 exists in the track (a later frame of the chunk, or have_next = 1), the forward pass
 *            did not restart at t + 1 and r_{t+1} has a finite positive maximum.  A forward restart cuts the chain in both directions.
 * UNLINKED   r_t = p_t and mm_t = s_t bit for bit (s_t = ldexpf(scores, -exponent_t)), every successor pointer -1, complete = 1.
 * LINKED     e3 = the THREE STAGES above (k, then j, then i) on the scaled r_{t+1} with the REVERSED taps w_rev[d] = w[-d]: the step
 *            from x to x + d has the score the forward pass gives the predecessor offset -d.  The winning offsets compose into the
 *            successor voxel z(x) as they compose into the predecessor there.  step = keep * e3(x), jump = uniform * best_r(t + 1).
 *            If jump > step: m = jump, successor peak_r(t + 1), jump bit set; otherwise m = step with successor z(x).
 *            r_t = p_t * m,  mm_t = s_t * m,  complete_t = complete_{t+1}.
 * RESCALING  of r as of a: M = max r (from 0.0f, strictly greater wins, lowest index among equals, a NaN never), e = ilogb(M),
 *            r <- ldexpf(r, -e), best_r = ldexpf(M, -e), peak_r its index.
 * DEATH      linked, but M is not a finite number > 0: the backward chain restarts here with r_t = p_t (M, e, peak from p), every
 *            successor pointer -1, the raw max-marginals NaN, and complete = 0 for this frame and, through the links, for every
 *            earlier frame of the segment.  The frame reports no max-marginal: the five outputs below are -1 / NaN.
 *   prob, taps, G, radius, floor: as for the forward pass.  scores: scores_out of se_volume_viterbi_keep_f32 for these frames;
 *   exponent, restarted: the forward pass's.  index [frames][rows]: the path x*_t of these frames (se_volume_viterbi_path_i32: the
 *   path call for a chunk precedes the backward call for it); a frame whose index is not in 0..voxels-1 has no path voxel: -1 / NaN.
 *   r_state [rows][voxels] float32, link_state [rows] int32 (peak_r of the chunk's first frame where the frame before it is linked
 *   to it, -1 otherwise), best_state [rows] float32, complete_state [rows] int32: in (read only with have_next = 1) / out.
 *   Outputs [frames][rows], all maxima under the one total order (greater value, then lower index; only values > 0 count):
 *   mm_best, mm_peak   the maximum of mm_t over the row and its voxel
 *   path_value         mm_t(x*_t)
 *   alt_value, alt_index  the maximum of mm_t over the voxels at Chebyshev distance in voxel indices > separation from x*_t: the
 *                      best trajectory that is somewhere else in this frame; -1 / NaN where the window leaves nothing > 0
 *   complete           1: the max-marginals of this frame span the whole segment behind it
 *   r_best, r_exponent best_r and e of the frame
 *   succ               NULL or [frames][rows][voxels] int32: the successor's flat index, plus 1 << 30 for a jump, or -1.  It MAY BE
 *                      THE MEMORY OF `scores`: a thread reads a voxel's score before it writes that voxel's pointer.
 *   max_marginals      NULL or [frames][rows][voxels] float32: the raw mm_t
 *   scratch            se_volume_viterbi_back_scratch_bytes(rows, G, radius) bytes, 4-byte aligned; 0 for a shape out of range
 * Three launches per frame (the k / j stage kernel of the forward pass, unchanged, on r with the reversed taps; the i stage fused with
 * the composition, step or jump, the two products, the window test and four (max, lowest index) records per workgroup; the fold) and
 * two per call.  No atomics and no sums: bitwise reproducible and independent of how the frames are cut into chunks.  BYTE MODEL per
 * frame, row and voxel: the forward pass's 28 B, the scores read (4 B) and the pointers written (4 B): 36 B; 4 B more with
 * max_marginals.  SE_ERR_BAD_ARG, with nothing launched: a null pointer other than succ and max_marginals, a pointer that is not
 * 4-byte aligned, the shape limits of the forward pass, separation < 0, have_next other than 0 / 1, a short scratch.
 *
 * se_volume_viterbi_branch_i32: one lane per row over one stored chunk: from the anchors (anchor [frames][rows] int32: a voxel at the
 * anchor frame of a segment, -1 elsewhere) back through `back` to the segment's start and on through `succ` to its end.
 *   direction -1   chunks LAST FIRST: x = the anchor, or what the frame behind points back to; index = x (-1: no branch passes),
 *                  jumped from the back-pointer at x; a restarted frame ends the walk.  Writes every frame.  cursor [rows]: x carried.
 *   direction +1   afterwards, chunks FIRST TO LAST: from the anchor, x_{t+1} = succ_t[x_t] & (2^30 - 1), jumped_{t+1} its jump bit;
 *                  writes the frames it reaches and leaves the anchors' own.  cursor [rows]: the successor pointer carried.
 *   have_carry     0: the first call of a direction; 1: cursor is read.
 * An index outside 0..voxels-1 found in anchor, back, succ or cursor is never followed.  SE_ERR_BAD_ARG: a null or misaligned pointer,
 * frames < 1, rows outside 1..65535, voxels outside 1..128^3, direction other than -1 / +1, have_carry other than 0 / 1.            */
int se_volume_viterbi_keep_f32(const float* prob, const float* taps, float* state, int* peak_state, float* best_state, int* back_out,
                               int* peak, float* best, int* exponent, int* restarted, float* scores_out, void* scratch,
                               long long scratch_bytes, int frames, int rows, int voxels, int G, int radius, float floor,
                               const int* have_prior, void* stream);
int se_volume_viterbi_back_f32(const float* prob, const float* scores, const int* exponent, const int* restarted,
                               const int* index, const float* taps, float* r_state, int* link_state, float* best_state,
                               int* complete_state, float* mm_best, int* mm_peak, float* path_value, float* alt_value, int* alt_index,
                               int* complete, float* r_best, int* r_exponent, int* succ, float* max_marginals, void* scratch,
                               long long scratch_bytes, int frames, int rows, int voxels, int G, int radius, float floor,
                               int separation, int have_next, void* stream);
long long se_volume_viterbi_back_scratch_bytes(int rows, int G, int radius);
int se_volume_viterbi_branch_i32(const int* back, const int* succ, const int* restarted, const int* anchor, int* cursor, int* index,
                                 int* jumped, int frames, int rows, int voxels, int direction, int have_carry, void* stream);

/* Skeleton-coupled joints: sum-product belief propagation over the kinematic tree of the joint volumes, with a spherical-shell
 * bone-length factor on every edge (sceneego_amd/skeleton_prior.py: SkeletonPrior; VoxelNetwork_depth.skeleton_prior returns one).  The
 * reference forces bone lengths onto a finished pose (utils/skeleton.py: kinematic_parents, _skeleton_resize); this couples the whole
 * distributions inside one frame - the in-frame counterpart of se_volume_filter_f32.  A convention, not a calibrated model: the softmaxed
 * volume is read as a likelihood, a Gaussian shell of width tau as the bone model and a uniform floor as the chance that the bone prior
 * is wrong for an edge.  The beliefs have the shape and the meaning of the volumes.  tests/skeleton_prior_model.py restates the
 * definition in float64.
 * TREE       J joints, 1..32; parent[j] < j for j >= 1 and parent[0] = 0 (HOST int array, read during the call).  ch(j): the children of j
 *            in ascending order.  The reference's kinematic_parents {0,0,1,2,0,4,5,1,7,8,9,4,11,12,13} is one; the fifteenth line of its
 *            Skeleton.lines, hip to hip (7, 11), closes a loop and is not part of the tree.
 * TAPS       [rows][(2R+1)^3] float32 on the DEVICE, row j the edge parent[j] -> j (row 0 is unused), dense, index
 *            ((di+R)(2R+1) + dj+R)(2R+1) + dk+R.  The caller computes them in float64 and rounds to float32:
 *            w(d) = exp(-(|d| h - L_j)^2 / (2 tau^2)), exactly 0 where | |d| h - L_j | > 3 tau, normalised to sum 1; h the voxel edge.
 *            R in 0..min(24, G - 1) covers every edge: R = ceil((max L + 3 tau) / h).
 * CORRELATE  corr(a, w)(x) = sum over d with w(d) != 0 and x + d inside the grid of w(d) a(x + d): zero-padded (mass that leaves the grid
 *            is lost), exact-zero taps are skipped.  The Python layer builds symmetric taps (w(d) = w(-d)), so one operator serves both
 *            directions; the entry points do not check the symmetry.
 * UPWARD     j = J-1 .. 1:  A_j = p_j prod_{c in ch(j)} U_c,  s_j = sum A_j,  U_j = (1 - floor) corr(A_j, w_j) / s_j + floor / N
 * DOWNWARD   j = 0 .. J-1 (D_0 absent):  T_j = p_j D_j prod_c U_c,  Z_j = sum T_j,  b_j = T_j / Z_j,  joints_j = (sum T_j coord) / Z_j;
 *            then for each child c:  E = p_j D_j prod_{c' != c} U_c',  t_c = sum E,  D_c = (1 - floor) corr(E, w_c) / t_c + floor / N
 *            Products are taken left to right (p, D, the U in ascending order) in float32; 1 - floor and floor / N are float32.
 * FALLBACK   a frame falls back when any of its s_j, t_c, Z_j is not a finite number > 0 (a NaN or inf anywhere in the frame's volumes
 *            gets there through the sums).  Then all J beliefs of that frame are p, copied bit for bit, joints = sum p coord and
 *            coupled = 0; evidence still holds the Z_j as computed.  Other frames are unaffected.
 *   prob       [frames][J][voxels] float32 probabilities; voxels = G^3, flat index n = (i G + j) G + k; frames are independent
 *   coord      [voxels][3] float32 voxel-centre coordinates
 *   beliefs    NULL or [frames][J][voxels] float32         joints  [frames][J][3] float32
 *   evidence   [frames][J] float32: Z_j, how well joint j's own volume agrees with what the rest of the skeleton predicts for it
 *   coupled    [frames] int32: 1, or 0 where the frame fell back
 *   scratch    se_skeleton_couple_scratch_bytes(frames, J, G, R) bytes, 4-byte aligned; 0 for a shape out of range.  About 3 J G^3
 *              floats for each of min(frames, 4) frames: longer calls walk their frames in groups of four.
 * The tree is processed by depth level: per level a product-and-sum pass, a fold of the sums and one correlation launch for all the
 * level's edges and frames (33 launches and one for the run table with the reference tree, per group of four frames).  No atomics; every sum
 * is taken in an order fixed by the shape and the taps alone (skeleton_prior.hip states it): a correlation output is a chain of at most
 * SE_SK_SHELL_CHAIN(R) roundings, a row sum one of at most SE_SK_SUM_CHAIN.  Bitwise identical from run to run and independent of how
 * frames are batched into calls.  Allocates nothing (legal inside hipGraph capture).
 * SE_ERR_BAD_ARG, with nothing launched: a null pointer other than beliefs, a pointer that is not 4-byte aligned, J outside 1..32,
 * parent[0] != 0 or a parent[j] outside 0..j-1, G outside 2..128, voxels != G^3, R outside 0..min(24, G - 1), floor outside [0, 1] or
 * NaN, frames < 1, scratch_bytes below se_skeleton_couple_scratch_bytes(frames, J, G, R).
 *
 * se_shell_correlate_f32 is the hot path on its own:  out[r] = scale_mul * corr(a[r], taps[tap_row[r]]) / s[r] + add  for `rows`
 * volumes a[r] of G^3 float32 (computed as fmaf(scale_mul, corr / s[r], add)); s [rows] float32 and tap_row [rows] int32 are read from
 * DEVICE memory; taps [tap_rows][(2R+1)^3].  A tap_row outside 0..tap_rows-1 fills its row with NaN.  scratch:
 * se_shell_correlate_scratch_bytes(tap_rows, R) bytes for the run table (per column of a block the first and the last run of non-zero
 * taps), built by a small launch before the correlation.  SE_ERR_BAD_ARG: a null or misaligned pointer, out == a, rows or tap_rows
 * outside 1..65535, G outside 2..128, R outside 0..min(24, G - 1), a short scratch.                                                  */
#define SE_SK_SHELL_CHAIN(R) ((2 * (R) + 1) * (2 * (R) + 1) + 2 * (R))
#define SE_SK_SUM_CHAIN 142
int se_shell_correlate_f32(const float* a, const float* taps, const int* tap_row, const float* s, float* out, void* scratch,
                           long long scratch_bytes, int rows, int tap_rows, int G, int R, float scale_mul, float add, void* stream);
long long se_shell_correlate_scratch_bytes(int tap_rows, int R);
int se_skeleton_couple_f32(const float* prob, const float* coord, const float* taps, const int* parent, float* beliefs, float* joints,
                           float* evidence, int* coupled, void* scratch, long long scratch_bytes, int frames, int J, int voxels, int G,
                           int R, float floor, void* stream);
long long se_skeleton_couple_scratch_bytes(int frames, int J, int G, int R);

/* Edge statistics of the skeleton model: the E-step sums of an EM fit of the bone lengths, tau and floor to a sequence
 * (sceneego_amd/skeleton_fit.py: SkeletonModelFit; VoxelNetwork_depth.skeleton_fit returns one).  The edge factor (1 - floor) w_L,tau(d)
 * + floor / N is a two-component mixture whose shell part is an exponential family in (|d|, |d|^2) on a fixed set of taps.  Everything
 * not stated here is se_skeleton_couple_f32's: the TREE, the TAPS layout, the zero-padded CORRELATE, the floor, the product order and
 * the FALLBACK rule.  tests/skeleton_fit_model.py restates the definition in float64.
 *   taps       block c is w_c.  taps_r, taps_r2: the same layout, w1_c = float32(w64_c r) and w2_c = float32(w64_c r^2), r(d) = |d| h in
 *              metres and w64_c the float64 block before rounding, computed by the caller.  A tap with w_c(d) == 0 is skipped in all three
 *              blocks: the run table is built from w_c alone.
 * Per frame and edge c = 1..J-1, with A_c, s_c (upward), E_c = p_j D_j prod_{c' != c} U_c', t_c (downward, j = parent[c]) and Z_j as in
 * se_skeleton_couple_f32:
 *   S0 = sum_x E_c(x) corr(A_c, w_c)(x),  S1 = sum_x E_c(x) corr(A_c, w1_c)(x),  S2 = sum_x E_c(x) corr(A_c, w2_c)(x),
 *   SJ = ((floor / N) t_c) s_c   in float32, floor / N as the coupling forms it.
 * The posterior mass of a shell step on the edge is m = (1 - floor) S0 / ((1 - floor) S0 + SJ), of a jump 1 - m; the expected bone
 * length given a step is S1 / S0 and its square S2 / S0.  (1 - floor) S0 + SJ = s_c Z_parent(c), and the frame's likelihood is
 * ln Z_0 + sum_{c >= 1} ln s_c: the quotients are left to the caller, in float64.
 *   stats      [frames][J][4] float32: S0, S1, S2, SJ; row 0 is zero
 *   norms      [frames][J][3] float32: s_j, t_j, Z_j; s_0 and t_0 are NaN (the root sends no message and receives none)
 *   valid      [frames] int32: 0 where se_skeleton_couple_f32 would fall back.  The statistics of such a frame are written as computed.
 *   scratch    se_skeleton_edge_stats_scratch_bytes(frames, J, G, R) bytes, 4-byte aligned; 0 for a shape out of range.  About 4 J G^3
 *              floats for each of min(frames, 4) frames (E_c can no longer overwrite A_c) and 16 J (2R+1)^3 bytes for the three tap
 *              blocks interleaved.
 * It is se_skeleton_couple_f32's two passes by depth level on the same product, fold and correlation kernels, so Z equals that call's
 * `evidence` and valid its `coupled`, bit for bit; one moments launch follows each downward level, no belief is formed and no volume is
 * written for the statistics.  No atomics.  Each of the three correlation values behind S0, S1, S2 is a chain of at most
 * SE_SK_SHELL_CHAIN(R) roundings; behind it a lane folds its four outputs with e(x) by fused multiply-adds (4), the workgroup folds its
 * lanes (6 + 2), and one wave folds the row's G ceil(G / 16) ceil(G / 64) workgroup records: lane l takes records l, l + 64, ... in
 * sequence, then a butterfly (6): SE_SK_MOMENT_CHAIN(G) roundings on the longest path, 22 at 64^3.  The order depends on (G, R) and
 * the taps alone: bitwise identical from run to run and independent of how frames are batched into calls.  Allocates nothing.
 * SE_ERR_BAD_ARG, with nothing launched: as se_skeleton_couple_f32, for its own pointers (none may be null) and scratch size.
 *
 * se_shell_moments_f32 is the hot path on its own: out[r] = (S0, S1, S2) of the `rows` pairs (e[r], a[r]) of G^3 float32 with the blocks
 * tap_row[r] (int32 [rows] on the DEVICE) of taps, taps_r, taps_r2 [tap_rows][(2R+1)^3]; out [rows][3] float32.  A tap_row outside
 * 0..tap_rows-1 gives NaN for its row.  scratch: se_shell_moments_scratch_bytes(rows, tap_rows, G, R) bytes (the run table, the
 * workgroup records and the interleaved taps).  SE_ERR_BAD_ARG: a null or misaligned pointer, rows or tap_rows outside 1..65535, G
 * outside 2..128, R outside 0..min(24, G - 1), a short scratch.                                                                      */
#define SE_SK_MOMENT_CHAIN(G) (18 + ((G) * (((G) + 15) / 16) * (((G) + 63) / 64) + 63) / 64)
int se_shell_moments_f32(const float* e, const float* a, const float* taps, const float* taps_r, const float* taps_r2,
                         const int* tap_row, float* out, void* scratch, long long scratch_bytes, int rows, int tap_rows, int G, int R,
                         void* stream);
long long se_shell_moments_scratch_bytes(int rows, int tap_rows, int G, int R);
int se_skeleton_edge_stats_f32(const float* prob, const float* taps, const float* taps_r, const float* taps_r2, const int* parent,
                               float* stats, float* norms, int* valid, void* scratch, long long scratch_bytes, int frames, int J,
                               int voxels, int G, int R, float floor, void* stream);
long long se_skeleton_edge_stats_scratch_bytes(int frames, int J, int G, int R);

/* Pose samples: ancestral draws of whole poses from the posterior of se_skeleton_couple_f32's model (sceneego_amd/skeleton_prior.py:
 * SkeletonPrior.sample).  That posterior is prod_j p_j(x_j) prod_c F_c(x_parent(c), x_c), normalised, with the edge factor
 * F_c(x, y) = (1 - floor) w_c(y - x) + floor / N for y inside the grid: CORRELATE's own orientation, the child is y = x_parent + d with
 * weight taps[c][d], NO tap reversal.  With the upward products A_j = p_j prod_{c in ch(j)} U_c ancestral sampling is exact:
 *     x_0 ~ A_0;   x_c ~ A_c(y) F_c(x_parent(c), y)  for c = 1..J-1 ascending (parent[c] < c),
 * and the marginals of the samples are the coupling's beliefs.  It adds no convention to the coupling's.  Everything not stated here
 * is se_skeleton_couple_f32's: the TREE, the TAPS layout, CORRELATE, the floor and the product order.  Two entry points.
 *
 * se_skeleton_upward_f32: the UPWARD pass of se_skeleton_couple_f32 on the same product, fold, run-table and correlation kernels, and
 * one level more, the root's product A_0 = p_0 prod_c U_c with its sum (the coupling forms it in its downward pass, as T_0).
 *   upward     [frames][J][voxels] float32: A_j.  It must not be prob.
 *   sums       [frames][J] float32: s_j = sum A_j, also for j = 0.  For j >= 1 they equal se_skeleton_edge_stats_f32's norms[..][0] and
 *              s_0 equals se_skeleton_couple_f32's evidence[..][0], bit for bit.
 *   valid      [frames] int32: 1 iff every s_j, j = 0..J-1, is a finite number > 0.  WEAKER than the coupling's FALLBACK rule, which also
 *              looks at t_c and Z_j: coupled = 1 implies valid = 1, not the other way round.
 *   scratch    se_skeleton_upward_scratch_bytes(frames, J, G, R) bytes, 4-byte aligned; 0 for a shape out of range.  About J G^3 floats
 *              (the messages U) for each of min(frames, 4) frames: longer calls walk their frames in groups of four, and the result
 *              does not depend on the grouping.
 * SE_ERR_BAD_ARG, with nothing launched: as se_skeleton_couple_f32, for this call's own pointers (none may be null) and scratch size.
 *
 * se_skeleton_sample_f32: `samples` poses per frame from the A_j.  tests/skeleton_sampler_model.py restates what follows in numpy
 * float64 and index and kind are compared with it BIT FOR BIT: all arithmetic is float64, one rounding per operation (no fused
 * multiply-add), every sum SEQUENTIAL in ascending index.  keep = (double)(1.0f - floor), uniform = (double)(floor / (float)voxels)
 * (float32, as the coupling forms them).  CATEGORICAL DRAW and the 53-bit uniforms: as for se_volume_sample_f32.
 * SUMS       Rs[i][j] = sum_k A, P[i] = sum_j Rs[i][j] of every (frame, joint): se_volume_sample_f32's sums pass with rows = J.
 * GLOBAL DRAW from A_j with (u1, u2, u3): i from P, j from Rs[i][.], k from A[i][j][.]; total_j is the last running sum of P.  INVALID
 *            (index -1) when total_j is not a finite number > 0.
 * WINDOW DRAW of child c given the parent's voxel x, over the taps d that stay inside the grid (clipped ranges per axis, ascending):
 *            v(d) = (double)A_c(x + d) (double)taps[c][d], an exact product; v(d) = 0 where the tap is exactly 0 WHATEVER A_c holds there
 *            (a NaN under a zero tap is passed over in these sums, as CORRELATE skips zero taps; it never shows in index or kind,
            because total_c below is formed from the whole volume and holds that NaN: such a joint has no usable mass either way);
            r[di][dj] = sum_dk v,  q[di] = sum_dj r[di][dj],
 *            Wsum = sum_di q[di];  step = keep Wsum, jump = uniform total_c, mass = step + jump.  A mass that is not a finite number
 *            > 0: the joint is drawn as an unlinked one.  Otherwise it is a jump iff u0 mass >= step: a global draw from A_c; else a
 *            step: di from q, dj from r[di][.], dk from v(di, dj, .), with (u1, u2, u3).
 * CHAIN      per sample and frame, j = 0..J-1 ascending: the root and every joint whose parent's draw is invalid take a global draw
 *            (kind 2); a linked joint the window draw (kind 0 a step, 1 a jump; an unusable mass gives kind 2).
 * UNIFORMS   Philox4x32-10, key (seed_lo, seed_hi), counter (first_sample + sample, first_frame + frame, joint, block); block 0 gives
 *            u0, u1 and block 1 u2, u3.  The indices are GLOBAL: the result depends neither on how the frames are cut into calls nor
 *            on how the samples are split.  Sample s of 16 is sample s of 64.
 *   upward     [frames][J][voxels] float32, non-negative: se_skeleton_upward_f32's.  Read only.
 *   valid      NULL (every frame is valid) or [frames] int32: a frame with valid[f] == 0 writes index -1 and kind 2 for every joint and
 *              sample, and the walk reads nothing of its `upward`.
 *   index      [samples][frames][J] int32: the flat voxel, -1 when invalid       kind  [samples][frames][J] int32: 0, 1 or 2
 *   samples >= 1;  first_sample + samples and first_frame + frames at most 2^32, neither offset negative
 *   scratch    se_skeleton_sample_scratch_bytes(frames, J, G) bytes, 8-byte aligned: frames J (G^2 + G) doubles; 0 out of range.
 * Two launches on `stream`: the sums, then the walk, one workgroup of 256 per (sample, frame) that loops over the joints inside the
 * launch; thread 0 of that workgroup writes index and kind.  No atomics; bitwise identical from run to run.  Allocates nothing.
 * SE_ERR_BAD_ARG, with nothing launched: a null pointer other than valid, a pointer that is not 4-byte aligned (scratch: 8-byte), J
 * outside 1..32, parent[0] != 0 or a parent[j] outside 0..j-1, G outside 2..128, voxels != G^3, R outside 0..min(24, G - 1), floor outside
 * [0, 1] or NaN, frames < 1, samples < 1, an offset out of range, scratch_bytes below se_skeleton_sample_scratch_bytes(frames, J, G). */
int se_skeleton_upward_f32(const float* prob, const float* taps, const int* parent, float* upward, float* sums, int* valid, void* scratch,
                           long long scratch_bytes, int frames, int J, int voxels, int G, int R, float floor, void* stream);
long long se_skeleton_upward_scratch_bytes(int frames, int J, int G, int R);
int se_skeleton_sample_f32(const float* upward, const int* valid, const float* taps, const int* parent, int* index, int* kind,
                           void* scratch, long long scratch_bytes, int frames, int J, int voxels, int G, int R, float floor, int samples,
                           long long first_sample, long long first_frame, unsigned int seed_lo, unsigned int seed_hi, void* stream);
long long se_skeleton_sample_scratch_bytes(int frames, int J, int G);

/* Most probable pose: the max-product pass over the kinematic tree that goes with se_skeleton_couple_f32, as se_volume_viterbi_f32
 * goes with the filter (sceneego_amd/skeleton_pose.py: SkeletonPose; VoxelNetwork_depth.skeleton_pose returns one).  The coupling gives
 * per joint a marginal and its expectation; this gives the single most probable configuration of all J joints of a frame under the same
 * model: the same TREE, the same TAPS (block j of the shells is the edge parent[j] -> j, unchanged) and the same floor.
 * MODEL NOTE: the score of an edge is max((1 - floor) w_j(d), floor / N), within a factor of 2 of the coupling's (1 - floor) w_j + floor /
 * N, as the Viterbi pass relates to the filter.  No other convention is added.
 * tests/skeleton_pose_model.py restates the definition in numpy float32 and every output is compared with it BIT FOR BIT: all arithmetic
 * is float32, one rounding per operation (no fused multiply-add), float32 gradual underflow is part of the definition.
 *   prob, taps, parent, G, R, floor, frames, J, voxels, flat index n = (i G + j) G + k: as for se_skeleton_couple_f32.  Domain: values
 *   >= 0 or NaN.   keep = 1.0f - floor,  uniform = floor / (float)voxels   (floor rounded to float32 first)
 * Joints are taken by depth level, deepest first.  Per joint j:
 * PRODUCT    A_j = p_j, then times m_c for each child c in ascending order: one rounding per factor, left to right.
 * ROW MAX    M_j = max A_j taken from 0.0f: a strictly greater value wins, the lowest index wins among equals, a NaN never wins; peak_j
 *            is the winning index.
 * RESCALE    e_j = ilogb(M_j),  s_j = ldexpf(A_j, -e_j): exact but for underflow,  best_j = ldexpf(M_j, -e_j) in [1, 2).  Unscaled, a
 *            leaf-to-root product at 64^3 underflows float32 many times over.
 * MESSAGE    to the parent, j > 0:  e3_j(x) = max over d with w_j(d) != 0 and x + d inside the grid of s_j(x + d) * w_j(d), from 0.0f,
 *            cand > best takes it: a value that does not depend on the order of the taps.  Its argument is the LOWEST TAP INDEX among
 *            the taps that attain it (taps count di, then dj, then dk ascending: the lowest child voxel), -1 when e3_j(x) = 0.
 *            step = keep * e3_j(x),  jump = uniform * best_j.  Where jump > step: m_j(x) = jump and the predecessor is peak_j, marked
 *            as a jump; otherwise m_j(x) = step and the predecessor is x + d*.
 * BACK-WALK  x_0 = peak_0; for j = 1..J-1 ascending x_j is the predecessor of edge j at x_parent(j).
 * FALLBACK   a frame in which some M_j is not a finite number > 0 is not solved: solved = 0, every joint takes the peak of its own p_j
 *            by the ROW MAX rule (index -1 where p_j has none), jumped = 0, exponent = 0, best_root = NaN.  Other frames are unaffected.
 *            A single NaN cell does NOT cause this: it never wins a maximum and is passed over (se_skeleton_couple_f32 differs: there
 *            a NaN reaches the sums and the frame falls back).
 *   index      [frames][J] int32: x_j                jumped  [frames][J] int32: 1 where edge j jumped (the root: 0)
 *   exponent   [frames][J] int32: e_j                best_root [frames] float32: best_0          solved [frames] int32
 *              log score of the pose = ln best_0 + ln 2 * sum_j e_j, for the caller to sum in float64
 *   scratch    se_skeleton_pose_scratch_bytes(frames, J, G, R) bytes, 4-byte aligned; 0 for a shape out of range.  About 2 J G^3 floats
 *              (A / s and m) for each of min(frames, 4) frames: longer calls walk their frames in groups of four.
 * Per level a product pass with one (max, lowest index) record per chunk, a fold of the records and one max-correlation launch for all
 * the level's edges and frames (the rescaling is applied as the source planes are staged); the back-walk recomputes the argument of
 * each edge at the one voxel it is needed at, by the same single multiplications (18 launches and one for the run table with the
 * reference tree, per group of four frames).  No atomics and no sums: bitwise identical from run to run and independent of how frames
 * are batched into calls.  Allocates nothing.
 * SE_ERR_BAD_ARG, with nothing launched: a null pointer, a pointer that is not 4-byte aligned, J outside 1..32, parent[0] != 0 or a
 * parent[j] outside 0..j-1, G outside 2..128, voxels != G^3, R outside 0..min(24, G - 1), floor outside [0, 1] or NaN, frames < 1,
 * scratch_bytes below se_skeleton_pose_scratch_bytes(frames, J, G, R).
 *
 * se_shell_maxcorr_f32 is the hot path on its own:  out[r](x) = scale_mul * e3(x)  with s = a[r] unscaled and w = taps[tap_row[r]], for
 * `rows` volumes of G^3 float32; tap_row [rows] int32 on the DEVICE; a tap_row outside 0..tap_rows-1 fills its row with NaN.  scratch:
 * se_shell_correlate_scratch_bytes(tap_rows, R) bytes, the same run table.  SE_ERR_BAD_ARG as se_shell_correlate_f32.
 * se_shell_argmax_i32: per row r and queried voxel query[q] (int32 [queries] on the device) out_tap[r][q] = the lowest attaining tap
 * index of e3 there, or -1, and out_value[r][q] = e3.  A tap_row or a query out of range gives -1 and NaN.  The back-walk uses the
 * same device function.  SE_ERR_BAD_ARG: a null or misaligned pointer, rows or tap_rows outside 1..65535, queries < 1, G outside
 * 2..128, R outside 0..min(24, G - 1).                                                                                                */
int se_shell_maxcorr_f32(const float* a, const float* taps, const int* tap_row, float* out, void* scratch, long long scratch_bytes,
                         int rows, int tap_rows, int G, int R, float scale_mul, void* stream);
int se_shell_argmax_i32(const float* a, const float* taps, const int* tap_row, const int* query, int* out_tap, float* out_value,
                        int rows, int queries, int tap_rows, int G, int R, void* stream);
int se_skeleton_pose_f32(const float* prob, const float* taps, const int* parent, int* index, int* jumped, int* exponent,
                         float* best_root, int* solved, void* scratch, long long scratch_bytes, int frames, int J, int voxels, int G,
                         int R, float floor, void* stream);
long long se_skeleton_pose_scratch_bytes(int frames, int J, int G, int R);

/* Runner-up poses: the downward max-product pass that goes with se_skeleton_pose_f32, as the downward sum-product pass goes with the
 * upward one in se_skeleton_couple_f32 (sceneego_amd/skeleton_pose.py: SkeletonPose.alternatives).  It gives for every joint and voxel
 * the MAX-MARGINAL, the score of the best whole pose that puts that joint there, and from it per joint (the ANCHOR) the best pose that
 * places the anchor outside a window around its voxel in the most probable pose.  Model, arguments, arithmetic and the ROW MAX rule are
 * se_skeleton_pose_f32's; tests/skeleton_alternatives_model.py restates the definition in numpy float32 and every output is compared
 * with it BIT FOR BIT.   separation = S >= 0: the half-width of the window, in voxels.
 * UPWARD     se_skeleton_pose_f32's pass, unchanged: A_j, M_j at peak_j, e_j, s_j = ldexpf(A_j, -e_j), m_j, the pose x*_j, solved.
 * DOWNWARD   joints by depth level, shallowest first; d_0 is absent.
 *            mu_0 = s_0;  mu_j = s_j * d_j for j > 0, one rounding: the max-marginal of j, scaled.
 *            Per child c of j:  E_c = p_j, then times d_j if j > 0, then times m_c' for every OTHER child c' of j in ascending order:
 *            one rounding per factor, left to right.   G_c = max E_c at epeak_c (ROW MAX),  q_c = ilogb(G_c),
 *            t_c = ldexpf(E_c, -q_c),  tbest_c = ldexpf(G_c, -q_c).   e3(y) = max over d with w_c(d) != 0 and y + d inside the grid of
 *            t_c(y + d) * w_c(d), with the lowest attaining tap d* (MESSAGE above: the same operator on the same block of taps, which
 *            is the transposed edge for taps with w_c(d) = w_c(-d), as sceneego_amd.skeleton_prior.shell_taps builds them; not checked).
 *            step = keep * e3(y),  jump = uniform * tbest_c,  d_c(y) = jump > step ? jump : step.  The parent voxel behind d_c(y) is
 *            epeak_c for a jump, otherwise y + d* (epeak_c where step = jump = 0: not reached from a value > 0).
 * EXPONENTS  returned as integers for the caller to sum:  Esub_j = e_j + sum over the children c of Esub_c;  F_0 = 0,
 *            F_c = F_parent(c) + q_c + sum over the siblings c' != c of Esub_c'.  The natural logarithm of the max-marginal of j at x is
 *            ln mu_j(x) + ln 2 * (Esub_j + F_j); in exact arithmetic its maximum over x is the log score of the pose, for every j.
 * RECORDS    mm_best_a at mm_peak_a: the ROW MAX of mu_a;  pose_value_a = mu_a(x*_a);  alt_value_a at alt_index_a: the ROW MAX of mu_a
 *            over the voxels whose Chebyshev distance in voxel indices from x*_a is > S (alt_index -1, alt_value 0: none is > 0).
 * WALK       anchor a with alt_index_a >= 0:  x_a = alt_index_a; up to the root, the parent of u takes the parent voxel behind d_u at
 *            x_u; then for j = 1..J-1 ascending and not yet set x_j is the predecessor of upward edge j at x_parent(j) (BACK-WALK
 *            above).  alt_jumped[a][j] = 1 where the edge parent[j] -> j was taken as a jump, in either direction.  In exact arithmetic
 *            this is the best pose with joint a outside the window and its score is alt_value_a with its exponent.  An anchor with
 *            alt_index -1 has an alt_pose row of -1.
 * FALLBACK   a frame that is not solved keeps se_skeleton_pose_f32's fallback outputs.  Such a frame, or one in which some G_c is not a
 *            finite number > 0, is not complete: complete = 0, alt_index, mm_peak and alt_pose -1, alt_value, mm_best and pose_value
 *            NaN, down_exponent and alt_jumped 0, its max_marginals rows p copied bit for bit.  Other frames are unaffected.  A single
 *            NaN cell does not cause this.
 *   index, jumped, exponent, best_root, solved: as se_skeleton_pose_f32 writes them, identical bits
 *   down_exponent [frames][J] int32: q_j (q_0 = 0)      mm_best, pose_value, alt_value [frames][J] float32
 *   mm_peak, alt_index [frames][J] int32                alt_pose, alt_jumped [frames][J][J] int32 (anchor, joint)
 *   complete   [frames] int32                           max_marginals [frames][J][voxels] float32 or NULL: mu_j as computed
 *   scratch    se_skeleton_alternatives_scratch_bytes(frames, J, G, R) bytes, 4-byte aligned; 0 for a shape out of range.  About
 *              4 J G^3 floats (A, m, E, d) for each of min(frames, 4) frames.
 * After the upward launches: per level below the root one product pass over all its (parent, child) pairs and frames, a fold of its
 * records and one max-correlation launch (the kernel and the instantiation of the upward pass: 2 (J - 1) max-correlations per frame in
 * all); then one record pass over mu, its fold, and the walks of all anchors side by side (grid anchors x frames).  No atomics and no
 * sums: bitwise identical from run to run and independent of how frames are batched into calls.  Allocates nothing.
 * SE_ERR_BAD_ARG, with nothing launched: as se_skeleton_pose_f32 (max_marginals may be NULL), separation < 0, max_marginals == prob,
 * scratch_bytes below se_skeleton_alternatives_scratch_bytes(frames, J, G, R).                                                       */
int se_skeleton_alternatives_f32(const float* prob, const float* taps, const int* parent, int separation, int* index, int* jumped,
                                 int* exponent, float* best_root, int* solved, int* down_exponent, float* mm_best, float* pose_value,
                                 float* alt_value, int* mm_peak, int* alt_index, int* alt_pose, int* alt_jumped, int* complete,
                                 float* max_marginals, void* scratch, long long scratch_bytes, int frames, int J, int voxels, int G,
                                 int R, float floor, void* stream);
long long se_skeleton_alternatives_scratch_bytes(int frames, int J, int G, int R);

/* Baseline JPEG encoder (no counterpart in the reference; sceneego_amd/jpeg_encode.py writes the file headers around it).
 *   frames    uint8 [batch][height][width][3] on the device, R, G, B (bgr = 0) or B, G, R (bgr = 1); any height, width in 1..65535
 *   quant_luma, quant_chroma   HOST pointers: unsigned short [64], natural order, every value in 1..255 (baseline tables)
 *   subsampling   444 or 420 (chroma averaged 2x2)           restart_rows   0: no restart markers; n: a restart interval of n MCU
 *             rows (n * MCUs per row <= 65535; n beyond the frame's MCU rows means one interval, the caller writes the DRI)
 *   out       uint8 [batch][capacity]: per frame the entropy-coded scan, with the 00 after every FF byte, the RSTm markers between
 *             intervals and the 1-bits that fill the last byte of every interval: what stands between the SOS header and EOI
 *   length    int32 [batch]: bytes of the frame's scan in out, 0 when it did not fit
 *   status    int32 [batch][2]: {0, scan bytes} or, when the scan needs more than `capacity`, {1, bytes needed}; nothing is ever
 *             written at or beyond `capacity` bytes of a frame's slot
 *   scratch   se_jpeg_encode_scratch_bytes(batch, height, width, subsampling) bytes of device workspace, 16-byte aligned; the
 *             helper allocates nothing and returns SE_ERR_BAD_ARG for a bad shape (more than 2^31 / 1664 blocks in a frame included)
 * Arithmetic (integer only, libjpeg's: jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c, jchuff.c; tests/jpeg_encode_model.py restates
 * it and the result equals libjpeg-turbo's byte for byte):
 *   colour    Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *             Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   edges     a plane's last column and row are replicated out to whole blocks.  4:2:0 chroma: sample (cy, cx) is
 *             (a + b + c + d + 1 + (cx & 1)) >> 2 of the pixels (min(2 cy', H-1) | min(2 cy'+1, H-1), min(2 cx, W-1) | min(2 cx+1,
 *             W-1)) with cy' = min(cy, ceil(H/2) - 1).  4:2:0 luma: an MCU holds 2x2 blocks; a block outside ceil(W/8) x ceil(H/8)
 *             has all AC coefficients zero and the DC of the block before it in the MCU (left neighbour; lower row: block 1)
 *   DCT       jfdctint.c for 8-bit samples minus 128 (CONST_BITS 13, PASS1_BITS 2, rows then columns)
 *   quantiser sign(c) * ((|c| + (8 q >> 1)) / (8 q))
 *   entropy   the four Annex K.3 Huffman tables; DC differences per component in MCU order, reset at every restart interval; runs of
 *             16 zeros as ZRL, EOB unless coefficient 63 is non-zero
 * Eight kernel launches on `stream`, nothing allocated, no memset node: legal under hipGraph capture; bitwise reproducible.
 * SE_ERR_BAD_ARG: a null pointer, a bad shape, batch outside 1..65535, subsampling not 444 / 420, a table value outside 1..255,
 * capacity < 0 or > 2^31-1, scratch too small or misaligned, restart_rows < 0 or an interval of more than 65535 MCUs. */
long long se_jpeg_encode_scratch_bytes(int batch, int height, int width, int subsampling);
int se_jpeg_encode_u8(const unsigned char* frames, int batch, int height, int width, int bgr, const unsigned short* quant_luma,
                      const unsigned short* quant_chroma, int subsampling, int restart_rows, unsigned char* out, long long capacity,
                      int* length, int* status, void* scratch, long long scratch_bytes, void* stream);

/* Lossless PNG encoder (no counterpart in the reference; sceneego_amd/png_encode.py writes the signature and the chunks around it).
 *   frames    uint8 [batch][height][width][channels] on the device; channels 3 (R, G, B: colour type 2) or 1 (gray: colour type 0);
 *             bit depth 8, no interlace; R = 1 + width * channels, height * R < 2^31
 *   out       uint8 [batch][capacity]: per frame the complete zlib stream (78 01, the deflate blocks, Adler-32), the payload of one IDAT
 *   capacity  at least se_png_encode_bound(height, width, channels) = 2 + sum over segments of (len + 10) + 4, which no stream exceeds
 *             (a segment is stored when no Huffman form is smaller); a smaller capacity is SE_ERR_BAD_ARG, so there is no retry path
 *   length    int32 [batch]: bytes of the frame's stream          status   int32 [batch][2]: {0, bytes}
 *   scratch   se_png_encode_scratch_bytes(batch, height, width, channels) bytes of device workspace, 16-byte aligned; the helpers
 *             allocate nothing and return SE_ERR_BAD_ARG for a bad shape
 * The bytes (integer rules only; DESIGN.md 4h2 states them, tests/png_encode_model.py restates them and the kernel equals it byte
 * for byte):
 *   filter    per row the filter 0..4 with the smallest sum of min(v, 256 - v) of its filtered bytes, ties to the lowest number
 *   segments  the filtered stream in pieces of 16384 bytes, one deflate block each
 *   parse     greedy over the candidate distances (1, channels; duplicates removed): the longest run (<= 258, not beyond the
 *             segment's end, never before the stream's first byte, but back into the segment before), the first listed among
 *             equals; a match from 3 bytes on
 *   codes     per segment minimum-redundancy lengths of the counted symbols sorted by (count, symbol), limited to 15 bits (7 for the
 *             code-length code) by miniz's Kraft repair; at least two coded distance symbols
 *   block     the smallest of the stored, fixed and dynamic forms by exact bit count, ties in that order; every block but the last
 *             is followed by an empty stored block unless it is stored itself, so segments join on byte boundaries
 * Four kernel launches on `stream`, nothing allocated, no memset node, no synchronisation: legal under hipGraph capture; bitwise
 * reproducible and independent of the batch a frame is in.
 * SE_ERR_BAD_ARG: a null pointer, batch outside 1..65535, a non-positive size, channels not 1 / 3, height * R >= 2^31, capacity below
 * the bound or above 2^31-1, scratch too small or misaligned, length / status misaligned. */
long long se_png_encode_scratch_bytes(int batch, int height, int width, int channels);
long long se_png_encode_bound(int height, int width, int channels);
int se_png_encode_u8(const unsigned char* frames, unsigned char* out, int* length, int* status, void* scratch, long long scratch_bytes,
                     int batch, int height, int width, int channels, long long capacity, void* stream);

/* Volume renderer (no counterpart in the reference; sceneego_amd/render.py: SceneRenderer.render_volumes / overlay_volumes): a
 * maximum-intensity projection of the 15 per-joint volumes along every pixel's ray, composited joint by joint over a picture
 * se_render_resolve_f64 / se_render_overlay_f64 made.  All arithmetic is float64, unfused, in the order written here
 * (tests/volume_render_model.py restates it).  `view` is a HOST pointer, read during the call; every other pointer is device memory.
 *   volumes  [B][15][G][G][G] float32 (x, y, z; z fastest), softmaxed or ReLU        packed  [B][G^3][16] float32, 16-byte aligned,
 *            se_render_volume_packed_bytes(batch, grid) bytes (-1: bad shape): cell-interleaved copy written by
 *            se_render_volume_pack_f32 (slot 15 is 0); the two marches read it, not `volumes`
 *   scale    [B][15] float64        joint_mask  bit j set: joint j is drawn.  Joint j of frame b is OFF when its bit is clear or
 *            scale[b][j] is not finite or <= 0
 *   rays     as for se_render_resolve_f64 (view: pinhole table, out_h x out_w) / se_render_overlay_f64 (overlay: the calibrated unit rays)
 *   base     the picture to draw over, uint8 (R, G, B), shape of out; may be `out` itself (in place)
 * Grid (op.build_coord_volume(G, S), camera frame): pos = (-(S / 2), -(S / 2), 0), h = S / (double)(G - 1); boundary k of axis a is
 *   bnd_a(k) = pos_a + ((double)k - 0.5) * h, cell i covers [bnd_a(i), bnd_a(i + 1)), the box is [bnd_a(0), bnd_a(G)) per axis.
 * Ray o + s d.  Overlay: o = 0, d = rays[y][x] (s is distance).  View, with R = view[0..8] row-major and t = view[9..11] (q = R p + t):
 *   o_i = -((R[0][i] t[0] + R[1][i] t[1]) + R[2][i] t[2]), d_i = (R[0][i] p.x + R[1][i] p.y) + R[2][i] p.z for the pinhole ray p (s is
 *   view-space z, the quantity in the z-buffer key).  A ray with a non-finite component misses.
 * Limit: +inf; view with zbuf != NULL: (double)(float of zbuf >> 32) unless the key is all-ones ("no point"); overlay with depth !=
 *   NULL: (double)depth[b][(y depth_h) / height][(x depth_w) / width]; a NaN limit misses (the rule of se_render_overlay_f64: shown
 *   only where s < depth).
 * Range: s0 = near, s1 = limit; per axis a = x, y, z: if d_a == 0 the ray misses unless bnd_a(0) <= o_a < bnd_a(G) (no division);
 *   else inv_a = 1 / d_a, ta = (bnd_a(0) - o_a) * inv_a, tb = (bnd_a(G) - o_a) * inv_a, tn = ta < tb ? ta : tb, tf = the other;
 *   if tn > s0: s0 = tn; if tf < s1: s1 = tf.  The ray misses unless s0 < s1.
 * Walk (Amanatides-Woo): start index i_a = floor(u) clamped into 0..G-1 with u = ((o_a + s0 * d_a) - pos_a) / h + 0.5 (a NaN: 0);
 *   step_a = sign(d_a); next_a = (bnd_a(i_a + (step_a > 0 ? 1 : 0)) - o_a) * inv_a, +inf when d_a == 0, recomputed from the index after
 *   every step (no running sum).  The start cell counts.  Then repeatedly: a = x; if next_y < next_a: a = y; if next_z < next_a: a = z
 *   (strict: of equal ones the first); stop unless next_a < s1 (the next cell's entry parameter); i_a += step_a; stop when it leaves
 *   0..G-1; the cell counts.
 * Maximum: m_j = max over the counted cells of (double)p_j[cell] * scale_j, taken as v > m from m = 0 (a NaN never wins; the kernel
 *   takes the float32 maximum and multiplies once, which is the same number for a scale > 0).
 * Composite: c = (double)base channel; for j = 0..14 ascending, joints that are not off: g = gain * m_j, a = (g < 1 ? g : 1) *
 *   opacity, c = c + a * ((double)palette[j][channel] - c); out = (uint8)floor(c + 0.5).  A miss, an all-zero volume and a zero mask
 *   leave the base picture byte for byte.
 * One launch each, nothing allocated, no memset node: legal under hipGraph capture; bitwise reproducible.
 * SE_ERR_BAD_ARG: a null pointer (zbuf / depth may be NULL: no occlusion), batch outside 1..65535, grid outside 2..1024, a
 *   non-positive size, packed misaligned or packed_bytes too small, cuboid_side <= 0, > 1e6 or NaN, near < 0, > 1e6 or NaN, gain < 0,
 *   > 1e30 or NaN,
 *   opacity outside [0, 1], a mask bit above 14, a non-finite view. */
/* per joint (R, G, B): the neck neutral, right-side joints (1-3, 7-10) warm, left-side joints (4-6, 11-14) cold */
#define SE_RENDER_VOLUME_PALETTE                                                                                                  \
    {{235, 235, 235}, {255, 60, 30}, {255, 120, 20}, {255, 185, 10}, {30, 90, 255}, {20, 160, 255}, {10, 225, 255}, {200, 20, 60}, \
     {230, 40, 120}, {250, 80, 170}, {255, 140, 210}, {70, 40, 210}, {40, 70, 160}, {20, 150, 150}, {40, 210, 130}}
void se_render_volume_palette(unsigned char* rgb /* HOST, 45 bytes */);
long long se_render_volume_packed_bytes(int batch, int grid);
int se_render_volume_pack_f32(const float* volumes, float* packed, long long packed_bytes, int batch, int grid, void* stream);
int se_render_volume_view_f64(const float* packed, const double* scale, const double* rays, const double* view,
                              const unsigned long long* zbuf, const unsigned char* base, unsigned char* out, int batch, int out_h,
                              int out_w, int grid, double cuboid_side, double near, unsigned int joint_mask, double gain,
                              double opacity, void* stream);
int se_render_volume_overlay_f64(const float* packed, const double* scale, const double* rays, const float* depth,
                                 const unsigned char* base, unsigned char* out, int batch, int height, int width, int depth_h,
                                 int depth_w, int grid, double cuboid_side, double near, unsigned int joint_mask, double gain,
                                 double opacity, void* stream);

#ifdef SE_DEVTOOLS
/* Development builds only (csrc/build.sh --devtools; absent from the production library): A/B kernel selection for
 * tools/bench_conv.py and the cycle-stamp diagnostics.  The selector is thread-local; 0 is the production dispatch.  Every number
 * chooses among kernels that production runs for some shape, or among instances of a production kernel template:
 *   float32 3D convolutions (se_conv3d_plan, csrc/conv3d.hip, states each once):
 *     1 - 9     no Winograd kernel (LDS-tiled direct, small-level and direct kernels)
 *     10 - 19   no 2-D Winograd kernel; 18 / 19: grid / in-workgroup split-K for every small level
 *     21 - 23   3^3 on the LDS-tiled direct kernel with 8 x 8 x {4, 8, 16} output tiles
 *     30        1-D F(4,3) in place of the 2-D Winograd kernels
 *     40        the production families;  64: the 2-D family stays on F(4,3) x F(2,3)
 *     41 - 60   3^3: experiment / attribution instances of the F(4,3) x F(2,3) kernel (csrc/conv3d_wino2d.hip)
 *     47        7^3: F(4,7) in place of F(6,7)
 *   bf16 3D convolutions (csrc/conv3d_bf16_tiled.hip): 1 = 7^3 on 8 x 8 x 8 tiles, 4 = 3^3 on 4 x 4 x 16 tiles, 5 = 7^3 dz-phase form
 *   2D convolutions (csrc/conv2d_1x1.hip, csrc/conv2d_3x3.hip): 73 - 79 */
void se_debug_set_variant(int variant);
/* u64 device buffer [workgroups][8 waves][6] ([8] for F(6,7)) that the cycle-stamp builds (-DSE_STAMPPP, -DSE_STAMP47, -DSE_STAMP67)
 * of the 1-D Winograd kernels fill; other builds never read it. */
void se_debug_set_stamp_buffer(void* device_buffer);
#endif

#ifdef __cplusplus
}
#endif
#endif /* SCENEEGO_HIP_H */
