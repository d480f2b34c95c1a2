/* cpr_hip.h -- C ABI of libcprhip.so: the MI355X (gfx950) kernels of the CPR / P2PNet point-localization hot path.
 *
 * Conventions:
 *   - every function returns 0, CPR_ERR_ARG (-1001, shape/pointer check failed), CPR_ERR_UNSUPPORTED (-1002) or
 *     -(hipError_t); nothing is thrown; the Python host raises RuntimeError on non-zero
 *   - all pointers are DEVICE pointers unless marked [host]; the caller allocates every output and workspace
 *     (no hidden allocation, no ownership transfer); the library keeps NO mutable state: every call is a pure function of
 *     its arguments and may be issued from any host thread on any stream (what a launch did -- e.g. which template instance
 *     the tile heuristic picked -- comes back through [host] out-parameters, never through a "last call" global); it reads no
 *     environment variable either.
 *     The only exception is the measurement build (-DCPR_BENCH_HOOKS, libcprhip_bench.so, see the end of this file)
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); no host synchronisation inside
 *   - activations are NHWC fp32; index outputs are int64 (torch long) where the reference returns long
 * Each entry cites the reference interface it replaces (T/ = TOV_mmdetection/).
 */
#ifndef CPR_HIP_H
#define CPR_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define CPR_ERR_ARG (-1001)
#define CPR_ERR_UNSUPPORTED (-1002)

int cpr_version(void);

/* ---- conv stack ------------------------------------------------------------------------------------------------
 * Replaces ATen/cuDNN conv2d + eval BatchNorm + ReLU + residual add as used by
 *   ResNet.forward / Bottleneck.forward  T/mmdet/models/backbones/resnet.py:262-302,630-645
 *   FPN.forward                          T/mmdet/models/necks/fpn.py:166-194
 *   CPRHead.forward_single               T/mmdet/models/point/dense_heads/cpr_head.py:1033-1043
 *   P2PHead.forward_single               T/mmdet/models/point/dense_heads/p2p_head.py:113-123
 * in  (N,H,W,Cin)  wgt [Cout][KH][KW][Cin] rows padded to Kpad  out (N,OH,OW,Cout)
 * epilogue  y = acc*scale[c] + bias[c] (+ residual[m][c]) (ReLU);   scale/bias/residual may be NULL
 * in_a/in_b (N,Cin) optional: input is read as relu?(x*a+b) (fused GroupNorm-apply of the producer; needs H*W%128==0)
 * gn_part optional [N*OH*OW/128][Cout][2]: per-tile per-channel (sum, sumsq) of the output (needs OH*OW%128==0)
 * Cin must be a multiple of 32, or 4 (3-channel stem padded with a zero channel).
 * flags: CPR_CONV_* bits below.  variant_out [host, may be NULL]: bm*1e6 + bn*1e3 + mode*100 + xf*10 + pipe of the template
 * instance that was launched (for profilers; with CPR_CONV_COLSUM the caller needs bm to size the partials). */
#define CPR_CONV_RELU 1     /* ReLU in the epilogue */
#define CPR_CONV_OUT_BF16 2 /* write bf16 (the 3-channel stem runs on the fp32 kernel and hands bf16 to the bf16 layers) */
#define CPR_CONV_RES_MASK 4 /* residual is a ReLU mask source: out = residual > 0 ? v : 0 (backward of a fused ReLU) */
#define CPR_CONV_COLSUM 8   /* gn_part [ceil(M/bm)][Cout][2] holds per-tile per-channel sums for a whole-tensor column sum */
int cpr_conv2d_fwd(const float* in, const float* wgt, float* out, const float* scale, const float* bias,
                   const float* residual, const float* in_a, const float* in_b, float* gn_part, int N, int H, int W,
                   int Cin, int Cout, int KH, int KW, int stride, int pad, int Kpad, int flags, int in_relu,
                   int* variant_out, void* stream);
/* The same with dilated taps: the 3x3 conv2 of a dilated ResNet stage (T/mmdet/models/backbones/resnet.py:36-47, 175-200: padding =
 * dilation) and, over dy with the data-gradient pack (padding 2 dil - dil = dil), its data gradient.  KH = KW = 3, stride 1, pad == dil,
 * Cin % 32 == 0, Kpad = 9 Cin; tap (kh, kw) reads pixel (oy + (kh - 1) dil, ox + (kw - 1) dil), OH = H, OW = W.  wgt is the pack of
 * cpr_conv2d_fwd, unchanged.  Epilogue: scale, bias, residual, CPR_CONV_RELU, CPR_CONV_RES_MASK, CPR_CONV_COLSUM (gn_part then holds the
 * column-sum partials and must be given; without the flag it must be NULL).  in_a / in_b, in_relu, GroupNorm partials,
 * CPR_CONV_OUT_BF16, another stride or pad != dil: CPR_ERR_ARG before any launch.  dil == 1 is cpr_conv2d_fwd, bit for bit.  Direct
 * kernel only (no Winograd, streamed or dual form). */
int cpr_conv2d_fwd_dil(const float* in, const float* wgt, float* out, const float* scale, const float* bias,
                       const float* residual, const float* in_a, const float* in_b, float* gn_part, int N, int H, int W,
                       int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, int Kpad, int flags, int in_relu,
                       int* variant_out, void* stream);

/* First block of a ResNet stage (Bottleneck.forward, T/mmdet/models/backbones/resnet.py:262-302 with the projection shortcut
 * built by ResLayer, T/mmdet/models/utils/res_layer.py / resnet.py:564-610): out = relu?((conv(in, wgt) * scale + bias)
 * + (conv1x1(in2, wgt2; stride2, unpadded) * scale2 + bias2)) in ONE launch -- the shortcut map is never stored.  Both
 * convolutions produce the same (N, OH, OW, Cout) grid; in2 is (N, H2, W2, Cin2), wgt2 [Cout][Kpad2 = Cin2]; Cin, Cin2
 * multiples of 32.  Bit-identical to cpr_conv2d_fwd(in2, wgt2) followed by cpr_conv2d_fwd(in, wgt, residual = that). */
int cpr_conv2d_dual_fwd(const float* in, const float* wgt, const float* in2, const float* wgt2, float* out,
                        const float* scale, const float* bias, const float* scale2, const float* bias2, int N, int H, int W,
                        int Cin, int Cout, int KH, int KW, int stride, int pad, int Kpad, int H2, int W2, int Cin2,
                        int stride2, int Kpad2, int flags, int* variant_out, void* stream);

/* The HBM-bound 1x1 convs of the bottleneck (conv3 + bn3 + shortcut add + ReLU and the like, T/mmdet/models/backbones/resnet.py:
 * 262-302) as a stream: one persistent workgroup per CU, weight panel resident in LDS, pixel tiles through LDS-DMA
 * (csrc/conv1x1_stream.hip).  in [M][Cin], wgt [Cout][Cin], out / residual [M][Cout]; Cin in {64, 128}: M a multiple of
 * 8192 / Cin, Cout a multiple of 16384 / Cin; Cin = 256: M a multiple of 128, Cout of 64 (a power of two up to 2048); flags = CPR_CONV_RELU | CPR_CONV_RES_MASK; CPR_ERR_UNSUPPORTED otherwise.
 * cpr_conv2d_fwd takes this path by itself for such shapes when the launch has >= 1024 tiles; the results are bit-identical to
 * its tiled kernel (same accumulation order, same epilogue), this entry exists for tests and tools. */
int cpr_conv1x1_stream_fwd(const float* in, const float* wgt, float* out, const float* scale, const float* bias,
                           const float* residual, long long M, int Cin, int Cout, int flags, void* stream);

/* Weight gradient of a conv (k = 1, or k = 3 with padding 1; stride 1 or 2) on the bf16 matrix cores -- the mixed-precision training
 * step (reference analogue: torch autograd under mmcv's Fp16OptimizerHook, T/mmdet/apis/train.py:116-119).  dy (N,OH,OW,Cout),
 * OH = (H + 2 (k/2) - k) / stride + 1, and x (N,H,W,Cin) fp32 or bf16 (dy_bf16, x_bf16; fp32 maps are rounded on the way in), grad
 * [Cout][Cin][k][k] fp32 (accumulate: +=), Cin % 64 == 0, Cout % 64 == 0.  Both maps bf16: the pixel-major kernel of
 * csrc/conv_wgrad_bf16_tn.hip (reads the NHWC maps as they are through ds_read_b64_tr_b16).  Otherwise -- or for a shape beyond that
 * kernel's index range -- both maps are rewritten channel-major over a zero-bordered pixel axis (bf16) and every tap is an NT GEMM on the
 * LDS-DMA kernel (stride 1, Cin % 256 == 0 only); the partials of either path are split over the pixels and summed in fp32
 * (csrc/conv_wgrad_bf16.hip).  ws: cpr_conv_wgrad_bf16_workspace_s(...) x 256 bytes; the query returns units of 256 bytes, or
 * CPR_ERR_UNSUPPORTED exactly where cpr_conv_wgrad_bf16_s is for maps of those dtypes. */
int cpr_conv_wgrad_bf16_workspace_s(int N, int H, int W, int Cin, int Cout, int k, int stride, int dy_bf16, int x_bf16);
int cpr_conv_wgrad_bf16_s(const void* dy, int dy_bf16, const void* x, int x_bf16, float* grad, void* ws, int N, int H, int W, int Cin,
                          int Cout, int k, int stride, int accumulate, void* stream);

/* 3x3 / stride 1 / pad 1 convolution as fused Winograd F(2x2,3x3) on the fp32 matrix cores (2.25x fewer multiplies than
 * cpr_conv2d_fwd; same call sites: the CPR head towers cpr_head.py:1033-1043, the FPN output conv fpn.py:190-194, the 3x3 of
 * every stride-1 bottleneck resnet.py:630-645).  The transforms only add/subtract, the result differs from the direct fp32
 * sum by ~1e-6 of the map's max per layer (tests/test_gpu_wino.py states the bound).
 *   cpr_wino_pack_weights: wgt = the cpr_conv2d_fwd layout [Cout][3][3][Cin] (row stride Kpad) -> u, 16*Cin*Cout floats
 *                          (G g G^T per (cout, cin), stored as the kernel's LDS chunk images); Cin % 8 == 0, Cout % 64 == 0
 *                          (the conv itself needs Cin % 16 == 0, Cin >= 32).
 *   cpr_conv3x3_wino_fwd:  in (N,H,W,Cin) -> out (N,H,W,Cout) = conv * scale[c] + bias[c] (ReLU when flags & CPR_CONV_RELU);
 *                          in_a/in_b (N,Cin) optional (Cin <= 512): the input is read as relu?(x*a+b), in_relu selects the ReLU
 *                          (GroupNorm apply of the producing layer fused into the load, as in cpr_conv2d_fwd);
 *                          layout: CPR_WINO_IN_B8 / CPR_WINO_OUT_B8 -- `in` / `out` are channel-blocked [N][C/8][H][W][8]
 *                          instead of NHWC (whole cache lines per 8-channel K chunk: the fast form between chained layers);
 *                          gn_part [N * ceil(H/16) * ceil(W/16)][Cout][2] (may be NULL): per-channel (sum, sumsq) of every 16x16
 *                          output region (an image's regions are contiguous: cpr_gn_finalize with P = regions per image).
 *                          Tensors < 2 GiB (CPR_ERR_UNSUPPORTED).
 *   cpr_gn_apply_b8:       channel-blocked x -> NHWC y = relu?(x*a+b) (a, b NULL: layout conversion only). */
#define CPR_WINO_IN_B8 1
#define CPR_WINO_OUT_B8 2
int cpr_wino_pack_weights(const float* wgt, float* u, int Cin, int Cout, int Kpad, void* stream);
int cpr_conv3x3_wino_fwd(const float* in, const float* u, float* out, const float* scale, const float* bias,
                         const float* in_a, const float* in_b, float* gn_part, int N, int H, int W, int Cin, int Cout,
                         int flags, int in_relu, int layout, void* stream);
/* The two-workgroups-per-CU form of the same convolution (csrc/conv_wino32.hip, round 4): 4-wave workgroups on 8 x 16 pixel
 * regions with 4-channel K chunks, < 80 KB of LDS each, so two are resident per CU and one's epilogue / prologue hides behind the
 * other's MFMAs.  Same arguments as cpr_conv3x3_wino_fwd except: `u` comes from cpr_wino32_pack_weights (16 * Cin * Cout floats,
 * chunks of 4 input channels; Cin % 8 == 0, Cin >= 16, Cout % 64 == 0), gn_part holds cpr_conv3x3_wino32_slots(H, W) slots per
 * image (one per 8 x 16 region), a fused input affine needs Cin <= 256.  Agrees with cpr_conv3x3_wino_fwd to fp32 rounding
 * (different accumulation order), not bit for bit. */
int cpr_wino32_pack_weights(const float* wgt, float* u, int Cin, int Cout, int Kpad, void* stream);
int cpr_conv3x3_wino32_slots(int H, int W);
int cpr_conv3x3_wino32_fwd(const float* in, const float* u, float* out, const float* scale, const float* bias,
                           const float* in_a, const float* in_b, float* gn_part, int N, int H, int W, int Cin, int Cout,
                           int flags, int in_relu, int layout, void* stream);
int cpr_gn_apply_b8(const float* x, const float* a, const float* b, float* y, int N, int H, int W, int C, int relu,
                    void* stream);

/* bf16 compute mode (BASELINE.json configs[4]): bf16 activations / weights / residual, fp32 accumulate
 * (v_mfma_f32_32x32x16_bf16), K chunks of 64 (Cin % 64 == 0, Kpad == KH*KW*Cin), output bf16 or fp32 (out_fp32).
 * No fused producer-GroupNorm input; GroupNorm statistics come from the fp32 accumulators.
 * variant_out [host, may be NULL]: bm*1000 + bn of the launched instance.
 * wgt_frag [may be NULL; Cout % 256 == 0 only]: a second image of the same weights in MFMA-fragment order,
 * [cout / 64][k / 16][j = 0, 1][lane = l + 32 h][8] = wgt[64 g + 2 l + j][16 ks + 8 h .. + 8]; with it the 256 x 256 tile's launches
 * take the instance that loads the weight operand straight into registers (conv_bf16_dma_kernel<4, 2, 4, true>). */
int cpr_conv2d_fwd_bf16(const void* in, const void* wgt, const void* wgt_frag, void* out, const float* scale, const float* bias,
                        const void* residual, float* gn_part, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                        int stride, int pad, int Kpad, int relu, int out_fp32, int* variant_out, void* stream);
/* Mask mode of the call above (relu == 2; the mixed-precision backward, training.py: a data gradient is a forward convolution of the
 * gradient map with the rotated weights): `residual` is the bf16 map a forward ReLU produced, out = v where that map is positive, 0
 * elsewhere (nothing is added), and gn_part receives per-channel SUMS of the masked result, [slots][Cout][2] floats with the sum in
 * element 0 (cpr_part_colsum adds the slots up).  Only the LDS-DMA instances know the mode: cpr_conv2d_bf16_mask_slots returns the
 * number of slots a launch of this shape writes, or 0 when the shape would not run in mask mode (cpr_conv2d_fwd_bf16 then returns
 * CPR_ERR_UNSUPPORTED for relu == 2).  Reference: torch autograd's ReLU backward + conv2d input gradient + the bias-gradient row sum,
 * three kernels behind mmcv's Fp16OptimizerHook (T/mmdet/apis/train.py:116-119). */
int cpr_conv2d_bf16_mask_slots(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int out_fp32);
/* The block-boundary data gradient of the same backward in one launch: g = mask > 0 ? conv(in, wgt) + add32 : 0 (add32: the shortcut
 * gradient, fp32, the output's shape), written twice -- out32 (fp32: the shortcut chain stays fp32) and out16 (its bf16 rounding, what
 * the next weight / data gradients read) -- with the column sums of g in part (slots: cpr_conv2d_bf16_mask_slots with out_fp32 = 2;
 * 0 = no instance for this shape, the call then returns CPR_ERR_UNSUPPORTED).  Replaces conv + fp32 store + one streaming pass
 * (cpr_relu_bwd_colsum with add): 20 bytes per element -> 12.  wgt_frag is required (the instances are the pair-epilogue ones). */
int cpr_conv2d_dgrad_bf16_fused(const void* in, const void* wgt, const void* wgt_frag, float* out32, void* out16, const float* add32,
                                const void* mask, float* part, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                                int pad, int Kpad, int* variant_out, void* stream);
/* bf16 compute mode stem: conv 7x7 / stride 2 / pad 3, 3 -> 64 channels + folded BatchNorm + ReLU (resnet.py:630-636) on the
 * bf16 matrix cores.  in: layout 0 = (N,H,W,4) fp32 (4th channel ignored), layout 1 = (N,3,H,W) fp32 planes (the NCHW network input); wgt (64, 224) bf16 with k = (kh * 8 + kw) * 4 + c (kw = 7 and
 * c = 3 zero), out (N, (H-1)/2+1, (W-1)/2+1, 64) bf16.  CPR_ERR_UNSUPPORTED when the output reaches 2 GiB. */
int cpr_stem7x7s2_bf16(const float* in, const void* wgt, const float* scale, const float* bias, void* out, int N, int H, int W,
                       int relu, int layout, void* stream);
/* The same stem with the max-pool 3x3 / stride 2 / pad 1 (resnet.py:637) fused: out (N, PH, PW, 64) bf16, PH = (OH-1)/2+1.
 * Bit-identical to cpr_stem7x7s2_bf16 (relu = 1) followed by cpr_maxpool3x3s2_bf16. */
int cpr_stem7x7s2_pool_bf16(const float* in, const void* wgt, const float* scale, const float* bias, void* out, int N, int H,
                            int W, int layout, void* stream);
int cpr_maxpool3x3s2_bf16(const void* in, void* out, int N, int H, int W, int C, void* stream);
int cpr_gn_stats_bf16(const void* x, float* part, int N, int HW, int C, int P, void* stream);
int cpr_gn_apply_bf16(const void* x, const float* a, const float* b, const void* up, void* y, int N, int H, int W,
                      int C, int UH, int UW, int relu, void* stream);

/* network input (N,C<=4,H,W) NCHW -> (N,H,W,4) NHWC, missing channels zero */
int cpr_nchw_to_nhwc4(const float* in, float* out, int N, int C, int H, int W, void* stream);
/* (N,H,W,C) -> dense (N,C,H,W) (export in the reference's layout) */
int cpr_nhwc_to_nchw(const float* in, float* out, int N, int C, int H, int W, void* stream);
/* nn.MaxPool2d(3, 2, 1) of the ResNet stem (resnet.py:610,637); NHWC */
/* The ResNet stem in one kernel, exact fp32 (resnet.py:630-637): conv 7x7 / stride 2 / pad 3, 3 -> 64 + folded BatchNorm + ReLU
 * + max-pool 3x3 / stride 2 / pad 1.  in: layout 0 = (N,H,W,4) fp32 (4th channel ignored), layout 1 = (N,3,H,W) fp32 planes; wgt (64, 154) fp32 = [cout][kh][kw * 3 + c] with
 * slot 21 of every kernel row zero, out (N, PH, PW, 64) fp32, OH = (H-1)/2+1, PH = (OH-1)/2+1. */
int cpr_stem7x7s2_pool_f32(const float* in, const float* wgt, const float* scale, const float* bias, float* out, int N, int H,
                           int W, int layout, void* stream);
int cpr_maxpool3x3s2(const float* in, float* out, int N, int H, int W, int C, void* stream);
/* The deep stem of ResNetV1d in exact fp32 (resnet.py:564-596, 630-638; csrc/stem_deep.hip): conv 3x3 / 2, 3 -> 32; conv 3x3, 32 -> 32;
 * conv 3x3, 32 -> 64, each + folded BatchNorm + ReLU, then max-pool 3x3 / 2 / pad 1 in the third conv's epilogue.  in: layout 0 =
 * (N,H,W,4) fp32 (4th channel ignored), layout 1 = (N,3,H,W) fp32 planes (same bits either way).  w1 (32, 64), w2 (32, 288),
 * w3 (64, 288): the fp32 packs of cpr_pack_weights ([cout][kh][kw][cin'], cin' = 4 / 32 / 32); s* / b* the folded BatchNorms.  mid1, mid2: caller-allocated (N, OH, OW, 32) fp32, OH = (H-1)/2+1.  out (N, PH, PW, 64), PH = (OH-1)/2+1: fp32, or
 * bf16 (out_bf16 = 1: one rounding of the fp32 result). */
int cpr_stem_deep_fwd(const float* in, const float* w1, const float* s1, const float* b1, const float* w2, const float* s2,
                      const float* b2, const float* w3, const float* s3, const float* b3, float* mid1, float* mid2, void* out, int N,
                      int H, int W, int layout, int out_bf16, void* stream);
/* The RegNet stem (regnet.py:237-249): conv 3x3 / 2 / pad 1, 3 -> 32, + folded BatchNorm + ReLU, no max-pool -- the first launch of
 * cpr_stem_deep_fwd alone (same layouts, same pack w (32, 64)) -> out (N, OH, OW, 32) fp32.
 * cpr_stem3x3s2_wgrad (csrc/stem3x3_bwd.hip): gw (32, 3, 3, 3) = its weight gradient given dy (N, OH, OW, 32) and the image as the
 * forward read it; the pixels are split into slices whose partials (ws: cpr_stem3x3s2_wgrad_workspace(N, H, W) floats) are added in
 * ascending order by a second kernel -- no atomics. */
int cpr_stem3x3s2_fwd(const float* in, const float* w, const float* scale, const float* bias, float* out, int N, int H, int W,
                      int layout, void* stream);
int cpr_stem3x3s2_wgrad_workspace(int N, int H, int W);
int cpr_stem3x3s2_wgrad(const float* dy, const float* in, float* gw, float* ws, int N, int H, int W, int layout, void* stream);
/* nn.AvgPool2d(s, s, ceil_mode=True, count_include_pad=False) on NHWC maps (the avg_down shortcut, res_layer.py:39-60): in (N,H,W,C) ->
 * out (N,ceil(H/s),ceil(W/s),C); a last window of an odd map divides by its in-map elements.  bf16 = 0: fp32 maps (C % 4 == 0),
 * 1: bf16 maps (C % 8 == 0); fp32 accumulation in a fixed order; s >= 2. */
int cpr_avgpool_fwd(const void* in, void* out, int N, int H, int W, int C, int s, int bf16, void* stream);
/* its backward in gather form (no atomics): dx[h, w] = g[h/s, w/s] / count + add[h, w] (add optional: another gradient of the same
 * map, the shape and type of dx) */
int cpr_avgpool_bwd(const void* g, const void* add, void* dx, int N, int H, int W, int C, int s, int bf16, void* stream);
/* Recording instances (training with a trainable stem): the same pooled map, bit for bit, and next to it arg (N, PH, PW, 64) uint8 =
 * the window position 0..8 (row-major) of each maximum, the first of tied positions (torch's max_pool2d rule), 255 where the pooled
 * value is 0 (the ReLU passes no gradient there).  The bf16 instances take the argmax of their own bf16-rounded values. */
int cpr_maxpool3x3s2_rec(const float* in, float* out, unsigned char* arg, int N, int H, int W, int C, void* stream);
int cpr_maxpool3x3s2_bf16_rec(const void* in, void* out, unsigned char* arg, int N, int H, int W, int C, void* stream);
int cpr_stem7x7s2_pool_f32_rec(const float* in, const float* wgt, const float* scale, const float* bias, float* out,
                               unsigned char* arg, int N, int H, int W, int layout, void* stream);
int cpr_stem7x7s2_pool_bf16_rec(const float* in, const void* wgt, const float* scale, const float* bias, void* out,
                                unsigned char* arg, int N, int H, int W, int layout, void* stream);
/* Stem backward (csrc/stem_bwd.hip).  cpr_stem_pool_bwd: pooled gradient dp (N, PH, PW, 64) fp32 + the recorded arg map -> dy
 * (N, OH, OW, 64) fp32, the gradient at the BatchNorm output (through max-pool and ReLU; each conv pixel sums the windows that chose
 * it, pooled row then column ascending), and part [cpr_stem_pool_bwd_blocks(N*OH*OW)][64][2] per-block column sums of dy (element 0).
 * cpr_stem_wgrad_f32: gw (64, 3, 7, 7) = the weight gradient of conv 7x7 / 2 / pad 3 given dy (N, OH, OW, 64) and the image (layout 0:
 * (N, H, W, 4) fp32, layout 1: (N, 3, H, W) fp32), exact fp32 on the matrix pipe, deterministic; ws: cpr_stem_wgrad_f32_workspace
 * floats. */
int cpr_stem_pool_bwd_blocks(long long M);
int cpr_stem_pool_bwd(const float* dp, const unsigned char* arg, float* dy, float* part, int N, int OH, int OW, void* stream);
int cpr_stem_wgrad_f32_workspace(int N, int H, int W);
int cpr_stem_wgrad_f32(const float* dy, const float* in, float* gw, float* ws, int N, int H, int W, int layout, void* stream);

/* GroupNorm of mmcv ConvModule (fpn.py:124-144, cpr_head.py:990-991) as three streaming steps:
 *   stats    part [N][P][C][2] per-slot per-channel (sum, sumsq)
 *   finalize per (image, channel) affine a = rstd*gamma, b = beta - mean*a   (y = x*a + b); mean/rstd optional (N,G)
 *   apply    y = x*a + b (ReLU) (+ nearest-upsampled `up` (N,UH,UW,C): the FPN top-down add, fpn.py:179-188) */
int cpr_gn_stats(const float* x, float* part, int N, int HW, int C, int P, void* stream);
int cpr_gn_finalize(const float* part, const float* gamma, const float* beta, float* a_out, float* b_out,
                    float* mean_out, float* rstd_out, int N, int P, int C, int G, int HW, float eps, void* stream);
int cpr_gn_apply(const float* x, const float* a, const float* b, const float* up, float* y, int N, int H, int W,
                 int C, int UH, int UW, int relu, void* stream);

/* ---- CPR point kernels -----------------------------------------------------------------------------------------
 * pseudo_bbox_to_center (cpr_head.py:1293-1301): boxes (n,4) -> centers (n,2) */
int cpr_box_centers(const float* boxes, float* centers, int n, void* stream);

/* Probability types of CPRHead.get_cls_prob (cpr_head.py:1080-1099), argument `prob_type` below:
 *   0 sigmoid   1 softmax over the class dim   2 normed_sigmoid (sigmoid, then L_p normalisation over the class dim,
 *   p = norm_p)   3 (cpr_mil_loss only) the cls channels already hold probabilities. */
#define CPR_PROB_SIGMOID 0
#define CPR_PROB_SOFTMAX 1
#define CPR_PROB_NORMED_SIGMOID 2
#define CPR_PROB_IDENTITY 3

/* CPRHead.get_pts_outs for EVERY pixel (cls_out / ins_out = nn.Linear(Cin -> C), cpr_head.py:1007-1014,1045-1078) as one
 * HBM-streaming pass: x (N,HW,Cin) fp32 NHWC, w (J,Cin), bias (J) -> out (N,HW,J); in_a/in_b (N,Cin) optional: the input
 * is read as relu?(x*a+b) (GroupNorm-apply of the last tower layer fused into the load).  Small J only: returns
 * CPR_ERR_UNSUPPORTED when J > 8 or Cin is not 64, 128, 192 or 256 (the caller then uses cpr_conv2d_fwd). */
int cpr_logit_project(const float* x, const float* w, const float* bias, const float* in_a, const float* in_b,
                      float* out, int N, int HW, int Cin, int J, int in_relu, void* stream);

/* OutCirclePtFeatGenerator.generate + neg branch of CPRHead.loss0 (cpr_head.py:254-290,1219-1228):
 * logit (N,H,W,J) (class logits in channels [0,C)); annotated points in CSR form (centers (P,2), labels (P),
 * gt_start (N+1)) -- with num_refine > 1 every refine point is a row, carrying its gt's label;
 * pad_hw (N,2) int32.  mask (N*H*W, C) uint8 = the reference's neg `valid`; partial[] (double, N*ceil(H*W*C/256))
 * = block partial sums of gfocal(prob(logit), 0, valid).  d2_thr = smallest fp32 whose torch-CPU sqrt is
 * >= stride*radius (the reference thresholds cdist, i.e. a sqrt).  n_partial [host, may be NULL] receives the count.
 * mask_classes = C, or 1 with C = 2 (normal_cfg.out_bg_cls, cpr_head.py:953: the one-class validity broadcasts over
 * [class, background] outputs).  CPR_ERR_ARG when stride <= 0, N > 65535 or H*W*C (rounded up to whole 256-thread blocks)
 * does not fit an int. */
int cpr_neg_mask_loss(const float* logit, int J, const float* centers, const int* labels, const int* gt_start,
                      const int* pad_hw, unsigned char* mask, double* partial, int N, int H, int W, int C,
                      float stride, float d2_thr, float eps, int class_wise, int prob_type, float norm_p,
                      int mask_classes, int* n_partial, void* stream);

/* CirclePtFeatGenerator.generate (cpr_head.py:453-497,172-199): bag points (rings + the point itself last), validity
 * and bilinear samples of a J-channel NHWC map, one bag per annotated / refine point.  offsets (K-1,2) from the host.
 * pts (G,K,2) valid (G,K) out (G,K,J).  align_corners: the generators' align_corners=True form (cpr_head.py:81-84: grid
 * 2x/(w-1)-1, zeros padding instead of the border clip); pad_value (J) or NULL: what a dropped tap contributes per unit of
 * weight -- the projection's bias when the map holds logits (the reference samples zero FEATURES, then applies the Linear). */
int cpr_bag_sample(const float* map, int J, const float* centers, const int* gt_img, const int* pad_hw,
                   const float* offsets, float* pts, unsigned char* valid, float* out, int G, int K, int H, int W,
                   float stride, int align_corners, const float* pad_value, void* stream);

/* GridCirclesPtFeatGenerator.generate (cpr_head.py:296-352,405-438): per gt (R refine points each, points (G*R,2),
 * gt_img (G)) every grid point within radius_px of any of its refine points, row-major, zero-padded to Kmax, then the R
 * refine points in reversed order.  pts (G,Kmax+R,2), valid (G,Kmax+R) u8, out (G,Kmax+R,J) (grid entries = map value of
 * the cell, refine points = bilinear samples, padding slots = pad_value (J) or 0 when NULL: the reference pads with zero
 * FEATURES, i.e. the projection's bias on a logit map), count (G) int32 = grid points found (> Kmax: the reference raises),
 * ws_cell (G,Kmax+R) int32 workspace. */
int cpr_grid_bag(const float* map, int J, const float* points, const int* gt_img, int R, int Kmax, float radius_px,
                 const float* pad_value, float* pts, unsigned char* valid, int* ws_cell, int* count, float* out, int G,
                 int H, int W, float stride, int align_corners, void* stream);

/* MILLoss.forward / AllPosLoss.forward + gt loss + neg normalisation (multi_instance_learning_loss.py:153-243,
 * cpr_head.py:1159-1228).  logits (entries,J): cls in [0,C), ins in [ins_off, ins_off + C*(1+binary_ins)).
 * Bag b = entries [b*bag_stride + bag_off, + bag_len): covers refine_bag_policy independent_with_gt_bag (stride K),
 * merge_to_gt_bag (stride R*K, len R*K) and only_refine_bag (off si*K) without re-packing.  Annotated-point ("gt") loss
 * entries of bag b: b*bag_stride + ctr_off + j*ctr_stride (j < ctr_count), used when b % ctr_mod == 0.
 * labels / gt_weight are per bag.  allpos = AllPosLoss instead of MILLoss.  bag_ws (num_bags,5) workspace.
 * out5 = {gt_loss, pos_loss, bag_acc, neg_loss, num_sample} (device scalars, no host sync); neg_from_gt: average the
 * negative loss over the gt count instead of num_sample (with_mil_loss = False).  CPR_ERR_ARG when ins_off < 0, J < C,
 * ctr_stride < 0 (with ctr_count > 0) or an annotated-point entry falls outside its bag's stride. */
int cpr_mil_loss(const float* logits, int J, int ins_off, const unsigned char* valid, const int* labels,
                 const float* gt_weight, float* bag_ws, const double* neg_partial, int n_partial, int num_bags,
                 int bag_stride, int bag_off, int bag_len, int ctr_off, int ctr_stride, int ctr_count, int ctr_mod,
                 int C, float eps, int prob_type, float norm_p, int binary_ins, int allpos, float w_mil, float w_gt,
                 float w_neg, int neg_from_gt, float* out5, void* stream);

/* PointRefiner.refine_single (cpr_head.py:711-850).  A gt owns Kt = Rv*Kv bag entries (Rv sub-bags of Kv; entry Kv-1 is
 * the annotated point); centers holds ctr_stride points per gt of which the first Rv take part in the nearest filter.
 * refine_pts (G,2), scores (G), not_refine (G) u8, chosen (G,Kt) u8.  score_max: return_score_type 'max'
 * (cpr_head.py:840-842) instead of the mean of the kept probabilities. */
int cpr_refine(const float* logits, int J, const float* pts, const unsigned char* valid, const float* centers, int Rv,
               int ctr_stride, const int* labels, const int* gt_img, const int* gt_start, const int* img_hw,
               const unsigned char* not_refine_in, float* refine_pts, float* scores, unsigned char* not_refine,
               unsigned char* chosen, int G, int Kt, int Kv, int C, int prob_type, float norm_p, float gt_alpha,
               float merge_th, float refine_th, int use_nearest, int use_classify, int score_max, void* stream);

/* ---- assigners -------------------------------------------------------------------------------------------------
 * PointAssigner.assign (T/mmdet/core/bbox/assigners/point_assigner.py:23-133): points (n,3)=(x,y,stride),
 * gt_bboxes (k,4) -> gt_inds (n) int64 (0 bg, j+1 = gt j).  ws_best (n) float, ws_lvl (n) int32 workspaces. */
int cpr_point_assign(const float* points, const float* gt_bboxes, int n, int k, float scale, int pos_num,
                     long long* gt_inds, float* ws_best, int* ws_lvl, void* stream);

/* FocalLossCost + DisCostV2 (T/mmdet/core/bbox/match_costs/match_cost.py:84-100,197-214):
 * costT (G,M) = transpose of the reference's (M,G) cost; pred (M,pred_stride>=2), logits (M,C), gt (G,2);
 * p_norm = DisCostV2's p: 1 (|dx|+|dy|) or 2 (torch.cdist's Euclidean forms) */
int cpr_hungarian_cost(const float* pred, int pred_stride, const float* logits, int C, const float* gt,
                       const int* labels, float* costT, int M, int G, float w_cls, float alpha, float gamma,
                       float eps, float w_dis, float fx, float fy, int p_norm, void* stream);
/* The general cost matrix of HungarianAssignerV2 / HungarianAssigner (hungarian_assigner.py:15-145,166-229): any list of the costs of
 * T/mmdet/core/bbox/match_costs/match_cost.py, summed as ``sum(cls_costs) + sum(reg_costs)`` sums them.  terms [host]: 6 floats per
 * term (type, weight, a, b, c, d), the ncls classification terms first -- cls 0 FocalLossCost (alpha, gamma, eps), 1 ClassificationCost
 * (-softmax[label]), 2 ClassificationCostV2(use_sigmoid) (-sigmoid[label]), 3 ZeroCost; reg 0 DisCostV2 (p, fx, fy) on points (pdim 2),
 * 1 BBoxL1Cost, 2 IoUCost 'iou', 3 IoUCost 'giou' on xyxy boxes (pdim 4).  costT (G, M) as cpr_hungarian_cost. */
int cpr_match_cost(const float* pred, int pdim, const float* logits, int C, const float* gt, const int* labels, float* costT,
                   int M, int G, const float* terms, int ncls, int nreg, void* stream);

/* The linear_sum_assignment loop of HungarianAssignerV2.assign (hungarian_assigner.py:229-268; replaces scipy and
 * the device->host->device round trip), including scipy's tie-breaking order.  A batch of problems, one workgroup
 * each: problem b has costT at cost_off[b] (G_b x M_b, M_b >= G_b), column arrays at col_off[b], row arrays at
 * row_off[b].  gt_inds (sum M) int64: 0 background, j+1 = gt j.  status[b] != 0: infeasible.
 * Workspaces: per column ws_v/ws_spc (double), ws_path/ws_row4col/ws_cols/ws_remaining/ws_pos (int32), ws_sc/ws_active
 * (uint8); per row ws_u (double), ws_col4row (int32), ws_sr (uint8).  max_cols / max_rows: [host] upper bounds of M_b / G_b
 * over the batch (0 = unknown): when max_cols <= 32768 and topk * max_rows < 65534 the search state of a row lives in
 * registers / LDS (one 4-byte cost read per column per scan instead of ~33 bytes of state; same results bit for bit). */
int cpr_lsa_topk(const float* costT, const int* m_of, const int* g_of, const long long* cost_off,
                 const long long* col_off, const long long* row_off, int num_problems, int topk, long long* gt_inds,
                 double* ws_v, double* ws_spc, int* ws_path, int* ws_row4col, unsigned char* ws_sc,
                 unsigned char* ws_active, int* ws_cols, int* ws_remaining, int* ws_pos, double* ws_u,
                 int* ws_col4row, unsigned char* ws_sr, int* status, int max_cols, int max_rows, void* stream);

/* ---- P2P inference ---------------------------------------------------------------------------------------------
 * per-level top-k of P2PHead._get_bboxes_single (p2p_head.py:367-373): scores (n) -> k largest, sorted descending
 * (ties: lower index first).  k <= 4096.  out_vals (k) float, out_idx (k) int64. */
int cpr_topk_desc(const float* scores, int n, int k, float* out_vals, long long* out_idx, void* stream);

/* Candidate list of multiclass_nms (T/mmdet/core/post_processing/bbox_nms.py:28-60): every (proposal, class) pair with
 * scores[p][c] > score_thr (scores (n,C+1), last column = background), row-major order; boxes (n, box_stride) with
 * box_stride = 4 (shared by the classes) or 4*C; factors (n) optional score_factors.  Outputs sized n*C:
 * cand_boxes (.,4), cand_scores, cand_labels (int32), cand_inds (int64, p*C + c), count (1) int32. */
int cpr_nms_candidates(const float* boxes, int box_stride, const float* scores, const float* factors, int n, int C,
                       float score_thr, float* cand_boxes, float* cand_scores, int* cand_labels, long long* cand_inds,
                       int* count, void* stream);
/* mmcv.ops.nms.batched_nms as called by multiclass_nms (T/mmdet/core/post_processing/bbox_nms.py:85; mmcv-full
 * 1.3.x, third-party): class-offset trick, sort by score (descending, ties by index), greedy IoU > thr suppression.
 * boxes (n,4), scores (n), labels (n) int32.  keep_idx (n) int64: indices of kept boxes in descending score order; num_keep (1)
 * int32.  ws_order (n) int32, ws_boxes (n,4) float, ws_mask cpr_nms_workspace(n) uint64 words.  No candidate ceiling below
 * 262 144 (round 6; the reference has none: bbox_nms.py:7-94): above 8192 candidates the pair mask is computed and scanned a
 * band of 8192 rows at a time, the removed bits and the keep count carried from band to band. */
int cpr_nms_workspace(int n);
int cpr_nms(const float* boxes, const float* scores, const int* labels, int n, float iou_thr, long long* keep_idx,
            int* num_keep, int* ws_order, float* ws_boxes, unsigned long long* ws_mask, void* stream);
/* The same three stages for ALL images of a batch with no host round trip in between (P2PHead.get_bboxes loops
 * _get_bboxes_single over the images, p2p_head.py:330-343; each image's torch.topk / nonzero / nms sync the host there):
 *   cpr_topk_desc_batched        scores (B, n) -> vals (B, k), idx (B, k) (segment-relative), one workgroup per image
 *   cpr_nms_candidates_batched   boxes (B, n, box_stride), scores (B, n, C+1), factors (B, n) or NULL -> slabs of capacity
 *                                n * C per image: cand_boxes (B, n*C, 4), cand_scores / labels / inds (B, n*C), count (B) [device]
 *   cpr_nms_batched              reads the per-image candidate counts n_dev (B) FROM THE DEVICE; keep_idx (B, cap) slab-relative,
 *                                num_keep (B) [device]; ws_order (B, cap) int32, ws_boxes (B, cap, 4), ws_mask B * ws_stride
 *                                64-bit words, ws_stride >= max(cap * ceil(cap / 64), next pow2 >= cap); cap <= 16384
 * The caller reads (count, num_keep) once per batch. */
int cpr_topk_desc_batched(const float* scores, int B, int n, int k, float* out_vals, long long* out_idx, void* stream);
int cpr_nms_candidates_batched(const float* boxes, int box_stride, const float* scores, const float* factors, int B, int n,
                               int C, float score_thr, float* cand_boxes, float* cand_scores, int* cand_labels,
                               long long* cand_inds, int* count, void* stream);
int cpr_nms_batched(const float* boxes, const float* scores, const int* labels, const int* n_dev, int B, int cap,
                    float iou_thr, long long* keep_idx, int* num_keep, int* ws_order, float* ws_boxes,
                    unsigned long long* ws_mask, long long ws_stride, void* stream);

/* P2PHead.get_pred_points (p2p_head.py:125-170): reg (N,H,W,2k) -> pred (N,H*W*k,3) = anchor + point_anchor*stride +
 * reg*gamma*stride, third column = stride; anchor (same shape) optional.  point_anchor (k,2). */
int cpr_p2p_decode(const float* reg, const float* point_anchor, float* pred, float* anchor, int N, int H, int W, int k,
                   float stride, float gamma, void* stream);
/* max_c sigmoid(logits[m][c]) -> out (M): the score P2PHead._get_bboxes_single ranks with (p2p_head.py:362-369) */
/* out (N,H,W,J) = bias[j] + sum over the 3x3 taps of R[n][y+kh-1][x+kw-1][(kh*3+kw)*J + j] (taps outside the map add 0):
 * the second half of a 3x3 / pad 1 convolution with J output channels computed as a 1x1 projection to 9 J tap responses
 * (P2PHead's cls_out / reg_out, p2p_head.py:84-123: 1-2 output channels).  bias may be NULL. */
int cpr_tap_sum3x3(const float* R, const float* bias, float* out, int N, int H, int W, int J, void* stream);
int cpr_rowmax_sigmoid(const float* logits, float* out, long long M, int C, void* stream);
/* elementwise sigmoid with the bits of torch's CPU kernel (p2p_head.py:362: the scores that order top-k and NMS) */
int cpr_sigmoid(const float* x, float* y, long long n, void* stream);
/* P2PHead.loss_single + sample_result_to_target (p2p_head.py:220-248,308-328) straight from gt_inds (B,M) int64.
 * cls_mode 0: sigmoid focal loss (T/mmdet/models/losses/focal_loss.py:11-56), averaged by the batch's positives; 1: CrossEntropyLoss
 * (use_sigmoid=True) = BCE with logits on the one-hot labels (cross_entropy_loss.py:58-99), averaged by ALL proposals of the batch
 * (p2p_head.py:222-224); 2: softmax cross entropy over C = num_classes + 1 logits, background last.  reg_mode 0: SmoothL1(beta)
 * (smooth_l1_loss.py:11-28), 1: MSE (mse_loss.py), 2: L1; averaged by the positives.  (1, 1) are the reference head's own defaults
 * (p2p_head.py:38-46), (0, 0) the shipped config.  ws_partial (B*ceil(M/256)*3) double; out (B,2) = per image {loss_cls, loss_pts}. */
int cpr_p2p_loss(const float* logits, const float* pred, const long long* gt_inds, const float* gt_pts,
                 const int* gt_labels, const int* gt_start, double* ws_partial, float* out, int B, int M, int C,
                 float alpha, float gamma, float beta, float pos_w, float neg_w, float reg_norm, float w_cls,
                 float w_reg, int cls_mode, int reg_mode, void* stream);

/* ---- training step: backward + optimizer ------------------------------------------------
 * The reference gets these from torch autograd over mmcv ConvModule / nn.GroupNorm / F.grid_sample and
 * torch.optim.SGD driven by mmcv's OptimizerHook (T/configs2/COCO/CPRNet/CPR_R50_FPN_1x_coco_coarse.py optimizer /
 * optimizer_config); tests/test_gpu_backward.py checks every function against torch autograd on the oracle.
 *
 * weight gradient of conv2d_fwd: dy (N,OH,OW,Cout) x (N,H,W,Cin) NHWC fp32 -> grad_w [Cout][Cin][KH][KW] (the
 * parameter's own layout).  Optional fused input transform x' = max(x*in_a[n,c]+in_b[n,c], in_relu?0:-inf) (the
 * GroupNorm(+ReLU) the forward applied on load).  ws: cpr_conv2d_wgrad_workspace(...) floats.  Cin%4==0, Cout%4==0. */
/* benchmark hook: main-loop ablations of the plain weight-gradient kernel (1 no loads, 2 no LDS stores, 4 no barrier,
 * 8 no fragment reads, 3 = 1|2, 15 = all); results are wrong by construction, 0 restores the product kernel */
int cpr_conv2d_wgrad_workspace(int N, int OH, int OW, int Cin, int Cout, int KH, int KW);
int cpr_conv2d_wgrad(const float* dy, const float* x, const float* in_a, const float* in_b, float* grad_w, float* ws,
                     int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int in_relu,
                     int accumulate, void* stream);
/* The same weight gradient with dilated taps (tap step dil >= 1): x is read at (oy stride + kh dil - pad, ox stride + kw dil - pad),
 * OH = (H + 2 pad - dil (KH - 1) - 1) / stride + 1.  No fused input transform.  ws: cpr_conv2d_wgrad_workspace of the same shapes; the
 * slabs are summed in the same fixed order (no atomics).  dil == 1 is cpr_conv2d_wgrad, bit for bit. */
int cpr_conv2d_wgrad_dil(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int Cin, int Cout, int KH,
                         int KW, int stride, int pad, int dil, int accumulate, void* stream);
/* The same weight gradient for 3x3 / stride 1 / pad 1 layers as fused Winograd F(2x2,3x3) (the adjoint of
 * cpr_conv3x3_wino_fwd with respect to the weights: 2.25x fewer multiplies; csrc/conv_wino_wgrad.hip).  Cin % 64 == 0,
 * Cout % 64 == 0; ws: cpr_conv3x3_wino_wgrad_workspace(...) floats (split-K partials, reduced inside the call). */
int cpr_conv3x3_wino_wgrad_workspace(int N, int H, int W, int Cin, int Cout);
int cpr_conv3x3_wino_wgrad(const float* dy, const float* x, const float* in_a, const float* in_b, float* grad_w, float* ws,
                           int N, int H, int W, int Cin, int Cout, int in_relu, int accumulate, void* stream);
/* nn.GroupNorm (+ReLU) backward from the raw conv output x, the forward affine a,b (N,C), mean/rstd (N,G):
 * dx (N,HW,C), dgamma/dbeta (C).  ws_part N*P*C*2 floats, ws_k 2*N*G + 2*N*C floats.
 * N, HW, P > 0; C % 4 == 0 with C / 4 dividing 256; G > 0 dividing C (any C / G >= 1); anything else is CPR_ERR_ARG. */
int cpr_gn_bwd(const float* x, const float* dz, const float* a, const float* b, const float* mean, const float* rstd,
               const float* gamma, float* dx, float* dgamma, float* dbeta, float* ws_part, float* ws_k, int N, int HW,
               int C, int G, int P, int relu, int accumulate, void* stream);
/* The same backward reading the bf16 map the mixed-precision forward recorded (widened in registers: the values are those of
 * cpr_gn_bwd on the widened map) and writing dx (fp32) and / or dx_bf16 (its round-to-nearest-even narrowing, what the bf16 weight /
 * data gradient kernels read) -- at least one of the two. */
int cpr_gn_bwd_bf16(const void* x_bf16, const float* dz, const float* a, const float* b, const float* mean, const float* rstd,
                    const float* gamma, float* dx, void* dx_bf16, float* dgamma, float* dbeta, float* ws_part, float* ws_k, int N,
                    int HW, int C, int G, int P, int relu, int accumulate, void* stream);
/* ... with the upstream gradient dz in bf16 as well (round 6: the bf16 data gradient of the layer above writes it in bf16) */
int cpr_gn_bwd_bf16_dz16(const void* x_bf16, const void* dz_bf16, const float* a, const float* b, const float* mean, const float* rstd,
                         const float* gamma, float* dx, void* dx_bf16, float* dgamma, float* dbeta, float* ws_part, float* ws_k,
                         int N, int HW, int C, int G, int P, int relu, int accumulate, void* stream);
/* FPN top-down path backward (fpn.py:176-185): dcoarse (N,UH,UW,C) (+)= sum over the nearest-upsample children of dfine */
int cpr_upsample_add_bwd(const float* dfine, float* dcoarse, int N, int H, int W, int UH, int UW, int C, int accumulate,
                         void* stream);
/* backward of the fused conv epilogue y = relu?(conv*scale + shift (+ identity)) of an eval-mode BatchNorm
 * (resnet.py Bottleneck.forward): g = dy*(y>0) (y NULL: g = dy) is the shortcut gradient and the un-scaled conv-output
 * gradient; colsum (C) (+)= per-channel sums of g (= dshift; also the Linear/conv bias gradient).  (M,C) row-major,
 * C%4==0.  g_out may be NULL (sums only).  ws_part: cpr_relu_bwd_colsum_ws(M, C) floats. */
int cpr_relu_bwd_colsum_ws(long long M, int C);
int cpr_relu_bwd_colsum(const float* dy, const float* add, const void* y, int y_bf16, float* g_out, void* g16_out, float* colsum,
                        float* ws_part, long long M, int C, int accumulate, void* stream);   /* y_bf16: y is the bf16 map the mixed-precision
                        forward recorded; g16_out (optional): the bf16 rounding of g, written by the same pass; add (optional, fp32, same
                        shape): g = (dy + add) masked -- the shortcut gradient joining a block's data gradient (round 6) */
/* column sums (C) of a conv output from the epilogue partials cpr_conv2d_fwd wrote into gn_part [tiles][C][2];
 * ws: 64*C floats */
int cpr_part_colsum(const float* part, float* out, float* ws, int tiles, int C, void* stream);
/* parameter side of the folded BN: Gw = cpr_conv2d_wgrad(g, x) [Cout][K] -> in place dW = scale[c]*Gw[c];
 * dgamma = inv_sigma*(<W[c],Gw[c]> - mean*colsum_g), dbeta = colsum_g (either may be NULL). */
int cpr_bn_fold_bwd(float* Gw, const float* weight, const float* scale, const float* mean, const float* inv_sigma,
                    const float* colsum_g, float* dgamma, float* dbeta, int Cout, int K, void* stream);
/* the same with the column sums still in a conv epilogue's partials [tiles][Cout][2] (element 0 = sum; mask mode / fused data gradients of
 * cpr_conv2d_fwd_bf16, CPR_CONV_COLSUM of cpr_conv2d_fwd): the kernel adds each channel's column up itself (fixed order) */
int cpr_bn_fold_bwd_part(float* Gw, const float* weight, const float* scale, const float* mean, const float* inv_sigma, const float* part,
                         int tiles, float* dgamma, float* dbeta, int Cout, int K, void* stream);
/* y = alpha*x + beta*y on flat fp32 buffers */
int cpr_axpby(float* y, const float* x, float alpha, float beta, long long n, void* stream);
/* phase decomposition of a stride-s data gradient: dst[n, s*i+py, s*j+px, :] += src[n, i+sh, j+sw, :] for all targets
 * inside (H, W); src (N,Hs,Ws,C) = the stride-1 sub-convolution over dy that serves output parity (py, px) */
int cpr_phase_scatter_add(const float* src, float* dst, int N, int Hs, int Ws, int C, int H, int W, int py, int px,
                          int sh, int sw, int s, void* stream);
/* out (N,H,W,C) = dy (N,OH,OW,C) with s-1 zeros inserted between pixels (data gradient of a stride-s conv as a
 * stride-1 conv over the dilated gradient) */
int cpr_zero_insert(const float* dy, float* out, int N, int OH, int OW, int C, int H, int W, int s, void* stream);
/* ---- grouped 3x3 convolution (ResNeXt conv2; csrc/conv_group.hip), NHWC fp32, plain fp32 FMA -------------------------------
 * C input and output channels in C / cg groups, cg in {4, 8, 16, 24, 32, 40, 48, 56}, padding 1, stride 1 or 2; the parameter is
 * (C, cg, 3, 3).
 * An output channel is multiplied against the cg input channels of its own group and nothing else (9 * cg FMAs per output, tap-major,
 * input channel ascending): bit-repeatable, and an image of a batch equals its single-image run.
 * cpr_pack_weights_grouped: the parameter -> the kernel's image (9 * cg * C floats): transpose 0 the forward pack, 1 the data-gradient
 * pack (per group in / out channels swapped, taps flipped, scale[C] -- the forward conv's folded BatchNorm, or NULL -- multiplied in).
 * _multi: a device table of jobs { const float* w; const float* scale; float* out; int C, cg, transpose, block0, nblocks, pad; }
 * (48 bytes, ascending block0), one launch of total_blocks workgroups -- the same bits as the single launches. */
int cpr_pack_weights_grouped(const float* w, const float* scale, float* out, int C, int cg, int transpose, void* stream);
int cpr_pack_weights_grouped_multi(const void* jobs_dev, int n, int total_blocks, void* stream);
/* out (N,OH,OW,C) = relu?(conv(x (N,H,W,C), wp) * scale[c] + bias[c]); scale / bias may be NULL (the raw form); flags: CPR_CONV_RELU
 * only (no residual, no GroupNorm statistics, no fused input affine: anything else is CPR_ERR_ARG).  The data gradient of a grouped
 * conv is this call over dy (zero-inserted for stride 2) with the data-gradient pack and stride 1. */
int cpr_conv_group_fwd(const float* x, const float* wp, float* out, const float* scale, const float* bias, int N, int H, int W, int C,
                       int cg, int stride, int flags, void* stream);
/* grad_w (C, cg, 3, 3) (+)= dy (N,OH,OW,C) against x (N,H,W,C) within each group.  The pixels are split into slices whose partials (ws:
 * cpr_conv_group_wgrad_workspace(...) floats) are added in ascending order by a second kernel -- no atomics. */
int cpr_conv_group_wgrad_workspace(int N, int OH, int OW, int C, int cg);
int cpr_conv_group_wgrad(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int cg, int stride,
                         int accumulate, void* stream);
/* The same two over maps whose pixels are Cp floats apart (RegNet: widths that are no multiple of 32 live at Cp = roundup(C, 32);
 * Cp >= C, Cp % 4 == 0).  The pad channels [C, Cp) of x / dy are never read (NaN there changes no output bit); the forward writes the pad
 * channels of out as +0.0 itself.  Pack, workspace and grad_w are those of C and cg.  Cp == C with cg in {4, 8, 16, 32} launches what
 * cpr_conv_group_fwd / _wgrad launch. */
int cpr_conv_group_fwd_pitch(const float* x, const float* wp, float* out, const float* scale, const float* bias, int N, int H, int W,
                             int C, int Cp, int cg, int stride, int flags, void* stream);
int cpr_conv_group_wgrad_pitch(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int Cp, int cg,
                               int stride, int accumulate, void* stream);
/* The grouped 3x3 with dilated taps (a dilated ResNeXt stage: stride 1, padding = tap step = dil >= 1, OH = H, OW = W), unpitched maps:
 * forward -- over dy with the data-gradient pack, the data gradient -- and weight gradient.  Packs and workspace query are those of
 * cpr_conv_group_fwd / _wgrad; still 9 * cg FMAs per output, tap-major: bit-repeatable and batch independent.  dil == 1 launches what
 * the undilated entries launch at stride 1. */
int cpr_conv_group_fwd_dil(const float* x, const float* wp, float* out, const float* scale, const float* bias, int N, int H, int W,
                           int C, int cg, int dil, int flags, void* stream);
int cpr_conv_group_wgrad_dil(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int cg, int dil,
                             int accumulate, void* stream);
/* ---- Res2Net slice kernels (Bottle2neck's 3x3 chain; csrc/res2net.hip), NHWC fp32, plain fp32 FMA ------------------------------
 * A slice is the channels [off, off + width) of a map whose pixels are `pitch` floats apart.  width even, 2 .. 512; every offset and
 * pitch even and every base pointer 8-byte aligned (the kernels move float2), off + width <= pitch: anything else is CPR_ERR_ARG before
 * any launch, and so are a NULL map, a stride other than 1 / 2 and an `add` operand at stride 2.  More than 2^31 - 1 pixels or blocks:
 * CPR_ERR_UNSUPPORTED.  Every kernel writes its own slice and nothing else.
 * cpr_res2_pack_weights: the parameter (width, width, 3, 3) -> the kernel's image (9 * width * width floats): transpose 0 the forward
 * pack, 1 the data-gradient pack (in / out channels swapped, taps flipped, scale[width] -- the forward conv's folded BatchNorm, or
 * NULL -- multiplied in). */
int cpr_res2_pack_weights(const float* w, const float* scale, float* out, int width, int transpose, void* stream);
/* out slice (N,OH,OW) = relu?(conv3x3(x slice [+ add slice], wp) * scale[c] + bias[c]), padding 1; add (same resolution, stride 1 only),
 * scale and bias may be NULL; x + add is rounded once to fp32 and a padding pixel contributes 0.  flags: CPR_CONV_RELU only.
 * transposed 0: the conv, (IH, IW) -> (OH, OW) = ((IH - 1) / stride + 1, (IW - 1) / stride + 1).  transposed 1: the data gradient with the
 * data-gradient pack: x is the gradient slice at (IH, IW) = ((OH - 1) / stride + 1, ...), out the layer's input size (OH, OW) -- a stride-2
 * layer in gather form, so 17 x 23 and 18 x 23 inputs are told apart by (OH, OW).  9 * width FMAs per output, tap-major, input channel
 * ascending: bit-repeatable, and an image of a batch equals its single-image run. */
int cpr_res2_conv_fwd(const float* x, int x_pitch, int x_off, const float* add, int add_pitch, int add_off, const float* wp, float* out,
                      int out_pitch, int out_off, const float* scale, const float* bias, int N, int IH, int IW, int OH, int OW, int width,
                      int stride, int transposed, int flags, void* stream);
/* grad_w (width, width, 3, 3) (+)= dy slice (N,OH,OW) against the x slice [+ add slice] (N,H,W).  The pixels are split over workgroups whose
 * partials (ws: cpr_res2_conv_wgrad_workspace(...) floats) are added in ascending order by a second kernel -- no atomics. */
int cpr_res2_conv_wgrad_workspace(int N, int OH, int OW, int width);
int cpr_res2_conv_wgrad(const float* dy, int dy_pitch, int dy_off, const float* x, int x_pitch, int x_off, const float* add, int add_pitch,
                        int add_off, float* grad_w, float* ws, int N, int H, int W, int width, int stride, int accumulate, void* stream);
/* Backward of a slice's ReLU, in place: g slice = (g slice (+ carry slice)) * (y slice > 0) over M pixels, and colsum[width] = the
 * per-channel sums of the result (chunk partials in ws, cpr_res2_relu_bwd_colsum_ws(M, width) floats, added in ascending order: no
 * atomics).  carry may be NULL.  _ws: M <= 0 or a width the slice kernels do not take is CPR_ERR_ARG, 2^31 floats or more
 * CPR_ERR_UNSUPPORTED. */
int cpr_res2_relu_bwd_colsum_ws(long long M, int width);
int cpr_res2_relu_bwd_colsum(float* g, int g_pitch, int g_off, const float* carry, int c_pitch, int c_off, const float* y, int y_pitch,
                             int y_off, float* colsum, float* ws, long long M, int width, void* stream);
/* The last slice of a stage block: stride 2: AvgPool2d(3, 2, padding 1) with the divisor always 9 (count_include_pad), (H, W) ->
 * ((H - 1) / 2 + 1, (W - 1) / 2 + 1); stride 1: the slice copied.  _bwd: dx slice (N,H,W) = its adjoint over the dy slice. */
int cpr_res2_pool_fwd(const float* x, int x_pitch, int x_off, float* out, int out_pitch, int out_off, int N, int H, int W, int width,
                      int stride, void* stream);
int cpr_res2_pool_bwd(const float* dy, int dy_pitch, int dy_off, float* dx, int dx_pitch, int dx_off, int N, int H, int W, int width,
                      int stride, void* stream);
/* ---- ResNeSt split attention, radix 2 (resnest.py:40-150; csrc/splat.hip), NHWC fp32 -------------------------------------------------
 * u (N,H,W,2w): the block's 3x3 conv + bn0 + ReLU output, channel r*w + c = split r of channel c.  w % 4 == 0, 4 .. 1024, inter 1 .. 1024,
 * pool 0 / 1, and N <= 65535 in the three reductions (gap, attn_grad, apply_bwd): anything else (and a NULL map) is CPR_ERR_ARG before any launch; 2^31 pixels or more is CPR_ERR_UNSUPPORTED.
 * Pixel reductions run per (image, chunk of pixels), cpr_splat_chunks(H, W, w) chunks per image -- a function of (H, W, w) alone --
 * and the chunk partials (ws) are added in ascending order by a second launch: no atomics, bit-repeatable, batch-independent.
 * cpr_splat_gap: g[n,c] = mean over pixels of u[n,p,c] + u[n,p,w+c].  ws: N * chunks * w floats. */
int cpr_splat_chunks(int H, int W, int w);
int cpr_splat_gap(const float* u, float* g, float* ws, int N, int H, int W, int w, void* stream);
/* One workgroup per image: z = relu(s1 * (fc1w g + fc1b) + t1) (fc1w (inter, w); s1 / t1 the folded eval BatchNorm), a = fc2w z + fc2b
 * (fc2w (2w, inter)), att[n,r,c] = softmax over r of a[n, r*w + c] (the maximum subtracted, expf).  z (N, inter) may be NULL. */
int cpr_splat_attn(const float* g, const float* fc1w, const float* fc1b, const float* s1, const float* t1, const float* fc2w,
                   const float* fc2b, float* att, float* z, int N, int w, int inter, void* stream);
/* out = sum_r att[n,r,c] * u[n,p,r*w+c] (N,H,W,w), or with pool AvgPool2d(3, 2, padding 1) of it in the same launch: (N,(H-1)/2+1,
 * (W-1)/2+1,w), out-of-range taps contribute 0, the divisor is always 9. */
int cpr_splat_apply(const float* u, const float* att, float* out, int N, int H, int W, int w, int pool, void* stream);
/* datt[n,r,c] = sum over pixels of dv[n,p,c] * u[n,p,r*w+c]; dv = dout (N,H,W,w), or with pool the pool's adjoint of dout
 * (N,(H-1)/2+1,(W-1)/2+1,w) in gather form.  ws: N * chunks * 2w floats. */
int cpr_splat_attn_grad(const float* dout, const float* u, float* datt, float* ws, int N, int H, int W, int w, int pool, void* stream);
/* Per image: da = att * (datt - sum_r att * datt), dz = fc2w^T da, dh' = dz * (z > 0), dh = s1 * dh', dg (N,w) = fc1w^T dh.  Then the
 * parameter gradients, images added in ascending order (each may be NULL): fc2w / fc2b from da and z, fc1w / fc1b from dh and g, the
 * eval BatchNorm's weight / bias from dh' and xhat = (fc1w g + fc1b - mean) * inv_sigma.  ws: N * (2w + 3 * inter) floats. */
int cpr_splat_attn_bwd(const float* att, const float* datt, const float* z, const float* g, const float* fc1w, const float* fc1b,
                       const float* s1, const float* mean, const float* inv_sigma, const float* fc2w, float* dg, float* ws, float* gfc1w,
                       float* gfc1b, float* gbnw, float* gbnb, float* gfc2w, float* gfc2b, int N, int w, int inter, void* stream);
/* du[n,p,r*w+c] = (att[n,r,c] * dv[n,p,c] + dg[n,c] / (H*W)) * (u > 0) and colsum[2w], its per-channel sums over images and pixels
 * (chunks of an image, then images, ascending).  ws: N * chunks * 2w + N * 2w floats. */
int cpr_splat_apply_bwd(const float* dout, const float* u, const float* att, const float* dg, float* du, float* colsum, float* ws, int N,
                        int H, int W, int w, int pool, void* stream);
/* MobileNetV2 (T/mmdet/models/backbones/mobilenet_v2.py, T/mmdet/models/utils/inverted_residual.py; csrc/mbv2.hip): the depthwise 3x3
 * convolution (groups == channels), padding 1, stride 1 or 2, and the ReLU6 passes around it.  fp32 NHWC maps at the channel pitch
 * Cp = roundup(C, 32), C % 8 == 0: pad channels [C, Cp) of an input are never read, pad channels of an output are written as +0.0.  No
 * atomics: every element is a fixed-order sum (bit-repeatable, an image of a batch equals its single-image run); reductions over pixels
 * go through per-workgroup partials in a caller-allocated workspace, added in ascending order by a second kernel.  A shape outside
 * these rules, another stride or an undefined flag bit: CPR_ERR_ARG before any launch.
 * cpr_dw3x3_pack: w (C,1,3,3) -> wp [9][Cp] tap-major, pad 0, scale[c] (optional) multiplied in (the data-gradient pack carries the
 *   folded BatchNorm scale); run again on the same buffers it overwrites the pack in place (the backbone rebuilds its packs instead). */
#define CPR_DW_IN_CLAMP6 1 /* the input is read as min(x, 6): its producer's epilogue wrote ReLU(v), the upper clamp happens on load */
#define CPR_DW_RELU6 2     /* out = min(max(v, 0), 6) */
int cpr_dw3x3_pack(const float* w, const float* scale, float* wp, int C, void* stream);
/* y (N,OH,OW) = act(scale[c] * sum_{kh,kw} in(x)[n, oh s + kh - 1, ow s + kw - 1, c] * w[c,kh,kw] + bias[c]), zero outside the map,
 * (OH, OW) = ((H - 1) / s + 1, (W - 1) / s + 1); scale / bias (C) may be NULL (both NULL, flags 0: the raw form). */
int cpr_dw3x3_fwd(const float* x, const float* wp, const float* scale, const float* bias, float* y, int N, int H, int W, int C, int stride,
                  int flags, void* stream);
/* dx (N,H,W) = sum over the taps with (h + 1 - kh) % s == 0, (w + 1 - kw) % s == 0 and the quotient in range of
 * dy[n, (h + 1 - kh) / s, (w + 1 - kw) / s, c] * wp[kh,kw,c] -- the gather form, no zero insertion; dy (N,(H-1)/s+1,(W-1)/s+1).
 * add (optional, dx's shape) is summed in, then mask (optional, dx's shape: the ReLU(v) map of the layer's producer) keeps the element
 * where 0 < mask < 6 (both strict, torch's hardtanh backward).  colsum (optional, (C)): the per-channel sums of dx; then ws holds
 * cpr_dw3x3_dgrad_workspace(N, H, W, C) floats. */
int cpr_dw3x3_dgrad_workspace(int N, int H, int W, int C);
int cpr_dw3x3_dgrad(const float* dy, const float* wp, const float* add, const float* mask, float* dx, float* colsum, float* ws, int N, int H,
                    int W, int C, int stride, void* stream);
/* grad_w (C,1,3,3) (+)= sum_{n,oh,ow} dy[n,oh,ow,c] * in(x)[n, oh s + kh - 1, ow s + kw - 1, c]; x (N,H,W), in_clamp6 (0 / 1) reads
 * min(x, 6); accumulate (0 / 1): one more rounded addition onto grad_w.  ws: cpr_dw3x3_wgrad_workspace(N, H, W, C, stride) floats. */
int cpr_dw3x3_wgrad_workspace(int N, int H, int W, int C, int stride);
int cpr_dw3x3_wgrad(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int stride, int in_clamp6,
                    int accumulate, void* stream);
/* The ReLU6 twin of cpr_relu_bwd_colsum: g = (dy (+ add)) * (0 < y < 6) and colsum (C) = its per-channel sums; (M,C) row-major,
 * C % 4 == 0.  y is a clamped map or the ReLU(v) map (the predicate is the same).  y NULL: the column sums of dy alone (g_out may then
 * be NULL, add must be).  ws: cpr_relu6_bwd_colsum_ws(M, C) floats. */
int cpr_relu6_bwd_colsum_ws(long long M, int C);
int cpr_relu6_bwd_colsum(const float* dy, const float* add, const float* y, float* g_out, float* colsum, float* ws, long long M, int C,
                         void* stream);
/* x = min(x, 6) in place over n floats (n % 4 == 0): a ReLU(v) map that leaves the backbone with no clamping consumer */
int cpr_clamp6(float* x, long long n, void* stream);
/* FPN extra pyramid levels (fpn.py:195-217; csrc/fpn_extra.hip), NHWC, 16 bytes of channels per lane.
 * cpr_subsample2: out (N,(H+1)/2,(W+1)/2,C) = y[:, ::2, ::2, :] with y = x, or x*a[n,c] + b[n,c] when a/b (N,C) are given (the producer's
 * pending GroupNorm affine, cpr_gn_apply's arithmetic) -- F.max_pool2d(y, 1, stride=2) bit for bit.  x/out fp32 (C%4==0) or bf16
 * (x_bf16, C%8==0). */
int cpr_subsample2(const void* x, int x_bf16, const float* a, const float* b, void* out, int N, int H, int W, int C, void* stream);
/* its backward joined with the finer level's own gradient: out (N,H,W,C) = dfine + zero_insert(dcoarse (N,(H+1)/2,(W+1)/2,C)), one pass */
int cpr_subsample2_bwd_add(const float* dfine, const float* dcoarse, float* out, int N, int H, int W, int C, void* stream);
/* relu_before_extra_convs: out = dz + (y > 0 ? d : 0) on flat buffers of n floats (n%4==0); y fp32, or bf16 with y_bf16 */
int cpr_relu_mask_add(const float* dz, const float* d, const void* y, int y_bf16, float* out, long long n, void* stream);
/* PAFPN bottom-up sum (pafpn.py:131-135; csrc/pafpn.hip): y (N,H,W,C) = (x1*a1[n,c] + b1[n,c]) + (x2*a2[n,c] + b2[n,c]), two raw conv outputs
 * under the pending GroupNorm affines (N,C) of their layers, one streaming pass; y may be x1 or x2.  fp32 (C%4==0, C<=1024), or _bf16: both
 * maps and y bf16 (C%8==0, C<=2048), fp32 arithmetic, one rounding.  N*H*W < 2^31. */
int cpr_gn_apply2(const float* x1, const float* a1, const float* b1, const float* x2, const float* a2, const float* b2, float* y, int N, int H,
                  int W, int C, void* stream);
int cpr_gn_apply2_bf16(const void* x1, const float* a1, const float* b1, const void* x2, const float* a2, const float* b2, void* y, int N,
                       int H, int W, int C, void* stream);
/* BFP neck, the Balanced Feature Pyramid (bfp.py:69-101; csrc/bfp.hip), NHWC.  One launch each over a HOST table of L <= 8 levels,
 * finest first; r = refine_level, (h, w) = the size of level r.  A level finer than r is pooled to (h, w) by adaptive max (window i of an
 * axis = [floor(i*in/out), ceil((i+1)*in/out)), first maximum in row-major order), level r and coarser ones are resized by nearest
 * (src = min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out: sy, sx are formed by the HOST in fp32); the scatter runs
 * the other way round.  a, b (N,C): the pending GroupNorm affine of a raw level, applied on load, or both null.  arg: the recorded argmax
 * of every pooled window, (N, out_h, out_w, C) window-local codes -- uint8 (ly << 4 | lx) when no window side exceeds 16, else with
 * arg_wide uint16 (ly << 8 | lx); CPR_ERR_UNSUPPORTED for a window beyond the chosen width.
 *   cpr_bfp_gather        x = level_i [a, b]; sy = (float)H/h, sx = (float)W/w (levels >= r); arg: optional record (levels < r).
 *                         bsf (N,h,w,C) = (sum_i feat_i) / L
 *   cpr_bfp_scatter       x = level_i [a, b], y = out_i = residual_i + level_i; sy = (float)h/H, sx = (float)w/W (levels < r); arg: optional
 *                         record (levels > r).  ref (N,h,w,C): the refined map, materialised, or raw under ref_a, ref_b (N,C) AND ReLU
 *   cpr_bfp_scatter_bwd   x = g_i (the level's shape), sy / sx as in the scatter, arg: its record (levels > r).  d_ref (N,h,w,C) = the sum
 *                         over the levels in ascending order, gather form, no atomics
 *   cpr_bfp_gather_bwd    x = g_i, y = d_level_i = g_i + (d_bsf / L routed back), sy / sx as in the gather, arg: its record (levels < r)
 * fp32: C%4==0; _bf16: levels, bsf / ref and out_i bf16, C%8==0, fp32 arithmetic, one rounding at the store.  The backward maps are fp32.
 * Every map below 2^31 elements.  Bit-repeatable; an image's result does not depend on the batch. */
typedef struct cpr_bfp_level {
    const void* x;
    const float* a;
    const float* b;
    void* y;
    void* arg;
    int H, W;
    float sy, sx;
} cpr_bfp_level;
int cpr_bfp_gather(const cpr_bfp_level* levels, int L, int refine_level, float* bsf, int N, int C, int arg_wide, void* stream);
int cpr_bfp_gather_bf16(const cpr_bfp_level* levels, int L, int refine_level, void* bsf, int N, int C, int arg_wide, void* stream);
int cpr_bfp_scatter(const cpr_bfp_level* levels, int L, int refine_level, const float* ref, const float* ref_a, const float* ref_b, int N,
                    int C, int arg_wide, void* stream);
int cpr_bfp_scatter_bf16(const cpr_bfp_level* levels, int L, int refine_level, const void* ref, const float* ref_a, const float* ref_b,
                         int N, int C, int arg_wide, void* stream);
int cpr_bfp_scatter_bwd(const cpr_bfp_level* levels, int L, int refine_level, float* d_ref, int N, int C, int arg_wide, void* stream);
int cpr_bfp_gather_bwd(const cpr_bfp_level* levels, int L, int refine_level, const float* d_bsf, int N, int C, int arg_wide, void* stream);
/* HRFPN neck (hrfpn.py:76-99; csrc/hrfpn.hip), NHWC.  reduction_conv(cat_i(bilinear_i(x_i))) = bias + y_0 + sum_{i>=1} bilinear_i(y_i)
 * with y_i the 1x1 conv of level i by its column slice of the reduction weight, at the level's own resolution.  Levels come in HOST
 * tables, finest first; level i is (N, H0 >> i, W0 >> i, C).  bilinear_i is torch's F.interpolate(scale_factor=2^i, mode='bilinear',
 * align_corners=False): src = max(0, (dst + 0.5) / 2^i - 0.5), taps floor(src) and min(floor(src) + 1, in - 1).
 *   cpr_hrfpn_fuse        levels = y_0 .. y_{L-1}, L <= 4, H_i << i == H0 and W_i << i == W0 (else CPR_ERR_ARG: the reference's cat
 *                         fails there); bias (C) or null.  out (N,H0,W0,C) = bias + y_0 + sum_i bilinear_i(y_i), fp32 sum in that order,
 *                         the four taps of a level in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1)
 *   cpr_hrfpn_pool        levels = the pooled outputs 1 .. K1 (K1 <= 4), level k = F.avg_pool2d(out, 2^k, 2^k): floor mode, (H0 >> k,
 *                         W0 >> k), none empty; every level from `out` itself, window in row-major order, one launch
 *   cpr_hrfpn_pool_bwd    gs = g_0 .. g_{K-1} (fp32), K <= 5.  d_out = g_0 + sum_k g_k[y >> k, x >> k] / 4^k inside level k's floor
 *                         region; part [cpr_hrfpn_pool_bwd_blocks(N, H0, W0)][C][2]: per-block column sums of d_out (element 0 = sum),
 *                         what cpr_part_colsum reduces
 *   cpr_hrfpn_fuse_bwd    dys = dy_1 .. dy_{L1} (fp32 outputs, L1 <= 3), H_i << i == H0: the adjoint of bilinear_i applied to d_out, gather
 *                         form through LDS, destination rows ascending, within a row columns ascending (the row sum first)
 * fp32: C%4==0; _bf16: maps bf16, C%8==0, fp32 arithmetic, one rounding at the store.  The backward maps are fp32.  Every map below
 * 2^31 elements, N and H0 at most 65535.  No atomics: bit-repeatable; an image's result does not depend on the batch. */
typedef struct cpr_hrfpn_level {
    void* p;
    int H, W;
} cpr_hrfpn_level;
int cpr_hrfpn_fuse(const cpr_hrfpn_level* levels, int L, const float* bias, float* out, int N, int C, void* stream);
int cpr_hrfpn_fuse_bf16(const cpr_hrfpn_level* levels, int L, const float* bias, void* out, int N, int C, void* stream);
int cpr_hrfpn_pool(const float* out, int H0, int W0, const cpr_hrfpn_level* levels, int K1, int N, int C, void* stream);
int cpr_hrfpn_pool_bf16(const void* out, int H0, int W0, const cpr_hrfpn_level* levels, int K1, int N, int C, void* stream);
int cpr_hrfpn_pool_bwd_blocks(int N, int H0, int W0);
int cpr_hrfpn_pool_bwd(const cpr_hrfpn_level* gs, int K, float* d_out, float* part, int N, int C, void* stream);
int cpr_hrfpn_fuse_bwd(const float* d_out, int H0, int W0, const cpr_hrfpn_level* dys, int L1, int N, int C, void* stream);
/* HRNet branch exchange (hrnet.py:182-199, HRModule.forward; csrc/hrnet.hip), NHWC fp32, C%4==0.
 *   cpr_hrnet_fuse       out (N,H,W,C) = ReLU(t_0 + t_1 + ..): T <= 4 terms from a HOST table.  Term (p, k), k in 0..3: a map
 *                        (N, H >> k, W >> k, C) read at [y >> k, x >> k] -- torch's nearest rule for the scale factor 2^k; k = 0 is a map
 *                        at the output's size.  H % 2^k == 0 and W % 2^k == 0, else CPR_ERR_ARG.  The fp32 sum runs left to right in
 *                        table order, no multiply; ReLU(v) = v <= 0 ? +0.0 : v (a NaN stays a NaN)
 *   cpr_hrnet_fuse_bwd   g (N,H,W,C) = y <= 0 ? +0.0 : dy; pools[k - 1] = pool_k (N, H >> k, W >> k, C), k = 1..K (K <= 3, HOST array of
 *                        K pointers; H % 2^K == 0 and W % 2^K == 0): the sum of g over the 2^k x 2^k block, the adjoint of the nearest
 *                        upsample.  Order: pool_1 = ((g[2y,2x] + g[2y,2x+1]) + g[2y+1,2x]) + g[2y+1,2x+1], pool_k the same expression
 *                        over pool_{k-1}.  part [cpr_hrnet_fuse_bwd_blocks(N, H, W, C, K)][C][2]: per-block column sums of g (element
 *                        0 = sum; a lane adds its cells' pool_K values in ascending cell order, the block its lanes in ascending
 *                        order), what cpr_part_colsum reduces
 * Every map below 2^31 elements, N and H at most 65535.  No atomics: bit-repeatable; an image's result does not depend on the batch. */
typedef struct cpr_hrnet_term {
    const void* p;
    int k;
} cpr_hrnet_term;
int cpr_hrnet_fuse(const cpr_hrnet_term* terms, int T, float* out, int N, int H, int W, int C, void* stream);
int cpr_hrnet_fuse_bwd_blocks(int N, int H, int W, int C, int K);
int cpr_hrnet_fuse_bwd(const float* dy, const float* y, float* g, float* const* pools, int K, float* part, int N, int H, int W, int C,
                       void* stream);
/* d(gt_loss + pos_loss + neg_loss)/d(logit map) of CPRHead.loss (cpr_head.py:1101-1229): negative-grid term, MIL bag
 * and gt-centre terms taken back through the bilinear taps -- deterministically: every bag's taps are gathered into a
 * win x win cell window (win >= 2 * ceil(max |offset| / stride) + 3; win_ws (G, win, win, J) fp32 and win_org (G, 2) int32
 * are caller workspaces), the windows are added per image in gt order (gt_img must ascend).  Inputs are the forward's own
 * buffers (neg mask, out5, bag logits, valid, bag_ws).  dbag_ws (G,K,J) workspace; dmap (N,H,W,Jd), Jd >= J, fully written.
 * upstream: NULL (the three losses enter the total with weight 1) or [device] 5 floats, the gradient of the total wrt
 * (gt_loss, pos_loss, bag_acc, neg_loss, num_sample) as torch autograd hands it to the head's loss Function; entries 2 and 4
 * carry no gradient and are ignored. */
int cpr_loss_bwd(const float* lmap, const unsigned char* neg_mask, const float* out5, const float* bag_logits,
                 const unsigned char* valid, const int* labels, const float* gt_weight, const float* bag_ws,
                 const float* centers, const int* gt_img, const float* offsets, float* dbag_ws, float* dmap, float* win_ws,
                 int* win_org, int win, int N, int H, int W, int J, int Jd, int ins_off, int G, int K, int C, float stride,
                 float eps, float w_mil, float w_gt, float w_neg, const float* upstream, void* stream);
/* win == 0 in cpr_loss_bwd: the bag logits were NOT sampled from the logit map (CPRHead num_cls_fcs > 0 samples the features and
 * runs them through the FC stack, cpr_head.py:1055-1059) -- dmap then holds the negative-grid term alone and dbag_ws (G,K,J) is
 * the gradient wrt the bag logits.  cpr_bag_gather_bwd is the gather stage on its own: dsample (G,K,J), the gradient wrt the
 * bilinear samples of a (N,H,W,.) map, is ADDED onto dmap (N,H,W,Jd) through bag_sample's taps (same windows, same order). */
int cpr_bag_gather_bwd(const float* dsample, int J, const float* centers, const int* gt_img, const float* offsets,
                       float* win_ws, int* win_org, int win, float* dmap, int N, int H, int W, int Jd, int G, int K,
                       float stride, void* stream);
/* The gather stage for bags whose taps are not ring offsets around a centre (round 5): GridCirclesPtFeatGenerator bags
 * (cpr_head.py:296-352,405-438) and align_corners=True sampling (:73-93,126).  Entries are the forward's own outputs: pts (G,Kt,2)
 * and code (G,Kt) -- cpr_grid_bag's ws_cell: cell index y*W+x | -1 padding slot | <= -2 bilinear sample at pts; NULL = every entry
 * is a bilinear sample (cpr_bag_sample).  dsample (G,Kt,J) is ADDED onto dmap (N,H,W,Jd) per image in gt order (gt_img ascends),
 * deterministically.  wout_ws (G*Kt) and dbias (J): both or neither; dbias <- sum over entries of (weight of the entry's dropped
 * taps) * dsample, the share of the projection's bias when the sampled map held logits (pad_value of cpr_bag_sample / cpr_grid_bag). */
int cpr_bag_points_gather_bwd(const float* dsample, int J, const float* pts, const int* code, const int* gt_img, float* dmap,
                              float* wout_ws, float* dbias, int N, int H, int W, int Jd, int G, int Kt, float stride,
                              int align_corners, void* stream);
/* The same loss gradients for every CPRHead loss option the forward kernels take (round 5): prob_type 0 sigmoid / 1 softmax /
 * 2 normed_sigmoid(norm_p) class probabilities (cpr_head.py:1080-1099), MILLoss(binary_ins) / AllPosLoss
 * (multi_instance_learning_loss.py:153-243), the bag / annotated-point geometry of cpr_mil_loss (refine_bag_policy, gt_loss_type:
 * cpr_head.py:1159-1211), C = classifier outputs (num_classes + 1 with out_bg_cls), neg_from_gt (with_mil_loss=False: the negative
 * term is averaged over the annotated-point positives).  dmap (N,H,W,Jd) <- the negative-grid term alone; dbag
 * (num_bags * bag_stride, J) <- the gradient wrt every bag entry's logits, NOT gathered (cpr_bag_gather_bwd /
 * cpr_bag_points_gather_bwd add it onto dmap).  neg_mask NULL: no negative-grid term (loss_cfg with_neg=False), dmap <- zeros. */
int cpr_loss_bwd_general(const float* lmap, const unsigned char* neg_mask, const float* out5, const float* bag_logits,
                         const unsigned char* valid, const int* labels, const float* gt_weight, const float* bag_ws, float* dbag,
                         float* dmap, int N, int H, int W, int J, int Jd, int ins_off, int num_bags, int bag_stride, int bag_off,
                         int bag_len, int ctr_off, int ctr_stride, int ctr_count, int ctr_mod, int C, float eps, int prob_type,
                         float norm_p, int binary_ins, int allpos, float w_mil, float w_gt, float w_neg, int neg_from_gt,
                         const float* upstream, void* stream);
/* OIHW fp32 master weights -> the conv kernels' layout [rows][KH][KW][cols'] (row stride Kpad, zero padded).
 * transpose 0: forward pack (rows = O).  transpose 1: data-gradient pack (rows = I, taps flipped, optional per-O scale =
 * the folded BatchNorm scale of the forward conv).  colsp = padded column count (4 for <= 4 channels). */
int cpr_pack_weights(const float* w, const float* scale, float* out, int O, int I, int KH, int KW, int colsp, int Kpad,
                     int transpose, void* stream);
/* The same packs for the bf16 conv kernels: out [rows][KH][KW][cols] bf16 (cols even, no padding), each element the
 * round-to-nearest-even of the fp32 value cpr_pack_weights would write; frag (NULL or rows % 64 == 0, KH*KW*cols % 16 == 0): the
 * same values in the fragment order cpr_conv2d_fwd_bf16's wgt_frag documents.  One launch per layer. */
int cpr_pack_weights_bf16(const float* w, const float* scale, void* out, void* frag, int O, int I, int KH, int KW, int transpose,
                          void* stream);
/* One idle wave for `ticks` of the 100 MHz wall clock (<= 1 s) on `stream`: a probe for whether two streams share a hardware queue
 * (the HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES queues; two of these launches on one queue run back to back). */
int cpr_spin(long long ticks, void* stream);
/* eval-mode BatchNorm (resnet.py norm_eval) -> conv-epilogue affine: scale = gamma/sqrt(var+eps), shift = beta - mean*scale,
 * inv_sigma (optional) = 1/sqrt(var+eps) */
int cpr_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* scale,
                float* shift, float* inv_sigma, int C, void* stream);
/* training-mode BatchNorm (ResNet norm_eval=False: T/mmdet/models/backbones/resnet.py:647-657, torch.nn.BatchNorm2d in training mode)
 * on an NHWC fp32 map y (M, C), M = N*H*W > 1, C % 64 == 0.  ws: cpr_bn_train_ws(M, C) floats.
 * cpr_bn_batch_stats: mean, rstd = 1/sqrt(biased var + eps), scale = gamma*rstd and shift = beta - mean*scale (each (C); scale /
 *   shift may be NULL); running_mean / running_var (both or neither) updated in place with the unbiased variance,
 *   num_batches_tracked (int64, may be NULL when momentum >= 0) incremented; momentum < 0 = torch's momentum None (1 / count).
 *   Per-(row block, channel) Welford partials merged by Chan's formula in a fixed order: bit-repeatable, no float atomics.
 *   center / cmean / cshift (all or none): the centred form for maps whose mean is far above their spread -- center = the map's
 *   first row, cmean = mean - center, cshift = beta - cmean*scale, so that (y - center)*scale + cshift normalises with an exact
 *   first difference.
 * cpr_bn_apply: out = [ReLU]((y - center)*scale + shift [+ residual] [+ (y2 - center2)*scale2 + shift2]); center / center2 may be
 *   NULL (= 0); residual and y2 are exclusive (y2: the projection shortcut of a bottleneck, never materialised).
 * cpr_bn_train_bwd: g = dout * (z > 0) (z = the recorded post-ReLU output, or NULL: g = dout); xhat = ((y - center) - mean)*rstd
 *   (center NULL = 0; with the centred statistics: center, cmean); dbeta = sum g, dgamma = sum g*xhat (either may be NULL),
 *   dy = gamma*rstd*(g - dbeta/M - xhat*dgamma/M). */
int cpr_bn_train_ws(long long M, int C);
int cpr_bn_batch_stats(const float* y, const float* gamma, const float* beta, float* running_mean, float* running_var,
                       long long* num_batches_tracked, float momentum, float eps, float* mean, float* rstd, float* scale, float* shift,
                       float* center, float* cmean, float* cshift, float* ws, long long M, int C, void* stream);
int cpr_bn_apply(const float* y, const float* center, const float* scale, const float* shift, const float* residual, const float* y2,
                 const float* center2, const float* scale2, const float* shift2, float* out, long long M, int C, int relu, void* stream);
int cpr_bn_train_bwd(const float* dout, const float* z, const float* y, const float* center, const float* mean, const float* rstd,
                     const float* gamma, float* dy, float* dgamma, float* dbeta, float* ws, long long M, int C, void* stream);
/* SyncBN: the batch statistics of training-mode BatchNorm over the rows of ALL ranks (norm_cfg=dict(type='SyncBN'): mmcv's
 * build_norm_layer -> torch.nn.SyncBatchNorm at T/mmdet/models/backbones/resnet.py:33-34, :160-162, :606; the collective
 * between the two halves is the caller's, torch.distributed.all_gather_into_tensor).  The finalize step of cpr_bn_batch_stats and of
 * cpr_bn_train_bwd in split form; a rank's map may hold a single row (M >= 1).  ws: cpr_bn_sync_ws(M, C) floats, shared by a local call
 * and the merge call that follows it.  Exchange records are fp64, gathered rank-major:
 *   statistics (2C + 1): [0, C) the absolute mean of this rank's rows, [C, 2C) their M2, [2C] the row count (an integer value);
 *   backward   (2C):     [0, C) sum g, [C, 2C) sum g*(y - mean) over this rank's rows.
 * cpr_bn_sync_stats_local: y -> record.
 * cpr_bn_sync_stats_merge: records (R, 2C + 1) merged in rank order by Chan's k-group form in fp64 -> the vectors of cpr_bn_batch_stats
 *   (biased variance over the global count), the running buffers (unbiased variance over the global count - 1) and num_batches_tracked
 *   (+ 1) updated as there, count (1 double, may be NULL) = the global row count.  y: THIS rank's map -- center = its first row, so
 *   center / cmean / cshift are rank-local; mean, rstd, scale, shift and the running buffers are functions of the records alone
 *   (bit-identical on every rank).
 * cpr_bn_sync_bwd_local: record, and this rank's dbeta = sum g, dgamma = rstd * sum g*(y - mean) over its OWN rows (either may be
 *   NULL) -- torch's SyncBatchNorm hands each rank its local parameter-gradient sums, the gradient reducer averages them.  mean / center
 *   as cpr_bn_train_bwd (the centred statistics: center, cmean).
 * cpr_bn_sync_bwd_merge: records (R, 2C) summed in rank order in fp64, count = the global row count (device, from the statistics
 *   merge) -> dy = gamma*rstd*(g - sum g / count - xhat * sum g*xhat / count), sums over all ranks. */
int cpr_bn_sync_ws(long long M, int C);
int cpr_bn_sync_stats_local(const float* y, double* record, float* ws, long long M, int C, void* stream);
int cpr_bn_sync_stats_merge(const double* records, int R, const float* y, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, long long* num_batches_tracked, float momentum, float eps, float* mean, float* rstd,
                            float* scale, float* shift, float* center, float* cmean, float* cshift, double* count, int C, void* stream);
int cpr_bn_sync_bwd_local(const float* dout, const float* z, const float* y, const float* center, const float* mean, const float* rstd,
                          float* dgamma, float* dbeta, double* record, float* ws, long long M, int C, void* stream);
int cpr_bn_sync_bwd_merge(const double* records, int R, const double* count, const float* dout, const float* z, const float* y,
                          const float* center, const float* mean, const float* rstd, const float* gamma, float* dy, float* ws, long long M,
                          int C, void* stream);
/* P2PHead's output convolutions in the bf16 compute mode (csrc/p2p_out_bf16.hip): a 3x3 / pad 1 / stride 1 conv with bias from the
 * RAW bf16 NHWC map x (N,H,W,Cin) of the last tower layer -- read as relu(a*x + b) with its per-(image, channel) GroupNorm affine
 * a, b (N,Cin) fp32, the activation never written -- to J output channels.  w (J,Cin,3,3) and bias (J) fp32 (the nn.Conv2d
 * parameters as they are).  Cin in {64, 128, 192, 256}, 1 <= J <= 8, any H, W; returns CPR_ERR_UNSUPPORTED outside that.
 * Arithmetic: every bf16 element widened exactly, relu(fmaf(a, x, b)) in fp32, products and sums fp32 (no bf16 rounding of the
 * activation).
 * cpr_p2p_out_bf16_fwd: out (N,H,W,J) fp32.  taps (N,H,W,9J) fp32 workspace: the tap responses, summed by cpr_tap_sum3x3 (the
 *   second of the two launches this entry enqueues).
 * cpr_p2p_out_bf16_dgrad: dx (N,H,W,Cin) <- the gradient wrt the ACTIVATED input, sum over taps and j of dout * w (x, a, b not
 *   needed); dout (N,H,W,J) fp32 with row stride ldd >= J (a channel-padded gradient map is read as it is); out_bf16: dx is bf16,
 *   each element the round-to-nearest-even of the fp32 value, else fp32.
 * cpr_p2p_out_bf16_wgrad: gw (J,Cin,3,3) and gb (J) WRITTEN (caller-given, e.g. a trainer's gradient views) from dout and the
 *   activated map.  Per-wave partials over fixed pixel ranges into ws (cpr_p2p_out_bf16_wgrad_ws floats), summed in a fixed order
 *   by a finalize launch: bit-repeatable, no float atomics. */
int cpr_p2p_out_bf16_fwd(const void* x, const float* a, const float* b, const float* w, const float* bias, float* taps, float* out,
                         int N, int H, int W, int Cin, int J, void* stream);
int cpr_p2p_out_bf16_dgrad(const float* dout, int ldd, const float* w, void* dx, int out_bf16, int N, int H, int W, int Cin, int J,
                           void* stream);
int cpr_p2p_out_bf16_wgrad_ws(int N, int H, int W, int Cin, int J);
int cpr_p2p_out_bf16_wgrad(const void* x, const float* a, const float* b, const float* dout, int ldd, float* gw, float* gb, float* ws,
                           int N, int H, int W, int Cin, int J, void* stream);
/* Multi-tensor forms of cpr_bn_fold and cpr_pack_weights_bf16 (round 6; the per-step refresh of the mixed-precision / fp32 training
 * step, layers._PackCache.refresh_all): one launch over a DEVICE table of 64-byte jobs --
 *   fold job: { const float *gamma, *beta, *mean, *var; float *scale, *shift, *inv (each may be NULL); int C; float eps; }
 *   pack job: { const float* w; const float* scale; void* out; void* frag; int O, I, KH, KW, transpose, block0, nblocks, pad; }
 * (pack jobs in ascending block0; job j owns workgroups [block0, block0 + nblocks) of the total_blocks launched).  Results are
 * bit for bit the single-tensor entries'. */
int cpr_bn_fold_multi(const void* jobs_dev, int n, int max_c, void* stream);
/* ... and of cpr_pack_weights (fp32 packs): job { const float* w; const float* scale; float* out; int nblocks, pad;
 * int O, I, KH, KW, colsp, Kpad, transpose, block0; } */
int cpr_pack_weights_multi(const void* jobs_dev, int n, int total_blocks, void* stream);
int cpr_pack_weights_bf16_multi(const void* jobs_dev, int n, int total_blocks, void* stream);
/* gradient of sum_b (loss_cls[b] + loss_pts[b]) of cpr_p2p_loss wrt the class logits (B*M, C) and the regression output
 * (p2p_head.py:220-248; sigmoid focal loss with its un-detached focal weight, SmoothL1 through
 * pred = anchor + (point_anchor + reg*gamma_p)*stride).  npos: device scalar, positives in the batch.  dcls (B*M, Cp),
 * dreg (B*M, Rp): channel-padded for the conv gradient kernels, padding columns written as zero.  upstream: NULL (every loss
 * term enters the total with weight 1) or [device] (B, 2) gradients of the total wrt (loss_cls[b], loss_pts[b]) -- what
 * torch autograd hands the head's loss Function (replaces loss.backward() through p2p_head.py:220-248). */
int cpr_p2p_loss_bwd(const float* logits, const float* pred, const long long* gt_inds, const float* gt_pts,
                     const int* gt_labels, const int* gt_start, const float* npos, float* dcls, float* dreg, int B, int M,
                     int C, int Cp, int Rp, float alpha, float gamma, float beta, float pos_w, float neg_w, float reg_norm,
                     float w_cls, float w_reg, float gamma_p, const float* upstream, int cls_mode, int reg_mode, void* stream);
/* the same gradient for L FPN levels and P points per cell (L <= 8, P >= 1), written straight into every level's output-conv
 * gradient maps: the proposal rows m in [0, M) are the levels' concatenation, level l owning [level_off[l], level_off[l] +
 * level_hw[l] * P) cell-major (the table must tile [0, M) exactly).  Class c of point p goes to channel p*C + c of level_dcls[l]
 * (B, H_l, W_l, level_cp[l] >= P*C), coordinate k to channel p*2 + k of level_dreg[l] (B, H_l, W_l, level_rp[l] >= 2P); padding
 * channels are written as zero.  The tables are HOST arrays of L entries.  The CrossEntropyLoss average runs over all B*M rows.
 * L = 1, P = 1 gives cpr_p2p_loss_bwd's output bit for bit. */
int cpr_p2p_loss_bwd_levels(const float* logits, const float* pred, const long long* gt_inds, const float* gt_pts,
                            const int* gt_labels, const int* gt_start, const float* npos, int B, int M, int C, int P, int L,
                            const int* level_hw, const int* level_off, const int* level_cp, const int* level_rp,
                            float* const* level_dcls, float* const* level_dreg, float alpha, float gamma, float beta, float pos_w,
                            float neg_w, float reg_norm, float w_cls, float w_reg, float gamma_p, const float* upstream,
                            int cls_mode, int reg_mode, void* stream);
/* sum of squares of a flat gradient buffer into out[0] (double; accumulate across buffers); ws_partial 1024 doubles */
int cpr_grad_sumsq(const float* g, long long n, double* ws_partial, double* out, int accumulate, void* stream);
/* torch.optim.SGD step (momentum, weight decay) with clip_grad_norm_'s coefficient taken from norm2 on the device:
 * g = min(1, max_norm/(sqrt(norm2)*grad_scale+1e-6)) * grad_scale * grad + wd*p; buf = first ? g : mu*buf+g; p -= lr*buf */
int cpr_sgd_step(float* p, const float* grad, float* buf, const double* norm2, long long n, float lr, float mu, float wd,
                 float max_norm, float grad_scale, int first, void* stream);
/* torch.optim.Adam / AdamW step (amsgrad=False) on one flat fp32 buffer with the clip coefficient of cpr_sgd_step; the P2P
 * configs train with optimizer = dict(type='Adam', lr=1e-4) + grad_clip max_norm 35
 * (configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py:86-93, configs2/COCO/p2p/p2p_r50_fpns4_1x_fl_sl1_coco.py:
 * 141-143, both configs2/DOTA/p2p/ configs: 152-154).  torch's op order, each op rounded:
 *   g = coef*grad (+ wd*p: Adam);  p *= 1 - lr*wd (AdamW, decoupled=1);  m = lerp(m, g, 1-beta1);  v = v*beta2 + (1-beta2)*g*g;
 *   p += -step_size * (m / (sqrt(v)/bc2_sqrt + eps))
 * step_size = lr/(1-beta1^t), bc2_sqrt = sqrt(1-beta2^t): computed by the caller in double, t = 1 at the first step. */
int cpr_adam_step(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, const double* norm2, long long n, double lr,
                  double beta1, double beta2, double eps, double wd, float step_size, float bc2_sqrt, float max_norm,
                  float grad_scale, int decoupled, void* stream);

/* ---- data side feeding the path ----------------------------------------------------------
 * RandomFlip(horizontal) -> Normalize -> Pad(0 after normalisation) -> channels-last float of the mmdet pipeline
 * (T/mmdet/datasets/pipelines/transforms.py:431-480,560-680, formating.py:180-214) in one pass: img (N,H,W,3) uint8
 * decoded images on the device -> out (N,Hp,Wp,4) fp32, the stem's input layout (4th channel and padding zero).
 * mean3 / stdinv3: HOST pointers to 3 floats (stdinv = float32(1/float64(std)) as mmcv.imnormalize_); flip (N) int32
 * device flags or NULL. */
int cpr_preprocess_u8(const unsigned char* img, const int* flip, const float* mean3, const float* stdinv3, int to_rgb,
                      float* out, int N, int H, int W, int Hp, int Wp, void* stream);
/* Box side of Resize(scale 1) -> RandomFlip, in place: clip every box to its image when `clip` (Resize._resize_bboxes,
 * bbox_clip_border=True, transforms.py:241-249), then mirror it when flip[img] (RandomFlip.bbox_flip, :397-415).
 * boxes (n,4) xyxy, img_of (n) image index, flip (N), img_hw (N,2) int32 = img_shape[:2] */
int cpr_clip_flip_boxes(float* boxes, const int* img_of, const int* flip, const int* img_hw, int n, int clip,
                        void* stream);

/* Resize in all its forms and the test-time wrappers (MultiScaleFlipAug, the fork's CroppedTilesFlipAug) in front of the same tail:
 *   crop -> cv2.resize(INTER_LINEAR) of the uint8 image -> horizontal flip -> Normalize -> Pad -> (Hp, Wp, 4) fp32
 * ONE launch for a table of jobs: a ragged training batch, or all tiles x scales x flips of one test image (tiles are crop
 * rectangles of one upload).  The resize is OpenCV's 8-bit fixed-point bilinear (11-bit coefficients, x taps clamped with their
 * coefficient, y rows clamped; csrc/preprocess.hip restates it), so an identity size returns the source exactly.
 * A job: `src` device address of pixel (0,0) of a decoded uint8 HWC BGR image of src_w x src_h with `pitch` bytes per row; crop
 * (x0, y0, cw, ch) inside it; resized size (dw, dh); scale_x = 1. / ((double)dw / cw), scale_y likewise (double, set by the host);
 * flip; out_off = first pixel of its slot in `out`, in pixels; (Hp, Wp) >= (dh, dw) its padded size.  Every job writes its whole
 * slot (zeros outside dh x dw and in the 4th channel). */
typedef struct cpr_preprocess_job {
    const unsigned char* src;
    long long out_off;
    double scale_x, scale_y;
    int pitch, src_w, src_h, x0, y0, cw, ch, dw, dh, flip, Hp, Wp;
} cpr_preprocess_job;
/* jobs_dev: n_jobs records ON THE DEVICE (n_jobs <= 65535; 0 is a no-op); mean3 / stdinv3 HOST pointers as for cpr_preprocess_u8;
 * out holds total_out_pixels (< 2^31) pixels of 4 floats.  CPR_ERR_ARG for a null table / output or a bad count.  The table is device
 * memory, so a job's geometry is checked where it is read: a job whose crop leaves its image or whose slot leaves `out` writes nothing
 * (ops.preprocess_jobs refuses it on the host copy, with the same error, before the upload). */
int cpr_preprocess_jobs_u8(const void* jobs_dev, int n_jobs, const float* mean3, const float* stdinv3, int to_rgb, float* out,
                           long long total_out_pixels, void* stream);
/* Box side of Resize -> RandomFlip at any scale, in place: box * scale4[img] in fp32 (the float32 scale_factor array of
 * Resize._resize_img; one rounding per coordinate), clip to the RESIZED img_shape when `clip`, mirror when flip[img]
 * (transforms.py:241-249, :397-415).  scale4 (N,4) fp32, img_hw (N,2) int32 = resized img_shape[:2]; the rest as cpr_clip_flip_boxes. */
int cpr_scale_clip_flip_boxes(float* boxes, const int* img_of, const int* flip, const int* img_hw, const float* scale4, int n,
                              int clip, void* stream);

/* ---- Darknet-53 (T/mmdet/models/backbones/darknet.py; csrc/darknet.hip), fp32 NHWC maps, 16 bytes of channels per lane.  The dense
 * conv epilogues know ReLU only: a Darknet ConvModule (conv -> BN -> LeakyReLU, darknet.py:45-47, :121, :205-208) runs its conv in the
 * raw folded form and these passes apply the activation.
 * cpr_leaky_fwd: out = (z > 0 ? z : z * slope) (+ res) over n floats (n % 4 == 0) -- F.leaky_relu bit for bit (the product is rounded,
 * then the sum: no FMA), NaN propagates, -0.0 stays -0.0.  res (optional): the ResBlock's ``out + residual`` (darknet.py:53).  out may
 * be z. */
int cpr_leaky_fwd(const float* z, const float* res, float* out, long long n, float slope, void* stream);
/* The LeakyReLU twin of cpr_relu_bwd_colsum / cpr_relu6_bwd_colsum: s = dy (+ add, optional, one rounding), g = y > 0 ? s : s * slope
 * (torch's leaky_relu_backward: the slope at y == 0) and colsum (C) = the per-channel sums of g; (M, C) row-major, C % 4 == 0.  y is the
 * pre-activation or the activated map (0 <= slope: the predicate is the same).  g_out may be NULL (the sums alone).  Per-workgroup
 * partials in ws (cpr_leaky_bwd_colsum_ws(M, C) floats) are added in ascending order by a second kernel -- no atomics. */
int cpr_leaky_bwd_colsum_ws(long long M, int C);
int cpr_leaky_bwd_colsum(const float* dy, const float* add, const float* y, float* g_out, float* colsum, float* ws, long long M, int C,
                         float slope, void* stream);
/* Weight gradient of Darknet's first conv (darknet.py:121: 3x3 / stride 1 / pad 1, 3 -> 32), the stride-1 sibling of
 * cpr_stem3x3s2_wgrad: gw (32, 3, 3, 3) = sum over n, h, w of dy[n, h, w, o] * in[n, h + kh - 1, w + kw - 1, c], zero outside the image;
 * dy (N, H, W, 32); in: layout 0 (N, H, W, 4) fp32 (4th channel ignored), layout 1 (N, 3, H, W) planes.  Pixel slices
 * (ws: cpr_stem3x3s1_wgrad_workspace(N, H, W) floats) are added in ascending order by a second kernel -- no atomics. */
int cpr_stem3x3s1_wgrad_workspace(int N, int H, int W);
int cpr_stem3x3s1_wgrad(const float* dy, const float* in, float* gw, float* ws, int N, int H, int W, int layout, void* stream);

/* ---- CTResNetNeck (T/mmdet/models/necks/ct_resnet_neck.py; csrc/deconv.hip): the transposed convolution 4x4 / stride 2 / padding 1
 * without bias, fp32 NHWC, on the fp32 matrix pipe.
 * cpr_pack_weights_deconv: the nn.ConvTranspose2d weight w (Cin, Cout, 4, 4) -> out, 16 * Cin * Cout floats: one [Cout][4 * Cin] GEMM image
 * per output-parity class, out[2a + b][co][(2t + u) * Cin + ci] = w[ci][co][1 - a + 2t][1 - b + 2u] (K ordered tap row, tap column, cin).
 * cpr_deconv4x4s2_fwd: out (N, 2H, 2W, Cout), out[n, 2i + a, 2j + b, co] = epi(sum_{t, u, ci} in[n, i + a - t, j + b - u, ci] * w[ci][co][..])
 * with taps outside the map contributing zero; one launch for the four classes, the interleaved map written directly (no scatter pass, no
 * atomics; a fixed k-ordered fp32 chain per element, independent of N and of the tile).  epi(v) = v * scale[co] + bias[co], then ReLU with
 * flags = CPR_CONV_RELU; scale / bias may each be NULL (both NULL: the raw sums).  variant_out (optional): BM * 10^6 + BN * 10^3 + 1 of the
 * tile instance that ran.  Cin % 32 == 0 and Cout % 32 == 0, else CPR_ERR_ARG before any launch. */
int cpr_pack_weights_deconv(const float* w, float* out, int Cin, int Cout, void* stream);
int cpr_deconv4x4s2_fwd(const float* in, const float* wgt, float* out, const float* scale, const float* bias, int N, int H, int W, int Cin,
                        int Cout, int flags, int* variant_out, void* stream);

/* ---- measurement build only (-DCPR_BENCH_HOOKS; python -m pointtinybenchmark_amd.build --bench-hooks) ------------------
 * Process-global, not thread-safe switches used by the scripts under tools/ to A/B the conv kernels.  NOT part of the
 * product library. */
#ifdef CPR_BENCH_HOOKS
int cpr_conv_force_tile(int bm, int bn); /* force the conv output tile (0 = heuristic, 64, 128) */
int cpr_conv_set_pipeline(int mode);     /* K-loop schedule: 1 = interleaved (product), 0 = phase-separated */
int cpr_conv_set_stream(int on);         /* 0 = the streamed 1x1 kernel (conv1x1_stream.hip) is never chosen by cpr_conv2d_fwd (A/B) */
int cpr_conv_set_ablation(int mode);     /* loop ablations: results are WRONG when non-zero */
int cpr_wgrad_set_ablation(int mode);    /* same for the weight-gradient kernel */
int cpr_conv_set_extra_lds(int bytes);   /* occupancy probe: dynamic LDS added to every direct-conv launch */
int cpr_wino_set_variant(int sched, int ablate); /* Winograd: sched 1 = the other placement of the patch transform (see conv_wino.hip); loop ablations */
int cpr_bf16_set_dma(int on);            /* bf16 mode: 0 = every layer on the register-staged kernels (A/B of conv_bf16_dma.hip) */
int cpr_bf16_set_wfrag(int on);          /* bf16 mode: 0 = ignore wgt_frag (A/B of the weights-direct-to-registers instance) */
int cpr_wino_set_staging(int var, int tpx);      /* Winograd: staging variant (kernel template VAR) and cout tiles per XCD; -1 = the product's choice */
int cpr_wino32_set_debug(int ablate, int wg_per_cu, int stagger_pct); /* conv_wino32.hip: loop ablations, workgroups per CU (1 / 2), stagger of the second wave of workgroups */
int cpr_lsa_phase_clocks(long long* host_out, int reset);            /* assign.hip: shader clocks workgroup 0 of lsa_topk_reg_kernel spent per phase (8 values) */
int cpr_bn_set_finalize_only(int on);    /* bn_train.hip: 1 = every entry skips its streaming passes (part / apply), so the finalize / local / merge launches can be timed alone; results are WRONG */
#endif

#ifdef __cplusplus
}
#endif
#endif /* CPR_HIP_H */
