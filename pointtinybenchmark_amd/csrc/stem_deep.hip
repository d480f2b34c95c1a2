// The deep stem of ResNetV1d (T/mmdet/models/backbones/resnet.py:564-596, 630-638) and the average pool of its avg_down shortcut
// (T/mmdet/models/utils/res_layer.py:39-60).
//
// Deep stem: image -> conv 3x3 / 2, 3 -> 32 -> conv 3x3, 32 -> 32 -> conv 3x3, 32 -> 64, each + folded eval-BatchNorm + ReLU, then
// max-pool 3x3 / 2 / pad 1 -> (N, H/4, W/4, 64) NHWC.  Exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32) in both compute
// modes; the bf16 mode differs only in the last store (one bf16 rounding of the pooled fp32 value).  Three launches:
//   A  stem_deep_a_kernel      3 -> 32, stride 2.  The patch sits in LDS as 4-float pixels (the 4th zero), so the 12 floats of a
//                              kernel row are contiguous for every output pixel: K = 3 rows x 12 = 18 MFMA steps.
//   B  stem_deep_bc_kernel<32, false>   32 -> 32: a workgroup owns 16 rows x 32 columns; a 32-pixel row segment x 32 couts is one
//                              32 x 32 MFMA block, K = 9 taps x 32 channels = 144 steps.
//   C  stem_deep_bc_kernel<64, true>    32 -> 64 + the max-pool in its epilogue: a workgroup owns 4 x 16 POOLED pixels = 9 x 33
//                              conv outputs (one halo row / column recomputed), BN + ReLU -> LDS -> 3x3 / 2 max -> 16-byte stores;
//                              the 64-channel conv map never reaches memory.
// Operand layout of B and C: LDS pixels of 32 + 4 floats (144 bytes: a quarter-wave's 16-byte reads fall on 16 distinct bank
// quads).  One 16-byte read feeds four MFMA steps: in steps 4 g .. 4 g + 3 of a tap the lanes of half h supply channels
// 8 g + 4 h .. 8 g + 4 h + 3 -- the order of the k index within a tap is free as long as both operands agree, and the weight rows
// ([cout][tap][channel], 288 + 4 floats in LDS) are read the same way.  All three weight images are the implicit-GEMM kernel's
// fp32 packs (ops.PackedConv: [cout][kh][kw][cin'], rows of Kpad floats), so the pack cache refreshes them like any other layer's.
#include "common.h"
#include <type_traits>

typedef __attribute__((ext_vector_type(2))) __bf16 sd_bf16x2;

// ------------------------------------------------------------------------------------------------------------ conv A: 3 -> 32 / 2
constexpr int SDA_TR = 16, SDA_TC = 32;                           // output tile
constexpr int SDA_PH = 2 * SDA_TR + 1, SDA_PW = 2 * SDA_TC + 1;   // patch: 33 rows x 65 pixels of 4 floats (the 4th zero)
constexpr int SDA_WROW = 36;                                      // floats per cout: 3 x 3 x 4, the implicit-GEMM pack's order

struct StemDeepAParams {
    const float* in;       // layout 0: (N, H, W, 4) fp32, 4th channel ignored; layout 1: (N, 3, H, W) fp32 planes
    const float* wgt;      // (32, wstride): [cout][kh][kw][4], channel 3 zero (ops.PackedConv of the 3-channel conv)
    const float* scale;    // folded BatchNorm (32)
    const float* bias;
    float* out;            // (N, OH, OW, 32)
    int N, H, W, OH, OW, tilesY, tilesX, layout, wstride;
};

__global__ __launch_bounds__(512) void stem_deep_a_kernel(StemDeepAParams p) {
    __shared__ __attribute__((aligned(16))) float patch[SDA_PH * SDA_PW * 4];
    __shared__ __attribute__((aligned(16))) float wl[32 * SDA_WROW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b = blockIdx.x;
    const int tx = b % p.tilesX;
    b /= p.tilesX;
    const int ty = b % p.tilesY;
    const int n = b / p.tilesY;
    const int r0 = SDA_TR * ty, c0 = SDA_TC * tx;
    const int iy0 = 2 * r0 - 1, ix0 = 2 * c0 - 1;
    for (int u = tid; u < 32 * SDA_WROW; u += 512) wl[u] = p.wgt[(u / SDA_WROW) * p.wstride + u % SDA_WROW];
    // (layout 1: the network input as torch hands it over, three planes; both layouts leave the same floats in LDS)
    const size_t plane = (size_t)p.H * p.W;
    const float* img = p.in + (size_t)n * plane * (p.layout ? 3 : 4);
    for (int u = tid; u < SDA_PH * SDA_PW; u += 512) {
        const int py = u / SDA_PW, px = u - py * SDA_PW;
        const int iy = iy0 + py, ix = ix0 + px;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
            const size_t o = (size_t)iy * p.W + ix;
            if (p.layout) { v[0] = img[o]; v[1] = img[plane + o]; v[2] = img[2 * plane + o]; }
            else v = *reinterpret_cast<const f32x4*>(img + o * 4);
            v[3] = 0.f;
        }
        *reinterpret_cast<f32x4*>(patch + u * 4) = v;
    }
    __syncthreads();

    const int l31 = lane & 31, half = lane >> 5;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    // wave w owns output rows w and w + 8 of the tile; lane (m, half): output column m.  Six MFMA steps per kernel row: in the first
    // four the lanes of half h supply the four floats of pixel kw = h, in the last two channels 2 h, 2 h + 1 of pixel kw = 2 (the
    // order of k within a kernel row is free as long as both operands agree)
    const float* a0 = patch + ((2 * wave) * SDA_PW + 2 * l31) * 4;
    const float* a1 = a0 + 16 * SDA_PW * 4;
    const float* bp = wl + l31 * SDA_WROW;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + kh * 12 + 4 * half);
        const f32x2 bw = *reinterpret_cast<const f32x2*>(bp + kh * 12 + 8 + 2 * half);
        const f32x4 av0 = *reinterpret_cast<const f32x4*>(a0 + kh * SDA_PW * 4 + 4 * half);
        const f32x4 av1 = *reinterpret_cast<const f32x4*>(a1 + kh * SDA_PW * 4 + 4 * half);
        const f32x2 aw0 = *reinterpret_cast<const f32x2*>(a0 + kh * SDA_PW * 4 + 8 + 2 * half);
        const f32x2 aw1 = *reinterpret_cast<const f32x2*>(a1 + kh * SDA_PW * 4 + 8 + 2 * half);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], bv[s], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], bv[s], acc[1], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw0[s], bw[s], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw1[s], bw[s], acc[1], 0, 0, 0);
        }
    }
    // D layout of a 32 x 32 block: col = lane & 31 (cout), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (pixel)
    const float sc = p.scale[l31], bi = p.bias[l31];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = r0 + wave + 8 * i;
        if (row >= p.OH) continue;
        float* orow = p.out + ((size_t)n * p.OH + row) * p.OW * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int col = c0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (col < p.OW) orow[(size_t)col * 32] = fmaxf(acc[i][r] * sc + bi, 0.f);
        }
    }
}

// -------------------------------------------------------------------------------- convs B / C: 32 -> NOUT, 3x3 / 1 / pad 1 (+ pool)
constexpr int SD_PIX = 36;                                        // floats per LDS pixel
constexpr int SD_WROW = 292;                                      // floats per cout in LDS and in the weight image: 9 x 32 + 4

template <int NOUT, bool POOL>
struct StemDeepGeom {
    static constexpr int TR = POOL ? 9 : 16;                      // conv rows of a tile
    static constexpr int PR = TR + 2, PC = POOL ? 35 : 34;        // patch rows / columns
    static constexpr int NBLK = POOL ? 10 : 16;                   // 32-pixel blocks: the rows (+ the halo column)
    static constexpr int NJ = NOUT / 32;                          // cout blocks
    static constexpr int PER_WAVE = POOL ? 3 : 2;                 // pixel blocks per wave (8 waves)
    static constexpr int PATCH = PR * PC * SD_PIX;
    static constexpr int WGT = NOUT * SD_WROW;
    static constexpr int CT = POOL ? 9 * 33 * NOUT : 0;           // the conv tile of the pooling epilogue (over patch + weights)
    static constexpr int LDS = PATCH + WGT > CT ? PATCH + WGT : CT;
};

struct StemDeepBCParams {
    const float* in;       // (N, H, W, 32) fp32
    const float* wgt;      // (NOUT, 288): [cout][tap][channel]
    const float* scale;    // folded BatchNorm (NOUT)
    const float* bias;
    void* out;             // (N, H, W, NOUT) fp32, or with the pool (N, PH, PW, NOUT) fp32 / bf16
    int N, H, W, PH, PW, tilesY, tilesX, out_bf16;
};

template <int NOUT, bool POOL>
__global__ __launch_bounds__(512) void stem_deep_bc_kernel(StemDeepBCParams p) {
    typedef StemDeepGeom<NOUT, POOL> G;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* patch = smem;
    float* wl = smem + G::PATCH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b = blockIdx.x;
    const int tx = b % p.tilesX;
    b /= p.tilesX;
    const int ty = b % p.tilesY;
    const int n = b / p.tilesY;
    const int r0 = POOL ? 8 * ty - 1 : 16 * ty, c0 = POOL ? 32 * tx - 1 : 32 * tx;   // first conv row / column of the tile

    for (int u = tid; u < NOUT * 72; u += 512)                    // rows of 288 floats -> rows of 292
        *reinterpret_cast<f32x4*>(wl + (u / 72) * SD_WROW + (u % 72) * 4) = *reinterpret_cast<const f32x4*>(p.wgt + u * 4);
    const float* img = p.in + (size_t)n * p.H * p.W * 32;
    for (int u = tid; u < G::PR * G::PC * 8; u += 512) {
        const int pix = u >> 3, q = u & 7;
        const int py = pix / G::PC, px = pix - py * G::PC;
        const int iy = r0 - 1 + py, ix = c0 - 1 + px;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
            v = *reinterpret_cast<const f32x4*>(img + ((size_t)iy * p.W + ix) * 32 + q * 4);
        *reinterpret_cast<f32x4*>(patch + pix * SD_PIX + q * 4) = v;
    }
    __syncthreads();

    const int l31 = lane & 31, half = lane >> 5;
    const int jb = POOL ? (wave & 1) : 0, qb = POOL ? (wave >> 1) : wave;
    constexpr int QS = POOL ? 4 : 8;                              // block stride between a wave's blocks
    f32x16 acc[G::PER_WAVE];
    int abase[G::PER_WAVE];
#pragma unroll
    for (int i = 0; i < G::PER_WAVE; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        int q = qb + QS * i;
        if (q >= G::NBLK) q = G::NBLK - 1;                         // (a wave without a third block recomputes the last one, unused)
        int prow, pcol;
        if (!POOL) { prow = q; pcol = l31; }
        else if (q < 9) { prow = q; pcol = l31 + 1; }
        else { prow = l31 < 8 ? l31 : 8; pcol = 0; }               // the halo column: rows r0 + min(m, 8)
        abase[i] = (prow * G::PC + pcol) * SD_PIX + 4 * half;
    }
    const bool third = !POOL || qb + QS * 2 < G::NBLK;            // wave-uniform
    const float* bptr = wl + (jb * 32 + l31) * SD_WROW + 4 * half;
    auto kloop = [&](auto nbc) {
        constexpr int NB = decltype(nbc)::value;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap - kh * 3;
            const float* prow = patch + (kh * G::PC + kw) * SD_PIX;
            const float* brow = bptr + tap * 32;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(brow + 8 * g);
                f32x4 av[NB];
#pragma unroll
                for (int i = 0; i < NB; ++i) av[i] = *reinterpret_cast<const f32x4*>(prow + abase[i] + 8 * g);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < NB; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][s], bv[s], acc[i], 0, 0, 0);
            }
        }
    };
    if (POOL && !third) kloop(std::integral_constant<int, G::PER_WAVE - 1>{});
    else kloop(std::integral_constant<int, G::PER_WAVE>{});

    const int c = jb * 32 + l31;
    const float sc = p.scale[c], bi = p.bias[c];
    if constexpr (!POOL) {
        float* out = reinterpret_cast<float*>(p.out);
#pragma unroll
        for (int i = 0; i < G::PER_WAVE; ++i) {
            const int row = r0 + qb + QS * i;
            if (row >= p.H) continue;
            float* orow = out + ((size_t)n * p.H + row) * p.W * NOUT + c;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = c0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (col < p.W) orow[(size_t)col * NOUT] = fmaxf(acc[i][r] * sc + bi, 0.f);
            }
        }
    } else {
        float* ct = smem;                                         // [9][33][NOUT]
        __syncthreads();                                          // every operand read of the K loop is done
#pragma unroll
        for (int i = 0; i < G::PER_WAVE; ++i) {
            const int q = qb + QS * i;
            if (q >= G::NBLK) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
                const int row = q < 9 ? q : m, col = q < 9 ? m + 1 : 0;
                const int cr = r0 + row, cc = c0 + col;
                // out-of-map conv positions hold 0 = the pool's -inf padding behind a ReLU (every window has its valid centre)
                const bool ok = (unsigned)cr < (unsigned)p.H && (unsigned)cc < (unsigned)p.W;
                if (q < 9 || m < 9) ct[(row * 33 + col) * NOUT + c] = ok ? fmaxf(acc[i][r] * sc + bi, 0.f) : 0.f;
            }
        }
        __syncthreads();
        // pooled pixel (py, px) of the tile, cout quad g: rows 2 py .. 2 py + 2, columns 2 px .. 2 px + 2 of the conv tile
        constexpr int QD = NOUT / 4;
        for (int u = tid; u < 4 * 16 * QD; u += 512) {
            const int g = u % QD, px = (u / QD) & 15, py = u / (QD * 16);
            const int gy = 4 * ty + py, gx = 16 * tx + px;
            if (gy >= p.PH || gx >= p.PW) continue;
            f32x4 mx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(ct + ((2 * py + dy) * 33 + 2 * px + dx) * NOUT + g * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], v[e]);
                }
            const size_t o = (((size_t)n * p.PH + gy) * p.PW + gx) * NOUT + g * 4;
            if (p.out_bf16) {
                uint2 w;
                w.x = __builtin_bit_cast(unsigned, sd_bf16x2{(__bf16)mx[0], (__bf16)mx[1]});
                w.y = __builtin_bit_cast(unsigned, sd_bf16x2{(__bf16)mx[2], (__bf16)mx[3]});
                *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p.out) + o) = w;
            } else {
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.out) + o) = mx;
            }
        }
    }
}

template <int NOUT, bool POOL>
static int stem_deep_bc_launch(StemDeepBCParams p, hipStream_t stream) {
    typedef StemDeepGeom<NOUT, POOL> G;
    static bool configured = false;                               // more than the default 64 KB of dynamic LDS
    const int bytes = G::LDS * (int)sizeof(float);
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_deep_bc_kernel<NOUT, POOL>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return -(int)e;
        configured = true;
    }
    const long long blocks = (long long)p.N * p.tilesY * p.tilesX;
    if (blocks >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((stem_deep_bc_kernel<NOUT, POOL>), dim3((unsigned)blocks), dim3(512), bytes, stream, p);
    CPR_LAUNCH_STATUS();
}

// in: the image (layout 0 NHWC4 / 1 planes) -> out (N, PH, PW, 64) fp32 (out_bf16 = 0) or bf16 (1); mid1, mid2: caller-allocated
// (N, OH, OW, 32) fp32 maps, OH = (H-1)/2+1, PH = (OH-1)/2+1.  w1 (32, 64), w2 (32, 288), w3 (64, 288): the fp32 implicit-GEMM
// packs of the three convs; s* / b*: the folded BatchNorms (required).
extern "C" int cpr_stem_deep_fwd(const float* in, const float* w1, const float* s1, const float* b1, const float* w2, const float* s2,
                                 const float* b2, const float* w3, const float* s3, const float* b3, float* mid1, float* mid2,
                                 void* out, int N, int H, int W, int layout, int out_bf16, hipStream_t stream) {
    CPR_CHECK_ARG(in && w1 && s1 && b1 && w2 && s2 && b2 && w3 && s3 && b3 && mid1 && mid2 && out);
    CPR_CHECK_ARG(N > 0 && H > 0 && W > 0 && (layout == 0 || layout == 1) && (out_bf16 == 0 || out_bf16 == 1));
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    StemDeepAParams a;
    a.in = in; a.wgt = w1; a.scale = s1; a.bias = b1; a.out = mid1;
    a.N = N; a.H = H; a.W = W; a.OH = OH; a.OW = OW; a.layout = layout; a.wstride = 64;
    a.tilesY = cdiv(OH, SDA_TR);
    a.tilesX = cdiv(OW, SDA_TC);
    const long long blocks = (long long)N * a.tilesY * a.tilesX;
    if (blocks >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(stem_deep_a_kernel, dim3((unsigned)blocks), dim3(512), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return -(int)e;
    StemDeepBCParams q;
    q.in = mid1; q.wgt = w2; q.scale = s2; q.bias = b2; q.out = mid2;
    q.N = N; q.H = OH; q.W = OW; q.PH = 0; q.PW = 0; q.out_bf16 = 0;
    q.tilesY = cdiv(OH, 16);
    q.tilesX = cdiv(OW, 32);
    int rc = stem_deep_bc_launch<32, false>(q, stream);
    if (rc != CPR_OK) return rc;
    q.in = mid2; q.wgt = w3; q.scale = s3; q.bias = b3; q.out = out;
    q.PH = (OH - 1) / 2 + 1;
    q.PW = (OW - 1) / 2 + 1;
    q.out_bf16 = out_bf16;
    q.tilesY = cdiv(q.PH, 4);
    q.tilesX = cdiv(q.PW, 16);
    return stem_deep_bc_launch<64, true>(q, stream);
}

// Launch A alone: the RegNet stem (T/mmdet/models/backbones/regnet.py:237-249: conv 3x3 / 2 / pad 1, 3 -> 32, + BatchNorm + ReLU, no
// max-pool).  in: layout 0 (N, H, W, 4) / 1 (N, 3, H, W) planes; w (32, 64): the fp32 implicit-GEMM pack; out (N, OH, OW, 32) fp32.
extern "C" int cpr_stem3x3s2_fwd(const float* in, const float* w, const float* scale, const float* bias, float* out, int N, int H, int W,
                                 int layout, hipStream_t stream) {
    CPR_CHECK_ARG(in && w && scale && bias && out && N > 0 && H > 0 && W > 0 && (layout == 0 || layout == 1));
    StemDeepAParams a;
    a.in = in; a.wgt = w; a.scale = scale; a.bias = bias; a.out = out;
    a.N = N; a.H = H; a.W = W; a.OH = (H - 1) / 2 + 1; a.OW = (W - 1) / 2 + 1; a.layout = layout; a.wstride = 64;
    a.tilesY = cdiv(a.OH, SDA_TR);
    a.tilesX = cdiv(a.OW, SDA_TC);
    const long long blocks = (long long)N * a.tilesY * a.tilesX;
    if (blocks >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(stem_deep_a_kernel, dim3((unsigned)blocks), dim3(512), 0, stream, a);
    CPR_LAUNCH_STATUS();
}

// ------------------------------------------------------------------------------------------------- average pool (avg_down shortcut)
// nn.AvgPool2d(s, s, ceil_mode=True, count_include_pad=False) on NHWC maps: OH = ceil(H / s); a last window of an odd map holds fewer
// rows / columns and divides by the number of in-map elements.  16 bytes per lane (4 fp32 / 8 bf16 channels), fp32 accumulation row
// by row, column by column; the quotient is rounded once (and once more to bf16).
template <typename T> struct AvgVec;
template <> struct AvgVec<float> {
    static constexpr int E = 4;
    struct V { float v[4]; };
    static __device__ __forceinline__ V ld(const float* p) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        return V{{t[0], t[1], t[2], t[3]}};
    }
    static __device__ __forceinline__ void st(float* p, const V& a) {
        *reinterpret_cast<f32x4*>(p) = f32x4{a.v[0], a.v[1], a.v[2], a.v[3]};
    }
};
template <> struct AvgVec<unsigned short> {
    static constexpr int E = 8;
    struct V { float v[8]; };
    static __device__ __forceinline__ V ld(const unsigned short* p) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {t.x, t.y, t.z, t.w};
        V a;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a.v[2 * i] = __uint_as_float(w[i] << 16);
            a.v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
        return a;
    }
    static __device__ __forceinline__ void st(unsigned short* p, const V& a) {
        uint4 t;
        t.x = __builtin_bit_cast(unsigned, sd_bf16x2{(__bf16)a.v[0], (__bf16)a.v[1]});
        t.y = __builtin_bit_cast(unsigned, sd_bf16x2{(__bf16)a.v[2], (__bf16)a.v[3]});
        t.z = __builtin_bit_cast(unsigned, sd_bf16x2{(__bf16)a.v[4], (__bf16)a.v[5]});
        t.w = __builtin_bit_cast(unsigned, sd_bf16x2{(__bf16)a.v[6], (__bf16)a.v[7]});
        *reinterpret_cast<uint4*>(p) = t;
    }
};

template <typename T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const T* __restrict__ in, T* __restrict__ out, int N, int H, int W, int CV,
                                                          int OH, int OW, int s) {
    typedef AvgVec<T> A;
    const long long total = (long long)N * OH * OW * CV;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % CV);
        long long r = idx / CV;
        const int ow = (int)(r % OW);
        r /= OW;
        const int oh = (int)(r % OH);
        const int n = (int)(r / OH);
        const int h1 = min(H, (oh + 1) * s), w1 = min(W, (ow + 1) * s);
        typename A::V acc;
#pragma unroll
        for (int e = 0; e < A::E; ++e) acc.v[e] = 0.f;
        for (int h = oh * s; h < h1; ++h)
            for (int w = ow * s; w < w1; ++w) {
                const typename A::V v = A::ld(in + ((((size_t)n * H + h) * W + w) * CV + c) * A::E);
#pragma unroll
                for (int e = 0; e < A::E; ++e) acc.v[e] = __fadd_rn(acc.v[e], v.v[e]);
            }
        const float cnt = (float)((h1 - oh * s) * (w1 - ow * s));
#pragma unroll
        for (int e = 0; e < A::E; ++e) acc.v[e] = __fdiv_rn(acc.v[e], cnt);
        A::st(out + idx * A::E, acc);
    }
}

// gather form of the backward: dx[h, w] = g[h / s, w / s] / count (+ add[h, w]); no atomics, every element written once
template <typename T, bool ADD>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const T* __restrict__ g, const T* __restrict__ add, T* __restrict__ dx, int N,
                                                          int H, int W, int CV, int OH, int OW, int s) {
    typedef AvgVec<T> A;
    const long long total = (long long)N * H * W * CV;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % CV);
        long long r = idx / CV;
        const int w = (int)(r % W);
        r /= W;
        const int h = (int)(r % H);
        const int n = (int)(r / H);
        const int oh = h / s, ow = w / s;
        const float cnt = (float)((min(H, (oh + 1) * s) - oh * s) * (min(W, (ow + 1) * s) - ow * s));
        typename A::V v = A::ld(g + ((((size_t)n * OH + oh) * OW + ow) * CV + c) * A::E);
#pragma unroll
        for (int e = 0; e < A::E; ++e) v.v[e] = __fdiv_rn(v.v[e], cnt);
        if constexpr (ADD) {
            const typename A::V a = A::ld(add + idx * A::E);
#pragma unroll
            for (int e = 0; e < A::E; ++e) v.v[e] = __fadd_rn(v.v[e], a.v[e]);
        }
        A::st(dx + idx * A::E, v);
    }
}

static int avgpool_grid(long long total) {
    const long long blocks = cdivll(total, 256);
    return (int)(blocks < 65536 ? (blocks > 0 ? blocks : 1) : 65536);
}

// in (N,H,W,C) -> out (N,ceil(H/s),ceil(W/s),C); bf16 = 0: fp32 maps (C % 4 == 0), 1: bf16 maps (C % 8 == 0); s >= 2
extern "C" int cpr_avgpool_fwd(const void* in, void* out, int N, int H, int W, int C, int s, int bf16, hipStream_t stream) {
    CPR_CHECK_ARG(in && out && N > 0 && H > 0 && W > 0 && C > 0 && s >= 2 && (bf16 == 0 || bf16 == 1) && C % (bf16 ? 8 : 4) == 0);
    const int OH = cdiv(H, s), OW = cdiv(W, s), CV = C / (bf16 ? 8 : 4);
    const int grid = avgpool_grid((long long)N * OH * OW * CV);
    if (bf16)
        hipLaunchKernelGGL(avgpool_fwd_kernel<unsigned short>, dim3(grid), dim3(256), 0, stream, (const unsigned short*)in,
                           (unsigned short*)out, N, H, W, CV, OH, OW, s);
    else
        hipLaunchKernelGGL(avgpool_fwd_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)in, (float*)out, N, H, W, CV, OH,
                           OW, s);
    CPR_LAUNCH_STATUS();
}
// g (N,ceil(H/s),ceil(W/s),C) -> dx (N,H,W,C) = g[h/s, w/s] / count + add (optional, the shape and type of dx; may be dx itself)
extern "C" int cpr_avgpool_bwd(const void* g, const void* add, void* dx, int N, int H, int W, int C, int s, int bf16,
                               hipStream_t stream) {
    CPR_CHECK_ARG(g && dx && N > 0 && H > 0 && W > 0 && C > 0 && s >= 2 && (bf16 == 0 || bf16 == 1) && C % (bf16 ? 8 : 4) == 0);
    const int OH = cdiv(H, s), OW = cdiv(W, s), CV = C / (bf16 ? 8 : 4);
    const int grid = avgpool_grid((long long)N * H * W * CV);
#define CPR_AVG_BWD(T, ADD)                                                                                                   \
    hipLaunchKernelGGL((avgpool_bwd_kernel<T, ADD>), dim3(grid), dim3(256), 0, stream, (const T*)g, (const T*)add, (T*)dx, N, H, W, CV, \
                       OH, OW, s)
    if (bf16) {
        if (add) CPR_AVG_BWD(unsigned short, true);
        else CPR_AVG_BWD(unsigned short, false);
    } else {
        if (add) CPR_AVG_BWD(float, true);
        else CPR_AVG_BWD(float, false);
    }
#undef CPR_AVG_BWD
    CPR_LAUNCH_STATUS();
}
