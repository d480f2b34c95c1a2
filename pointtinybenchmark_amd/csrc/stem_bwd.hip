// Backward of the standard ResNet stem (T/mmdet/models/backbones/resnet.py:630-637): conv 7x7 / stride 2 / pad 3, 3 -> 64,
// BatchNorm, ReLU, max-pool 3x3 / stride 2 / pad 1.  Two kernels:
//
//   stem_pool_bwd_kernel   the pooled gradient dp (N, PH, PW, 64) and the byte map the recording forward wrote next to the pooled
//                          map (window position 0..8 of each maximum, first of ties; 255 where the ReLU killed it) -> the gradient at
//                          the BatchNorm output dy (N, OH, OW, 64), i.e. through max-pool and ReLU.  Gather form: a conv-output pixel
//                          sums the (at most 2 x 2) windows that chose it, pooled row ascending, then pooled column ascending -- no
//                          atomics.  Also leaves per-block column sums of dy ([blocks][64][2], element 0 = sum: the TilePartials
//                          cpr_bn_fold_bwd_part reads).  Streaming: dp + byte map read once, dy written once.
//
//   stem_wgrad_kernel      Gw[co][kh][kw][ci] = sum_m dy[m][co] * img[n, ci, 2 oy + kh - 3, 2 ox + kw - 3], exact fp32 on the matrix
//                          pipe (v_mfma_f32_32x32x2_f32), reading the network input in either layout the forward accepts.  The GEMM is
//                          (64 couts) x (K = 7 kernel rows x 22) reduced over PIXELS.  As in the forward (csrc/stem_f32.hip) the input
//                          patch sits in LDS as 3-channel pixels, so the 21 floats of a kernel row are contiguous for every output pixel
//                          and slot 21 (one pixel further) keeps a k index from straddling two rows; slot 21 is computed and dropped.
//                          A workgroup walks conv-output tiles of 16 x 32 pixels: s, s + S, s + 2 S, ... with S = min(tiles, 512), a
//                          function of the shape only.  Wave w owns cout half w & 1 and tile rows (w >> 1) + 4 i; per step of 2 pixels
//                          it reads one dword of dy (A operand: the 32 couts of its half), five LDS dwords of the patch (B operands: the
//                          5 x 32 k columns) and issues 5 MFMAs.  The four row groups of a cout half are summed through LDS in a fixed
//                          order, the workgroup's partial goes to ws[s][64][154], and stem_wgrad_reduce_kernel adds the S partials in
//                          order into the (64, 3, 7, 7) gradient.  Deterministic run to run.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------- max-pool + ReLU
constexpr int SPB_PIX = 1024;                 // conv-output pixels per block of stem_pool_bwd (one column-sum partial each)

__global__ __launch_bounds__(256) void stem_pool_bwd_kernel(const float* __restrict__ dp, const unsigned char* __restrict__ arg,
                                                            float* __restrict__ dy, float* __restrict__ part, long long M, int OH,
                                                            int OW, int PH, int PW) {
    __shared__ f32x4 red[16][16];
    const int q = threadIdx.x & 15, pl = threadIdx.x >> 4;      // channel quad, pixel lane
    const long long m0 = (long long)blockIdx.x * SPB_PIX;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    // (n, oy, ox) of the lane's first pixel by division once, then stepped by 16 pixels: no 64-bit division (a software sequence on
    // this ISA) per pixel
    long long n;
    int oy, ox;
    {
        const long long m = m0 + pl, r = m / OW;
        ox = (int)(m - r * OW);
        n = r / OH;
        oy = (int)(r - n * OH);
    }
#pragma unroll 2
    for (int it = 0; it < SPB_PIX / 16; ++it) {
        const long long m = m0 + it * 16 + pl;
        if (m >= M) break;
        if (it > 0) {
            ox += 16;
            while (ox >= OW) {
                ox -= OW;
                if (++oy == OH) { oy = 0; ++n; }
            }
        }
        // windows that contain (oy, ox): pooled row py covers conv rows 2 py - 1 .. 2 py + 1, so py0 = oy >> 1 (row offset 1 + (oy & 1))
        // and, for odd oy, py0 + 1 (offset 0).  All four candidate windows are loaded without branches (a missing one at a clamped
        // address with a position that never matches), so a lane's loads are all in flight at once; they add in the fixed order
        // (py0, px0), (py0, px1), (py1, px0), (py1, px1)
        const int py0 = oy >> 1, px0 = ox >> 1;
        const bool vy = (oy & 1) && py0 + 1 < PH, vx = (ox & 1) && px0 + 1 < PW;
        const int py1 = vy ? py0 + 1 : py0, px1 = vx ? px0 + 1 : px0;
        const unsigned wy0 = 1 + (oy & 1), wx0 = 1 + (ox & 1), NONE = 0x100u;
        const unsigned pos[4] = {wy0 * 3 + wx0, vx ? wy0 * 3 : NONE, vy ? wx0 : NONE, vx && vy ? 0u : NONE};
        const size_t r0 = ((size_t)n * PH + py0) * PW, r1 = ((size_t)n * PH + py1) * PW;
        const size_t o[4] = {(r0 + px0) * 64 + q * 4, (r0 + px1) * 64 + q * 4, (r1 + px0) * 64 + q * 4, (r1 + px1) * 64 + q * 4};
        unsigned k[4];
        f32x4 v[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            k[w] = *reinterpret_cast<const unsigned*>(arg + o[w]);
            v[w] = *reinterpret_cast<const f32x4*>(dp + o[w]);
        }
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (((k[w] >> (8 * e)) & 0xffu) == pos[w]) g[e] += v[w][e];
        *reinterpret_cast<f32x4*>(dy + (size_t)m * 64 + q * 4) = g;
        cs += g;
    }
    red[pl][q] = cs;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int c = threadIdx.x;
        float s = 0.f;
        for (int i = 0; i < 16; ++i) s += red[i][c >> 2][c & 3];
        part[((size_t)blockIdx.x * 64 + c) * 2] = s;
        part[((size_t)blockIdx.x * 64 + c) * 2 + 1] = 0.f;
    }
}

extern "C" int cpr_stem_pool_bwd_blocks(long long M) { return M > 0 ? (int)((M + SPB_PIX - 1) / SPB_PIX) : CPR_ERR_ARG; }

// dp (N, PH, PW, 64) fp32 + arg (N, PH, PW, 64) uint8 -> dy (N, OH, OW, 64) fp32 and part [cpr_stem_pool_bwd_blocks(N OH OW)][64][2]
extern "C" int cpr_stem_pool_bwd(const float* dp, const unsigned char* arg, float* dy, float* part, int N, int OH, int OW,
                                 hipStream_t stream) {
    CPR_CHECK_ARG(dp && arg && dy && part && N > 0 && OH > 0 && OW > 0);
    const int PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1;
    const long long M = (long long)N * OH * OW;
    const long long blocks = (M + SPB_PIX - 1) / SPB_PIX;
    if (blocks >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(stem_pool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dp, arg, dy, part, M, OH, OW, PH, PW);
    CPR_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------- weight gradient
constexpr int SW_TY = 16, SW_TX = 32;                             // conv-output tile
constexpr int SW_PH = 2 * SW_TY + 5, SW_PW = 2 * SW_TX + 6;       // patch: 37 rows x 70 pixels (69 + the slot-21 pixel)
constexpr int SW_PROW = SW_PW * 3;                                // 210 floats per patch row
constexpr int SW_PATCH_FLOATS = SW_PH * SW_PROW;                  // 7770
constexpr int SW_K = 154;                                         // 7 x 22
constexpr int SW_KP = 160;                                        // 5 MFMA column blocks
constexpr int SW_RED_FLOATS = 64 * SW_KP;                         // 10240: the cross-wave sum
constexpr int SW_LDS_FLOATS = SW_PATCH_FLOATS > SW_RED_FLOATS ? SW_PATCH_FLOATS : SW_RED_FLOATS;
constexpr int SW_MAX_SPLIT = 512;

struct StemWgradParams {
    const float* dy;       // (N, OH, OW, 64)
    const float* in;       // layout 0: (N, H, W, 4); layout 1: (N, 3, H, W)
    float* ws;             // [S][64][154]
    int N, H, W, OH, OW, tilesY, tilesX, tiles, S, layout;
};

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void stem_wgrad_kernel(StemWgradParams p) {
    __shared__ __attribute__((aligned(16))) float smem[SW_LDS_FLOATS];
    float* patch = smem;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int jb = wave & 1, grp = wave >> 1;
    int boff[5];                                                  // B operand: k column kb * 32 + l31 -> patch offset
#pragma unroll
    for (int kb = 0; kb < 5; ++kb) {
        const int k = kb * 32 + l31;
        boff[kb] = k < SW_K ? (k / 22) * SW_PROW + k % 22 : 0;
    }
    f32x16 acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const size_t plane = (size_t)p.H * p.W;

    for (int t = blockIdx.x; t < p.tiles; t += p.S) {
        int b = t;
        const int tx = b % p.tilesX;
        b /= p.tilesX;
        const int ty = b % p.tilesY;
        const int n = b / p.tilesY;
        const int oy0 = SW_TY * ty, ox0 = SW_TX * tx;
        const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
        const float* img = p.in + (size_t)n * plane * (p.layout ? 3 : 4);
        __syncthreads();                                          // the previous tile's patch reads are done
        for (int u = tid; u < SW_PH * SW_PW; u += 512) {
            const int py = u / SW_PW, px = u - py * SW_PW;
            const int iy = iy0 + py, ix = ix0 + px;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                const size_t o = (size_t)iy * p.W + ix;
                if (p.layout) { v[0] = img[o]; v[1] = img[plane + o]; v[2] = img[2 * plane + o]; }
                else v = *reinterpret_cast<const f32x4*>(img + o * 4);
            }
            float* d = patch + u * 3;
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
        }
        __syncthreads();
        const float* dyn = p.dy + (size_t)n * p.OH * p.OW * 64 + jb * 32 + l31;
        const int xlim = p.OW - ox0 - half;                       // pixel 2 s + half of a row is in the map when 2 s < xlim
#pragma unroll 1
        for (int ri = 0; ri < 2 * (SW_TY / 4); ++ri) {            // (a tile row in two halves of 16 pixels: 8 operand registers)
            const int row = grp + 4 * (ri >> 1), oy = oy0 + row, s0 = (ri & 1) * (SW_TX / 4);
            const float* drow = dyn + ((size_t)oy * p.OW + ox0 + 2 * s0 + half) * 64;
            float a[SW_TX / 4];                                   // A operand of step s: dy[pixel 2 s + half][cout of the half]
#pragma unroll
            for (int s = 0; s < SW_TX / 4; ++s) a[s] = oy < p.OH && 2 * (s0 + s) < xlim ? drow[s * 128] : 0.f;
            const float* prow = patch + (2 * row) * SW_PROW + 6 * half + 12 * s0;
#pragma unroll
            for (int s = 0; s < SW_TX / 4; ++s) {
                float bv[5];
#pragma unroll
                for (int kb = 0; kb < 5; ++kb) bv[kb] = prow[12 * s + boff[kb]];
#pragma unroll
                for (int kb = 0; kb < 5; ++kb) acc[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bv[kb], acc[kb], 0, 0, 0);
            }
        }
    }

    // D layout: column = lane & 31 (k), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (cout of the wave's half).  Row groups in order.
    float* red = smem;
    for (int g = 0; g < 4; ++g) {
        __syncthreads();
        if (grp == g) {
#pragma unroll
            for (int kb = 0; kb < 5; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    float* d = red + co * SW_KP + kb * 32 + l31;
                    *d = g == 0 ? acc[kb][r] : *d + acc[kb][r];
                }
        }
    }
    __syncthreads();
    float* dst = p.ws + (size_t)blockIdx.x * 64 * SW_K;
    for (int u = tid; u < 64 * SW_K; u += 512) {
        const int co = u / SW_K, k = u - co * SW_K;
        dst[u] = red[co * SW_KP + k];
    }
}

// the S partials in order -> gw (64, 3, 7, 7), torch's layout; slot 21 of every kernel row dropped
__global__ void stem_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, int S) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= 64 * SW_K) return;
    const int co = u / SW_K, k = u - co * SW_K, kh = k / 22, j = k - kh * 22;
    if (j == 21) return;
    const int kw = j / 3, ci = j - kw * 3;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += ws[(size_t)i * 64 * SW_K + u];
    gw[((co * 3 + ci) * 7 + kh) * 7 + kw] = s;
}

static void stem_wgrad_shape(int N, int H, int W, int* OH, int* OW, int* tilesY, int* tilesX, long long* tiles, int* S) {
    *OH = (H - 1) / 2 + 1;
    *OW = (W - 1) / 2 + 1;
    *tilesY = (*OH + SW_TY - 1) / SW_TY;
    *tilesX = (*OW + SW_TX - 1) / SW_TX;
    *tiles = (long long)N * *tilesY * *tilesX;
    *S = (int)(*tiles < SW_MAX_SPLIT ? *tiles : SW_MAX_SPLIT);
}

// workspace floats of cpr_stem_wgrad_f32 for an (N, 3, H, W) image
extern "C" int cpr_stem_wgrad_f32_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return CPR_ERR_ARG;
    int OH, OW, ty, tx, S;
    long long tiles;
    stem_wgrad_shape(N, H, W, &OH, &OW, &ty, &tx, &tiles, &S);
    return S * 64 * SW_K;
}

// dy (N, OH, OW, 64) fp32, in: layout 0 (N, H, W, 4) / layout 1 (N, 3, H, W) fp32 -> gw (64, 3, 7, 7) fp32 (written, not accumulated);
// ws: cpr_stem_wgrad_f32_workspace(N, H, W) floats.  OH = (H - 1) / 2 + 1.
extern "C" int cpr_stem_wgrad_f32(const float* dy, const float* in, float* gw, float* ws, int N, int H, int W, int layout,
                                  hipStream_t stream) {
    CPR_CHECK_ARG(dy && in && gw && ws && N > 0 && H > 0 && W > 0 && (layout == 0 || layout == 1));
    StemWgradParams p;
    long long tiles;
    stem_wgrad_shape(N, H, W, &p.OH, &p.OW, &p.tilesY, &p.tilesX, &tiles, &p.S);
    if (tiles >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    p.dy = dy; p.in = in; p.ws = ws;
    p.N = N; p.H = H; p.W = W; p.tiles = (int)tiles; p.layout = layout;
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3(p.S), dim3(512), 0, stream, p);
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((64 * SW_K + 255) / 256), dim3(256), 0, stream, ws, gw, p.S);
    CPR_LAUNCH_STATUS();
}
