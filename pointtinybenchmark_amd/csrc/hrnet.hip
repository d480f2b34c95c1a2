// HRNet branch exchange (T/mmdet/models/backbones/hrnet.py:182-199, HRModule.forward): output branch i of a module is
//     x_fuse[i] = ReLU(sum_j f_ij(x_j)),   f_ii = identity,
//                                          f_ij (j > i) = nearest-upsample by 2^(j-i) of BN(conv1x1(x_j)),
//                                          f_ij (j < i) = a chain of i - j stride-2 3x3 conv + BN (ReLU between them).
// The convs run on the dense conv kernels at their OWN resolution with the folded BN in the epilogue; the upsampled maps never exist.
// This file holds the two streaming kernels over NHWC fp32 maps that remain:
//   cpr_hrnet_fuse       out = ReLU(t_0 + t_1 + ..), up to 4 terms from a host table; term (p, k): a map at (H >> k, W >> k) read at
//                        [y >> k, x >> k] -- torch's nearest rule for the integer scale factor 2^k (k = 0: a map at the output's size).
//                        The fp32 sum runs left to right in table order and there is no multiply: the result is a pure function of the
//                        operand bits and the order.  ReLU(v) = v <= 0 ? +0.0 : v (a NaN stays a NaN, as in torch.relu).
//   cpr_hrnet_fuse_bwd   g = y <= 0 ? +0.0 : dy at full resolution (torch's threshold_backward: a NaN in y lets dy through), the pooled
//                        maps pool_k = the sum of g over 2^k x 2^k blocks for k = 1..K (the adjoint of the nearest upsample: a sum, not an average), and per-workgroup column sums of g.
// Summation order of the adjoint (no atomics anywhere):
//   pool_1[y, x] = ((g[2y, 2x] + g[2y, 2x+1]) + g[2y+1, 2x]) + g[2y+1, 2x+1]       the 2x2 block in row-major order, left to right
//   pool_k[y, x] = the same expression over pool_{k-1}, k = 2, 3
//   column sums: a lane adds its cells' top-level values (pool_K, or g itself for K = 0) in ascending cell order (cells of an image are
//   numbered row-major over the (H >> K, W >> K) grid; lane pl of a block takes cells p0 + pl, p0 + pl + PL, ..), then the block adds its
//   lanes in ascending pl.  Partials: [blocks][C][2], element 0 = the sum, element 1 = 0 -- what cpr_part_colsum reduces.
// Every output element comes from its own image alone and every block belongs to one image: bit-repeatable, and an image's maps and
// pools do not depend on the batch it sits in.
#include "common.h"

#define HRNET_MAX_TERMS 4
#define HRNET_MAX_K 3

struct HrnTerms {
    const float* p[HRNET_MAX_TERMS];
    int k[HRNET_MAX_TERMS];
};

struct HrnTerm {        // include/cpr_hip.h: cpr_hrnet_term
    const void* p;
    int k;
};

struct HrnPools {
    float* p[HRNET_MAX_K];
};

// ------------------------------------------------------------------------------------------------ forward
// one lane: one (pixel, channel quad) of out; grid (cdiv(W * CV, 256), H, N).  T, the term count, is a template argument: the loop
// unrolls and the T loads of a lane are all in flight before the first add
template <int T>
__global__ __launch_bounds__(256) void hrnet_fuse_kernel(const HrnTerms t, float* __restrict__ out, int H, int W, int CV) {
    const int lane = blockIdx.x * 256 + threadIdx.x;
    if (lane >= W * CV) return;
    const int x = lane / CV, cg = lane - x * CV, y = blockIdx.y, n = blockIdx.z;
    f32x4 v[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int k = t.k[i], Hk = H >> k, Wk = W >> k;
        v[i] = reinterpret_cast<const f32x4*>(t.p[i])[(((size_t)n * Hk + (y >> k)) * Wk + (x >> k)) * CV + cg];
    }
    f32x4 acc = v[0];
#pragma unroll
    for (int i = 1; i < T; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], v[i][e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = acc[e] <= 0.f ? 0.f : acc[e];      // (a NaN stays a NaN, as in torch.relu)
    reinterpret_cast<f32x4*>(out)[(((size_t)n * H + y) * W + x) * CV + cg] = acc;
}

// ------------------------------------------------------------------------------------------------ backward
// full-resolution pixels one lane walks (K <= 2: 16 >> 2K cells of 4^K pixels; K = 3: one cell of 64)
__host__ __device__ static inline int hrnet_cells_per_lane(int K) { return K >= 2 ? 1 : (K == 1 ? 4 : 16); }

__device__ __forceinline__ f32x4 add4(f32x4 a, f32x4 b) {
    return f32x4{__fadd_rn(a[0], b[0]), __fadd_rn(a[1], b[1]), __fadd_rn(a[2], b[2]), __fadd_rn(a[3], b[3])};
}

// the masked gradient of one pixel, stored to g
__device__ __forceinline__ f32x4 hrnet_mask_px(const f32x4* __restrict__ dy, const f32x4* __restrict__ y, f32x4* __restrict__ g, size_t o) {
    const f32x4 d = dy[o], m = y[o];
    const f32x4 r = {m[0] <= 0.f ? 0.f : d[0], m[1] <= 0.f ? 0.f : d[1], m[2] <= 0.f ? 0.f : d[2], m[3] <= 0.f ? 0.f : d[3]};
    g[o] = r;
    return r;
}

// level-LV cell (cy, cx) of image n: writes g (LV = 0) or pool_LV and everything below it, returns the cell's value
template <int LV>
__device__ __forceinline__ f32x4 hrnet_cell(const f32x4* __restrict__ dy, const f32x4* __restrict__ y, f32x4* __restrict__ g,
                                            const HrnPools& pools, int n, int H, int W, int CV, int cq, int cy, int cx) {
    if constexpr (LV == 0) {
        return hrnet_mask_px(dy, y, g, (((size_t)n * H + cy) * W + cx) * CV + cq);
    } else {
        const f32x4 a = hrnet_cell<LV - 1>(dy, y, g, pools, n, H, W, CV, cq, 2 * cy, 2 * cx);
        const f32x4 b = hrnet_cell<LV - 1>(dy, y, g, pools, n, H, W, CV, cq, 2 * cy, 2 * cx + 1);
        const f32x4 c = hrnet_cell<LV - 1>(dy, y, g, pools, n, H, W, CV, cq, 2 * cy + 1, 2 * cx);
        const f32x4 d = hrnet_cell<LV - 1>(dy, y, g, pools, n, H, W, CV, cq, 2 * cy + 1, 2 * cx + 1);
        const f32x4 s = add4(add4(add4(a, b), c), d);
        reinterpret_cast<f32x4*>(pools.p[LV - 1])[(((size_t)n * (H >> LV) + cy) * (W >> LV) + cx) * CV + cq] = s;
        return s;
    }
}

// grid (cdiv(cells, PL * cells_per_lane), cdiv(CV, 256), N), cells = (H >> K)(W >> K); a block: cw = min(CV - 256 blockIdx.y, 256)
// channel quads x PL = 256 / cw cell lanes
template <int K>
__global__ __launch_bounds__(256) void hrnet_fuse_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ g,
                                                             const HrnPools pools, float* __restrict__ part, int H, int W, int CV) {
    __shared__ f32x4 red[256];
    const int HK = H >> K, WK = W >> K, cells = HK * WK;
    const int c0 = blockIdx.y * 256, cw = CV - c0 < 256 ? CV - c0 : 256, PL = 256 / cw;
    const int pl = threadIdx.x / cw, q = threadIdx.x - pl * cw, n = blockIdx.z;
    const int per_block = PL * hrnet_cells_per_lane(K);
    const int p0 = blockIdx.x * per_block, p1 = p0 + per_block < cells ? p0 + per_block : cells;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    if (pl < PL) {
        for (int p = p0 + pl; p < p1; p += PL) {
            const int cy = p / WK, cx = p - cy * WK;
            const f32x4 s = hrnet_cell<K>(reinterpret_cast<const f32x4*>(dy), reinterpret_cast<const f32x4*>(y),
                                          reinterpret_cast<f32x4*>(g), pools, n, H, W, CV, c0 + q, cy, cx);
            cs = add4(cs, s);
        }
    }
    red[threadIdx.x] = cs;
    __syncthreads();
    if (threadIdx.x < cw) {
        f32x4 s = red[threadIdx.x];
        for (int i = 1; i < PL; ++i) s = add4(s, red[i * cw + threadIdx.x]);
        const size_t tile = (size_t)n * gridDim.x + blockIdx.x;
        f32x4* dst = reinterpret_cast<f32x4*>(part + (tile * CV * 4 + (size_t)(c0 + q) * 4) * 2);
        dst[0] = f32x4{s[0], 0.f, s[1], 0.f};
        dst[1] = f32x4{s[2], 0.f, s[3], 0.f};
    }
}

// ------------------------------------------------------------------------------------------------ launchers
static int hrnet_map_args(int N, int H, int W, int C, int K) {
    CPR_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && H <= 65535 && W > 0 && C > 0 && C % 4 == 0 && K >= 0 && K <= HRNET_MAX_K);
    CPR_CHECK_ARG((long long)N * H * W * C < (1ll << 31));
    CPR_CHECK_ARG(H % (1 << K) == 0 && W % (1 << K) == 0);
    return CPR_OK;
}

extern "C" int cpr_hrnet_fuse(const HrnTerm* terms, int T, float* out, int N, int H, int W, int C, hipStream_t stream) {
    CPR_CHECK_ARG(terms && out && T >= 1 && T <= HRNET_MAX_TERMS);
    HrnTerms t{};
    int kmax = 0;
    for (int i = 0; i < T; ++i) {
        CPR_CHECK_ARG(terms[i].p && terms[i].k >= 0 && terms[i].k <= HRNET_MAX_K);
        t.p[i] = reinterpret_cast<const float*>(terms[i].p), t.k[i] = terms[i].k;
        kmax = terms[i].k > kmax ? terms[i].k : kmax;
    }
    const int st = hrnet_map_args(N, H, W, C, kmax);
    if (st != CPR_OK) return st;
    const int CV = C / 4;
    const dim3 grid(cdiv(W * CV, 256), H, N);
    if (T == 1) hipLaunchKernelGGL(hrnet_fuse_kernel<1>, grid, dim3(256), 0, stream, t, out, H, W, CV);
    else if (T == 2) hipLaunchKernelGGL(hrnet_fuse_kernel<2>, grid, dim3(256), 0, stream, t, out, H, W, CV);
    else if (T == 3) hipLaunchKernelGGL(hrnet_fuse_kernel<3>, grid, dim3(256), 0, stream, t, out, H, W, CV);
    else hipLaunchKernelGGL(hrnet_fuse_kernel<4>, grid, dim3(256), 0, stream, t, out, H, W, CV);
    CPR_LAUNCH_STATUS();
}

// blocks along x of one image
static int hrnet_bwd_grid_x(int H, int W, int C, int K) {
    const int CV = C / 4, cw = CV < 256 ? CV : 256, PL = 256 / cw;
    return cdiv((H >> K) * (W >> K), PL * hrnet_cells_per_lane(K));
}

// column-sum partials cpr_hrnet_fuse_bwd writes for an (N, H, W, C) map and K pooled levels
extern "C" int cpr_hrnet_fuse_bwd_blocks(int N, int H, int W, int C, int K) {
    const int st = hrnet_map_args(N, H, W, C, K);
    if (st != CPR_OK) return st;
    const long long b = (long long)N * hrnet_bwd_grid_x(H, W, C, K);
    return b < (1ll << 31) ? (int)b : CPR_ERR_UNSUPPORTED;
}

// pools: K host pointers, pools[k - 1] = pool_k (N, H >> k, W >> k, C); part: [cpr_hrnet_fuse_bwd_blocks(N, H, W, C, K)][C][2]
extern "C" int cpr_hrnet_fuse_bwd(const float* dy, const float* y, float* g, float* const* pools, int K, float* part, int N, int H, int W,
                                  int C, hipStream_t stream) {
    CPR_CHECK_ARG(dy && y && g && part && (K == 0 || pools));
    const int st = hrnet_map_args(N, H, W, C, K);
    if (st != CPR_OK) return st;
    HrnPools ps{};
    for (int k = 0; k < K; ++k) {
        CPR_CHECK_ARG(pools[k]);
        ps.p[k] = pools[k];
    }
    const int CV = C / 4;
    const dim3 grid(hrnet_bwd_grid_x(H, W, C, K), cdiv(CV, 256), N);
    if (K == 0) hipLaunchKernelGGL(hrnet_fuse_bwd_kernel<0>, grid, dim3(256), 0, stream, dy, y, g, ps, part, H, W, CV);
    else if (K == 1) hipLaunchKernelGGL(hrnet_fuse_bwd_kernel<1>, grid, dim3(256), 0, stream, dy, y, g, ps, part, H, W, CV);
    else if (K == 2) hipLaunchKernelGGL(hrnet_fuse_bwd_kernel<2>, grid, dim3(256), 0, stream, dy, y, g, ps, part, H, W, CV);
    else hipLaunchKernelGGL(hrnet_fuse_bwd_kernel<3>, grid, dim3(256), 0, stream, dy, y, g, ps, part, H, W, CV);
    CPR_LAUNCH_STATUS();
}
