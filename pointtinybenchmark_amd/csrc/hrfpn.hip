// HRFPN neck (T/mmdet/models/necks/hrfpn.py:76-99): every backbone level is brought to the finest resolution by bilinear interpolation,
// the levels are concatenated, a 1x1 conv reduces them, and average pools of the reduced map feed one 3x3 conv per output level.
// Interpolation and the 1x1 conv are linear and bilinear weights sum to one, so
//     reduction_conv(cat_i(up_i(x_i))) = bias + y_0 + sum_{i>=1} up_i(y_i),   y_i = W_i * x_i at level i's OWN resolution
// (W_i: the column slice of the reduction weight that belongs to level i).  The 1x1 convs run on the dense / streamed conv kernels; the
// concatenated map never exists.  This file holds what remains, four streaming kernels over NHWC maps:
//   cpr_hrfpn_fuse[_bf16]   out = bias + y_0 + sum_{i=1..L-1} bilinear_i(y_i), L <= 4, level i at (H0 >> i, W0 >> i) with H_i << i == H0
//   cpr_hrfpn_pool[_bf16]   level k = avg_pool2d(out, 2^k, 2^k) (floor mode: (H0 >> k, W0 >> k), trailing rows / columns dropped),
//                           k = 1..K-1 in one launch, every level from `out` itself, window in row-major order
//   cpr_hrfpn_pool_bwd      d_out = g_0 + sum_k g_k[y >> k, x >> k] / 4^k inside level k's floor region, and the per-block column sums of
//                           d_out ([blocks][C][2], element 0 = sum: the TilePartials cpr_part_colsum reads; the reduction conv's bias gradient)
//   cpr_hrfpn_fuse_bwd      the adjoint of the bilinear part: d_out -> dy_i, i >= 1 (dy_0 is d_out itself), gather form
// Index rule, torch's F.interpolate(scale_factor=S=2^i, mode='bilinear', align_corners=False):
//   src = max(0, (dst + 0.5) / S - 0.5), x0 = floor(src), x1 = min(x0 + 1, in - 1), lambda = src - x0
// In units of 1 / (2 S) src is the integer max(0, 2 dst + 1 - S): x0 is a shift, lambda = (low bits) / (2 S), an exact dyadic number.
// No atomics; every sum runs in a fixed order (forward: bias, level 0, 1, 2, 3, within a level (y0,x0), (y0,x1), (y1,x0), (y1,x1);
// adjoint: destination row ascending, within a row column ascending, the row sum formed first).  Each output element is computed from
// its own image alone: bit-repeatable and independent of the batch size.  bf16: fp32 arithmetic, one rounding at the store.
#include "common.h"

#define HRFPN_MAX_LEVELS 4      // inputs of the fuse
#define HRFPN_MAX_OUTS 5        // outputs: level 0 and four pooled levels

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

struct HrLevel {        // include/cpr_hip.h: cpr_hrfpn_level
    void* p;
    int H, W;
};

struct HrTable {
    int L;
    void* p[HRFPN_MAX_OUTS];
    int H[HRFPN_MAX_OUTS], W[HRFPN_MAX_OUTS];
    int row0[HRFPN_MAX_OUTS + 1];       // pool: first grid row of every level
};

template <bool BF16>
__device__ __forceinline__ void ldv(const void* p, size_t vec, float (&v)[BF16 ? 8 : 4]) {
    if constexpr (BF16) {
        const uint4 u = reinterpret_cast<const uint4*>(p)[vec];
        v[0] = __uint_as_float(u.x << 16), v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16), v[3] = __uint_as_float(u.y & 0xffff0000u);
        v[4] = __uint_as_float(u.z << 16), v[5] = __uint_as_float(u.z & 0xffff0000u);
        v[6] = __uint_as_float(u.w << 16), v[7] = __uint_as_float(u.w & 0xffff0000u);
    } else {
        const f32x4 t = reinterpret_cast<const f32x4*>(p)[vec];
        v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
    }
}

template <bool BF16>
__device__ __forceinline__ void stv(void* p, size_t vec, const float (&v)[BF16 ? 8 : 4]) {
    if constexpr (BF16) {
        uint4 o;
        o.x = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v[0], (__bf16)v[1]});
        o.y = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v[2], (__bf16)v[3]});
        o.z = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v[4], (__bf16)v[5]});
        o.w = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v[6], (__bf16)v[7]});
        reinterpret_cast<uint4*>(p)[vec] = o;
    } else {
        reinterpret_cast<f32x4*>(p)[vec] = f32x4{v[0], v[1], v[2], v[3]};
    }
}

// 2^-e, e >= 0 small
__device__ __forceinline__ float pow2_neg(int e) { return __int_as_float((127 - e) << 23); }

// the two taps of destination cell d of an axis upsampled by 2^sh from `in` cells
__device__ __forceinline__ void bilinear_tap(int d, int sh, int in, int& a, int& b, float& lam) {
    int t2 = 2 * d + 1 - (1 << sh);       // src in units of 1 / (2 S)
    t2 = t2 < 0 ? 0 : t2;
    a = t2 >> (sh + 1);
    lam = (float)(t2 & ((2 << sh) - 1)) * pow2_neg(sh + 1);
    b = a + 1 < in ? a + 1 : in - 1;
}

// ------------------------------------------------------------------------------------------------ forward: fuse
// one lane: one (pixel, channel vector) of out; grid (cdiv(W0 * CV, 256), H0, N).  L, the input count, is a template argument: the level
// loop unrolls and the 1 + 4 (L - 1) loads of a lane are all in flight before the first is used
template <bool BF16, int L>
__global__ __launch_bounds__(256) void hrfpn_fuse_kernel(const HrTable t, const float* __restrict__ bias, void* __restrict__ out, int CV) {
    constexpr int V = BF16 ? 8 : 4;
    const int W0 = t.W[0], H0 = t.H[0];
    const int lane = blockIdx.x * 256 + threadIdx.x;
    if (lane >= W0 * CV) return;
    const int x = lane / CV, cg = lane - x * CV, y = blockIdx.y, n = blockIdx.z;
    float acc[V], v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    if (bias) {
#pragma unroll
        for (int k = 0; k < V; k += 4) {
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + cg * V + k);
            acc[k] = b4[0], acc[k + 1] = b4[1], acc[k + 2] = b4[2], acc[k + 3] = b4[3];
        }
    }
    const size_t o = (((size_t)n * H0 + y) * W0 + x) * CV + cg;
    ldv<BF16>(t.p[0], o, v);
    float tap[L > 1 ? 4 * (L - 1) : 1][V], w[L > 1 ? 4 * (L - 1) : 1];
#pragma unroll
    for (int i = 1; i < L; ++i) {
        const int Hi = t.H[i], Wi = t.W[i];
        int ya, yb, xa, xb;
        float ly, lx;
        bilinear_tap(y, i, Hi, ya, yb, ly);
        bilinear_tap(x, i, Wi, xa, xb, lx);
        float* wi = w + 4 * (i - 1);
        wi[0] = (1.f - ly) * (1.f - lx), wi[1] = (1.f - ly) * lx, wi[2] = ly * (1.f - lx), wi[3] = ly * lx;   // exact dyadic
        const size_t ra = ((size_t)n * Hi + ya) * Wi, rb = ((size_t)n * Hi + yb) * Wi;
        ldv<BF16>(t.p[i], (ra + xa) * CV + cg, tap[4 * (i - 1)]);
        ldv<BF16>(t.p[i], (ra + xb) * CV + cg, tap[4 * (i - 1) + 1]);
        ldv<BF16>(t.p[i], (rb + xa) * CV + cg, tap[4 * (i - 1) + 2]);
        ldv<BF16>(t.p[i], (rb + xb) * CV + cg, tap[4 * (i - 1) + 3]);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = __fadd_rn(acc[k], v[k]);
#pragma unroll
    for (int j = 0; j < 4 * (L - 1); ++j)
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = __fmaf_rn(w[j], tap[j][k], acc[k]);
    stv<BF16>(out, o, acc);
}

// ------------------------------------------------------------------------------------------------ forward: pool
// one lane: one (pooled pixel, channel vector) of one level; grid (cdiv(W_1 * CV, 256), sum_k H_k, N): a grid row is one row of one level
template <bool BF16>
__global__ __launch_bounds__(256) void hrfpn_pool_kernel(const HrTable t, const void* __restrict__ out, int H0, int W0, int CV) {
    constexpr int V = BF16 ? 8 : 4;
    int k = 0;          // table slot: level k + 1
    while (k + 1 < t.L && (int)blockIdx.y >= t.row0[k + 1]) ++k;
    const int Wk = t.W[k], Hk = t.H[k], sh = k + 1, P = 1 << sh;
    const int lane = blockIdx.x * 256 + threadIdx.x;
    if (lane >= Wk * CV) return;
    const int x = lane / CV, cg = lane - x * CV, y = blockIdx.y - t.row0[k], n = blockIdx.z;
    float acc[V], v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    for (int yy = 0; yy < P; ++yy) {
        const size_t row = (((size_t)n * H0 + (y << sh) + yy) * W0 + (x << sh)) * CV + cg;
#pragma unroll 4
        for (int xx = 0; xx < P; ++xx) {
            ldv<BF16>(out, row + (size_t)xx * CV, v);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = __fadd_rn(acc[j], v[j]);
        }
    }
    const float s = pow2_neg(2 * sh);
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] *= s;
    stv<BF16>(t.p[k], (((size_t)n * Hk + y) * Wk + x) * CV + cg, acc);
}

// ------------------------------------------------------------------------------------------------ backward: pool
constexpr int HPB_PIX = 256;        // pixels of one image per block of hrfpn_pool_bwd (one column-sum partial each)

// grid (cdiv(H0 * W0, HPB_PIX), cdiv(CV, 256), N); a block: cw = min(CV - 256 blockIdx.y, 256) channel quads x 256 / cw pixel lanes.
// t: the gradients g_0 .. g_{K-1} of the neck's output-conv inputs (fp32), level k at (H0 >> k, W0 >> k)
__global__ __launch_bounds__(256) void hrfpn_pool_bwd_kernel(const HrTable t, float* __restrict__ d_out, float* __restrict__ part, int CV) {
    __shared__ f32x4 red[256];
    const int H0 = t.H[0], W0 = t.W[0], HW = H0 * W0;
    const int c0 = blockIdx.y * 256, cw = CV - c0 < 256 ? CV - c0 : 256, PL = 256 / cw;
    const int pl = threadIdx.x / cw, q = threadIdx.x - pl * cw, n = blockIdx.z;
    const int p0 = blockIdx.x * HPB_PIX, p1 = p0 + HPB_PIX < HW ? p0 + HPB_PIX : HW;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    if (pl < PL) {
        for (int p = p0 + pl; p < p1; p += PL) {
            const int y = p / W0, x = p - y * W0;
            f32x4 g = reinterpret_cast<const f32x4*>(t.p[0])[((size_t)n * HW + p) * CV + c0 + q];
            for (int k = 1; k < t.L; ++k) {
                const int yk = y >> k, xk = x >> k;
                if (yk < t.H[k] && xk < t.W[k]) {
                    const f32x4 gk = reinterpret_cast<const f32x4*>(t.p[k])[(((size_t)n * t.H[k] + yk) * t.W[k] + xk) * CV + c0 + q];
                    g += gk * pow2_neg(2 * k);
                }
            }
            reinterpret_cast<f32x4*>(d_out)[((size_t)n * HW + p) * CV + c0 + q] = g;
            cs += g;
        }
    }
    red[threadIdx.x] = cs;
    __syncthreads();
    if (threadIdx.x < cw) {
        f32x4 s = red[threadIdx.x];
        for (int i = 1; i < PL; ++i) s += red[i * cw + threadIdx.x];
        const size_t tile = (size_t)n * gridDim.x + blockIdx.x;
        f32x4* dst = reinterpret_cast<f32x4*>(part + (tile * CV * 4 + (size_t)(c0 + q) * 4) * 2);
        dst[0] = f32x4{s[0], 0.f, s[1], 0.f};
        dst[1] = f32x4{s[2], 0.f, s[3], 0.f};
    }
}

// ------------------------------------------------------------------------------------------------ backward: fuse
constexpr int HFB_TX = 16, HFB_TY = 8, HFB_CV = 16;     // source tile (columns x rows) and channel quads of one block

// dy (N, Hi, Wi, C) = the adjoint of bilinear upsampling by S = 2^LS applied to d_out (N, H0, W0, C), H0 = Hi << LS.
// A block owns HFB_TY x HFB_TX source pixels x 16 channel quads; lane = (source column lx, channel quad cv).  It walks the (HFB_TY + 1) S
// destination rows whose taps touch its source rows in ascending order.  Each row segment -- the (HFB_TX + 1) S destination columns that
// touch its source columns, zeros outside the map -- goes through LDS once; a lane forms the row's weighted sum over its 2 S columns
// (ascending) and adds it, times the row weight, to the one or two source rows the destination row touches.  Destination rows come in
// groups of S: group r holds y = S (sy0 + r) - S / 2 + j, whose taps are source rows sy0 + r - 1 (weight 1 - lambda) and sy0 + r
// (weight lambda), lambda = (2 j + 1) / (2 S); where a clamp folds both taps onto the first / last source row the weight is 1.
// d_out is read (1 + 1/HFB_TX)(1 + 1/HFB_TY) times per level.  grid (tiles_x * tiles_y, cdiv(CV, 16), N)
template <int LS>
__global__ __launch_bounds__(256) void hrfpn_fuse_bwd_kernel(const float* __restrict__ d_out, float* __restrict__ dy, int H0, int W0,
                                                             int Hi, int Wi, int CV, int tiles_x) {
    constexpr int S = 1 << LS, ROWPIX = (HFB_TX + 1) * S;
    __shared__ f32x4 row[ROWPIX][HFB_CV + 1];       // + 1 quad: consecutive pixels start 4 banks apart
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, n = blockIdx.z;
    const int sx0 = tx * HFB_TX, sy0 = ty * HFB_TY, cv0 = blockIdx.y * HFB_CV;
    const int lx = threadIdx.x >> 4, cv = threadIdx.x & 15;
    const int sx = sx0 + lx, xbase = S * sx0 - S / 2;
    const bool cok = cv0 + cv < CV;
    const float inv2S = pow2_neg(LS + 1);
    const f32x4* src = reinterpret_cast<const f32x4*>(d_out);
    f32x4 acc[HFB_TY + 2];
#pragma unroll
    for (int r = 0; r < HFB_TY + 2; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r <= HFB_TY; ++r) {
        const int syA = sy0 + r - 1, syB = sy0 + r;
        for (int j = 0; j < S; ++j) {
            const int y = S * syB - S / 2 + j;
            if (y < 0 || y >= H0) continue;        // the same for the whole block
            __syncthreads();
            for (int e = threadIdx.x; e < ROWPIX * HFB_CV; e += 256) {
                const int px = e >> 4, c = e & 15, x = xbase + px;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (x >= 0 && x < W0 && cv0 + c < CV) v = src[(((size_t)n * H0 + y) * W0 + x) * CV + cv0 + c];
                row[px][c] = v;
            }
            __syncthreads();
            f32x4 rs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < S; ++jj) {        // taps whose second source column is sx
                const float w = sx == 0 ? 1.f : (float)(2 * jj + 1) * inv2S;
                rs += row[S * lx + jj][cv] * w;
            }
#pragma unroll
            for (int jj = 0; jj < S; ++jj) {        // taps whose first source column is sx
                const float w = sx >= Wi - 1 ? 1.f : 1.f - (float)(2 * jj + 1) * inv2S;
                rs += row[S * lx + S + jj][cv] * w;
            }
            const float lam = (float)(2 * j + 1) * inv2S;
            const float wA = syB > Hi - 1 ? 1.f : 1.f - lam, wB = syA < 0 ? 1.f : lam;
            acc[r] += rs * wA;
            acc[r + 1] += rs * wB;
        }
    }
    if (cok && sx < Wi) {
#pragma unroll
        for (int r = 0; r < HFB_TY; ++r)
            if (sy0 + r < Hi) reinterpret_cast<f32x4*>(dy)[(((size_t)n * Hi + sy0 + r) * Wi + sx) * CV + cv0 + cv] = acc[r + 1];
    }
}

// ------------------------------------------------------------------------------------------------ launchers
// levels[0] at (H0, W0), levels[i] at exactly (H0 >> i, W0 >> i) with nothing dropped when `exact` (the fuse: the reference's cat fails
// otherwise), else the floor (the pools)
static int hr_table(const HrLevel* levels, int L, int max_levels, int N, int C, int V, bool exact, HrTable& t) {
    CPR_CHECK_ARG(levels && L >= 1 && L <= max_levels && N > 0 && N <= 65535 && C > 0 && C % V == 0);
    t.L = L;
    for (int i = 0; i < L; ++i) {
        const HrLevel& lv = levels[i];
        CPR_CHECK_ARG(lv.p && lv.H > 0 && lv.W > 0 && lv.H == levels[0].H >> i && lv.W == levels[0].W >> i);
        if (exact) CPR_CHECK_ARG(lv.H << i == levels[0].H && lv.W << i == levels[0].W);
        CPR_CHECK_ARG((long long)N * lv.H * lv.W * C < (1ll << 31));
        t.p[i] = lv.p, t.H[i] = lv.H, t.W[i] = lv.W;
    }
    CPR_CHECK_ARG(levels[0].H <= 65535);
    return CPR_OK;
}

template <bool BF16>
static int hrfpn_fuse_launch(const HrLevel* levels, int L, const float* bias, void* out, int N, int C, hipStream_t stream) {
    constexpr int V = BF16 ? 8 : 4;
    HrTable t{};
    CPR_CHECK_ARG(out);
    const int st = hr_table(levels, L, HRFPN_MAX_LEVELS, N, C, V, true, t);
    if (st != CPR_OK) return st;
    const int CV = C / V;
    const dim3 grid(cdiv(t.W[0] * CV, 256), t.H[0], N);
    if (L == 1) hipLaunchKernelGGL((hrfpn_fuse_kernel<BF16, 1>), grid, dim3(256), 0, stream, t, bias, out, CV);
    else if (L == 2) hipLaunchKernelGGL((hrfpn_fuse_kernel<BF16, 2>), grid, dim3(256), 0, stream, t, bias, out, CV);
    else if (L == 3) hipLaunchKernelGGL((hrfpn_fuse_kernel<BF16, 3>), grid, dim3(256), 0, stream, t, bias, out, CV);
    else hipLaunchKernelGGL((hrfpn_fuse_kernel<BF16, 4>), grid, dim3(256), 0, stream, t, bias, out, CV);
    CPR_LAUNCH_STATUS();
}

// levels: the pooled levels 1 .. K1 (p: the output), level k at (H0 >> k, W0 >> k), none empty
template <bool BF16>
static int hrfpn_pool_launch(const void* out, int H0, int W0, const HrLevel* levels, int K1, int N, int C, hipStream_t stream) {
    constexpr int V = BF16 ? 8 : 4;
    CPR_CHECK_ARG(out && levels && K1 >= 1 && K1 < HRFPN_MAX_OUTS && H0 > 0 && W0 > 0 && N > 0 && N <= 65535 && C > 0 && C % V == 0);
    CPR_CHECK_ARG((long long)N * H0 * W0 * C < (1ll << 31));
    HrTable t{};
    t.L = K1;
    int rows = 0;
    for (int k = 0; k < K1; ++k) {
        const HrLevel& lv = levels[k];
        CPR_CHECK_ARG(lv.p && lv.H > 0 && lv.W > 0 && lv.H == H0 >> (k + 1) && lv.W == W0 >> (k + 1));
        t.p[k] = lv.p, t.H[k] = lv.H, t.W[k] = lv.W, t.row0[k] = rows;
        rows += lv.H;
    }
    t.row0[K1] = rows;
    CPR_CHECK_ARG(rows <= 65535);
    const int CV = C / V;
    hipLaunchKernelGGL(hrfpn_pool_kernel<BF16>, dim3(cdiv(t.W[0] * CV, 256), rows, N), dim3(256), 0, stream, t, out, H0, W0, CV);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_hrfpn_fuse(const HrLevel* levels, int L, const float* bias, float* out, int N, int C, hipStream_t stream) {
    return hrfpn_fuse_launch<false>(levels, L, bias, out, N, C, stream);
}
extern "C" int cpr_hrfpn_fuse_bf16(const HrLevel* levels, int L, const float* bias, void* out, int N, int C, hipStream_t stream) {
    return hrfpn_fuse_launch<true>(levels, L, bias, out, N, C, stream);
}
extern "C" int cpr_hrfpn_pool(const float* out, int H0, int W0, const HrLevel* levels, int K1, int N, int C, hipStream_t stream) {
    return hrfpn_pool_launch<false>(out, H0, W0, levels, K1, N, C, stream);
}
extern "C" int cpr_hrfpn_pool_bf16(const void* out, int H0, int W0, const HrLevel* levels, int K1, int N, int C, hipStream_t stream) {
    return hrfpn_pool_launch<true>(out, H0, W0, levels, K1, N, C, stream);
}

// column-sum partials cpr_hrfpn_pool_bwd writes for an (N, H0, W0, .) map
extern "C" int cpr_hrfpn_pool_bwd_blocks(int N, int H0, int W0) {
    if (N <= 0 || H0 <= 0 || W0 <= 0) return CPR_ERR_ARG;
    const long long b = (long long)N * cdivll((long long)H0 * W0, HPB_PIX);
    return b < (1ll << 31) ? (int)b : CPR_ERR_UNSUPPORTED;
}
// gs: g_0 .. g_{K-1} (fp32), level k at (H0 >> k, W0 >> k); part: [cpr_hrfpn_pool_bwd_blocks(N, H0, W0)][C][2]
extern "C" int cpr_hrfpn_pool_bwd(const HrLevel* gs, int K, float* d_out, float* part, int N, int C, hipStream_t stream) {
    HrTable t{};
    CPR_CHECK_ARG(d_out && part);
    const int st = hr_table(gs, K, HRFPN_MAX_OUTS, N, C, 4, false, t);
    if (st != CPR_OK) return st;
    const int CV = C / 4;
    hipLaunchKernelGGL(hrfpn_pool_bwd_kernel, dim3(cdiv(t.H[0] * t.W[0], HPB_PIX), cdiv(CV, 256), N), dim3(256), 0, stream, t, d_out, part,
                       CV);
    CPR_LAUNCH_STATUS();
}
// dys: dy_1 .. dy_{L1} (fp32 outputs), level i at (H0 >> i, W0 >> i) with H_i << i == H0; one launch per level
extern "C" int cpr_hrfpn_fuse_bwd(const float* d_out, int H0, int W0, const HrLevel* dys, int L1, int N, int C, hipStream_t stream) {
    CPR_CHECK_ARG(d_out && dys && L1 >= 1 && L1 < HRFPN_MAX_LEVELS && H0 > 0 && W0 > 0 && N > 0 && N <= 65535 && C > 0 && C % 4 == 0);
    CPR_CHECK_ARG((long long)N * H0 * W0 * C < (1ll << 31));
    for (int i = 1; i <= L1; ++i) {
        const HrLevel& lv = dys[i - 1];
        CPR_CHECK_ARG(lv.p && lv.H > 0 && lv.W > 0 && lv.H << i == H0 && lv.W << i == W0);
    }
    const int CV = C / 4;
    for (int i = 1; i <= L1; ++i) {
        const HrLevel& lv = dys[i - 1];
        const int tiles_x = cdiv(lv.W, HFB_TX), tiles_y = cdiv(lv.H, HFB_TY);
        const dim3 grid(tiles_x * tiles_y, cdiv(CV, HFB_CV), N);
        float* dy = reinterpret_cast<float*>(lv.p);
        if (i == 1) hipLaunchKernelGGL(hrfpn_fuse_bwd_kernel<1>, grid, dim3(256), 0, stream, d_out, dy, H0, W0, lv.H, lv.W, CV, tiles_x);
        else if (i == 2) hipLaunchKernelGGL(hrfpn_fuse_bwd_kernel<2>, grid, dim3(256), 0, stream, d_out, dy, H0, W0, lv.H, lv.W, CV, tiles_x);
        else hipLaunchKernelGGL(hrfpn_fuse_bwd_kernel<3>, grid, dim3(256), 0, stream, d_out, dy, H0, W0, lv.H, lv.W, CV, tiles_x);
    }
    CPR_LAUNCH_STATUS();
}
