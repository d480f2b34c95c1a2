// Darknet-53 kernels (gfx950, fp32): the LeakyReLU streaming passes around the dense convs -- forward (with the ResBlock's shortcut
// sum), backward with the per-channel column sums the folded BatchNorm rule needs -- and the weight gradient of the 3 -> 32 / stride 1
// first conv (T/mmdet/models/backbones/darknet.py:121).
//
// The dense conv epilogues know ReLU, not a negative slope, and stay as they are: a Darknet layer runs the conv in its raw folded form
// (scale, bias) and one pass over the map applies the activation.  The passes are bound by HBM: a lane owns one 16-byte channel quad.
//
// This file is built with floating-point contraction off (build.py EXACT_SOURCES): leaky_fwd and the g of leaky_bwd_colsum restate
// torch's CPU rules rounding for rounding -- the product z * slope is rounded to fp32, then the sum with the shortcut is rounded; an FMA
// would keep the product exact.  Where an FMA is wanted (the weight gradient) the source says fmaf.
//
// No atomics: the reductions over pixels (column sums, weight gradient) go through per-workgroup partials in a caller-allocated
// workspace and a second kernel that adds them in ascending order, so results are bit-repeatable and a row's g does not depend on the
// batch.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ LeakyReLU forward
// F.leaky_relu(z, slope) (+ res): z > 0 ? z : z * slope -- NaN takes the product branch and stays NaN, -0.0 * slope = -0.0
__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.f ? z : z * slope; }

__global__ __launch_bounds__(256) void leaky_fwd_kernel(const float* z, const float* res, float* out, long long n4, float slope) {
    // (z and out may alias: no __restrict__; a lane reads its quad before it writes it)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = reinterpret_cast<const f32x4*>(z)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = leaky(v[e], slope);
    if (res) {
        const f32x4 r = reinterpret_cast<const f32x4*>(res)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] + r[e];
    }
    reinterpret_cast<f32x4*>(out)[i] = v;
}

// ------------------------------------------------------------------------------------------------ LeakyReLU backward + column sums
__device__ __forceinline__ f32x4 lk_zero() {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return z;
}

// (M, C) row-major: s = dy (+ add), g = y > 0 ? s : s * slope (torch's leaky_relu_backward: the slope at y == 0) and this workgroup's
// column sums part[bx][C].  Workgroup bx owns rows [bx * rows, (bx + 1) * rows); lane (pl, q) walks rows pl, pl + PP, .. of channel
// quad q; the PP lanes of a quad are added in ascending pl.
__global__ __launch_bounds__(256) void leaky_bwd_colsum_kernel(const float* __restrict__ dy, const float* __restrict__ add,
                                                              const float* __restrict__ y, float* __restrict__ g_out,
                                                              float* __restrict__ part, long long M, int C, int Q, int PP, int rows,
                                                              float slope) {
    __shared__ f32x4 red[256];
    const int q = threadIdx.x % Q, pl = threadIdx.x / Q;
    const int c = (blockIdx.y * Q + q) * 4;
    const long long r0 = (long long)blockIdx.x * rows, r1 = min(M, r0 + rows);
    f32x4 cs = lk_zero();
    if (pl < PP && c < C) {
#pragma unroll 2
        for (long long r = r0 + pl; r < r1; r += PP) {
            const size_t o = (size_t)r * C + c;
            f32x4 g = *reinterpret_cast<const f32x4*>(dy + o);
            if (add) g += *reinterpret_cast<const f32x4*>(add + o);
            const f32x4 m = *reinterpret_cast<const f32x4*>(y + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = m[e] > 0.f ? g[e] : g[e] * slope;
            if (g_out) *reinterpret_cast<f32x4*>(g_out + o) = g;
            cs += g;
        }
    }
    red[threadIdx.x] = cs;
    __syncthreads();
    if (threadIdx.x < Q && c < C) {
        f32x4 s = red[threadIdx.x];
        for (int r = 1; r < PP; ++r) s += red[r * Q + threadIdx.x];
        *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * C + c) = s;
    }
}

// out[col] = sum over p of part[p][col] in a fixed order: 64 interleaved chains per column (chain j adds rows j, j + 64, .. ascending),
// then those 64 in ascending order.  16 columns per workgroup, so a step of a chain's 16 lanes reads one 64-byte segment.  A map of
// 16 x 320^2 x 64 leaves 3200 partial rows for 4 workgroups: the chains are short (50 rows) and the loop is unrolled, so that the loads
// of several rows are in flight -- with 16 chains of 800 dependent steps this kernel took longer than the streaming pass in front of it.
#define LK_FIN_CHAINS 64
__global__ __launch_bounds__(16 * LK_FIN_CHAINS) void leaky_colsum_finalize_kernel(const float* __restrict__ part, long long P, int C,
                                                                                float* __restrict__ out) {
    __shared__ float red[LK_FIN_CHAINS][17];
    const int cl = threadIdx.x & 15, j = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + cl;
    float s = 0.f;
    if (col < C) {
#pragma unroll 8
        for (long long p = j; p < P; p += LK_FIN_CHAINS) s += part[(size_t)p * C + col];
    }
    red[j][cl] = s;
    __syncthreads();
    if (j == 0 && col < C) {
        float t = red[0][cl];
        for (int k = 1; k < LK_FIN_CHAINS; ++k) t += red[k][cl];
        out[col] = t;
    }
}

// rows per workgroup: 512, halved until the launch has 2048 workgroups (8 per CU) or 16 rows are left.  Tall blocks leave few partial
// rows for the second kernel.
static int leaky_rows_per_block(long long M) {
    int rows = 512;
    while (rows > 16 && cdivll(M, rows) < 2048) rows >>= 1;
    return rows;
}

// ------------------------------------------------------------------------------------------------ stem 3x3 / stride 1 weight gradient
// gw (32, 3, 3, 3) = sum over the pixels of dy (N, H, W, 32) x the image around them (layout 0: (N, H, W, 4) fp32, 4th channel ignored;
// layout 1: (N, 3, H, W) fp32 planes), zero outside the image.  The stride-1 sibling of csrc/stem3x3_bwd.hip: a workgroup of 288 threads
// owns one slice of the flattened pixels, thread (tap, cout) keeps the three input channels' sums.  That kernel's one serial FMA chain
// per thread is its stated weakness; here a thread walks TWO pixels per step into independent accumulators (even pixels of the slice
// into one set, odd into the other, the two added at the end), so two loads and two chains are in flight.  Slice partials go to
// ws[slice][tap][cin][cout]; the reduce kernel adds them in ascending slice order and scatters to the parameter layout.
constexpr int S1_THREADS = 288;       // 9 taps x 32 couts
constexpr int S1_OUT = 864;           // 32 x 3 x 3 x 3
constexpr int S1_MAX_SLICES = 2048;   // 8 workgroups per CU
constexpr int S1_MIN_PIX = 64;        // the fewest pixels a slice is worth

struct S1Plan { int S; long long P; };
inline S1Plan s1_plan(long long M) {
    S1Plan pl;
    long long s = cdivll(M, S1_MIN_PIX);
    if (s > S1_MAX_SLICES) s = S1_MAX_SLICES;
    pl.P = cdivll(M, s);
    pl.S = (int)cdivll(M, pl.P);
    return pl;
}

template <int LAYOUT>
__device__ __forceinline__ void s1_tap(const float* __restrict__ in, long long n, int ih, int iw, int H, int W, size_t plane, float d,
                                       float& a0, float& a1, float& a2) {
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
        const size_t o = (size_t)ih * W + iw;
        if (LAYOUT) {
            const float* img = in + (size_t)n * plane * 3 + o;
            v0 = img[0]; v1 = img[plane]; v2 = img[2 * plane];
        } else {
            const f32x4 v = *reinterpret_cast<const f32x4*>(in + ((size_t)n * plane + o) * 4);
            v0 = v[0]; v1 = v[1]; v2 = v[2];
        }
    }
    a0 = fmaf(d, v0, a0); a1 = fmaf(d, v1, a1); a2 = fmaf(d, v2, a2);
}

template <int LAYOUT>
__global__ __launch_bounds__(S1_THREADS) void stem3x3s1_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ in,
                                                                     float* __restrict__ ws, long long M, int H, int W, long long P) {
    const int co = threadIdx.x & 31, tap = threadIdx.x >> 5;
    const int kh = tap / 3, kw = tap - 3 * kh;
    const long long pbeg = (long long)blockIdx.x * P;
    const long long pend = pbeg + P < M ? pbeg + P : M;
    const size_t plane = (size_t)H * W;
    int w = (int)(pbeg % W);
    long long r = pbeg / W;
    int h = (int)(r % H);
    long long n = r / H;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
    long long p = pbeg;
#pragma unroll 2
    for (; p + 1 < pend; p += 2) {
        int w2 = w + 1, h2 = h;
        long long n2 = n;
        if (w2 == W) {
            w2 = 0;
            if (++h2 == H) { h2 = 0; ++n2; }
        }
        const float d = dy[(size_t)p * 32 + co], e = dy[(size_t)(p + 1) * 32 + co];
        s1_tap<LAYOUT>(in, n, h - 1 + kh, w - 1 + kw, H, W, plane, d, a0, a1, a2);
        s1_tap<LAYOUT>(in, n2, h2 - 1 + kh, w2 - 1 + kw, H, W, plane, e, b0, b1, b2);
        w = w2 + 1; h = h2; n = n2;
        if (w == W) {
            w = 0;
            if (++h == H) { h = 0; ++n; }
        }
    }
    if (p < pend) s1_tap<LAYOUT>(in, n, h - 1 + kh, w - 1 + kw, H, W, plane, dy[(size_t)p * 32 + co], a0, a1, a2);
    float* o = ws + (size_t)blockIdx.x * S1_OUT + tap * 96 + co;
    o[0] = a0 + b0; o[32] = a1 + b1; o[64] = a2 + b2;
}

// gw[(co * 3 + ci) * 9 + tap] = sum over the slices, ascending
__global__ void stem3x3s1_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, int S) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= S1_OUT) return;
    float sum = 0.f;
#pragma unroll 16
    for (int s = 0; s < S; ++s) sum += ws[(size_t)s * S1_OUT + idx];      // (unrolled: the loads of 16 slices in flight, the adds in order)
    const int co = idx & 31, ci = (idx >> 5) % 3, tap = idx / 96;
    gw[(co * 3 + ci) * 9 + tap] = sum;
}

}  // namespace

// out = (z > 0 ? z : z * slope) (+ res) over n floats, n % 4 == 0; res optional; out may be z
extern "C" int cpr_leaky_fwd(const float* z, const float* res, float* out, long long n, float slope, hipStream_t stream) {
    CPR_CHECK_ARG(z && out && n > 0 && n % 4 == 0 && n / 4 / 256 < (1ll << 31) - 1);
    hipLaunchKernelGGL(leaky_fwd_kernel, dim3((unsigned)cdivll(n / 4, 256)), dim3(256), 0, stream, z, res, out, n / 4, slope);
    CPR_LAUNCH_STATUS();
}

// floats of workspace cpr_leaky_bwd_colsum needs for an (M, C) map
extern "C" int cpr_leaky_bwd_colsum_ws(long long M, int C) {
    if (M <= 0 || C <= 0 || C % 4 != 0) return CPR_ERR_ARG;
    const long long n = cdivll(M, leaky_rows_per_block(M)) * C;
    return n < (1ll << 31) ? (int)n : CPR_ERR_UNSUPPORTED;
}

extern "C" int cpr_leaky_bwd_colsum(const float* dy, const float* add, const float* y, float* g_out, float* colsum, float* ws, long long M,
                                    int C, float slope, hipStream_t stream) {
    CPR_CHECK_ARG(dy && y && colsum && ws && M > 0 && C > 0 && C % 4 == 0);
    const int rows = leaky_rows_per_block(M);
    const long long blocks = cdivll(M, rows);
    CPR_CHECK_ARG(blocks * C < (1ll << 31));
    const int Qtot = C / 4, Q = Qtot < 256 ? Qtot : 256;
    CPR_CHECK_ARG(cdiv(Qtot, Q) <= 65535);
    hipLaunchKernelGGL(leaky_bwd_colsum_kernel, dim3((unsigned)blocks, cdiv(Qtot, Q)), dim3(256), 0, stream, dy, add, y, g_out, ws, M, C, Q,
                       256 / Q, rows, slope);
    hipLaunchKernelGGL(leaky_colsum_finalize_kernel, dim3(cdiv(C, 16)), dim3(16 * LK_FIN_CHAINS), 0, stream, ws, blocks, C, colsum);
    CPR_LAUNCH_STATUS();
}

// workspace floats of cpr_stem3x3s1_wgrad for an (N, 3, H, W) image
extern "C" int cpr_stem3x3s1_wgrad_workspace(int N, int H, int W) {
    CPR_CHECK_ARG(N > 0 && H > 0 && W > 0);
    return s1_plan((long long)N * H * W).S * S1_OUT;
}

// dy (N, H, W, 32); in: the image (layout 0 NHWC4 / 1 planes); gw (32, 3, 3, 3) written; ws: the query's floats
extern "C" int cpr_stem3x3s1_wgrad(const float* dy, const float* in, float* gw, float* ws, int N, int H, int W, int layout,
                                   hipStream_t stream) {
    CPR_CHECK_ARG(dy && in && gw && ws && N > 0 && H > 0 && W > 0 && (layout == 0 || layout == 1));
    const long long M = (long long)N * H * W;
    const S1Plan pl = s1_plan(M);
    if (layout)
        hipLaunchKernelGGL(stem3x3s1_wgrad_kernel<1>, dim3(pl.S), dim3(S1_THREADS), 0, stream, dy, in, ws, M, H, W, pl.P);
    else
        hipLaunchKernelGGL(stem3x3s1_wgrad_kernel<0>, dim3(pl.S), dim3(S1_THREADS), 0, stream, dy, in, ws, M, H, W, pl.P);
    hipLaunchKernelGGL(stem3x3s1_wgrad_reduce_kernel, dim3(cdiv(S1_OUT, 256)), dim3(256), 0, stream, ws, gw, pl.S);
    CPR_LAUNCH_STATUS();
}
