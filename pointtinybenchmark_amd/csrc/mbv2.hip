// MobileNetV2 kernels (gfx950, fp32): the depthwise 3x3 convolution -- forward, data gradient, weight gradient -- and the ReLU6
// streaming passes around it.
//
// A depthwise 3x3 does 9 FMAs per output element against 8 bytes of traffic (read x once, write y once): it is bound by HBM, not by the
// ALUs, so these are streaming kernels and not members of the grouped family of conv_group.hip (9 * cg FMAs per output, cg >= 4).
//
// Layout: NHWC maps at the channel pitch Cp = roundup(C, 32), C % 8 == 0.  Pad channels [C, Cp) of an input are never read; pad channels
// of an output are written as +0.0.  A lane owns one channel quad (16 bytes) of one map column and walks DOWN a strip of output rows with
// the 3x3 window in registers: a step loads the one (stride 1) or two (stride 2) input rows that are new and keeps the rest, so an input
// element reaches a lane's registers once per strip and column tap (3 lanes of neighbouring columns, which sit in the same workgroup and
// hit its L1) instead of nine times.  Lanes of a workgroup cover consecutive (column, quad) pairs, i.e. one contiguous span of a map row.
//
// No atomics: every output element is one lane's fixed-order sum (taps kh, kw ascending), so results are bit-repeatable and an image of
// a batch equals its single-image run.  The reductions over pixels (column sums, weight gradient) go through per-workgroup partials in
// a caller-allocated workspace and a second kernel that adds them in ascending order.
#include "common.h"

// cpr_dw3x3_fwd `flags`: restated from include/cpr_hip.h as common.h restates the conv flags (the public header declares streams as
// void* and is not included by the kernels); tests/test_mobilenet_v2_host.py holds the header, this file and ops.py to the same values
#define CPR_DW_IN_CLAMP6 1
#define CPR_DW_RELU6 2

namespace {

#define DW_WGRAD_WGS 1024

struct DwGrid {
    int Cp, Qtot, Q, PP, CG, R, colblocks, strips;
    long long P;      // workgroups that write a partial row: N * strips * colblocks
};

// rows: the rows the strips divide (output rows of the forward and the weight gradient, input rows of the data gradient), cols alike
static bool dw_grid(int N, int rows, int cols, int C, DwGrid* g, int min_wgs = 4096) {
    g->Cp = (C + 31) / 32 * 32;
    g->Qtot = g->Cp / 4;
    g->Q = g->Qtot < 256 ? g->Qtot : 256;
    g->PP = 256 / g->Q;
    g->CG = cdiv(g->Qtot, g->Q);
    g->colblocks = cdiv(cols, g->PP);
    // strip height: the whole column, halved until the launch has min_wgs workgroups (4096: 16 per CU) or 4 rows are left.  Tall strips
    // read few halo rows again (2 / R) and leave few partial rows for the second stage of a reduction.  The weight gradient asks for
    // 1024: a workgroup's partial is 9 * C floats whatever it read, so its lanes must walk many pixels each (20 x 20 x 960, B = 64:
    // 8960 workgroups of 3 rows wrote 310 MB of partials for 98 MB of operands; 1280 of 20 rows write 44 MB).
    int R = rows;
    while (R > 4 && (long long)N * g->CG * g->colblocks * cdiv(rows, R) < min_wgs) R = (R + 1) >> 1;
    g->R = R;
    g->strips = cdiv(rows, R);
    g->P = (long long)N * g->strips * g->colblocks;
    return (long long)N * g->CG <= 65535 && g->strips <= 65535;
}

struct DwLane {
    int c, col, pl, q, n;
    bool on;      // this lane owns a column of the map and a channel quad below the pitch
};

__device__ __forceinline__ DwLane dw_lane(int Q, int PP, int CG, int Qtot, int cols) {
    DwLane l;
    l.q = threadIdx.x % Q;
    l.pl = threadIdx.x / Q;
    const int gi = blockIdx.z % CG;
    l.n = blockIdx.z / CG;
    const int qg = gi * Q + l.q;
    l.c = qg * 4;
    l.col = blockIdx.x * PP + l.pl;
    l.on = l.pl < PP && qg < Qtot && l.col < cols;
    return l;
}

__device__ __forceinline__ f32x4 dw_zero() {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return z;
}

// one row of the window: the three taps of input row r around input column c0 + 1 (zero outside the map)
__device__ __forceinline__ void dw_load_row(const float* __restrict__ img, int r, int c0, int H, int W, int Cp, int c, bool clamp, f32x4* dst) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int col = c0 + k;
        f32x4 v = dw_zero();
        if (r >= 0 && r < H && col >= 0 && col < W) {
            v = *reinterpret_cast<const f32x4*>(img + ((size_t)r * W + col) * Cp + c);
            if (clamp) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fminf(v[e], 6.f);
            }
        }
        dst[k] = v;
    }
}

// walks output rows [o0, o1) of output column `ocol`: f(orow, win) sees win[kh * 3 + kw] = in[orow * S + kh - 1][ocol * S + kw - 1]
template <int S, class F>
__device__ __forceinline__ void dw_walk(const float* __restrict__ img, int H, int W, int Cp, int c, int ocol, int o0, int o1, bool clamp, F&& f) {
    f32x4 win[9];
    const int c0 = ocol * S - 1;
    if (S == 1) {
        dw_load_row(img, o0 - 1, c0, H, W, Cp, c, clamp, win + 3);
        dw_load_row(img, o0, c0, H, W, Cp, c, clamp, win + 6);
    } else {
        dw_load_row(img, o0 * 2 - 1, c0, H, W, Cp, c, clamp, win + 6);
    }
    for (int o = o0; o < o1; ++o) {
        if (S == 1) {
#pragma unroll
            for (int k = 0; k < 6; ++k) win[k] = win[k + 3];
            dw_load_row(img, o + 1, c0, H, W, Cp, c, clamp, win + 6);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) win[k] = win[k + 6];
            dw_load_row(img, o * 2, c0, H, W, Cp, c, clamp, win + 3);
            dw_load_row(img, o * 2 + 1, c0, H, W, Cp, c, clamp, win + 6);
        }
        f(o, win);
    }
}

// ------------------------------------------------------------------------------------------------ pack
// (C,1,3,3) -> [9][Cp] tap-major, pad channels zero, `scale` (optional, (C)) multiplied in: the forward pack, the data-gradient pack
// (scale = the folded BatchNorm's); run again on the same buffers it overwrites the pack in place
__global__ void dw_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ wp, int C, int Cp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * Cp) return;
    const int t = i / Cp, c = i % Cp;
    float v = 0.f;
    if (c < C) v = scale ? w[c * 9 + t] * scale[c] : w[c * 9 + t];
    wp[i] = v;
}

// ------------------------------------------------------------------------------------------------ forward
template <int S>
__global__ __launch_bounds__(256) void dw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ scale,
                                                     const float* __restrict__ bias, float* __restrict__ y, int H, int W, int OH, int OW,
                                                     int C, int Cp, int Q, int PP, int CG, int R, int flags) {
    const DwLane l = dw_lane(Q, PP, CG, Cp / 4, OW);
    if (!l.on) return;
    const int o0 = blockIdx.y * R, o1 = min(OH, o0 + R);
    float* yo = y + (size_t)l.n * OH * OW * Cp + l.c;
    if (l.c >= C) {      // a pad quad: +0.0, nothing read
        for (int o = o0; o < o1; ++o) *reinterpret_cast<f32x4*>(yo + ((size_t)o * OW + l.col) * Cp) = dw_zero();
        return;
    }
    f32x4 wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * Cp + l.c);
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, bi = dw_zero();
    if (scale) sc = *reinterpret_cast<const f32x4*>(scale + l.c);
    if (bias) bi = *reinterpret_cast<const f32x4*>(bias + l.c);
    const bool affine = scale || bias, relu6 = flags & CPR_DW_RELU6;
    dw_walk<S>(x + (size_t)l.n * H * W * Cp, H, W, Cp, l.c, l.col, o0, o1, flags & CPR_DW_IN_CLAMP6, [&](int o, const f32x4* win) {
        f32x4 acc = dw_zero();
#pragma unroll
        for (int t = 0; t < 9; ++t) acc += win[t] * wt[t];
        if (affine) acc = acc * sc + bi;
        if (relu6) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fminf(fmaxf(acc[e], 0.f), 6.f);
        }
        *reinterpret_cast<f32x4*>(yo + ((size_t)o * OW + l.col) * Cp) = acc;
    });
}

// ------------------------------------------------------------------------------------------------ per-workgroup partial sums
// the lanes of a workgroup that share a channel quad (one per column lane pl) are added in ascending pl; lanes that are off hold zeros
__device__ __forceinline__ void dw_block_sum(f32x4 v, f32x4* red, int Q, int PP, float* dst /* this workgroup's row + channel, or null */) {
    red[threadIdx.x] = v;
    __syncthreads();
    if (dst && threadIdx.x < Q) {
        f32x4 s = red[threadIdx.x];
        for (int r = 1; r < PP; ++r) s += red[r * Q + threadIdx.x];
        *reinterpret_cast<f32x4*>(dst) = s;
    }
    __syncthreads();
}

// out[col] (+)= sum over p ascending of part[p][col]: 16 interleaved chains per column, then those 16 in order.  taps > 1: the column
// tap * C + c lands at c * taps + tap (the (C,1,3,3) weight gradient).
__global__ __launch_bounds__(256) void dw_finalize_kernel(const float* __restrict__ part, long long P, int ncol, float* __restrict__ out, int C,
                                                          int taps, int accumulate) {
    __shared__ float red[16][17];
    const int cl = threadIdx.x & 15, j = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + cl;
    float s = 0.f;
    if (col < ncol)
        for (long long p = j; p < P; p += 16) s += part[(size_t)p * ncol + col];
    red[j][cl] = s;
    __syncthreads();
    if (j == 0 && col < ncol) {
        float t = red[0][cl];
        for (int k = 1; k < 16; ++k) t += red[k][cl];
        const int o = taps > 1 ? (col % C) * taps + col / C : col;
        out[o] = accumulate ? out[o] + t : t;
    }
}

// ------------------------------------------------------------------------------------------------ data gradient
// the epilogue of a data-gradient element: + add, ReLU6 mask of the producer's recorded map, store, column-sum term
__device__ __forceinline__ f32x4 dw_dgrad_epilogue(f32x4 v, size_t o, const float* __restrict__ add, const float* __restrict__ mask,
                                                   float* __restrict__ dx) {
    if (add) v += *reinterpret_cast<const f32x4*>(add + o);
    if (mask) {
        const f32x4 m = *reinterpret_cast<const f32x4*>(mask + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (m[e] > 0.f && m[e] < 6.f) ? v[e] : 0.f;
    }
    *reinterpret_cast<f32x4*>(dx + o) = v;
    return v;
}

// dx (N,H,W) from dy (N,OH,OW); S == 1: the forward walk over dy with the taps flipped; S == 2: the gather over the taps whose
// division is exact (no zero insertion).  part (optional): this workgroup's column sums, row (n * strips + strip) * colblocks + bx.
template <int S>
__global__ __launch_bounds__(256) void dw_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ wp, const float* __restrict__ add,
                                                       const float* __restrict__ mask, float* __restrict__ dx, float* __restrict__ part,
                                                       int H, int W, int OH, int OW, int C, int Cp, int Q, int PP, int CG, int R) {
    __shared__ f32x4 red[256];
    const DwLane l = dw_lane(Q, PP, CG, Cp / 4, W);
    const int h0 = blockIdx.y * R, h1 = min(H, h0 + R);
    const size_t img = (size_t)l.n * H * W * Cp;
    f32x4 cs = dw_zero();
    const bool real = l.on && l.c < C;
    if (l.on && !real) {
        for (int h = h0; h < h1; ++h) *reinterpret_cast<f32x4*>(dx + img + ((size_t)h * W + l.col) * Cp + l.c) = dw_zero();
    } else if (real) {
        f32x4 wt[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * Cp + l.c);
        const float* dyi = dy + (size_t)l.n * OH * OW * Cp;
        if (S == 1) {
            dw_walk<1>(dyi, OH, OW, Cp, l.c, l.col, h0, h1, false, [&](int h, const f32x4* win) {
                f32x4 acc = dw_zero();
#pragma unroll
                for (int t = 0; t < 9; ++t) acc += win[t] * wt[8 - t];
                cs += dw_dgrad_epilogue(acc, img + ((size_t)h * W + l.col) * Cp + l.c, add, mask, dx);
            });
        } else {
            for (int h = h0; h < h1; ++h) {
                f32x4 acc = dw_zero();
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int th = h + 1 - kh;
                    if (th < 0 || (th & 1) || (th >> 1) >= OH) continue;
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int tw = l.col + 1 - kw;
                        if (tw < 0 || (tw & 1) || (tw >> 1) >= OW) continue;
                        acc += *reinterpret_cast<const f32x4*>(dyi + ((size_t)(th >> 1) * OW + (tw >> 1)) * Cp + l.c) * wt[kh * 3 + kw];
                    }
                }
                cs += dw_dgrad_epilogue(acc, img + ((size_t)h * W + l.col) * Cp + l.c, add, mask, dx);
            }
        }
    }
    if (part) {      // (uniform over the workgroup)
        const size_t row = ((size_t)l.n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        dw_block_sum(cs, red, Q, PP, (threadIdx.x < Q && l.c < C) ? part + row * C + l.c : nullptr);
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// part[row][tap][C]: this workgroup's sum over its strip of dy * clamp_in(x) per tap
template <int S>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ part, int H,
                                                       int W, int OH, int OW, int C, int Cp, int Q, int PP, int CG, int R, int clamp) {
    __shared__ f32x4 red[256];
    const DwLane l = dw_lane(Q, PP, CG, Cp / 4, OW);
    const int o0 = blockIdx.y * R, o1 = min(OH, o0 + R);
    f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = dw_zero();
    if (l.on && l.c < C) {
        const float* dyi = dy + (size_t)l.n * OH * OW * Cp + l.c;
        dw_walk<S>(x + (size_t)l.n * H * W * Cp, H, W, Cp, l.c, l.col, o0, o1, clamp, [&](int o, const f32x4* win) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(dyi + ((size_t)o * OW + l.col) * Cp);
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[t] += d * win[t];
        });
    }
    const size_t row = ((size_t)l.n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const bool writer = threadIdx.x < Q && l.c < C;
#pragma unroll
    for (int t = 0; t < 9; ++t) dw_block_sum(acc[t], red, Q, PP, writer ? part + (row * 9 + t) * C + l.c : nullptr);
}

// ------------------------------------------------------------------------------------------------ ReLU6 backward + column sums, clamp
// (M, C) row-major: g = (dy (+ add)) * (0 < y < 6) (y null: g = dy, g_out may be null) and this workgroup's column sums part[bx][C]
__global__ __launch_bounds__(256) void relu6_bwd_colsum_kernel(const float* __restrict__ dy, const float* __restrict__ add, const float* __restrict__ y,
                                                              float* __restrict__ g_out, float* __restrict__ part, long long M, int C, int Q,
                                                              int PP, int rows) {
    __shared__ f32x4 red[256];
    const int q = threadIdx.x % Q, pl = threadIdx.x / Q;
    const int c = (blockIdx.y * Q + q) * 4;
    const long long r0 = (long long)blockIdx.x * rows, r1 = min(M, r0 + rows);
    f32x4 cs = dw_zero();
    if (pl < PP && c < C) {
        for (long long r = r0 + pl; r < r1; r += PP) {
            const size_t o = (size_t)r * C + c;
            f32x4 g = *reinterpret_cast<const f32x4*>(dy + o);
            if (add) g += *reinterpret_cast<const f32x4*>(add + o);
            if (y) {
                const f32x4 m = *reinterpret_cast<const f32x4*>(y + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = (m[e] > 0.f && m[e] < 6.f) ? g[e] : 0.f;
            }
            if (g_out) *reinterpret_cast<f32x4*>(g_out + o) = g;
            cs += g;
        }
    }
    dw_block_sum(cs, red, Q, PP, (threadIdx.x < Q && c < C) ? part + (size_t)blockIdx.x * C + c : nullptr);
}

__global__ void clamp6_kernel(float* __restrict__ x, long long n4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = reinterpret_cast<f32x4*>(x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fminf(v[e], 6.f);
    reinterpret_cast<f32x4*>(x)[i] = v;
}

static int relu6_rows_per_block(long long M) {
    int rows = 128;
    while (rows > 16 && cdivll(M, rows) < 2048) rows >>= 1;
    return rows;
}

static bool dw_shape_ok(int N, int H, int W, int C, int stride) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || (stride != 1 && stride != 2)) return false;
    return (long long)H * W * ((C + 31) / 32 * 32) < (1ll << 29);      // one image below 2 GiB
}

static void dw_finalize(const float* part, long long P, int ncol, float* out, int C, int taps, int accumulate, hipStream_t stream) {
    hipLaunchKernelGGL(dw_finalize_kernel, dim3(cdiv(ncol, 16)), dim3(256), 0, stream, part, P, ncol, out, C, taps, accumulate);
}

}  // namespace

extern "C" int cpr_dw3x3_pack(const float* w, const float* scale, float* wp, int C, hipStream_t stream) {
    CPR_CHECK_ARG(w && wp && C > 0 && C % 8 == 0);
    const int Cp = (C + 31) / 32 * 32;
    hipLaunchKernelGGL(dw_pack_kernel, dim3(cdiv(9 * Cp, 256)), dim3(256), 0, stream, w, scale, wp, C, Cp);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_dw3x3_fwd(const float* x, const float* wp, const float* scale, const float* bias, float* y, int N, int H, int W, int C,
                             int stride, int flags, hipStream_t stream) {
    CPR_CHECK_ARG(x && wp && y && dw_shape_ok(N, H, W, C, stride) && (flags & ~(CPR_DW_IN_CLAMP6 | CPR_DW_RELU6)) == 0);
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    DwGrid g;
    CPR_CHECK_ARG(dw_grid(N, OH, OW, C, &g));
    const dim3 grid(g.colblocks, g.strips, N * g.CG);
    if (stride == 1) hipLaunchKernelGGL(dw_fwd_kernel<1>, grid, dim3(256), 0, stream, x, wp, scale, bias, y, H, W, OH, OW, C, g.Cp, g.Q, g.PP, g.CG, g.R, flags);
    else hipLaunchKernelGGL(dw_fwd_kernel<2>, grid, dim3(256), 0, stream, x, wp, scale, bias, y, H, W, OH, OW, C, g.Cp, g.Q, g.PP, g.CG, g.R, flags);
    CPR_LAUNCH_STATUS();
}

// floats of workspace the column sums of cpr_dw3x3_dgrad need for a data gradient (N,H,W,C)
extern "C" int cpr_dw3x3_dgrad_workspace(int N, int H, int W, int C) {
    DwGrid g;
    if (!dw_shape_ok(N, H, W, C, 1) || !dw_grid(N, H, W, C, &g)) return CPR_ERR_ARG;
    const long long n = g.P * C;
    return n < (1ll << 31) ? (int)n : CPR_ERR_UNSUPPORTED;
}

extern "C" int cpr_dw3x3_dgrad(const float* dy, const float* wp, const float* add, const float* mask, float* dx, float* colsum, float* ws,
                               int N, int H, int W, int C, int stride, hipStream_t stream) {
    CPR_CHECK_ARG(dy && wp && dx && dw_shape_ok(N, H, W, C, stride) && (!colsum || ws));
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    DwGrid g;
    CPR_CHECK_ARG(dw_grid(N, H, W, C, &g));
    const dim3 grid(g.colblocks, g.strips, N * g.CG);
    float* part = colsum ? ws : nullptr;
    if (stride == 1) hipLaunchKernelGGL(dw_dgrad_kernel<1>, grid, dim3(256), 0, stream, dy, wp, add, mask, dx, part, H, W, OH, OW, C, g.Cp, g.Q, g.PP, g.CG, g.R);
    else hipLaunchKernelGGL(dw_dgrad_kernel<2>, grid, dim3(256), 0, stream, dy, wp, add, mask, dx, part, H, W, OH, OW, C, g.Cp, g.Q, g.PP, g.CG, g.R);
    if (colsum) dw_finalize(part, g.P, C, colsum, C, 1, 0, stream);
    CPR_LAUNCH_STATUS();
}

// floats of workspace cpr_dw3x3_wgrad needs; (H, W): the layer's input size
extern "C" int cpr_dw3x3_wgrad_workspace(int N, int H, int W, int C, int stride) {
    DwGrid g;
    if (!dw_shape_ok(N, H, W, C, stride) || !dw_grid(N, (H - 1) / stride + 1, (W - 1) / stride + 1, C, &g, DW_WGRAD_WGS)) return CPR_ERR_ARG;
    const long long n = g.P * 9 * C;
    return n < (1ll << 31) ? (int)n : CPR_ERR_UNSUPPORTED;
}

extern "C" int cpr_dw3x3_wgrad(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int stride, int in_clamp6,
                               int accumulate, hipStream_t stream) {
    CPR_CHECK_ARG(dy && x && grad_w && ws && dw_shape_ok(N, H, W, C, stride) && (in_clamp6 & ~1) == 0 && (accumulate & ~1) == 0);
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    DwGrid g;
    CPR_CHECK_ARG(dw_grid(N, OH, OW, C, &g, DW_WGRAD_WGS) && g.P * 9 * C < (1ll << 31));
    const dim3 grid(g.colblocks, g.strips, N * g.CG);
    if (stride == 1) hipLaunchKernelGGL(dw_wgrad_kernel<1>, grid, dim3(256), 0, stream, dy, x, ws, H, W, OH, OW, C, g.Cp, g.Q, g.PP, g.CG, g.R, in_clamp6);
    else hipLaunchKernelGGL(dw_wgrad_kernel<2>, grid, dim3(256), 0, stream, dy, x, ws, H, W, OH, OW, C, g.Cp, g.Q, g.PP, g.CG, g.R, in_clamp6);
    dw_finalize(ws, g.P, 9 * C, grad_w, C, 9, accumulate, stream);
    CPR_LAUNCH_STATUS();
}

// floats of workspace cpr_relu6_bwd_colsum needs for an (M, C) map
extern "C" int cpr_relu6_bwd_colsum_ws(long long M, int C) {
    if (M <= 0 || C <= 0 || C % 4 != 0) return CPR_ERR_ARG;
    const long long n = cdivll(M, relu6_rows_per_block(M)) * C;
    return n < (1ll << 31) ? (int)n : CPR_ERR_UNSUPPORTED;
}

extern "C" int cpr_relu6_bwd_colsum(const float* dy, const float* add, const float* y, float* g_out, float* colsum, float* ws, long long M,
                                    int C, hipStream_t stream) {
    CPR_CHECK_ARG(dy && colsum && ws && M > 0 && C > 0 && C % 4 == 0 && (y || !add));
    const int rows = relu6_rows_per_block(M);
    const long long blocks = cdivll(M, rows);
    CPR_CHECK_ARG(blocks * C < (1ll << 31));
    const int Qtot = C / 4, Q = Qtot < 256 ? Qtot : 256;
    hipLaunchKernelGGL(relu6_bwd_colsum_kernel, dim3((unsigned)blocks, cdiv(Qtot, Q)), dim3(256), 0, stream, dy, add, y, g_out, ws, M, C, Q,
                       256 / Q, rows);
    dw_finalize(ws, blocks, C, colsum, C, 1, 0, stream);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_clamp6(float* x, long long n, hipStream_t stream) {
    CPR_CHECK_ARG(x && n > 0 && n % 4 == 0 && n / 4 / 256 < (1ll << 31) - 1);
    hipLaunchKernelGGL(clamp6_kernel, dim3((unsigned)cdivll(n / 4, 256)), dim3(256), 0, stream, x, n / 4);
    CPR_LAUNCH_STATUS();
}
