// P2PHead's output convolutions (cls_out / reg_out: 3x3, pad 1, stride 1, Cin -> J <= 8, bias) on the bf16 map of the last tower
// layer, for the bf16 compute mode.  Every kernel reads the RAW bf16 conv output x (N,H,W,Cin) of that layer with its
// per-(image, channel) GroupNorm affine (a, b) and the ReLU applied on load -- the activation relu(a*x + b) is never written.
// Arithmetic (held by tests/test_gpu_p2p_bf16.py): each bf16 element is widened exactly, relu(fmaf(a, x, b)) is fp32, products and
// sums are fp32 FMAs; nothing is rounded to bf16 except the optional bf16 output of the data gradient (round to nearest even).
//
//   forward   one THREAD per pixel: the pixel's Cin channels (16-byte loads, every map element read from HBM once) against the
//             9 J tap weights of each channel -- the weight addresses are wave-uniform, so they are scalar loads and SGPR operands
//             of the FMAs -- into 9 J tap responses R (N,H,W,9J) fp32; then the tap sum of cpr_tap_sum3x3 (csrc/postproc.hip), the
//             same second half as the fp32 mode's 1x1-projection form.  9 J FMAs per input element: at J <= 2 the map read
//             dominates.
//   dgrad     one WAVE per (pixel, channel group): lane = input channel, the 9 J weights of its channels held in VGPRs; the 9
//             neighbouring dout rows (J floats each) are wave-uniform scalar loads.  Writes fp32 or bf16 (N,H,W,Cin).
//   wgrad     the same wave layout over a contiguous pixel range: per-lane accumulators of the 9 J weight gradients of its channels
//             (+ the bias gradient, wave-uniform) -> per-wave partials in a workspace -> a finalize kernel sums the partials in
//             ascending range order.  No float atomics: the result is bit-repeatable.
#include "common.h"

__device__ __forceinline__ float bf16_widen(unsigned short u) { return __uint_as_float((unsigned)u << 16); }

// ------------------------------------------------------------------------------------------------------------------ forward
template <int J>
__global__ __launch_bounds__(256) void p2p_out_taps_kernel(const unsigned short* __restrict__ x, const float* __restrict__ a,
                                                           const float* __restrict__ b, const float* __restrict__ w,
                                                           float* __restrict__ R, long long npix, int HW, int Cin) {
    constexpr int T = 9 * J;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const long long n = p / HW;
    const unsigned short* xp = x + (size_t)p * Cin;
    const float* ap = a + (size_t)n * Cin;
    const float* bp = b + (size_t)n * Cin;
    float acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += 8) {
        const uint4 u = *reinterpret_cast<const uint4*>(xp + c0);
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap + c0), a1 = *reinterpret_cast<const f32x4*>(ap + c0 + 4);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp + c0), b1 = *reinterpret_cast<const f32x4*>(bp + c0 + 4);
        float v[8];
        v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
        v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
        v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
        v[0] = fmaxf(fmaf(a0.x, v[0], b0.x), 0.f); v[1] = fmaxf(fmaf(a0.y, v[1], b0.y), 0.f);
        v[2] = fmaxf(fmaf(a0.z, v[2], b0.z), 0.f); v[3] = fmaxf(fmaf(a0.w, v[3], b0.w), 0.f);
        v[4] = fmaxf(fmaf(a1.x, v[4], b1.x), 0.f); v[5] = fmaxf(fmaf(a1.y, v[5], b1.y), 0.f);
        v[6] = fmaxf(fmaf(a1.z, v[6], b1.z), 0.f); v[7] = fmaxf(fmaf(a1.w, v[7], b1.w), 0.f);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const float* wc = w + ((size_t)j * Cin + c0 + i) * 9;     // uniform: scalar loads
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[t * J + j] = fmaf(v[i], wc[t], acc[t * J + j]);
            }
    }
    float* rp = R + (size_t)p * T;
#pragma unroll
    for (int t = 0; t < T; ++t) rp[t] = acc[t];
}

extern "C" int cpr_tap_sum3x3(const float* R, const float* bias, float* out, int N, int H, int W, int J, hipStream_t stream);

extern "C" int cpr_p2p_out_bf16_fwd(const void* x, const float* a, const float* b, const float* w, const float* bias, float* taps,
                                    float* out, int N, int H, int W, int Cin, int J, hipStream_t stream) {
    CPR_CHECK_ARG(x && a && b && w && bias && taps && out && N > 0 && H > 0 && W > 0);
    if (J < 1 || J > 8 || Cin < 64 || Cin > 256 || Cin % 64 != 0) return CPR_ERR_UNSUPPORTED;
    const long long npix = (long long)N * H * W;
    const unsigned grid = (unsigned)cdivll(npix, 256);
    const unsigned short* xs = (const unsigned short*)x;
#define GO(J_) hipLaunchKernelGGL((p2p_out_taps_kernel<J_>), dim3(grid), dim3(256), 0, stream, xs, a, b, w, taps, npix, H * W, Cin)
    switch (J) {
        case 1: GO(1); break;
        case 2: GO(2); break;
        case 3: GO(3); break;
        case 4: GO(4); break;
        case 5: GO(5); break;
        case 6: GO(6); break;
        case 7: GO(7); break;
        default: GO(8); break;
    }
#undef GO
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return -(int)e;
    return cpr_tap_sum3x3(taps, bias, out, N, H, W, J, stream);
}

// ------------------------------------------------------------------------------------------------------------------ shared
// The wave layout of the two backward kernels: a wave owns channel group g (KW blocks of 64 channels, lane = channel within a block)
// and walks pixels.  The dout row of output pixel (oy, ox) is read at a clamped in-map address and zeroed when (oy, ox) lies outside
// the map, so the nine loads of a pixel carry no branch and can all be in flight together.
template <int J>
__device__ __forceinline__ void load_taps(const float* __restrict__ dout, int ldd, long long nbase, int y, int x, int H, int W,
                                          float (&d)[9][J]) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int oy = y - kh + 1, ox = x - kw + 1;
            const bool in = (unsigned)oy < (unsigned)H && (unsigned)ox < (unsigned)W;
            const int cy = min(max(oy, 0), H - 1), cx = min(max(ox, 0), W - 1);
            const float* dp = dout + ((size_t)nbase + (size_t)cy * W + cx) * ldd;
#pragma unroll
            for (int j = 0; j < J; ++j) d[kh * 3 + kw][j] = in ? dp[j] : 0.f;
        }
}

// ------------------------------------------------------------------------------------------------------------------ dgrad
// dx[n,y,x,c] = sum_{kh,kw,j} dout[n, y-kh+1, x-kw+1, j] * w[j][c][kh][kw]   (the gradient wrt the activated input)
template <int J, int KW, bool OUT16>
__global__ __launch_bounds__(64) void p2p_out_dgrad_kernel(const float* __restrict__ dout, int ldd, const float* __restrict__ w,
                                                           void* __restrict__ dx, long long npix, int H, int W, int Cin, int G,
                                                           int ppw) {
    const int lane = threadIdx.x;
    const int g = blockIdx.x % G;
    const long long p0 = (long long)(blockIdx.x / G) * ppw;
    float wr[KW][9][J];
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int c = (g * KW + k) * 64 + lane;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int t = 0; t < 9; ++t) wr[k][t][j] = w[((size_t)j * Cin + c) * 9 + t];
    }
    const int HW = H * W;
    const long long pend = p0 + ppw < npix ? p0 + ppw : npix;
    for (long long p = p0; p < pend; ++p) {
        const long long n = p / HW;
        const int r = (int)(p - n * HW);
        const int y = r / W, x = r - (r / W) * W;
        float d[9][J];
        load_taps<J>(dout, ldd, n * HW, y, x, H, W, d);
        float acc[KW];
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int j = 0; j < J; ++j) s = fmaf(d[t][j], wr[k][t][j], s);
            acc[k] = s;
        }
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const size_t o = (size_t)p * Cin + (g * KW + k) * 64 + lane;
            if (OUT16)
                reinterpret_cast<__bf16*>(dx)[o] = (__bf16)acc[k];      // round to nearest even
            else
                reinterpret_cast<float*>(dx)[o] = acc[k];
        }
    }
}

template <int J, bool OUT16>
static void launch_dgrad(const float* dout, int ldd, const float* w, void* dx, long long npix, int H, int W, int Cin,
                         hipStream_t stream) {
    // J <= 4: a wave covers every channel (KW = Cin / 64); J > 4: one 64-channel block per wave (VGPRs: 9 J KW weights)
    const int KB = Cin / 64;
    const int KW = J <= 4 ? KB : 1;
    const int G = KB / KW;
    const int ppw = 16;
    const unsigned grid = (unsigned)(cdivll(npix, ppw) * G);
#define GO(KW_) hipLaunchKernelGGL((p2p_out_dgrad_kernel<J, KW_, OUT16>), dim3(grid), dim3(64), 0, stream, dout, ldd, w, dx, npix, H, W, \
                                   Cin, G, ppw)
    if constexpr (J > 4) {
        GO(1);
    } else {
        switch (KW) {
            case 1: GO(1); break;
            case 2: GO(2); break;
            case 3: GO(3); break;
            default: GO(4); break;
        }
    }
#undef GO
}

extern "C" int cpr_p2p_out_bf16_dgrad(const float* dout, int ldd, const float* w, void* dx, int out_bf16, int N, int H, int W,
                                      int Cin, int J, hipStream_t stream) {
    CPR_CHECK_ARG(dout && w && dx && N > 0 && H > 0 && W > 0 && ldd >= J);
    if (J < 1 || J > 8 || Cin < 64 || Cin > 256 || Cin % 64 != 0) return CPR_ERR_UNSUPPORTED;
    const long long npix = (long long)N * H * W;
#define GO(J_)                                                                                     \
    do {                                                                                           \
        if (out_bf16) launch_dgrad<J_, true>(dout, ldd, w, dx, npix, H, W, Cin, stream);          \
        else launch_dgrad<J_, false>(dout, ldd, w, dx, npix, H, W, Cin, stream);                  \
    } while (0)
    switch (J) {
        case 1: GO(1); break;
        case 2: GO(2); break;
        case 3: GO(3); break;
        case 4: GO(4); break;
        case 5: GO(5); break;
        case 6: GO(6); break;
        case 7: GO(7); break;
        default: GO(8); break;
    }
#undef GO
    CPR_LAUNCH_STATUS();
}

// ------------------------------------------------------------------------------------------------------------------ wgrad
// gw[j][c][kh][kw] = sum_{n,y,x} relu(a x + b)[n,y,x,c] * dout[n, y-kh+1, x-kw+1, j],  gb[j] = sum dout[..., j]
// Wave (range r, group g) sums its pixel range into ws[r][c][t][j] (its channels) and, for g = 0, wsb[r][j].
static int wgrad_ranges(long long npix, int G) {
    const long long want = 2048 / G;                 // ~8 waves per CU in all
    const long long by_pix = cdivll(npix, 64);       // at least 64 pixels per wave
    return (int)(want < by_pix ? want : by_pix);
}
static int wgrad_groups(int Cin, int J) { return J <= 4 ? 1 : Cin / 64; }

template <int J, int KW>
__global__ __launch_bounds__(64) void p2p_out_wgrad_kernel(const unsigned short* __restrict__ x, const float* __restrict__ a,
                                                           const float* __restrict__ b, const float* __restrict__ dout, int ldd,
                                                           float* __restrict__ ws, float* __restrict__ wsb, long long npix, int H,
                                                           int W, int Cin, int G, long long ppw) {
    const int lane = threadIdx.x;
    const int g = blockIdx.x % G;
    const int rg = blockIdx.x / G;
    const long long p0 = rg * ppw;
    const long long pend = p0 + ppw < npix ? p0 + ppw : npix;
    const int HW = H * W;
    float acc[KW][9][J];
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < J; ++j) acc[k][t][j] = 0.f;
    float bacc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) bacc[j] = 0.f;
    long long cur_n = -1;
    float an[KW], bn[KW];
    for (long long p = p0; p < pend; ++p) {
        const long long n = p / HW;
        if (n != cur_n) {            // (wave-uniform)
            cur_n = n;
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                const int c = (g * KW + k) * 64 + lane;
                an[k] = a[(size_t)n * Cin + c];
                bn[k] = b[(size_t)n * Cin + c];
            }
        }
        const int r = (int)(p - n * HW);
        const int y = r / W, xx = r - (r / W) * W;
        float v[KW];
#pragma unroll
        for (int k = 0; k < KW; ++k)
            v[k] = fmaxf(fmaf(an[k], bf16_widen(x[(size_t)p * Cin + (g * KW + k) * 64 + lane]), bn[k]), 0.f);
        float d[9][J];
        load_taps<J>(dout, ldd, n * HW, y, xx, H, W, d);
#pragma unroll
        for (int k = 0; k < KW; ++k)
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int j = 0; j < J; ++j) acc[k][t][j] = fmaf(v[k], d[t][j], acc[k][t][j]);
        const float* dp = dout + (size_t)p * ldd;
#pragma unroll
        for (int j = 0; j < J; ++j) bacc[j] += dp[j];
    }
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int c = (g * KW + k) * 64 + lane;
        float* o = ws + ((size_t)rg * Cin + c) * (9 * J);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < J; ++j) o[t * J + j] = acc[k][t][j];
    }
    if (g == 0 && lane == 0)
#pragma unroll
        for (int j = 0; j < J; ++j) wsb[(size_t)rg * J + j] = bacc[j];
}

// e < Cin*9J: gw[j][c][t] = sum_r ws[r][c][t][j] (ascending r); e in [Cin*9J, Cin*9J + J): gb[j] = sum_r wsb[r][j]
__global__ __launch_bounds__(256) void p2p_out_wgrad_finalize_kernel(const float* __restrict__ ws, const float* __restrict__ wsb,
                                                                     float* __restrict__ gw, float* __restrict__ gb, int R, int Cin,
                                                                     int J) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int E = Cin * 9 * J;
    if (e < E) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += ws[(size_t)r * E + e];
        const int c = e / (9 * J), t = (e / J) % 9, j = e % J;
        gw[((size_t)j * Cin + c) * 9 + t] = s;
    } else if (e < E + J) {
        const int j = e - E;
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += wsb[(size_t)r * J + j];
        gb[j] = s;
    }
}

template <int J>
static void launch_wgrad(const unsigned short* x, const float* a, const float* b, const float* dout, int ldd, float* ws, float* wsb,
                         long long npix, int H, int W, int Cin, int G, int R, long long ppw, hipStream_t stream) {
#define GO(KW_) hipLaunchKernelGGL((p2p_out_wgrad_kernel<J, KW_>), dim3(R * G), dim3(64), 0, stream, x, a, b, dout, ldd, ws, wsb, npix, \
                                   H, W, Cin, G, ppw)
    if constexpr (J > 4) {
        GO(1);
    } else {
        switch (Cin / 64) {
            case 1: GO(1); break;
            case 2: GO(2); break;
            case 3: GO(3); break;
            default: GO(4); break;
        }
    }
#undef GO
}

extern "C" int cpr_p2p_out_bf16_wgrad_ws(int N, int H, int W, int Cin, int J) {
    if (N <= 0 || H <= 0 || W <= 0 || J < 1 || J > 8 || Cin < 64 || Cin > 256 || Cin % 64 != 0) return CPR_ERR_UNSUPPORTED;
    const int R = wgrad_ranges((long long)N * H * W, wgrad_groups(Cin, J));
    return R * (Cin * 9 * J + J);
}

extern "C" int cpr_p2p_out_bf16_wgrad(const void* x, const float* a, const float* b, const float* dout, int ldd, float* gw,
                                      float* gb, float* ws, int N, int H, int W, int Cin, int J, hipStream_t stream) {
    CPR_CHECK_ARG(x && a && b && dout && gw && gb && ws && N > 0 && H > 0 && W > 0 && ldd >= J);
    if (J < 1 || J > 8 || Cin < 64 || Cin > 256 || Cin % 64 != 0) return CPR_ERR_UNSUPPORTED;
    const long long npix = (long long)N * H * W;
    const int G = wgrad_groups(Cin, J);
    const int R = wgrad_ranges(npix, G);
    const long long ppw = cdivll(npix, R);
    float* wsb = ws + (size_t)R * Cin * 9 * J;
    const unsigned short* xs = (const unsigned short*)x;
    switch (J) {
        case 1: launch_wgrad<1>(xs, a, b, dout, ldd, ws, wsb, npix, H, W, Cin, G, R, ppw, stream); break;
        case 2: launch_wgrad<2>(xs, a, b, dout, ldd, ws, wsb, npix, H, W, Cin, G, R, ppw, stream); break;
        case 3: launch_wgrad<3>(xs, a, b, dout, ldd, ws, wsb, npix, H, W, Cin, G, R, ppw, stream); break;
        case 4: launch_wgrad<4>(xs, a, b, dout, ldd, ws, wsb, npix, H, W, Cin, G, R, ppw, stream); break;
        case 5: launch_wgrad<5>(xs, a, b, dout, ldd, ws, wsb, npix, H, W, Cin, G, R, ppw, stream); break;
        case 6: launch_wgrad<6>(xs, a, b, dout, ldd, ws, wsb, npix, H, W, Cin, G, R, ppw, stream); break;
        case 7: launch_wgrad<7>(xs, a, b, dout, ldd, ws, wsb, npix, H, W, Cin, G, R, ppw, stream); break;
        default: launch_wgrad<8>(xs, a, b, dout, ldd, ws, wsb, npix, H, W, Cin, G, R, ppw, stream); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return -(int)e;
    const int E = Cin * 9 * J + J;
    hipLaunchKernelGGL(p2p_out_wgrad_finalize_kernel, dim3(cdiv(E, 256)), dim3(256), 0, stream, ws, wsb, gw, gb, R, Cin, J);
    CPR_LAUNCH_STATUS();
}
