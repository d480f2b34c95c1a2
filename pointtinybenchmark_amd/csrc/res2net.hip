// Res2Net slice kernels (Bottle2neck's hierarchical 3x3 chain), NHWC fp32: a dense 3x3 / padding 1 / stride 1 or 2 convolution of
// `width -> width` channels that reads a channel SLICE [x_off, x_off + width) of a map with row pitch x_pitch (optionally plus a slice of
// a second map, summed on load) and writes a slice of an output map -- so the chain runs on the block's two internal maps in place, with
// no split / contiguous / cat copies -- its data gradient (the same kernel over a gradient slice with the transposed pack; a stride-2
// layer in gather form), its weight gradient, and the last slice's 3x3 / stride-2 average pool with its backward.
//
// Plain fp32 FMA doing the exact work, 9 * width FMAs per output, in the manner of conv_group.hip.  The widths are even but no multiple
// of 4 (26, 14, ...), and slice i starts at channel i * width, so the only alignment every slice has is 8 bytes: every activation and
// weight access is a float2 (global_load_dwordx2).  Thread mapping (forward): lane <-> 2 consecutive output channels, consecutive lanes
// <-> consecutive channel pairs of one pixel quad, so a wave's stores are contiguous runs of the slice and its activation loads are
// broadcasts of one float2 per pixel (every lane of a pixel reads the same input channels).  A thread keeps 2 channels x R2_PX pixels of
// accumulators and walks tap -> input channel pair; the two float2 weights of a pair are reused over the R2_PX pixels, and the pack
// stores them so that this load is contiguous over the lanes: P[tap][in pair][j][out pair] float2.
// Accumulation order of an output: tap-major, input channel ascending, one fmaf each -- a function of nothing but the layer, so an
// image of a batch equals its single-image run bit for bit and two runs agree bit for bit.  A padding pixel contributes 0 to the
// summed operand (x + add is formed for in-range pixels only, rounded once).
//
// Weight gradient: thread <-> (2 output channels) x (2 input channels) x 9 taps = 36 accumulators over a slice of the flattened output
// pixels; the pixel-slice partials go to the workspace in the thread's own (coalesced) order and a second kernel adds them up in
// ascending order (no atomics) and scatters to the parameter layout (width, width, 3, 3).
#include "common.h"

namespace {

constexpr int R2_PX = 4;              // output pixels per thread (forward)
constexpr int R2_WG_THREADS = 65536;  // weight gradient: threads the split over pixels aims at (256 CUs x 256)
constexpr int R2_WG_MIN_PIX = 16;     // ... and the fewest pixels a pixel slice is worth
constexpr int R2_MAX_WIDTH = 512;

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x2 ldg2(const float* p) { return *reinterpret_cast<const f32x2*>(p); }

// OIHW (width, width, 3, 3) master -> P[tap][kp][j][pair][e]: the weight that multiplies input channel (2 kp + e) into output
// channel r = 2 pair + j at tap.
//   forward (transpose = 0): w[r][2 kp + e][tap]
//   dgrad   (transpose = 1): in / out swapped, taps flipped, the forward conv's folded scale multiplied in:
//                            w[2 kp + e][r][8 - tap] * scale[2 kp + e]
__global__ void res2_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ out, int width,
                                 int transpose) {
    const int w2 = width >> 1;
    const int total = 9 * width * width;
    for (int idx = blockIdx.x * (int)blockDim.x + (int)threadIdx.x; idx < total; idx += gridDim.x * (int)blockDim.x) {
        const int e = idx & 1;
        int t = idx >> 1;
        const int pair = t % w2; t /= w2;
        const int j = t & 1; t >>= 1;
        const int kp = t % w2;
        const int tap = t / w2;
        const int r = 2 * pair + j, k = 2 * kp + e;
        float v;
        if (transpose) v = w[((size_t)k * width + r) * 9 + (8 - tap)] * (scale ? scale[k] : 1.f);
        else v = w[((size_t)r * width + k) * 9 + tap];
        out[idx] = v;
    }
}

// up == 0: the conv proper, input map IH x IW, output OH x OW = ((IH - 1) / stride + 1, ...), tap (kh, kw) of output (oh, ow) reads
//          input (oh * stride - 1 + kh, ow * stride - 1 + kw).
// up == 1: the data gradient of a stride-2 layer in gather form: the input map (IH x IW) is the gradient at the layer's OUTPUT
//          resolution, the output map (OH x OW) has the layer's INPUT size, and tap (kh, kw) of output (oh, ow) reads the zero-inserted
//          gradient at (oh - 1 + kh, ow - 1 + kw): the gradient pixel at half those coordinates where both are even, else 0.
template <bool ADD>
__global__ __launch_bounds__(256) void res2_conv_kernel(const float* __restrict__ x, int x_pitch, int x_off,
                                                        const float* __restrict__ add, int add_pitch, int add_off,
                                                        const float* __restrict__ wp, float* __restrict__ out, int out_pitch, int out_off,
                                                        const float* __restrict__ scale, const float* __restrict__ bias, long long M,
                                                        int IH, int IW, int OH, int OW, int width, int stride, int up, int relu) {
    const int w2 = width >> 1;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int pair = (int)(gid % w2);
    const long long p0 = gid / w2 * R2_PX;
    if (p0 >= M) return;
    long long nb[R2_PX];       // first pixel of the image
    int ih0[R2_PX], iw0[R2_PX];
    bool live[R2_PX];
#pragma unroll
    for (int i = 0; i < R2_PX; ++i) {
        const long long p = p0 + i;
        live[i] = p < M;
        const long long q = live[i] ? p : M - 1;
        const int ow = (int)(q % OW);
        const long long t = q / OW;
        const int oh = (int)(t % OH);
        nb[i] = t / OH * IH * IW;
        ih0[i] = (up ? oh : oh * stride) - 1;
        iw0[i] = (up ? ow : ow * stride) - 1;
    }
    f32x2 acc[R2_PX];
#pragma unroll
    for (int i = 0; i < R2_PX; ++i) acc[i] = f32x2{0.f, 0.f};
    const f32x2* wq = reinterpret_cast<const f32x2*>(wp) + pair;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - 3 * kh;
        long long pix[R2_PX];
        bool ok[R2_PX];
#pragma unroll
        for (int i = 0; i < R2_PX; ++i) {
            int ih = ih0[i] + kh, iw = iw0[i] + kw;
            bool o = live[i] && ih >= 0 && iw >= 0;
            if (up) {
                o = o && !((ih | iw) & 1);
                ih >>= 1;
                iw >>= 1;
            }
            ok[i] = o && ih < IH && iw < IW;
            pix[i] = ok[i] ? nb[i] + (long long)ih * IW + iw : 0;
        }
        const f32x2* wr = wq + (size_t)tap * w2 * 2 * w2;
#pragma unroll 2
        for (int kp = 0; kp < w2; ++kp) {
            const f32x2 w0 = wr[(size_t)(2 * kp) * w2], w1 = wr[(size_t)(2 * kp + 1) * w2];
#pragma unroll
            for (int i = 0; i < R2_PX; ++i) {
                f32x2 v = f32x2{0.f, 0.f};
                if (ok[i]) {
                    v = ldg2(x + (size_t)pix[i] * x_pitch + x_off + 2 * kp);
                    if (ADD) {
                        const f32x2 u = ldg2(add + (size_t)pix[i] * add_pitch + add_off + 2 * kp);
                        v.x = __fadd_rn(v.x, u.x);
                        v.y = __fadd_rn(v.y, u.y);
                    }
                }
                f32x2 a = acc[i];
                a.x = fmaf(v.x, w0.x, a.x); a.x = fmaf(v.y, w0.y, a.x);
                a.y = fmaf(v.x, w1.x, a.y); a.y = fmaf(v.y, w1.y, a.y);
                acc[i] = a;
            }
        }
    }
    const int c = 2 * pair;
    const f32x2 s = scale ? ldg2(scale + c) : f32x2{1.f, 1.f};
    const f32x2 b = bias ? ldg2(bias + c) : f32x2{0.f, 0.f};
#pragma unroll
    for (int i = 0; i < R2_PX; ++i) {
        if (!live[i]) continue;
        f32x2 v = acc[i];
        if (scale) { v.x *= s.x; v.y *= s.y; }
        if (bias) { v.x += b.x; v.y += b.y; }
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); }
        *reinterpret_cast<f32x2*>(out + (size_t)(p0 + i) * out_pitch + out_off + c) = v;
    }
}

// pixel slices of the flattened output pixels for the weight gradient: a function of the launch's shapes only
struct R2WgPlan { int T, S; long long P; };
static inline R2WgPlan r2_wg_plan(long long M, int width) {
    R2WgPlan pl;
    pl.T = (width >> 1) * (width >> 1);
    long long s = R2_WG_THREADS / pl.T;
    const long long smax = cdivll(M, R2_WG_MIN_PIX);
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    pl.P = cdivll(M, s);
    pl.S = (int)cdivll(M, pl.P);
    return pl;
}

template <bool ADD>
__global__ __launch_bounds__(256) void res2_wgrad_kernel(const float* __restrict__ dy, int dy_pitch, int dy_off,
                                                         const float* __restrict__ x, int x_pitch, int x_off,
                                                         const float* __restrict__ add, int add_pitch, int add_off,
                                                         float* __restrict__ ws, long long M, int H, int W, int OH, int OW, int width,
                                                         int stride, int T, int S, long long P) {
    const int w2 = width >> 1;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int t = (int)(gid % T);
    const int s = (int)(gid / T);
    if (s >= S) return;
    const int co0 = 2 * (t % w2), ci0 = 2 * (t / w2);
    f32x2 acc[9][2];
#pragma unroll
    for (int a = 0; a < 9; ++a) acc[a][0] = acc[a][1] = f32x2{0.f, 0.f};
    const long long pbeg = (long long)s * P;
    const long long pend = pbeg + P < M ? pbeg + P : M;
    int ow = (int)(pbeg % OW);
    long long r = pbeg / OW;
    int oh = (int)(r % OH);
    long long n = r / OH;
    for (long long p = pbeg; p < pend; ++p) {
        const f32x2 d = ldg2(dy + (size_t)p * dy_pitch + dy_off + co0);
        const long long nb = n * H * W;
        const int ihb = oh * stride - 1, iwb = ow * stride - 1;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ih = ihb + tap / 3, iw = iwb + tap % 3;
            f32x2 v = f32x2{0.f, 0.f};
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
                const size_t pix = (size_t)(nb + (long long)ih * W + iw);
                v = ldg2(x + pix * x_pitch + x_off + ci0);
                if (ADD) {
                    const f32x2 u = ldg2(add + pix * add_pitch + add_off + ci0);
                    v.x = __fadd_rn(v.x, u.x);
                    v.y = __fadd_rn(v.y, u.y);
                }
            }
            f32x2* a = acc[tap];
            a[0].x = fmaf(d.x, v.x, a[0].x); a[0].y = fmaf(d.x, v.y, a[0].y);
            a[1].x = fmaf(d.y, v.x, a[1].x); a[1].y = fmaf(d.y, v.y, a[1].y);
        }
        if (++ow == OW) {
            ow = 0;
            if (++oh == OH) { oh = 0; ++n; }
        }
    }
    // pixel-slice partial in the thread's own order: ws[s][tap][j][t] float2 (e)
    f32x2* o = reinterpret_cast<f32x2*>(ws) + (size_t)s * 18 * T + t;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        o[(size_t)(tap * 2) * T] = acc[tap][0];
        o[(size_t)(tap * 2 + 1) * T] = acc[tap][1];
    }
}

// grad_w[(co * width + ci) * 9 + tap] (+)= sum over the pixel slices, ascending; one thread per entry, in the partials' order
__global__ void res2_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ grad_w, int width, int T, int S,
                                         int accumulate) {
    const int total = 36 * T;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += ws[(size_t)s * total + idx];
    const int e = idx & 1;
    int r = idx >> 1;
    const int t = r % T; r /= T;
    const int j = r & 1, tap = r >> 1;
    const int w2 = width >> 1;
    const size_t o = ((size_t)(2 * (t % w2) + j) * width + 2 * (t / w2) + e) * 9 + tap;
    grad_w[o] = accumulate ? grad_w[o] + sum : sum;
}

// The last slice of a stage block: AvgPool2d(3, stride 2, padding 1), count_include_pad -- the divisor is always 9 -- slice in, slice
// out; at stride 1 the slice is copied.  Taps are added in ascending (kh, kw) order, then one division.
__global__ void res2_pool_kernel(const float* __restrict__ x, int x_pitch, int x_off, float* __restrict__ out, int out_pitch, int out_off,
                                 long long total, int H, int W, int OH, int OW, int width, int stride) {
    const int w2 = width >> 1;
    for (long long gid = (long long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long long)gridDim.x * 256) {
        const int c = 2 * (int)(gid % w2);
        const long long p = gid / w2;
        f32x2 v;
        if (stride == 1) {
            v = ldg2(x + (size_t)p * x_pitch + x_off + c);
        } else {
            const int ow = (int)(p % OW);
            const long long t = p / OW;
            const int oh = (int)(t % OH);
            const long long nb = t / OH * H * W;
            f32x2 s = f32x2{0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ih = 2 * oh - 1 + tap / 3, iw = 2 * ow - 1 + tap % 3;
                if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
                    const f32x2 u = ldg2(x + (size_t)(nb + (long long)ih * W + iw) * x_pitch + x_off + c);
                    s.x += u.x;
                    s.y += u.y;
                }
            }
            v.x = __fdiv_rn(s.x, 9.f);
            v.y = __fdiv_rn(s.y, 9.f);
        }
        *reinterpret_cast<f32x2*>(out + (size_t)p * out_pitch + out_off + c) = v;
    }
}

// Its backward in gather form: dx(ih, iw) = (sum of the dy(oh, ow) whose window holds (ih, iw), ascending (oh, ow)) / 9.  At most
// 2 x 2 windows hold a pixel.  Stride 1: the copy.
__global__ void res2_pool_bwd_kernel(const float* __restrict__ dy, int dy_pitch, int dy_off, float* __restrict__ dx, int dx_pitch,
                                     int dx_off, long long total, int H, int W, int OH, int OW, int width, int stride) {
    const int w2 = width >> 1;
    for (long long gid = (long long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long long)gridDim.x * 256) {
        const int c = 2 * (int)(gid % w2);
        const long long p = gid / w2;
        f32x2 v;
        if (stride == 1) {
            v = ldg2(dy + (size_t)p * dy_pitch + dy_off + c);
        } else {
            const int iw = (int)(p % W);
            const long long t = p / W;
            const int ih = (int)(t % H);
            const long long nb = t / H * OH * OW;
            // windows oh with 2 oh - 1 <= ih <= 2 oh + 1: oh in [ih / 2, (ih + 1) / 2]
            f32x2 s = f32x2{0.f, 0.f};
            for (int oh = ih >> 1; oh <= ((ih + 1) >> 1); ++oh) {
                if (oh >= OH) continue;
                for (int ow = iw >> 1; ow <= ((iw + 1) >> 1); ++ow) {
                    if (ow >= OW) continue;
                    const f32x2 u = ldg2(dy + (size_t)(nb + (long long)oh * OW + ow) * dy_pitch + dy_off + c);
                    s.x += u.x;
                    s.y += u.y;
                }
            }
            v.x = __fdiv_rn(s.x, 9.f);
            v.y = __fdiv_rn(s.y, 9.f);
        }
        *reinterpret_cast<f32x2*>(dx + (size_t)p * dx_pitch + dx_off + c) = v;
    }
}

// Backward of a slice's ReLU, in place on the gradient slice: g = (G[slice] (+ carry slice)) * (y slice > 0), and the per-channel sums of
// g over the pixels.  Thread <-> (channel pair, chunk of R2_CS_PIX pixels); the chunk partials are added in ascending order by the second
// kernel (no atomics): the column sums are a function of the shapes alone.
constexpr int R2_CS_PIX = 256;
__global__ void res2_relu_bwd_kernel(float* __restrict__ g, int g_pitch, int g_off, const float* __restrict__ carry, int c_pitch, int c_off,
                                     const float* __restrict__ y, int y_pitch, int y_off, float* __restrict__ ws, long long M, int width,
                                     long long S) {
    const int w2 = width >> 1;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = 2 * (int)(gid % w2);
    const long long s = gid / w2;
    if (s >= S) return;
    const long long pend = (s + 1) * R2_CS_PIX < M ? (s + 1) * R2_CS_PIX : M;
    f32x2 sum = f32x2{0.f, 0.f};
    for (long long p = s * R2_CS_PIX; p < pend; ++p) {
        float* gp = g + (size_t)p * g_pitch + g_off + c;
        f32x2 v = ldg2(gp);
        if (carry) {
            const f32x2 u = ldg2(carry + (size_t)p * c_pitch + c_off + c);
            v.x += u.x;
            v.y += u.y;
        }
        const f32x2 m = ldg2(y + (size_t)p * y_pitch + y_off + c);
        v.x = m.x > 0.f ? v.x : 0.f;
        v.y = m.y > 0.f ? v.y : 0.f;
        *reinterpret_cast<f32x2*>(gp) = v;
        sum.x += v.x;
        sum.y += v.y;
    }
    *reinterpret_cast<f32x2*>(ws + (size_t)s * width + c) = sum;
}
__global__ void res2_colsum_reduce_kernel(const float* __restrict__ ws, float* __restrict__ colsum, int width, long long S) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= width) return;
    float sum = 0.f;
    for (long long s = 0; s < S; ++s) sum += ws[(size_t)s * width + c];
    colsum[c] = sum;
}

inline bool r2_width_ok(int width) { return width >= 2 && width <= R2_MAX_WIDTH && !(width & 1); }
// a slice [off, off + width) of a map with row pitch `pitch`, read / written as float2: inside the row, and 8-byte aligned in every row
inline bool r2_slice_ok(const void* p, int pitch, int off, int width) {
    return p && !((uintptr_t)p & 7) && pitch > 0 && !(pitch & 1) && off >= 0 && !(off & 1) && (long long)off + width <= pitch;
}
inline int r2_out(int in, int stride) { return (in - 1) / stride + 1; }

}  // namespace

extern "C" int cpr_res2_pack_weights(const float* w, const float* scale, float* out, int width, int transpose, hipStream_t stream) {
    CPR_CHECK_ARG(w && out && r2_width_ok(width) && (transpose == 0 || transpose == 1));
    const int total = 9 * width * width;
    const int grid = cdiv(total, 256) < 1024 ? cdiv(total, 256) : 1024;
    hipLaunchKernelGGL(res2_pack_kernel, dim3(grid), dim3(256), 0, stream, w, scale, out, width, transpose);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_res2_conv_fwd(const float* x, int x_pitch, int x_off, const float* add, int add_pitch, int add_off, const float* wp,
                                 float* out, int out_pitch, int out_off, const float* scale, const float* bias, int N, int IH, int IW,
                                 int OH, int OW, int width, int stride, int transposed, int flags, hipStream_t stream) {
    CPR_CHECK_ARG(wp && !((uintptr_t)wp & 7) && N > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0 && r2_width_ok(width));
    CPR_CHECK_ARG(stride == 1 || stride == 2);
    CPR_CHECK_ARG(transposed == 0 || transposed == 1);
    CPR_CHECK_ARG((flags & ~CPR_CONV_RELU) == 0);
    CPR_CHECK_ARG(r2_slice_ok(x, x_pitch, x_off, width) && r2_slice_ok(out, out_pitch, out_off, width));
    CPR_CHECK_ARG(!add || (stride == 1 && r2_slice_ok(add, add_pitch, add_off, width)));
    CPR_CHECK_ARG(!scale || !((uintptr_t)scale & 7));
    CPR_CHECK_ARG(!bias || !((uintptr_t)bias & 7));
    // the conv proper maps IH x IW -> OH x OW; the data gradient (transposed) maps the gradient at r2_out(OH) x r2_out(OW) back to OH x OW
    if (transposed) CPR_CHECK_ARG(IH == r2_out(OH, stride) && IW == r2_out(OW, stride));
    else CPR_CHECK_ARG(OH == r2_out(IH, stride) && OW == r2_out(IW, stride));
    const long long M = (long long)N * OH * OW;
    const long long blocks = cdivll(cdivll(M, R2_PX) * (width / 2), 256);
    if (blocks > 0x7fffffffll || (long long)N * IH * IW > 0x7fffffffll || M > 0x7fffffffll) return CPR_ERR_UNSUPPORTED;
    const int up = transposed && stride == 2, relu = flags & CPR_CONV_RELU;
    if (add)
        hipLaunchKernelGGL(res2_conv_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, x, x_pitch, x_off, add, add_pitch,
                           add_off, wp, out, out_pitch, out_off, scale, bias, M, IH, IW, OH, OW, width, up ? 1 : stride, up, relu);
    else
        hipLaunchKernelGGL(res2_conv_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, x, x_pitch, x_off, add, add_pitch,
                           add_off, wp, out, out_pitch, out_off, scale, bias, M, IH, IW, OH, OW, width, up ? 1 : stride, up, relu);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_res2_conv_wgrad_workspace(int N, int OH, int OW, int width) {
    CPR_CHECK_ARG(N > 0 && OH > 0 && OW > 0 && r2_width_ok(width));
    const long long M = (long long)N * OH * OW;
    const R2WgPlan pl = r2_wg_plan(M, width);
    const long long n = (long long)pl.S * pl.T * 36;
    return n < (1ll << 31) && M <= 0x7fffffffll ? (int)n : CPR_ERR_UNSUPPORTED;
}

extern "C" int cpr_res2_conv_wgrad(const float* dy, int dy_pitch, int dy_off, const float* x, int x_pitch, int x_off, const float* add,
                                   int add_pitch, int add_off, float* grad_w, float* ws, int N, int H, int W, int width, int stride,
                                   int accumulate, hipStream_t stream) {
    CPR_CHECK_ARG(grad_w && ws && !((uintptr_t)ws & 7) && N > 0 && H > 0 && W > 0 && r2_width_ok(width));
    CPR_CHECK_ARG(stride == 1 || stride == 2);
    CPR_CHECK_ARG(r2_slice_ok(dy, dy_pitch, dy_off, width) && r2_slice_ok(x, x_pitch, x_off, width));
    CPR_CHECK_ARG(!add || (stride == 1 && r2_slice_ok(add, add_pitch, add_off, width)));
    const int OH = r2_out(H, stride), OW = r2_out(W, stride);
    const long long M = (long long)N * OH * OW;
    const R2WgPlan pl = r2_wg_plan(M, width);
    // the workspace index and the pixel index of both maps (M <= N * H * W) stay inside int
    if ((long long)pl.S * pl.T * 36 >= (1ll << 31) || (long long)N * H * W > 0x7fffffffll || M > 0x7fffffffll) return CPR_ERR_UNSUPPORTED;
    const long long threads = (long long)pl.S * pl.T;
    const unsigned grid = (unsigned)cdivll(threads, 256);
    if (add)
        hipLaunchKernelGGL(res2_wgrad_kernel<true>, dim3(grid), dim3(256), 0, stream, dy, dy_pitch, dy_off, x, x_pitch, x_off, add,
                           add_pitch, add_off, ws, M, H, W, OH, OW, width, stride, pl.T, pl.S, pl.P);
    else
        hipLaunchKernelGGL(res2_wgrad_kernel<false>, dim3(grid), dim3(256), 0, stream, dy, dy_pitch, dy_off, x, x_pitch, x_off, add,
                           add_pitch, add_off, ws, M, H, W, OH, OW, width, stride, pl.T, pl.S, pl.P);
    hipLaunchKernelGGL(res2_wgrad_reduce_kernel, dim3(cdiv(36 * pl.T, 256)), dim3(256), 0, stream, ws, grad_w, width, pl.T, pl.S,
                       accumulate);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_res2_pool_fwd(const float* x, int x_pitch, int x_off, float* out, int out_pitch, int out_off, int N, int H, int W,
                                 int width, int stride, hipStream_t stream) {
    CPR_CHECK_ARG(N > 0 && H > 0 && W > 0 && r2_width_ok(width) && (stride == 1 || stride == 2));
    CPR_CHECK_ARG(r2_slice_ok(x, x_pitch, x_off, width) && r2_slice_ok(out, out_pitch, out_off, width));
    const int OH = r2_out(H, stride), OW = r2_out(W, stride);
    const long long total = (long long)N * OH * OW * (width / 2);
    // the pixel index of the larger map stays inside int (the kernel's own index is 64-bit and grid-strided)
    if ((long long)N * H * W > 0x7fffffffll) return CPR_ERR_UNSUPPORTED;
    const long long blocks = cdivll(total, 256);
    hipLaunchKernelGGL(res2_pool_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, x, x_pitch, x_off, out,
                       out_pitch, out_off, total, H, W, OH, OW, width, stride);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_res2_pool_bwd(const float* dy, int dy_pitch, int dy_off, float* dx, int dx_pitch, int dx_off, int N, int H, int W,
                                 int width, int stride, hipStream_t stream) {
    CPR_CHECK_ARG(N > 0 && H > 0 && W > 0 && r2_width_ok(width) && (stride == 1 || stride == 2));
    CPR_CHECK_ARG(r2_slice_ok(dy, dy_pitch, dy_off, width) && r2_slice_ok(dx, dx_pitch, dx_off, width));
    const int OH = r2_out(H, stride), OW = r2_out(W, stride);
    const long long total = (long long)N * H * W * (width / 2);
    // the pixel index of the larger map stays inside int (the kernel's own index is 64-bit and grid-strided)
    if ((long long)N * H * W > 0x7fffffffll) return CPR_ERR_UNSUPPORTED;
    const long long blocks = cdivll(total, 256);
    hipLaunchKernelGGL(res2_pool_bwd_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, dy, dy_pitch, dy_off,
                       dx, dx_pitch, dx_off, total, H, W, OH, OW, width, stride);
    CPR_LAUNCH_STATUS();
}

// floats of workspace cpr_res2_relu_bwd_colsum needs for M pixels of a slice: one row of `width` partials per chunk of R2_CS_PIX pixels
extern "C" int cpr_res2_relu_bwd_colsum_ws(long long M, int width) {
    if (M <= 0 || !r2_width_ok(width)) return CPR_ERR_ARG;
    if (M > 0x7fffffffll) return CPR_ERR_UNSUPPORTED;
    const long long n = cdivll(M, R2_CS_PIX) * width;
    return n < (1ll << 31) ? (int)n : CPR_ERR_UNSUPPORTED;
}

// g slice (in place) = (g slice (+ carry slice)) * (y slice > 0); colsum[width] = its per-channel sums over the M pixels.  carry may be NULL.
extern "C" int cpr_res2_relu_bwd_colsum(float* g, int g_pitch, int g_off, const float* carry, int c_pitch, int c_off, const float* y,
                                        int y_pitch, int y_off, float* colsum, float* ws, long long M, int width, hipStream_t stream) {
    CPR_CHECK_ARG(colsum && ws && !((uintptr_t)ws & 7) && M > 0 && r2_width_ok(width));
    CPR_CHECK_ARG(r2_slice_ok(g, g_pitch, g_off, width) && r2_slice_ok(y, y_pitch, y_off, width));
    CPR_CHECK_ARG(!carry || r2_slice_ok(carry, c_pitch, c_off, width));
    if (M > 0x7fffffffll) return CPR_ERR_UNSUPPORTED;      // the pixel index of every map stays inside int
    const long long S = cdivll(M, R2_CS_PIX);
    hipLaunchKernelGGL(res2_relu_bwd_kernel, dim3((unsigned)cdivll(S * (width / 2), 256)), dim3(256), 0, stream, g, g_pitch, g_off, carry,
                       c_pitch, c_off, y, y_pitch, y_off, ws, M, width, S);
    hipLaunchKernelGGL(res2_colsum_reduce_kernel, dim3(cdiv(width, 256)), dim3(256), 0, stream, ws, colsum, width, S);
    CPR_LAUNCH_STATUS();
}
