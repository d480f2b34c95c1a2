// Grouped 3x3 convolution (ResNeXt conv2: C -> C channels in G = C / cg groups, padding 1, stride 1 or 2), NHWC fp32: forward, data
// gradient (the same kernel over dy with the data-gradient pack) and weight gradient.
//
// Plain fp32 FMA, the exact work and nothing else: an output channel is multiplied against the cg input channels of its own group, 9 * cg
// FMAs per output (cg in {4, 8, 16, 24, 32, 40, 48, 56}: never another group's input channels -- group isolation holds by construction,
// not by zero weights).  A block-diagonal 32-wide MFMA tile would execute 32 / cg times the multiplies (8x at the
// 32x4d layer1 width).  Measured (profiles/resnext_bench.json): 0.6 .. 0.9 ms per layer of a 64 x 640^2 x50_32x4d forward,
// 17 .. 25 TFLOP/s executed -- bound by the vector pipe behind its loads, not by HBM.
//
// Thread mapping (forward): lane <-> 4 consecutive output channels, consecutive lanes <-> consecutive channel quads of ONE pixel, so every
// activation load / store of a wave is one contiguous run of the NHWC row (cg = 4: lane c reads exactly the float4 it owns; cg = 32: the
// 8 lanes of a group read the same 8 float4s, a broadcast).  A thread keeps 4 channels x GC_PX pixels of accumulators and walks
// tap -> 4-channel input chunk; the weights of a chunk (4 float4 per thread) are reused over the GC_PX pixels.  The pack stores them so
// that this load is contiguous over the lanes too: P[tap][chunk][j][C/4 quads] float4 (see pack_group_body).
// Accumulation order of an output: tap-major, input channel ascending, one fmaf each -- a function of nothing but the layer, so an image
// of a batch equals its single-image run bit for bit and two runs agree bit for bit.
//
// Weight gradient: thread <-> (4 output channels) x (4 input channels of their group) x 9 taps = 144 accumulators, over a slice of
// the flattened output pixels; slice partials go to the workspace in the thread's own (coalesced) order and a second kernel adds the
// slices up in ascending order (no atomics) and scatters to the parameter layout (C, cg, 3, 3).
//
// Channel pitch (RegNet: stage widths such as 72, 168, 432 that are no multiple of 32): the PITCH instances read and write maps whose
// pixels are Cp >= C floats apart (Cp = roundup(C, 32) in the product).  The pad channels [C, Cp) of an input are never read -- the
// threads of the pad quads take no part in the sums, so NaN there changes no output bit -- and the pad channels of the output are
// written as +0.0 by the kernel itself.  The pack, the workspace and the parameter gradient know nothing of the pitch.  Cp == C with
// one of the widths 4 / 8 / 16 / 32 launches the instances without the pitch argument, as before.
//
// Dilation (a dilated ResNeXt stage: stride 1, padding d, tap step d): the DIL instances start at ih0 = oh - d and step d pixels per tap;
// nothing else changes -- 9 * cg FMAs per output in the same tap-major order, so the bit-repeatability and batch independence above hold.
// Unpitched maps only.  The tap step is a compile-time 1 in every other instance.
#include "common.h"

namespace {

constexpr int GC_PX = 4;              // output pixels per thread (forward)
constexpr int GC_WG_THREADS = 65536;  // weight gradient: threads the split over pixels aims at (256 CUs x 256)
constexpr int GC_WG_MIN_PIX = 16;     // ... and the fewest pixels a slice is worth

__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// OIHW (C, cg, 3, 3) master -> P[tap][chunk][j][quad][e]: the weight that multiplies input channel (4 chunk + e) of the group into
// output channel r = 4 quad + j at tap.
//   forward  (transpose = 0): w[r][4 chunk + e][tap]
//   dgrad    (transpose = 1): per group in / out swapped, taps flipped, the forward conv's folded scale multiplied in:
//                             w[g0 + 4 chunk + e][r - g0][8 - tap] * scale[g0 + 4 chunk + e],  g0 = first channel of r's group
__device__ __forceinline__ void pack_group_body(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ out,
                                                int C, int cg, int transpose, int block, int nblocks) {
    const int C4 = C >> 2, chunks = cg >> 2;
    const int total = 9 * cg * C;
    for (int idx = block * (int)blockDim.x + (int)threadIdx.x; idx < total; idx += nblocks * (int)blockDim.x) {
        const int e = idx & 3;
        int t = idx >> 2;
        const int quad = t % C4; t /= C4;
        const int j = t & 3; t >>= 2;
        const int chunk = t % chunks;
        const int tap = t / chunks;
        const int r = 4 * quad + j, g0 = r / cg * cg, k = 4 * chunk + e;
        float v;
        if (transpose) v = w[((size_t)(g0 + k) * cg + (r - g0)) * 9 + (8 - tap)] * (scale ? scale[g0 + k] : 1.f);
        else v = w[((size_t)r * cg + k) * 9 + tap];
        out[idx] = v;
    }
}
__global__ void pack_group_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ out, int C, int cg,
                                  int transpose) {
    pack_group_body(w, scale, out, C, cg, transpose, blockIdx.x, gridDim.x);
}
struct GroupPackJob {      // 48 bytes; jobs in ascending block0
    const float* w; const float* scale; float* out;
    int C, cg, transpose, block0, nblocks, pad;
};
__global__ void pack_group_multi_kernel(const GroupPackJob* __restrict__ jobs, int n) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const GroupPackJob j = jobs[lo];
    pack_group_body(j.w, j.scale, j.out, j.C, j.cg, j.transpose, (int)blockIdx.x - j.block0, j.nblocks);
}

template <int CG, bool PITCH, bool DIL = false>
__global__ __launch_bounds__(256) void conv_group_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                             float* __restrict__ out, const float* __restrict__ scale,
                                                             const float* __restrict__ bias, long long M, int H, int W, int OH, int OW,
                                                             int C, int pitch, int stride, int relu, int dil) {
    static_assert(!(DIL && PITCH), "the dilated instances read unpitched maps");
    constexpr int CH = CG / 4, UNR = CH > 2 ? 2 : CH;
    const int dl = DIL ? dil : 1;                     // tap step = padding
    const int C4 = C >> 2;                            // quads of the pack: the real channels
    const int Cp = PITCH ? pitch : C;                 // floats between the pixels of x and of out
    const int Q = Cp >> 2;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int quad = (int)(gid % Q);
    const long long p0 = gid / Q * GC_PX;
    if (p0 >= M) return;
    if (PITCH && quad >= C4) {                        // a pad quad: exact zeros out, nothing read
#pragma unroll
        for (int i = 0; i < GC_PX; ++i)
            if (p0 + i < M) *reinterpret_cast<f32x4*>(out + (size_t)(p0 + i) * Cp + quad * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const int g0 = quad * 4 / CG * CG;                // first input channel of this thread's group
    const float* xb[GC_PX];
    int ih0[GC_PX], iw0[GC_PX];
    bool live[GC_PX];
#pragma unroll
    for (int i = 0; i < GC_PX; ++i) {
        const long long p = p0 + i;
        live[i] = p < M;
        const long long q = live[i] ? p : M - 1;
        const int ow = (int)(q % OW);
        const long long t = q / OW;
        const int oh = (int)(t % OH);
        const long long n = t / OH;
        ih0[i] = oh * stride - dl;
        iw0[i] = ow * stride - dl;
        xb[i] = x + (size_t)n * H * W * Cp + g0;
    }
    f32x4 acc[GC_PX];
#pragma unroll
    for (int i = 0; i < GC_PX; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4* wq = reinterpret_cast<const f32x4*>(wp) + quad;
#pragma unroll 1      // (unrolled, the scheduler hoists all 9 taps' loads and spills)
    for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - 3 * kh;
        const float* src[GC_PX];
        bool ok[GC_PX];
#pragma unroll
        for (int i = 0; i < GC_PX; ++i) {
            const int ih = ih0[i] + kh * dl, iw = iw0[i] + kw * dl;
            ok[i] = live[i] && ih >= 0 && ih < H && iw >= 0 && iw < W;
            src[i] = xb[i] + ((size_t)(ok[i] ? ih : 0) * W + (ok[i] ? iw : 0)) * Cp;
        }
#pragma unroll UNR
        for (int ch = 0; ch < CH; ++ch) {
            const f32x4* wr = wq + (size_t)((tap * CH + ch) * 4) * C4;
            const f32x4 w0 = wr[0], w1 = wr[C4], w2 = wr[2 * C4], w3 = wr[3 * C4];
#pragma unroll
            for (int i = 0; i < GC_PX; ++i) {
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (ok[i]) v = ldg4(src[i] + 4 * ch);
                f32x4 a = acc[i];
                a.x = fmaf(v.x, w0.x, a.x); a.x = fmaf(v.y, w0.y, a.x); a.x = fmaf(v.z, w0.z, a.x); a.x = fmaf(v.w, w0.w, a.x);
                a.y = fmaf(v.x, w1.x, a.y); a.y = fmaf(v.y, w1.y, a.y); a.y = fmaf(v.z, w1.z, a.y); a.y = fmaf(v.w, w1.w, a.y);
                a.z = fmaf(v.x, w2.x, a.z); a.z = fmaf(v.y, w2.y, a.z); a.z = fmaf(v.z, w2.z, a.z); a.z = fmaf(v.w, w2.w, a.z);
                a.w = fmaf(v.x, w3.x, a.w); a.w = fmaf(v.y, w3.y, a.w); a.w = fmaf(v.z, w3.z, a.w); a.w = fmaf(v.w, w3.w, a.w);
                acc[i] = a;
            }
        }
    }
    const int c = quad * 4;
    const f32x4 one = f32x4{1.f, 1.f, 1.f, 1.f}, zero = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 s = scale ? ldg4(scale + c) : one;
    const f32x4 b = bias ? ldg4(bias + c) : zero;
#pragma unroll
    for (int i = 0; i < GC_PX; ++i) {
        if (!live[i]) continue;
        f32x4 v = acc[i];
        if (scale) { v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w; }
        if (bias) { v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        *reinterpret_cast<f32x4*>(out + (size_t)(p0 + i) * Cp + c) = v;
    }
}

// slices of the flattened output pixels for the weight gradient: a function of the launch's shapes only
struct WgPlan { int T, S; long long P; };
static inline WgPlan wg_plan(long long M, int C, int cg) {
    WgPlan pl;
    pl.T = (C >> 2) * (cg >> 2);
    long long s = GC_WG_THREADS / pl.T;
    const long long smax = cdivll(M, GC_WG_MIN_PIX);
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    pl.P = cdivll(M, s);
    pl.S = (int)cdivll(M, pl.P);
    return pl;
}

template <bool PITCH, bool DIL = false>
__global__ __launch_bounds__(256, 2) void conv_group_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               float* __restrict__ ws, long long M, int H, int W, int OH, int OW, int C,
                                                               int pitch, int cg, int stride, int T, int S, long long P, int dil) {
    static_assert(!(DIL && PITCH), "the dilated instance reads unpitched maps");
    const int dl = DIL ? dil : 1;                     // tap step = padding
    const int C4 = C >> 2;
    const int Cp = PITCH ? pitch : C;                 // floats between the pixels of dy and of x; the threads cover real channels only
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int t = (int)(gid % T);
    const int s = (int)(gid / T);
    if (s >= S) return;
    const int quad = t % C4, ib = t / C4;
    const int co0 = 4 * quad;
    const int ci0 = co0 / cg * cg + 4 * ib;
    f32x4 acc[9][4];
#pragma unroll
    for (int a = 0; a < 9; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long long pbeg = (long long)s * P;
    const long long pend = pbeg + P < M ? pbeg + P : M;
    int ow = (int)(pbeg % OW);
    long long r = pbeg / OW;
    int oh = (int)(r % OH);
    long long n = r / OH;
    for (long long p = pbeg; p < pend; ++p) {
        const f32x4 d = ldg4(dy + (size_t)p * Cp + co0);
        const float* xn = x + (size_t)n * H * W * Cp + ci0;
        const int ihb = oh * stride - dl, iwb = ow * stride - dl;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ih = ihb + (tap / 3) * dl, iw = iwb + (tap % 3) * dl;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = ldg4(xn + ((size_t)ih * W + iw) * Cp);
            f32x4* a = acc[tap];
            a[0].x = fmaf(d.x, v.x, a[0].x); a[0].y = fmaf(d.x, v.y, a[0].y); a[0].z = fmaf(d.x, v.z, a[0].z); a[0].w = fmaf(d.x, v.w, a[0].w);
            a[1].x = fmaf(d.y, v.x, a[1].x); a[1].y = fmaf(d.y, v.y, a[1].y); a[1].z = fmaf(d.y, v.z, a[1].z); a[1].w = fmaf(d.y, v.w, a[1].w);
            a[2].x = fmaf(d.z, v.x, a[2].x); a[2].y = fmaf(d.z, v.y, a[2].y); a[2].z = fmaf(d.z, v.z, a[2].z); a[2].w = fmaf(d.z, v.w, a[2].w);
            a[3].x = fmaf(d.w, v.x, a[3].x); a[3].y = fmaf(d.w, v.y, a[3].y); a[3].z = fmaf(d.w, v.z, a[3].z); a[3].w = fmaf(d.w, v.w, a[3].w);
        }
        if (++ow == OW) {
            ow = 0;
            if (++oh == OH) { oh = 0; ++n; }
        }
    }
    // slice partial in the thread's own order: ws[s][tap][j][t] float4 (e)
    f32x4* o = reinterpret_cast<f32x4*>(ws) + (size_t)s * 36 * T + t;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[(size_t)(tap * 4 + j) * T] = acc[tap][j];
}

// grad_w[(co * cg + ci) * 9 + tap] (+)= sum over the slices, ascending; one thread per entry, in the partials' order (coalesced reads)
__global__ void conv_group_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ grad_w, int C, int cg, int T, int S,
                                               int accumulate) {
    const int total = 144 * T;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += ws[(size_t)s * total + idx];
    const int e = idx & 3;
    int r = idx >> 2;
    const int t = r % T; r /= T;
    const int j = r & 3, tap = r >> 2;
    const int C4 = C >> 2;
    const int quad = t % C4, ib = t / C4;
    const size_t o = ((size_t)(4 * quad + j) * cg + 4 * ib + e) * 9 + tap;
    grad_w[o] = accumulate ? grad_w[o] + sum : sum;
}

inline bool group_shape_ok(int C, int cg) {
    return (cg == 4 || (cg >= 8 && cg <= 56 && cg % 8 == 0)) && C > 0 && C % cg == 0 && C / 4 <= (1 << 20);
}
inline bool group_pitch_ok(int C, int Cp) { return Cp >= C && Cp % 4 == 0 && Cp / 4 <= (1 << 20); }
inline bool group_plain(int C, int Cp, int cg) { return Cp == C && (cg == 4 || cg == 8 || cg == 16 || cg == 32); }

int group_fwd(const float* x, const float* wp, float* out, const float* scale, const float* bias, int N, int H, int W, int C, int Cp,
              int cg, int stride, int flags, hipStream_t stream, int dil = 1) {
    CPR_CHECK_ARG(dil >= 1 && (dil == 1 || (stride == 1 && Cp == C)));      // dilated: stride 1 (OH = H with padding dil), unpitched
    CPR_CHECK_ARG(x && wp && out && N > 0 && H > 0 && W > 0 && group_shape_ok(C, cg) && group_pitch_ok(C, Cp) &&
                  (stride == 1 || stride == 2));
    CPR_CHECK_ARG((flags & ~CPR_CONV_RELU) == 0);      // no residual, no GroupNorm statistics, no bf16 output: ReLU is the only flag
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const long long M = (long long)N * OH * OW;
    const long long blocks = cdivll(cdivll(M, GC_PX) * (Cp / 4), 256);
    if (blocks > 0x7fffffffll) return CPR_ERR_UNSUPPORTED;
    const int relu = flags & CPR_CONV_RELU;
#define GC_LAUNCH(CG, PITCH)                                                                                                       \
    hipLaunchKernelGGL((conv_group_fwd_kernel<CG, PITCH>), dim3((unsigned)blocks), dim3(256), 0, stream, x, wp, out, scale, bias, M, H, \
                       W, OH, OW, C, Cp, stride, relu, dil)
    if (dil > 1) {
#define GC_LAUNCH_DIL(CG)                                                                                                          \
    hipLaunchKernelGGL((conv_group_fwd_kernel<CG, false, true>), dim3((unsigned)blocks), dim3(256), 0, stream, x, wp, out, scale, bias, \
                       M, H, W, OH, OW, C, Cp, stride, relu, dil)
        switch (cg) {
            case 4: GC_LAUNCH_DIL(4); break;
            case 8: GC_LAUNCH_DIL(8); break;
            case 16: GC_LAUNCH_DIL(16); break;
            case 24: GC_LAUNCH_DIL(24); break;
            case 32: GC_LAUNCH_DIL(32); break;
            case 40: GC_LAUNCH_DIL(40); break;
            case 48: GC_LAUNCH_DIL(48); break;
            default: GC_LAUNCH_DIL(56); break;
        }
#undef GC_LAUNCH_DIL
    } else if (group_plain(C, Cp, cg)) {
        switch (cg) {
            case 4: GC_LAUNCH(4, false); break;
            case 8: GC_LAUNCH(8, false); break;
            case 16: GC_LAUNCH(16, false); break;
            default: GC_LAUNCH(32, false); break;
        }
    } else {
        switch (cg) {
            case 4: GC_LAUNCH(4, true); break;
            case 8: GC_LAUNCH(8, true); break;
            case 16: GC_LAUNCH(16, true); break;
            case 24: GC_LAUNCH(24, true); break;
            case 32: GC_LAUNCH(32, true); break;
            case 40: GC_LAUNCH(40, true); break;
            case 48: GC_LAUNCH(48, true); break;
            default: GC_LAUNCH(56, true); break;
        }
    }
#undef GC_LAUNCH
    CPR_LAUNCH_STATUS();
}

}  // namespace

extern "C" int cpr_pack_weights_grouped(const float* w, const float* scale, float* out, int C, int cg, int transpose,
                                        hipStream_t stream) {
    CPR_CHECK_ARG(w && out && group_shape_ok(C, cg));
    const int total = 9 * cg * C;
    const int grid = cdiv(total, 256) < 1024 ? cdiv(total, 256) : 1024;
    hipLaunchKernelGGL(pack_group_kernel, dim3(grid), dim3(256), 0, stream, w, scale, out, C, cg, transpose);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_pack_weights_grouped_multi(const void* jobs_dev, int n, int total_blocks, hipStream_t stream) {
    CPR_CHECK_ARG(jobs_dev && n > 0 && total_blocks > 0);
    hipLaunchKernelGGL(pack_group_multi_kernel, dim3(total_blocks), dim3(256), 0, stream, (const GroupPackJob*)jobs_dev, n);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_conv_group_fwd(const float* x, const float* wp, float* out, const float* scale, const float* bias, int N, int H,
                                  int W, int C, int cg, int stride, int flags, hipStream_t stream) {
    return group_fwd(x, wp, out, scale, bias, N, H, W, C, C, cg, stride, flags, stream);
}
// the same over maps whose pixels are Cp floats apart (Cp >= C, Cp % 4 == 0): pad channels never read, written as +0.0
extern "C" int cpr_conv_group_fwd_pitch(const float* x, const float* wp, float* out, const float* scale, const float* bias, int N, int H,
                                        int W, int C, int Cp, int cg, int stride, int flags, hipStream_t stream) {
    return group_fwd(x, wp, out, scale, bias, N, H, W, C, Cp, cg, stride, flags, stream);
}

extern "C" int cpr_conv_group_wgrad_workspace(int N, int OH, int OW, int C, int cg) {
    CPR_CHECK_ARG(N > 0 && OH > 0 && OW > 0 && group_shape_ok(C, cg));
    const WgPlan pl = wg_plan((long long)N * OH * OW, C, cg);
    const long long n = (long long)pl.S * pl.T * 144;
    return n < (1ll << 31) ? (int)n : CPR_ERR_UNSUPPORTED;
}

static int group_wgrad(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int Cp, int cg, int stride,
                       int accumulate, hipStream_t stream, int dil = 1) {
    CPR_CHECK_ARG(dil >= 1 && (dil == 1 || (stride == 1 && Cp == C)));
    CPR_CHECK_ARG(dy && x && grad_w && ws && N > 0 && H > 0 && W > 0 && group_shape_ok(C, cg) && group_pitch_ok(C, Cp) &&
                  (stride == 1 || stride == 2));
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const long long M = (long long)N * OH * OW;
    const WgPlan pl = wg_plan(M, C, cg);
    if ((long long)pl.S * pl.T * 144 >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    const long long threads = (long long)pl.S * pl.T;
    if (dil > 1)
        hipLaunchKernelGGL((conv_group_wgrad_kernel<false, true>), dim3((unsigned)cdivll(threads, 256)), dim3(256), 0, stream, dy, x, ws, M,
                           H, W, OH, OW, C, Cp, cg, stride, pl.T, pl.S, pl.P, dil);
    else if (Cp == C)
        hipLaunchKernelGGL(conv_group_wgrad_kernel<false>, dim3((unsigned)cdivll(threads, 256)), dim3(256), 0, stream, dy, x, ws, M, H, W,
                           OH, OW, C, Cp, cg, stride, pl.T, pl.S, pl.P, 1);
    else
        hipLaunchKernelGGL(conv_group_wgrad_kernel<true>, dim3((unsigned)cdivll(threads, 256)), dim3(256), 0, stream, dy, x, ws, M, H, W,
                           OH, OW, C, Cp, cg, stride, pl.T, pl.S, pl.P, 1);
    hipLaunchKernelGGL(conv_group_wgrad_reduce_kernel, dim3(cdiv(144 * pl.T, 256)), dim3(256), 0, stream, ws, grad_w, C, cg, pl.T, pl.S,
                       accumulate);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_conv_group_wgrad(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int cg,
                                    int stride, int accumulate, hipStream_t stream) {
    return group_wgrad(dy, x, grad_w, ws, N, H, W, C, C, cg, stride, accumulate, stream);
}
// the same with dy and x at pitch Cp; workspace and grad_w as for cpr_conv_group_wgrad (they depend on C and cg alone)
extern "C" int cpr_conv_group_wgrad_pitch(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int Cp,
                                          int cg, int stride, int accumulate, hipStream_t stream) {
    return group_wgrad(dy, x, grad_w, ws, N, H, W, C, Cp, cg, stride, accumulate, stream);
}

// Dilated grouped 3x3 (stride 1, padding = tap step = dil >= 1, unpitched maps; a dilated ResNeXt stage): forward -- and, with the
// data-gradient pack over dy, the data gradient -- and weight gradient.  Same packs, same workspace query, same accumulation order as
// the undilated entries; dil == 1 launches exactly what they launch.
extern "C" int cpr_conv_group_fwd_dil(const float* x, const float* wp, float* out, const float* scale, const float* bias, int N, int H,
                                      int W, int C, int cg, int dil, int flags, hipStream_t stream) {
    return group_fwd(x, wp, out, scale, bias, N, H, W, C, C, cg, 1, flags, stream, dil);
}
extern "C" int cpr_conv_group_wgrad_dil(const float* dy, const float* x, float* grad_w, float* ws, int N, int H, int W, int C, int cg,
                                        int dil, int accumulate, hipStream_t stream) {
    return group_wgrad(dy, x, grad_w, ws, N, H, W, C, C, cg, 1, accumulate, stream, dil);
}
