// Weight gradient of the 3x3 / stride 2 / pad 1 stem conv, 3 -> 32 (the RegNet stem, T/mmdet/models/backbones/regnet.py:237-249, and the
// first conv of the deep stem, resnet.py:566-575): gw (32, 3, 3, 3) = sum over the output pixels of dy (N, OH, OW, 32) x the image as the
// forward read it (layout 0: (N, H, W, 4) fp32, 4th channel ignored; layout 1: (N, 3, H, W) fp32 planes).
//
// 864 outputs against millions of pixels: 2 * 864 FLOP per pixel read of 128 + 9 * 12 bytes (the image taps hit in L1 / L2), so the
// kernel is expected to be bound by its load issue, not by arithmetic (by counting; its time is in profiles/regnet_bench.json, no
// counter run has confirmed the bound) -- plain fp32 FMA, no matrix pipe (the 64 x 147 gradient of the 7x7 stem is 11x
// the work per pixel and does use it, csrc/stem_bwd.hip).  A workgroup of 288 threads owns one slice of the flattened output pixels:
// thread (tap, cout) keeps the three input channels' sums and walks the slice pixel by pixel -- its dy load is one contiguous 128-byte
// row per 32 lanes, its image load one 16-byte pixel (or three plane reads) shared by those 32 lanes.  Slice partials go to
// ws[slice][tap][cin][cout]; stem3x3_wgrad_reduce_kernel adds them in ascending slice order and scatters to the parameter layout.
// No atomics: a result is a function of the shapes and the operands alone.
#include "common.h"

namespace {

constexpr int S3_THREADS = 288;       // 9 taps x 32 couts
constexpr int S3_OUT = 864;           // 32 x 3 x 3 x 3
constexpr int S3_MAX_SLICES = 2048;   // 8 workgroups per CU
constexpr int S3_MIN_PIX = 64;        // the fewest pixels a slice is worth

struct S3Plan { int S; long long P; };
inline S3Plan s3_plan(long long M) {
    S3Plan pl;
    long long s = cdivll(M, S3_MIN_PIX);
    if (s > S3_MAX_SLICES) s = S3_MAX_SLICES;
    pl.P = cdivll(M, s);
    pl.S = (int)cdivll(M, pl.P);
    return pl;
}

template <int LAYOUT>
__global__ __launch_bounds__(S3_THREADS) void stem3x3_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ in,
                                                                   float* __restrict__ ws, long long M, int H, int W, int OH, int OW,
                                                                   long long P) {
    const int co = threadIdx.x & 31, tap = threadIdx.x >> 5;
    const int kh = tap / 3, kw = tap - 3 * kh;
    const long long pbeg = (long long)blockIdx.x * P;
    const long long pend = pbeg + P < M ? pbeg + P : M;
    const size_t plane = (size_t)H * W;
    int ow = (int)(pbeg % OW);
    long long r = pbeg / OW;
    int oh = (int)(r % OH);
    long long n = r / OH;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll 4
    for (long long p = pbeg; p < pend; ++p) {
        const float d = dy[(size_t)p * 32 + co];
        const int ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
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
        if (++ow == OW) {
            ow = 0;
            if (++oh == OH) { oh = 0; ++n; }
        }
    }
    float* o = ws + (size_t)blockIdx.x * S3_OUT + tap * 96 + co;
    o[0] = a0; o[32] = a1; o[64] = a2;
}

// gw[(co * 3 + ci) * 9 + tap] = sum over the slices, ascending
__global__ void stem3x3_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, int S) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= S3_OUT) return;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += ws[(size_t)s * S3_OUT + idx];
    const int co = idx & 31, ci = (idx >> 5) % 3, tap = idx / 96;
    gw[(co * 3 + ci) * 9 + tap] = sum;
}

}  // namespace

// workspace floats of cpr_stem3x3s2_wgrad for an (N, 3, H, W) image
extern "C" int cpr_stem3x3s2_wgrad_workspace(int N, int H, int W) {
    CPR_CHECK_ARG(N > 0 && H > 0 && W > 0);
    const long long M = (long long)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    return s3_plan(M).S * S3_OUT;
}

// dy (N, OH, OW, 32), OH = (H - 1) / 2 + 1; in: the image (layout 0 NHWC4 / 1 planes); gw (32, 3, 3, 3) written; ws: the query's floats
extern "C" int cpr_stem3x3s2_wgrad(const float* dy, const float* in, float* gw, float* ws, int N, int H, int W, int layout,
                                   hipStream_t stream) {
    CPR_CHECK_ARG(dy && in && gw && ws && N > 0 && H > 0 && W > 0 && (layout == 0 || layout == 1));
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const long long M = (long long)N * OH * OW;
    const S3Plan pl = s3_plan(M);
    if (layout)
        hipLaunchKernelGGL(stem3x3_wgrad_kernel<1>, dim3(pl.S), dim3(S3_THREADS), 0, stream, dy, in, ws, M, H, W, OH, OW, pl.P);
    else
        hipLaunchKernelGGL(stem3x3_wgrad_kernel<0>, dim3(pl.S), dim3(S3_THREADS), 0, stream, dy, in, ws, M, H, W, OH, OW, pl.P);
    hipLaunchKernelGGL(stem3x3_wgrad_reduce_kernel, dim3(cdiv(S3_OUT, 256)), dim3(256), 0, stream, ws, gw, pl.S);
    CPR_LAUNCH_STATUS();
}
