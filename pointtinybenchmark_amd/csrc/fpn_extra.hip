// FPN extra pyramid levels (num_outs > backbone laterals; T/mmdet/models/necks/fpn.py:195-217): small streaming kernels, one pass
// each, 16 bytes of channels per lane (4 fp32 / 8 bf16), NHWC.
//   cpr_subsample2          out[n,i,j,:] = y[n,2i,2j,:], y = x or x*a[n,c]+b[n,c] (the producer's pending GroupNorm affine, applied on
//                           load with gn_apply's own expression) -- F.max_pool2d(y, 1, stride=2): pure selection, (H+1)/2 x (W+1)/2
//   cpr_subsample2_bwd_add  out = dfine + zero_insert(dcoarse): the max-pool level's gradient joins the finer output's in one
//                           pass (no memset + scatter); one add per element at even (y, x), a copy elsewhere
//   cpr_relu_mask_add       out = dz + (y > 0 ? d : 0): relu_before_extra_convs -- the output level that feeds the next extra conv
//                           through a ReLU receives its head gradient plus the masked data gradient of that conv
#include "common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

__device__ __forceinline__ void widen8(const uint4 u, f32x4& v0, f32x4& v1) {
    v0 = f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
    v1 = f32x4{__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u), __uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u)};
}

// one lane per (output pixel, 16-byte channel vector); CV = C/4 (fp32) or C/8 (bf16)
template <bool BF16>
__global__ __launch_bounds__(256) void subsample2_kernel(const void* __restrict__ xin, const float* __restrict__ a,
                                                         const float* __restrict__ b, void* __restrict__ yout, int N, int H, int W,
                                                         int OH, int OW, int CV) {
    const long long total = (long long)N * OH * OW * CV;
    const int C = CV * (BF16 ? 8 : 4);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV);
        long long r = i / CV;
        const int ox = (int)(r % OW);
        r /= OW;
        const int oy = (int)(r % OH);
        const int n = (int)(r / OH);
        const size_t src = (((size_t)n * H + 2 * oy) * W + 2 * ox) * CV + c;
        if (BF16) {
            uint4 u = reinterpret_cast<const uint4*>(xin)[src];
            if (a) {
                f32x4 v0, v1;
                widen8(u, v0, v1);
                const float* ap = a + (size_t)n * C + c * 8;
                const float* bp = b + (size_t)n * C + c * 8;
                v0 = v0 * *reinterpret_cast<const f32x4*>(ap) + *reinterpret_cast<const f32x4*>(bp);
                v1 = v1 * *reinterpret_cast<const f32x4*>(ap + 4) + *reinterpret_cast<const f32x4*>(bp + 4);
                u.x = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v0[0], (__bf16)v0[1]});
                u.y = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v0[2], (__bf16)v0[3]});
                u.z = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v1[0], (__bf16)v1[1]});
                u.w = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v1[2], (__bf16)v1[3]});
            }
            reinterpret_cast<uint4*>(yout)[i] = u;
        } else {
            f32x4 v = reinterpret_cast<const f32x4*>(xin)[src];
            if (a) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(a + (size_t)n * C + c * 4);
                const f32x4 bv = *reinterpret_cast<const f32x4*>(b + (size_t)n * C + c * 4);
                v = v * av + bv;
            }
            reinterpret_cast<f32x4*>(yout)[i] = v;
        }
    }
}

static inline int stream_grid(long long total) { return (int)(cdivll(total, 256) < 32768 ? cdivll(total, 256) : 32768); }

extern "C" int cpr_subsample2(const void* x, int x_bf16, const float* a, const float* b, void* out, int N, int H, int W, int C,
                              hipStream_t stream) {
    CPR_CHECK_ARG(x && out && N > 0 && H > 0 && W > 0 && C > 0 && (a == nullptr) == (b == nullptr));
    CPR_CHECK_ARG(C % (x_bf16 ? 8 : 4) == 0);
    const int OH = (H + 1) / 2, OW = (W + 1) / 2, CV = C / (x_bf16 ? 8 : 4);
    const long long total = (long long)N * OH * OW * CV;
    if (x_bf16)
        hipLaunchKernelGGL(subsample2_kernel<true>, dim3(stream_grid(total)), dim3(256), 0, stream, x, a, b, out, N, H, W, OH, OW, CV);
    else
        hipLaunchKernelGGL(subsample2_kernel<false>, dim3(stream_grid(total)), dim3(256), 0, stream, x, a, b, out, N, H, W, OH, OW, CV);
    CPR_LAUNCH_STATUS();
}

__global__ __launch_bounds__(256) void subsample2_bwd_add_kernel(const float* __restrict__ dfine, const float* __restrict__ dcoarse,
                                                                 float* __restrict__ out, int N, int H, int W, int OH, int OW, int C4) {
    const long long total = (long long)N * H * W * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long r = i / C4;
        const int x = (int)(r % W);
        r /= W;
        const int y = (int)(r % H);
        const int n = (int)(r / H);
        f32x4 v = reinterpret_cast<const f32x4*>(dfine)[i];
        if (!((y | x) & 1))       // (y/2, x/2) < (OH, OW) holds for every even (y, x) < (H, W)
            v = v + reinterpret_cast<const f32x4*>(dcoarse)[(((size_t)n * OH + (y >> 1)) * OW + (x >> 1)) * C4 + c];
        reinterpret_cast<f32x4*>(out)[i] = v;
    }
}

extern "C" int cpr_subsample2_bwd_add(const float* dfine, const float* dcoarse, float* out, int N, int H, int W, int C,
                                      hipStream_t stream) {
    CPR_CHECK_ARG(dfine && dcoarse && out && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0);
    const long long total = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(subsample2_bwd_add_kernel, dim3(stream_grid(total)), dim3(256), 0, stream, dfine, dcoarse, out, N, H, W,
                       (H + 1) / 2, (W + 1) / 2, C / 4);
    CPR_LAUNCH_STATUS();
}

// y: the map the extra conv read (fp32, or the bf16 map of the mixed-precision forward); 4 channels per lane (16 bytes of dz / d / out)
template <bool BF16>
__global__ __launch_bounds__(256) void relu_mask_add_kernel(const float* __restrict__ dz, const float* __restrict__ d,
                                                            const void* __restrict__ y, float* __restrict__ out, long long n4) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const f32x4 g = reinterpret_cast<const f32x4*>(d)[i];
        f32x4 v = reinterpret_cast<const f32x4*>(dz)[i], yv;
        if (BF16) {
            const uint2 u = reinterpret_cast<const uint2*>(y)[i];
            yv = f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
        } else {
            yv = reinterpret_cast<const f32x4*>(y)[i];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] + (yv[e] > 0.f ? g[e] : 0.f);
        reinterpret_cast<f32x4*>(out)[i] = v;
    }
}

extern "C" int cpr_relu_mask_add(const float* dz, const float* d, const void* y, int y_bf16, float* out, long long n,
                                 hipStream_t stream) {
    CPR_CHECK_ARG(n >= 0 && n % 4 == 0);
    if (n == 0) return CPR_OK;
    CPR_CHECK_ARG(dz && d && y && out);
    if (y_bf16)
        hipLaunchKernelGGL(relu_mask_add_kernel<true>, dim3(stream_grid(n / 4)), dim3(256), 0, stream, dz, d, y, out, n / 4);
    else
        hipLaunchKernelGGL(relu_mask_add_kernel<false>, dim3(stream_grid(n / 4)), dim3(256), 0, stream, dz, d, y, out, n / 4);
    CPR_LAUNCH_STATUS();
}
