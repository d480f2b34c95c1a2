// PAFPN bottom-up path (T/mmdet/models/necks/pafpn.py:131-135): inter[i+1] += downsample_convs[i](inter[i]).  Both summands exist
// only as a raw conv output plus the per-(image, channel) GroupNorm affine of their layer, so the sum is ONE streaming pass:
//   cpr_gn_apply2[_bf16]    out[n,p,c] = (x1*a1[n,c] + b1[n,c]) + (x2*a2[n,c] + b2[n,c])
// three map-sized transfers (two reads, one write) where two gn_apply launches and an axpby move seven.  NHWC, 16 bytes of channels
// per lane (4 fp32 / 8 bf16).  A lane keeps its channel vector and walks pixels (the gn_apply_bf16_wide_kernel scheme): the four affine
// vectors sit in registers and are reloaded only when the image changes; 32-bit index arithmetic.  bf16: both maps are read as bf16,
// the arithmetic is fp32, one rounding on the way out.  In-place safe on either input (each lane reads its 16 bytes before it writes them).
#include "common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

__device__ __forceinline__ void widen8(const uint4 u, f32x4& v0, f32x4& v1) {
    v0 = f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
    v1 = f32x4{__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u), __uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u)};
}

// CV = C/4 (fp32) or C/8 (bf16) channel vectors per pixel, CV <= 256; PP = 256 / CV pixels per block step (lanes past PP * CV idle when
// CV does not divide 256).  NP = N * H * W pixels < 2^31; the last step of the walk is partial when PP does not divide NP.
template <bool BF16>
__global__ __launch_bounds__(256) void gn_apply2_kernel(const void* __restrict__ x1, const float* __restrict__ a1, const float* __restrict__ b1,
                                                        const void* __restrict__ x2, const float* __restrict__ a2, const float* __restrict__ b2,
                                                        void* __restrict__ y, int NP, int HW, int CV) {
    constexpr int V = BF16 ? 8 : 4;
    const int cg = threadIdx.x % CV, prow = threadIdx.x / CV, PP = 256 / CV;
    if (prow >= PP) return;
    const int C = CV * V;
    int ncur = -1;
    f32x4 p0, p1, q0, q1, s0, s1;       // a1, a2, b1 + b2: low / high four channels (fp32 uses the low four)
    for (long long pix = blockIdx.x * (long long)PP + prow; pix < NP; pix += (long long)gridDim.x * PP) {
        const int n = (int)(pix / HW);
        if (n != ncur) {
            ncur = n;
            const size_t t = (size_t)n * C + cg * V;
            p0 = *reinterpret_cast<const f32x4*>(a1 + t);
            q0 = *reinterpret_cast<const f32x4*>(a2 + t);
            s0 = *reinterpret_cast<const f32x4*>(b1 + t) + *reinterpret_cast<const f32x4*>(b2 + t);
            if (BF16) {
                p1 = *reinterpret_cast<const f32x4*>(a1 + t + 4);
                q1 = *reinterpret_cast<const f32x4*>(a2 + t + 4);
                s1 = *reinterpret_cast<const f32x4*>(b1 + t + 4) + *reinterpret_cast<const f32x4*>(b2 + t + 4);
            }
        }
        const size_t vec = (size_t)pix * CV + cg;
        if (BF16) {
            f32x4 u0, u1, w0, w1;
            widen8(reinterpret_cast<const uint4*>(x1)[vec], u0, u1);
            widen8(reinterpret_cast<const uint4*>(x2)[vec], w0, w1);
            u0 = u0 * p0 + (w0 * q0 + s0);
            u1 = u1 * p1 + (w1 * q1 + s1);
            uint4 o;
            o.x = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)u0[0], (__bf16)u0[1]});
            o.y = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)u0[2], (__bf16)u0[3]});
            o.z = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)u1[0], (__bf16)u1[1]});
            o.w = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)u1[2], (__bf16)u1[3]});
            reinterpret_cast<uint4*>(y)[vec] = o;
        } else {
            const f32x4 u = reinterpret_cast<const f32x4*>(x1)[vec], w = reinterpret_cast<const f32x4*>(x2)[vec];
            reinterpret_cast<f32x4*>(y)[vec] = u * p0 + (w * q0 + s0);
        }
    }
}

template <bool BF16>
static int gn_apply2_launch(const void* x1, const float* a1, const float* b1, const void* x2, const float* a2, const float* b2, void* y,
                            int N, int H, int W, int C, hipStream_t stream) {
    constexpr int V = BF16 ? 8 : 4;
    CPR_CHECK_ARG(x1 && a1 && b1 && x2 && a2 && b2 && y && N > 0 && H > 0 && W > 0 && C > 0 && C % V == 0 && C / V <= 256);
    const long long np = (long long)N * H * W;
    CPR_CHECK_ARG(np < (1ll << 31));
    const int CV = C / V, PP = 256 / CV;
    // two input streams want more loads in flight than gn_apply's one: measured at 16 x 160 x 160 x 256, grid caps 8192 / 16384 / 32768 /
    // 65536: fp32 0.250 / 0.242 / 0.228 / 0.209 ms, bf16 0.130 / 0.124 / 0.120 / 0.113 ms (two or four pixels per iteration instead: no gain)
    const long long blocks = cdivll(np, PP);
    const int grid = (int)(blocks < 65536 ? blocks : 65536);
    hipLaunchKernelGGL(gn_apply2_kernel<BF16>, dim3(grid), dim3(256), 0, stream, x1, a1, b1, x2, a2, b2, y, (int)np, H * W, CV);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_gn_apply2(const float* x1, const float* a1, const float* b1, const float* x2, const float* a2, const float* b2,
                             float* y, int N, int H, int W, int C, hipStream_t stream) {
    return gn_apply2_launch<false>(x1, a1, b1, x2, a2, b2, y, N, H, W, C, stream);
}

extern "C" int cpr_gn_apply2_bf16(const void* x1, const float* a1, const float* b1, const void* x2, const float* a2, const float* b2,
                                  void* y, int N, int H, int W, int C, hipStream_t stream) {
    return gn_apply2_launch<true>(x1, a1, b1, x2, a2, b2, y, N, H, W, C, stream);
}
