// Training-mode BatchNorm (batch statistics) on NHWC fp32 maps: ResNet(norm_eval=False), T/mmdet/models/backbones/resnet.py:647-657
// with torch.nn.BatchNorm2d in training mode.  A map y is (M, C) row-major, M = N*H*W, C % 64 == 0.
//
// Every streaming kernel has the same shape: blockIdx.y picks a group of <= 1024 channels, each thread owns 4 consecutive channels
// (one 16-byte access per row), 256 / (channels / 4) rows run side by side in a workgroup, 4 rows are in flight per thread, and
// blockIdx.x walks row blocks of `rows_per_block` rows (sized so a launch has >= 2048 workgroups on large maps).
//
// Statistics: every value is taken relative to a per-channel shift, the channel's first row (so a map whose mean is far above its
// spread keeps the precision of its spread in fp32); each thread keeps a Welford state (count, mean, M2) over its rows; the workgroup
// merges its threads by Chan's formula in a fixed order and writes one (mean, M2) per (row block, channel); the finalize kernel
// combines the row blocks in fp64 by Chan's k-group form (mean = sum n_b mean_b / M, M2 = sum (M2_b + n_b (mean_b - mean)^2)), again in a fixed order.  No E[y^2] - E[y]^2, no
// float atomics: the result is bit-repeatable and holds on maps whose mean is far above their spread.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;

struct Lanes {
    int c0, Q, PP, q, pl;
    long long r0, r1;
};

__device__ __forceinline__ Lanes lanes(long long M, int C, int rows_per_block) {
    Lanes l;
    l.c0 = blockIdx.y * 1024;
    l.Q = min(1024, C - l.c0) >> 2;
    l.PP = kThreads / l.Q;
    l.q = threadIdx.x % l.Q;
    l.pl = threadIdx.x / l.Q;
    l.r0 = (long long)blockIdx.x * rows_per_block;
    l.r1 = min(M, l.r0 + rows_per_block);
    return l;
}

long long bn_rows_per_block(long long M, int C) {
    const int groups = cdiv(C, 1024);
    const long long want = cdivll(M, cpr_max2(1, 2048 / groups));
    return cpr_max2(64, want);
}

// ---- statistics: per-(row block, channel) (mean, M2) -----------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) bn_stats_part_kernel(const float* __restrict__ y, float* __restrict__ part,
                                                                 long long* __restrict__ nbt, long long M, int C, int rows_per_block) {
    __shared__ float s_mean[kThreads * 4], s_m2[kThreads * 4];
    __shared__ int s_n[kThreads];
    const Lanes l = lanes(M, C, rows_per_block);
    float mean[4] = {0, 0, 0, 0}, m2[4] = {0, 0, 0, 0};
    int n = 0;
    if (l.pl < l.PP) {
        const f32x4 K = *reinterpret_cast<const f32x4*>(y + l.c0 + l.q * 4);      // the shift: row 0
        for (long long r = l.r0 + l.pl; r < l.r1; r += kUnroll * l.PP) {
            f32x4 v[kUnroll];
            bool ok[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long ru = r + (long long)u * l.PP;
                ok[u] = ru < l.r1;
                v[u] = *reinterpret_cast<const f32x4*>(y + (size_t)(ok[u] ? ru : r) * C + l.c0 + l.q * 4) - K;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if (!ok[u]) continue;
                ++n;
                const float inv = 1.f / (float)n;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = v[u][k] - mean[k];
                    mean[k] += d * inv;
                    m2[k] += d * (v[u][k] - mean[k]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s_mean[threadIdx.x * 4 + k] = mean[k];
        s_m2[threadIdx.x * 4 + k] = m2[k];
    }
    s_n[threadIdx.x] = l.pl < l.PP ? n : 0;
    __syncthreads();
    if (threadIdx.x < l.Q) {
        float na = 0, ma[4] = {0, 0, 0, 0}, Ma[4] = {0, 0, 0, 0};
        for (int p = 0; p < l.PP; ++p) {             // Chan, in row-lane order
            const int t = p * l.Q + l.q;
            const float nb = (float)s_n[t];
            if (nb == 0.f) continue;
            const float nn = na + nb, wb = nb / nn, wab = na * nb / nn;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = s_mean[t * 4 + k] - ma[k];
                ma[k] += d * wb;
                Ma[k] += s_m2[t * 4 + k] + d * d * wab;
            }
            na = nn;
        }
        float* o = part + ((size_t)blockIdx.x * C + l.c0 + l.q * 4) * 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = ma[k];
            o[2 * k + 1] = Ma[k];
        }
    }
    if (nbt && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *nbt += 1;     // read by the finalize launch (momentum None)
}

// 16 channels x 16 row-block slices per workgroup; slice s takes row blocks s, s + 16, ...; the slices are combined in slice order.
__global__ void __launch_bounds__(kThreads) bn_stats_finalize_kernel(
    const float* __restrict__ y, const float* __restrict__ part, int blocks, long long M, int C, int rows_per_block, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ running_mean, float* __restrict__ running_var, const long long* __restrict__ nbt,
    float momentum, float eps, float* __restrict__ mean_out, float* __restrict__ rstd_out, float* __restrict__ scale_out,
    float* __restrict__ shift_out, float* __restrict__ center_out, float* __restrict__ cmean_out, float* __restrict__ cshift_out) {
    __shared__ double red[16][17];
    const int cl = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const bool live = c < C;
    double s1 = 0;
    if (live)
        for (int b = s; b < blocks; b += 16) {
            const long long nb = min((long long)rows_per_block, M - (long long)b * rows_per_block);
            s1 += (double)nb * (double)part[((size_t)b * C + c) * 2];
        }
    red[s][cl] = s1;
    __syncthreads();
    double msh = 0;                                        // mean relative to the shift
    for (int k = 0; k < 16; ++k) msh += red[k][cl];
    msh /= (double)M;
    __syncthreads();
    double s2 = 0;
    if (live)
        for (int b = s; b < blocks; b += 16) {
            const long long nb = min((long long)rows_per_block, M - (long long)b * rows_per_block);
            const double d = (double)part[((size_t)b * C + c) * 2] - msh;
            s2 += (double)part[((size_t)b * C + c) * 2 + 1] + (double)nb * d * d;
        }
    red[s][cl] = s2;
    __syncthreads();
    if (s != 0 || !live) return;
    double m2 = 0;
    for (int k = 0; k < 16; ++k) m2 += red[k][cl];
    const double mu = (double)y[c] + msh;
    const double var = m2 / (double)M;                      // biased: what the normalisation uses
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double sc = (double)gamma[c] * rstd;
    mean_out[c] = (float)mu;
    rstd_out[c] = (float)rstd;
    if (scale_out) scale_out[c] = (float)sc;
    if (shift_out) shift_out[c] = (float)((double)beta[c] - mu * sc);
    if (center_out) {       // the centred form: xhat = (y - center - cmean) * rstd, out = (y - center) * scale + cshift
        center_out[c] = y[c];
        cmean_out[c] = (float)msh;
        cshift_out[c] = (float)((double)beta[c] - msh * sc);
    }
    if (running_mean) {
        const double m = momentum >= 0.f ? (double)momentum : 1.0 / (double)(*nbt);     // momentum None: cumulative average
        running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mu);
        running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (m2 / (double)(M - 1)));   // unbiased
    }
}

// ---- apply: out = [ReLU]((y - center) * scale + shift [+ residual] [+ (y2 - center2) * scale2 + shift2]) --------------------
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__global__ void __launch_bounds__(kThreads) bn_apply_kernel(
    const float* __restrict__ y, const float* __restrict__ center, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ residual, const float* __restrict__ y2, const float* __restrict__ center2,
    const float* __restrict__ scale2, const float* __restrict__ shift2, float* __restrict__ out, long long M, int C,
    int rows_per_block, int relu) {
    const Lanes l = lanes(M, C, rows_per_block);
    if (l.pl >= l.PP) return;
    const int ch = l.c0 + l.q * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 ce = center ? ld4(center + ch) : zero, sc = ld4(scale + ch), sh = ld4(shift + ch);
    f32x4 ce2 = zero, sc2 = zero, sh2 = zero;
    if (y2) {
        ce2 = center2 ? ld4(center2 + ch) : zero;
        sc2 = ld4(scale2 + ch);
        sh2 = ld4(shift2 + ch);
    }
    for (long long r = l.r0 + l.pl; r < l.r1; r += kUnroll * l.PP) {
        f32x4 v[kUnroll], a[kUnroll];
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const long long ru = r + (long long)u * l.PP;
            ok[u] = ru < l.r1;
            const size_t o = (size_t)(ok[u] ? ru : r) * C + ch;
            v[u] = ld4(y + o);
            if (residual) a[u] = ld4(residual + o);
            else if (y2) a[u] = ld4(y2 + o);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (!ok[u]) continue;
            f32x4 z;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float t = fmaf(v[u][k] - ce[k], sc[k], sh[k]);
                if (residual) t += a[u][k];
                else if (y2) t += fmaf(a[u][k] - ce2[k], sc2[k], sh2[k]);
                z[k] = relu ? fmaxf(t, 0.f) : t;
            }
            *reinterpret_cast<f32x4*>(out + (size_t)(r + (long long)u * l.PP) * C + ch) = z;
        }
    }
}

// ---- backward.  g = dout * (z > 0) (z: the recorded post-ReLU output; NULL = dout is already g) ------------------------------
// y - mean is taken as (y - center) - cmean (center NULL = 0): with center = a row of the map itself the first difference is exact
// reduce: per (row block, channel) (sum g, sum g * (y - mean))
__global__ void __launch_bounds__(kThreads) bn_bwd_part_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                               const float* __restrict__ y, const float* __restrict__ center,
                                                               const float* __restrict__ mean, float* __restrict__ part, long long M,
                                                               int C, int rows_per_block) {
    __shared__ float s_a[kThreads * 4], s_b[kThreads * 4];
    const Lanes l = lanes(M, C, rows_per_block);
    const int ch = l.c0 + l.q * 4;
    float sa[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
    if (l.pl < l.PP) {
        const f32x4 mu = ld4(mean + ch), ce = center ? ld4(center + ch) : f32x4{0.f, 0.f, 0.f, 0.f};
        for (long long r = l.r0 + l.pl; r < l.r1; r += kUnroll * l.PP) {
            f32x4 g[kUnroll], zv[kUnroll], yv[kUnroll];
            bool ok[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long ru = r + (long long)u * l.PP;
                ok[u] = ru < l.r1;
                const size_t o = (size_t)(ok[u] ? ru : r) * C + ch;
                g[u] = ld4(dout + o);
                if (z) zv[u] = ld4(z + o);
                yv[u] = ld4(y + o);
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if (!ok[u]) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float gk = (!z || zv[u][k] > 0.f) ? g[u][k] : 0.f;
                    sa[k] += gk;
                    sb[k] = fmaf(gk, (yv[u][k] - ce[k]) - mu[k], sb[k]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s_a[threadIdx.x * 4 + k] = l.pl < l.PP ? sa[k] : 0.f;
        s_b[threadIdx.x * 4 + k] = l.pl < l.PP ? sb[k] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < l.Q) {
        float a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
        for (int p = 0; p < l.PP; ++p) {
            const int t = p * l.Q + l.q;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[k] += s_a[t * 4 + k];
                b[k] += s_b[t * 4 + k];
            }
        }
        float* o = part + ((size_t)blockIdx.x * C + ch) * 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = a[k];
            o[2 * k + 1] = b[k];
        }
    }
}

// dbeta = sum g, dgamma = rstd * sum g (y - mean); coef[c] = (gamma * rstd, dbeta / M, rstd * dgamma / M, mean) for the apply pass
__global__ void __launch_bounds__(kThreads) bn_bwd_finalize_kernel(const float* __restrict__ part, int blocks, long long M, int C,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   const float* __restrict__ gamma, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, float* __restrict__ coef) {
    __shared__ double ra[16][17], rb[16][17];
    const int cl = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    double a = 0, b = 0;
    if (c < C)
        for (int k = s; k < blocks; k += 16) {
            a += (double)part[((size_t)k * C + c) * 2];
            b += (double)part[((size_t)k * C + c) * 2 + 1];
        }
    ra[s][cl] = a;
    rb[s][cl] = b;
    __syncthreads();
    if (s != 0 || c >= C) return;
    double sa = 0, sb = 0;
    for (int k = 0; k < 16; ++k) {
        sa += ra[k][cl];
        sb += rb[k][cl];
    }
    const double rs = (double)rstd[c];
    const double dg = rs * sb;
    if (dgamma) dgamma[c] = (float)dg;
    if (dbeta) dbeta[c] = (float)sa;
    coef[(size_t)c * 4 + 0] = (float)((double)gamma[c] * rs);
    coef[(size_t)c * 4 + 1] = (float)(sa / (double)M);
    coef[(size_t)c * 4 + 2] = (float)(rs * dg / (double)M);
    coef[(size_t)c * 4 + 3] = mean[c];
}

// dy = gamma * rstd * (g - dbeta / M - xhat * dgamma / M),  xhat * dgamma / M = ((y - center) - mean) * (rstd * dgamma / M)
__global__ void __launch_bounds__(kThreads) bn_bwd_apply_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                                const float* __restrict__ y, const float* __restrict__ coef,
                                                                const float* __restrict__ center, float* __restrict__ dy, long long M,
                                                                int C, int rows_per_block) {
    const Lanes l = lanes(M, C, rows_per_block);
    if (l.pl >= l.PP) return;
    const int ch = l.c0 + l.q * 4;
    const f32x4 ce = center ? ld4(center + ch) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 cf[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cf[k] = ld4(coef + (size_t)(ch + k) * 4);
    for (long long r = l.r0 + l.pl; r < l.r1; r += kUnroll * l.PP) {
        f32x4 g[kUnroll], zv[kUnroll], yv[kUnroll];
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const long long ru = r + (long long)u * l.PP;
            ok[u] = ru < l.r1;
            const size_t o = (size_t)(ok[u] ? ru : r) * C + ch;
            g[u] = ld4(dout + o);
            if (z) zv[u] = ld4(z + o);
            yv[u] = ld4(y + o);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (!ok[u]) continue;
            f32x4 d;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gk = (!z || zv[u][k] > 0.f) ? g[u][k] : 0.f;
                d[k] = cf[k][0] * (gk - cf[k][1] - ((yv[u][k] - ce[k]) - cf[k][3]) * cf[k][2]);
            }
            *reinterpret_cast<f32x4*>(dy + (size_t)(r + (long long)u * l.PP) * C + ch) = d;
        }
    }
}

// ---- SyncBN (torch.nn.SyncBatchNorm; mmcv build_norm_layer 'SyncBN'): the two finalize steps in split form, so that a collective can
// sit between "what this rank saw" and "what every rank uses".  The exchange records are fp64:
//   statistics  (2C + 1): [0, C) the ABSOLUTE mean of this rank's rows, [C, 2C) their M2, [2C] the row count (an exact integer value)
//   backward    (2C):     [0, C) sum g, [C, 2C) sum g * (y - mean) over this rank's rows, mean = the merged mean
// The local kernels keep the finalize kernels' shape (16 channels x 16 row-block slices per workgroup, fixed order); the merge kernels
// run one thread per channel over the R gathered records in rank order.  No atomics.
__global__ void __launch_bounds__(kThreads) bn_stats_local_kernel(const float* __restrict__ y, const float* __restrict__ part, int blocks,
                                                                  long long M, int C, int rows_per_block, double* __restrict__ record) {
    __shared__ double red[16][17];
    const int cl = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const bool live = c < C;
    double s1 = 0;
    if (live)
        for (int b = s; b < blocks; b += 16) {
            const long long nb = min((long long)rows_per_block, M - (long long)b * rows_per_block);
            s1 += (double)nb * (double)part[((size_t)b * C + c) * 2];
        }
    red[s][cl] = s1;
    __syncthreads();
    double msh = 0;                                        // mean relative to the shift (this rank's first row)
    for (int k = 0; k < 16; ++k) msh += red[k][cl];
    msh /= (double)M;
    __syncthreads();
    double s2 = 0;
    if (live)
        for (int b = s; b < blocks; b += 16) {
            const long long nb = min((long long)rows_per_block, M - (long long)b * rows_per_block);
            const double d = (double)part[((size_t)b * C + c) * 2] - msh;
            s2 += (double)part[((size_t)b * C + c) * 2 + 1] + (double)nb * d * d;
        }
    red[s][cl] = s2;
    __syncthreads();
    if (s != 0 || !live) return;
    double m2 = 0;
    for (int k = 0; k < 16; ++k) m2 += red[k][cl];
    record[c] = (double)y[c] + msh;
    record[(size_t)C + c] = m2;
    if (c == 0) record[(size_t)2 * C] = (double)M;
}

// One workgroup: every thread reads num_batches_tracked before thread 0 writes it back incremented (momentum None divides by the new
// count); each thread then owns channels c, c + 1024, ...
constexpr int kMergeThreads = 1024;
__global__ void __launch_bounds__(kMergeThreads) bn_stats_merge_kernel(
    const double* __restrict__ records, int R, const float* __restrict__ y, int C, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ running_mean, float* __restrict__ running_var, long long* nbt, float momentum,
    float eps, float* __restrict__ mean_out, float* __restrict__ rstd_out, float* __restrict__ scale_out, float* __restrict__ shift_out,
    float* __restrict__ center_out, float* __restrict__ cmean_out, float* __restrict__ cshift_out, double* __restrict__ count_out) {
    const long long seen = nbt ? *nbt + 1 : 0;
    __syncthreads();
    if (nbt && threadIdx.x == 0) *nbt = seen;
    const size_t ld = (size_t)2 * C + 1;
    double M = 0;
    for (int r = 0; r < R; ++r) M += records[r * ld + 2 * (size_t)C];
    if (threadIdx.x == 0 && count_out) *count_out = M;
    for (int c = threadIdx.x; c < C; c += kMergeThreads) {
        double s1 = 0;
        for (int r = 0; r < R; ++r) s1 += records[r * ld + 2 * (size_t)C] * records[r * ld + c];
        const double mu = s1 / M;
        double m2 = 0;
        for (int r = 0; r < R; ++r) {
            const double d = records[r * ld + c] - mu;
            m2 += records[r * ld + C + c] + records[r * ld + 2 * (size_t)C] * d * d;
        }
        const double var = m2 / M;                          // biased, over the global count: what the normalisation uses
        const double rstd = 1.0 / sqrt(var + (double)eps);
        const double sc = (double)gamma[c] * rstd;
        mean_out[c] = (float)mu;
        rstd_out[c] = (float)rstd;
        if (scale_out) scale_out[c] = (float)sc;
        if (shift_out) shift_out[c] = (float)((double)beta[c] - mu * sc);
        if (center_out) {                                   // rank-local: this rank's own first row
            const double msh = mu - (double)y[c];
            center_out[c] = y[c];
            cmean_out[c] = (float)msh;
            cshift_out[c] = (float)((double)beta[c] - msh * sc);
        }
        if (running_mean) {
            const double m = momentum >= 0.f ? (double)momentum : 1.0 / (double)seen;     // momentum None: cumulative average
            running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mu);
            running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (m2 / (M - 1.0)));   // unbiased, global M - 1
        }
    }
}

// this rank's dbeta = sum g and dgamma = rstd * sum g (y - mean) over its own rows (torch's SyncBatchNorm hands each rank its local
// parameter-gradient sums; the gradient reducer averages them), and the record
__global__ void __launch_bounds__(kThreads) bn_bwd_local_kernel(const float* __restrict__ part, int blocks, int C,
                                                                const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, double* __restrict__ record) {
    __shared__ double ra[16][17], rb[16][17];
    const int cl = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    double a = 0, b = 0;
    if (c < C)
        for (int k = s; k < blocks; k += 16) {
            a += (double)part[((size_t)k * C + c) * 2];
            b += (double)part[((size_t)k * C + c) * 2 + 1];
        }
    ra[s][cl] = a;
    rb[s][cl] = b;
    __syncthreads();
    if (s != 0 || c >= C) return;
    double sa = 0, sb = 0;
    for (int k = 0; k < 16; ++k) {
        sa += ra[k][cl];
        sb += rb[k][cl];
    }
    if (dgamma) dgamma[c] = (float)((double)rstd[c] * sb);
    if (dbeta) dbeta[c] = (float)sa;
    record[c] = sa;
    record[(size_t)C + c] = sb;
}

// coef for bn_bwd_apply_kernel from the sums over ALL ranks (rank order) and the global count
__global__ void __launch_bounds__(kThreads) bn_bwd_merge_kernel(const double* __restrict__ records, int R, int C,
                                                                const double* __restrict__ count, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                float* __restrict__ coef) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    double sa = 0, sb = 0;
    for (int r = 0; r < R; ++r) {
        sa += records[(size_t)r * 2 * C + c];
        sb += records[(size_t)r * 2 * C + C + c];
    }
    const double M = *count, rs = (double)rstd[c];
    coef[(size_t)c * 4 + 0] = (float)((double)gamma[c] * rs);
    coef[(size_t)c * 4 + 1] = (float)(sa / M);
    coef[(size_t)c * 4 + 2] = (float)(rs * (rs * sb) / M);
    coef[(size_t)c * 4 + 3] = mean[c];
}

bool bn_shape_ok(long long M, int C) { return M > 1 && C > 0 && C % 64 == 0; }
bool bn_sync_shape_ok(long long M, int C) { return M > 0 && C > 0 && C % 64 == 0; }      // a rank may hold a single row

#ifdef CPR_BENCH_HOOKS   // measurement build only (libcprhip_bench.so): the finalize / local / merge launches on their own
int bn_finalize_only = 0;
#define BN_STREAMING (!bn_finalize_only)
#else
#define BN_STREAMING true
#endif

}  // namespace

#ifdef CPR_BENCH_HOOKS
extern "C" int cpr_bn_set_finalize_only(int on) {   // 1: every bn_train.hip entry skips its streaming passes (part / apply): results WRONG
    bn_finalize_only = on != 0;
    return CPR_OK;
}
#endif

// floats of workspace the statistics / backward entries need for an (M, C) map
extern "C" int cpr_bn_train_ws(long long M, int C) {
    if (!bn_shape_ok(M, C)) return CPR_ERR_ARG;
    const long long n = cdivll(M, bn_rows_per_block(M, C)) * C * 2 + (long long)C * 4;
    return n < (1ll << 31) ? (int)n : CPR_ERR_UNSUPPORTED;
}

extern "C" int cpr_bn_batch_stats(const float* y, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                  long long* num_batches_tracked, float momentum, float eps, float* mean, float* rstd, float* scale,
                                  float* shift, float* center, float* cmean, float* cshift, float* ws, long long M, int C,
                                  hipStream_t stream) {
    CPR_CHECK_ARG(y && gamma && beta && mean && rstd && ws && bn_shape_ok(M, C));
    CPR_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr));
    CPR_CHECK_ARG((center == nullptr) == (cmean == nullptr) && (center == nullptr) == (cshift == nullptr));
    CPR_CHECK_ARG(momentum >= 0.f || num_batches_tracked);
    const int rpb = (int)bn_rows_per_block(M, C);
    const int blocks = (int)cdivll(M, rpb);
    if (BN_STREAMING)
        hipLaunchKernelGGL(bn_stats_part_kernel, dim3(blocks, cdiv(C, 1024)), dim3(kThreads), 0, stream, y, ws, num_batches_tracked, M, C,
                           rpb);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(cdiv(C, 16)), dim3(kThreads), 0, stream, y, ws, blocks, M, C, rpb, gamma, beta,
                       running_mean, running_var, num_batches_tracked, momentum, eps, mean, rstd, scale, shift, center, cmean, cshift);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_bn_apply(const float* y, const float* center, const float* scale, const float* shift, const float* residual,
                            const float* y2, const float* center2, const float* scale2, const float* shift2, float* out, long long M,
                            int C, int relu, hipStream_t stream) {
    CPR_CHECK_ARG(y && scale && shift && out && M > 0 && C > 0 && C % 64 == 0);
    CPR_CHECK_ARG(!(residual && y2) && (!y2 || (scale2 && shift2)));
    const int rpb = (int)bn_rows_per_block(M, C);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)cdivll(M, rpb), cdiv(C, 1024)), dim3(kThreads), 0, stream, y, center, scale,
                       shift, residual, y2, center2, scale2, shift2, out, M, C, rpb, relu);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_bn_train_bwd(const float* dout, const float* z, const float* y, const float* center, const float* mean, const float* rstd,
                                const float* gamma, float* dy, float* dgamma, float* dbeta, float* ws, long long M, int C,
                                hipStream_t stream) {
    CPR_CHECK_ARG(dout && y && mean && rstd && gamma && dy && ws && bn_shape_ok(M, C));
    const int rpb = (int)bn_rows_per_block(M, C);
    const int blocks = (int)cdivll(M, rpb);
    float* coef = ws + (size_t)blocks * C * 2;
    if (BN_STREAMING)
        hipLaunchKernelGGL(bn_bwd_part_kernel, dim3(blocks, cdiv(C, 1024)), dim3(kThreads), 0, stream, dout, z, y, center, mean, ws, M, C, rpb);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, 16)), dim3(kThreads), 0, stream, ws, blocks, M, C, mean, rstd, gamma,
                       dgamma, dbeta, coef);
    if (BN_STREAMING)
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(blocks, cdiv(C, 1024)), dim3(kThreads), 0, stream, dout, z, y, coef, center, dy, M, C, rpb);
    CPR_LAUNCH_STATUS();
}

// ---- SyncBN entries (see the kernels).  ws: cpr_bn_sync_ws(M, C) floats; records: (R, 2C + 1) / (R, 2C) doubles, rank-major
extern "C" int cpr_bn_sync_ws(long long M, int C) {
    if (!bn_sync_shape_ok(M, C)) return CPR_ERR_ARG;
    const long long n = cdivll(M, bn_rows_per_block(M, C)) * C * 2 + (long long)C * 4;
    return n < (1ll << 31) ? (int)n : CPR_ERR_UNSUPPORTED;
}

extern "C" int cpr_bn_sync_stats_local(const float* y, double* record, float* ws, long long M, int C, hipStream_t stream) {
    CPR_CHECK_ARG(y && record && ws && bn_sync_shape_ok(M, C));
    const int rpb = (int)bn_rows_per_block(M, C);
    const int blocks = (int)cdivll(M, rpb);
    if (BN_STREAMING)
        hipLaunchKernelGGL(bn_stats_part_kernel, dim3(blocks, cdiv(C, 1024)), dim3(kThreads), 0, stream, y, ws, (long long*)nullptr, M, C,
                           rpb);
    hipLaunchKernelGGL(bn_stats_local_kernel, dim3(cdiv(C, 16)), dim3(kThreads), 0, stream, y, ws, blocks, M, C, rpb, record);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_bn_sync_stats_merge(const double* records, int R, const float* y, const float* gamma, const float* beta,
                                       float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                                       float* mean, float* rstd, float* scale, float* shift, float* center, float* cmean, float* cshift,
                                       double* count, int C, hipStream_t stream) {
    CPR_CHECK_ARG(records && R > 0 && y && gamma && beta && mean && rstd && C > 0 && C % 64 == 0);
    CPR_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr));
    CPR_CHECK_ARG((center == nullptr) == (cmean == nullptr) && (center == nullptr) == (cshift == nullptr));
    CPR_CHECK_ARG(momentum >= 0.f || num_batches_tracked);
    hipLaunchKernelGGL(bn_stats_merge_kernel, dim3(1), dim3(kMergeThreads), 0, stream, records, R, y, C, gamma, beta, running_mean,
                       running_var, num_batches_tracked, momentum, eps, mean, rstd, scale, shift, center, cmean, cshift, count);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_bn_sync_bwd_local(const float* dout, const float* z, const float* y, const float* center, const float* mean,
                                     const float* rstd, float* dgamma, float* dbeta, double* record, float* ws, long long M, int C,
                                     hipStream_t stream) {
    CPR_CHECK_ARG(dout && y && mean && rstd && record && ws && bn_sync_shape_ok(M, C));
    const int rpb = (int)bn_rows_per_block(M, C);
    const int blocks = (int)cdivll(M, rpb);
    if (BN_STREAMING)
        hipLaunchKernelGGL(bn_bwd_part_kernel, dim3(blocks, cdiv(C, 1024)), dim3(kThreads), 0, stream, dout, z, y, center, mean, ws, M, C, rpb);
    hipLaunchKernelGGL(bn_bwd_local_kernel, dim3(cdiv(C, 16)), dim3(kThreads), 0, stream, ws, blocks, C, rstd, dgamma, dbeta, record);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_bn_sync_bwd_merge(const double* records, int R, const double* count, const float* dout, const float* z, const float* y,
                                     const float* center, const float* mean, const float* rstd, const float* gamma, float* dy, float* ws,
                                     long long M, int C, hipStream_t stream) {
    CPR_CHECK_ARG(records && R > 0 && count && dout && y && mean && rstd && gamma && dy && ws && bn_sync_shape_ok(M, C));
    const int rpb = (int)bn_rows_per_block(M, C);
    const int blocks = (int)cdivll(M, rpb);
    float* coef = ws + (size_t)blocks * C * 2;
    hipLaunchKernelGGL(bn_bwd_merge_kernel, dim3(cdiv(C, kThreads)), dim3(kThreads), 0, stream, records, R, C, count, mean, rstd, gamma, coef);
    if (BN_STREAMING)
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(blocks, cdiv(C, 1024)), dim3(kThreads), 0, stream, dout, z, y, coef, center, dy, M, C, rpb);
    CPR_LAUNCH_STATUS();
}
