// ResNeSt split attention, radix 2 (T/mmdet/models/backbones/resnest.py:40-150), fp32 NHWC.  u (N,H,W,2w) is the output of the block's
// 3x3 conv + bn0 + ReLU: channel r*w + c is split r of channel c.
//   splat_gap        g[n,c]     = mean over pixels of u[n,p,c] + u[n,p,w+c]
//   splat_attn       z = relu(s1*(fc1 g + b1) + t1), a = fc2 z + b2, att[n,r,c] = softmax over r of a[n,r*w+c]   (one workgroup per image)
//   splat_apply      v[n,p,c]   = att[n,0,c]*u[n,p,c] + att[n,1,c]*u[n,p,w+c], or directly AvgPool2d(3, 2, 1)(v) (divisor always 9)
//   splat_attn_grad  datt[n,r,c] = sum over pixels of dv[n,p,c]*u[n,p,r*w+c]; dv = dout, or the pool's adjoint of dout in gather form
//   splat_attn_bwd   softmax / fc2 / ReLU / folded bn1 / fc1 backward per image, then the parameter gradients summed over images
//   splat_apply_bwd  du[n,p,r*w+c] = (att[n,r,c]*dv[n,p,c] + dg[n,c]/(H*W)) * (u > 0) and its per-channel column sums
// The four map kernels are HBM streams: a lane owns 4 channels (16 bytes) of both splits and walks pixels, a wave reads contiguous runs.
// Every pixel reduction is per (image, chunk of 16 * (256 / (w/4)) pixels) -- a function of w alone, so of (H, W, w) per image -- with a
// lane's pixels added in walk order, the lanes of a channel in ascending order through LDS, the chunks in ascending order by a
// second launch: no atomics, bit-repeatable, and an image's result does not depend on the batch it sits in.
#include "common.h"

#define SPLAT_MAX_W 1024       // WV = w/4 <= 256 lanes of a workgroup; the per-image kernels keep 2w + inter floats in LDS
#define SPLAT_MAX_INTER 1024
#define SPLAT_WALK 16          // pixels a lane walks per chunk
#define SPLAT_ATTN_THREADS 1024 // the per-image kernels: 16 waves, one output row per wave at a time (a row's sum does not depend on the wave)

static inline int splat_pp(int w) { return 256 / (w / 4); }
static inline int splat_chunk(int w) { return SPLAT_WALK * splat_pp(w); }

extern "C" int cpr_splat_chunks(int H, int W, int w) {
    CPR_CHECK_ARG(H > 0 && W > 0 && w > 0 && w % 4 == 0 && w <= SPLAT_MAX_W);
    const long long hw = (long long)H * W;
    if (hw >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    return (int)cdivll(hw, splat_chunk(w));
}

// the gradient reaching v at input pixel (ih, iw): dout there, or (POOL) the adjoint of AvgPool2d(3, 2, 1): the windows of the outputs
// oh in [ih/2, (ih+1)/2], ow in [iw/2, (iw+1)/2] hold the pixel; oh ascending, then ow; one multiply by 1/9 at the end
template <bool POOL>
__device__ __forceinline__ f32x4 splat_dv(const float* __restrict__ dout, int n, int ih, int iw, int H, int W, int OH, int OW, int WV, int cv) {
    if (!POOL) return reinterpret_cast<const f32x4*>(dout)[((size_t)n * H * W + (size_t)ih * W + iw) * WV + cv];
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int oh = ih >> 1; oh <= ((ih + 1) >> 1); ++oh) {
        if (oh >= OH) break;
        for (int ow = iw >> 1; ow <= ((iw + 1) >> 1); ++ow) {
            if (ow >= OW) break;
            s += reinterpret_cast<const f32x4*>(dout)[((size_t)n * OH * OW + (size_t)oh * OW + ow) * WV + cv];
        }
    }
    return s * (1.f / 9.f);
}

// lanes (prow < PP, cv) of a workgroup hold NV partial vectors each; the lanes of prow 0 return the sum over prow = 0 .. PP-1 in that order
template <int NV>
__device__ __forceinline__ void splat_block_sum(f32x4 (&acc)[NV], f32x4* lds, int prow, int cv, int PP, int WV) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
        if (prow < PP) lds[(v * PP + prow) * WV + cv] = acc[v];
    __syncthreads();                                             // (every lane of the workgroup arrives, the idle tail too)
    if (prow == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            f32x4 s = lds[(v * PP) * WV + cv];
            for (int r = 1; r < PP; ++r) s += lds[(v * PP + r) * WV + cv];
            acc[v] = s;
        }
    }
}

// out[b, c] = scale * sum over r = 0 .. rows-1 (ascending) of in[b, r, c]
__global__ __launch_bounds__(256) void splat_rows_sum_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int rows, int cols,
                                                             float scale) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= (long long)B * cols) return;
    const int b = (int)(i / cols), c = (int)(i % cols);
    const float* p = in + (size_t)b * rows * cols + c;
    float s = p[0];
    for (int r = 1; r < rows; ++r) s += p[(size_t)r * cols];
    out[i] = s * scale;
}

static void splat_rows_sum(const float* in, float* out, int B, int rows, int cols, float scale, hipStream_t stream) {
    const long long n = (long long)B * cols;
    hipLaunchKernelGGL(splat_rows_sum_kernel, dim3((unsigned)cdivll(n, 256)), dim3(256), 0, stream, in, out, B, rows, cols, scale);
}

// grid (K, N): block (k, n) sums the pixels [k * CH, (k + 1) * CH) of image n into ws[n][k][w]
__global__ __launch_bounds__(256) void splat_gap_kernel(const float* __restrict__ u, float* __restrict__ ws, int HW, int WV, int CH) {
    __shared__ f32x4 lds[256];
    const int cv = threadIdx.x % WV, prow = threadIdx.x / WV, PP = 256 / WV;
    const int k = blockIdx.x, n = blockIdx.y;
    f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    if (prow < PP) {
        const int end = min(HW, (k + 1) * CH);
        for (int p = k * CH + prow; p < end; p += PP) {
            const f32x4* px = reinterpret_cast<const f32x4*>(u) + ((size_t)n * HW + p) * 2 * WV;
            acc[0] += px[cv] + px[WV + cv];
        }
    }
    splat_block_sum<1>(acc, lds, prow, cv, PP, WV);
    if (prow == 0) reinterpret_cast<f32x4*>(ws)[((size_t)n * gridDim.x + k) * WV + cv] = acc[0];
}

extern "C" int cpr_splat_gap(const float* u, float* g, float* ws, int N, int H, int W, int w, hipStream_t stream) {
    CPR_CHECK_ARG(u && g && ws && N > 0 && N <= 65535 && H > 0 && W > 0 && w > 0 && w % 4 == 0 && w <= SPLAT_MAX_W);
    const long long hw = (long long)H * W;
    if (hw * N >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    const int K = (int)cdivll(hw, splat_chunk(w));
    hipLaunchKernelGGL(splat_gap_kernel, dim3(K, N), dim3(256), 0, stream, u, ws, (int)hw, w / 4, splat_chunk(w));
    splat_rows_sum(ws, g, N, K, w, 1.f / (float)hw, stream);
    CPR_LAUNCH_STATUS();
}

// one wave per output row: out[j] = sum_c m[j, c] * v[c] (lanes stride over c, then the fixed butterfly of wave_sum)
__device__ __forceinline__ float splat_row_dot(const float* __restrict__ row, const float* v, int len, int lane) {
    float s = 0.f;
    for (int c = lane; c < len; c += 64) s = fmaf(row[c], v[c], s);
    return wave_sum(s);
}

__global__ __launch_bounds__(SPLAT_ATTN_THREADS) void splat_attn_kernel(const float* __restrict__ g, const float* __restrict__ fc1w, const float* __restrict__ fc1b,
                                                         const float* __restrict__ s1, const float* __restrict__ t1,
                                                         const float* __restrict__ fc2w, const float* __restrict__ fc2b,
                                                         float* __restrict__ att, float* __restrict__ z, int w, int inter) {
    __shared__ float sg[SPLAT_MAX_W], sz[SPLAT_MAX_INTER], sa[2 * SPLAT_MAX_W];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x, NW = NT >> 6;
    for (int c = tid; c < w; c += NT) sg[c] = g[(size_t)n * w + c];
    __syncthreads();
    for (int j = wave; j < inter; j += NW) {
        const float h = splat_row_dot(fc1w + (size_t)j * w, sg, w, lane) + fc1b[j];
        const float v = fmaxf(fmaf(s1[j], h, t1[j]), 0.f);
        if (lane == 0) {
            sz[j] = v;
            if (z) z[(size_t)n * inter + j] = v;
        }
    }
    __syncthreads();
    for (int k = wave; k < 2 * w; k += NW) {
        const float a = splat_row_dot(fc2w + (size_t)k * inter, sz, inter, lane) + fc2b[k];
        if (lane == 0) sa[k] = a;
    }
    __syncthreads();
    for (int c = tid; c < w; c += NT) {
        const float a0 = sa[c], a1 = sa[w + c], m = fmaxf(a0, a1);
        const float e0 = expf(a0 - m), e1 = expf(a1 - m), inv = 1.f / (e0 + e1);
        att[(size_t)n * 2 * w + c] = e0 * inv;
        att[(size_t)n * 2 * w + w + c] = e1 * inv;
    }
}

extern "C" int cpr_splat_attn(const float* g, const float* fc1w, const float* fc1b, const float* s1, const float* t1, const float* fc2w,
                              const float* fc2b, float* att, float* z, int N, int w, int inter, hipStream_t stream) {
    CPR_CHECK_ARG(g && fc1w && fc1b && s1 && t1 && fc2w && fc2b && att && N > 0 && w > 0 && w % 4 == 0 && w <= SPLAT_MAX_W && inter > 0 &&
                  inter <= SPLAT_MAX_INTER);
    hipLaunchKernelGGL(splat_attn_kernel, dim3(N), dim3(SPLAT_ATTN_THREADS), 0, stream, g, fc1w, fc1b, s1, t1, fc2w, fc2b, att, z, w, inter);
    CPR_LAUNCH_STATUS();
}

// NP output pixels; a lane keeps its image's two attention vectors and walks pixels.  POOL: out pixel (oh, ow) is the sum over the 3x3
// window at (2*oh - 1, 2*ow - 1) of v (taps row-major, out-of-range taps contribute 0) times 1/9; v never reaches memory
template <bool POOL>
__global__ __launch_bounds__(256) void splat_apply_kernel(const float* __restrict__ u, const float* __restrict__ att, float* __restrict__ out,
                                                          int NP, int H, int W, int OH, int OW, int WV) {
    const int cv = threadIdx.x % WV, prow = threadIdx.x / WV, PP = 256 / WV;
    if (prow >= PP) return;
    int ncur = -1;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
    const f32x4* u4 = reinterpret_cast<const f32x4*>(u);
    for (long long pix = blockIdx.x * (long long)PP + prow; pix < NP; pix += (long long)gridDim.x * PP) {
        const int n = (int)(pix / (OH * OW)), q = (int)(pix % (OH * OW));
        if (n != ncur) {
            ncur = n;
            a0 = reinterpret_cast<const f32x4*>(att)[(size_t)n * 2 * WV + cv];
            a1 = reinterpret_cast<const f32x4*>(att)[(size_t)n * 2 * WV + WV + cv];
        }
        f32x4 r;
        if (POOL) {
            const int oh = q / OW, ow = q % OW;
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = 2 * oh - 1 + kh;
                if (ih < 0 || ih >= H) continue;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = 2 * ow - 1 + kw;
                    if (iw < 0 || iw >= W) continue;
                    const f32x4* px = u4 + ((size_t)n * H * W + (size_t)ih * W + iw) * 2 * WV;
                    s += a0 * px[cv] + a1 * px[WV + cv];
                }
            }
            r = s * (1.f / 9.f);
        } else {
            const f32x4* px = u4 + (size_t)pix * 2 * WV;
            r = a0 * px[cv] + a1 * px[WV + cv];
        }
        reinterpret_cast<f32x4*>(out)[(size_t)pix * WV + cv] = r;
    }
}

extern "C" int cpr_splat_apply(const float* u, const float* att, float* out, int N, int H, int W, int w, int pool, hipStream_t stream) {
    CPR_CHECK_ARG(u && att && out && N > 0 && H > 0 && W > 0 && w > 0 && w % 4 == 0 && w <= SPLAT_MAX_W && (pool == 0 || pool == 1));
    const int OH = pool ? (H - 1) / 2 + 1 : H, OW = pool ? (W - 1) / 2 + 1 : W;
    const long long np = (long long)N * OH * OW;
    if ((long long)N * H * W >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    const int WV = w / 4, PP = 256 / WV;
    const long long blocks = cdivll(np, PP);
    const int grid = (int)(blocks < 65536 ? blocks : 65536);
    if (pool)
        hipLaunchKernelGGL(splat_apply_kernel<true>, dim3(grid), dim3(256), 0, stream, u, att, out, (int)np, H, W, OH, OW, WV);
    else
        hipLaunchKernelGGL(splat_apply_kernel<false>, dim3(grid), dim3(256), 0, stream, u, att, out, (int)np, H, W, OH, OW, WV);
    CPR_LAUNCH_STATUS();
}

// grid (K, N): block (k, n) sums dv * u over its pixel chunk into ws[n][k][2w]
template <bool POOL>
__global__ __launch_bounds__(256) void splat_attn_grad_kernel(const float* __restrict__ dout, const float* __restrict__ u, float* __restrict__ ws,
                                                              int H, int W, int OH, int OW, int WV, int CH) {
    __shared__ f32x4 lds[512];
    const int cv = threadIdx.x % WV, prow = threadIdx.x / WV, PP = 256 / WV;
    const int k = blockIdx.x, n = blockIdx.y, HW = H * W;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (prow < PP) {
        const int end = min(HW, (k + 1) * CH);
        for (int p = k * CH + prow; p < end; p += PP) {
            const f32x4 dv = splat_dv<POOL>(dout, n, p / W, p % W, H, W, OH, OW, WV, cv);
            const f32x4* px = reinterpret_cast<const f32x4*>(u) + ((size_t)n * HW + p) * 2 * WV;
            acc[0] += dv * px[cv];
            acc[1] += dv * px[WV + cv];
        }
    }
    splat_block_sum<2>(acc, lds, prow, cv, PP, WV);
    if (prow == 0) {
        f32x4* o = reinterpret_cast<f32x4*>(ws) + ((size_t)n * gridDim.x + k) * 2 * WV;
        o[cv] = acc[0];
        o[WV + cv] = acc[1];
    }
}

extern "C" int cpr_splat_attn_grad(const float* dout, const float* u, float* datt, float* ws, int N, int H, int W, int w, int pool,
                                   hipStream_t stream) {
    CPR_CHECK_ARG(dout && u && datt && ws && N > 0 && N <= 65535 && H > 0 && W > 0 && w > 0 && w % 4 == 0 && w <= SPLAT_MAX_W &&
                  (pool == 0 || pool == 1));
    const long long hw = (long long)H * W;
    if (hw * N >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    const int OH = pool ? (H - 1) / 2 + 1 : H, OW = pool ? (W - 1) / 2 + 1 : W;
    const int K = (int)cdivll(hw, splat_chunk(w));
    if (pool)
        hipLaunchKernelGGL(splat_attn_grad_kernel<true>, dim3(K, N), dim3(256), 0, stream, dout, u, ws, H, W, OH, OW, w / 4, splat_chunk(w));
    else
        hipLaunchKernelGGL(splat_attn_grad_kernel<false>, dim3(K, N), dim3(256), 0, stream, dout, u, ws, H, W, OH, OW, w / 4, splat_chunk(w));
    splat_rows_sum(ws, datt, N, K, 2 * w, 1.f, stream);
    CPR_LAUNCH_STATUS();
}

// per image: da (2w), dh' (inter), dh (inter), xhat (inter) into ws[n][2w + 3 * inter], dg[n][w]
__global__ __launch_bounds__(SPLAT_ATTN_THREADS) void splat_attn_bwd_kernel(const float* __restrict__ att, const float* __restrict__ datt, const float* __restrict__ z,
                                                             const float* __restrict__ g, const float* __restrict__ fc1w,
                                                             const float* __restrict__ fc1b, const float* __restrict__ s1,
                                                             const float* __restrict__ mean, const float* __restrict__ inv_sigma,
                                                             const float* __restrict__ fc2w, float* __restrict__ dg, float* __restrict__ ws,
                                                             int w, int inter) {
    __shared__ float sg[SPLAT_MAX_W], sda[2 * SPLAT_MAX_W], sdh[SPLAT_MAX_INTER];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x, NW = NT >> 6;
    float* wn = ws + (size_t)n * (2 * w + 3 * inter);
    float *wda = wn, *wdhp = wn + 2 * w, *wdh = wdhp + inter, *wxh = wdh + inter;
    for (int c = tid; c < w; c += NT) {
        sg[c] = g[(size_t)n * w + c];
        const float a0 = att[(size_t)n * 2 * w + c], a1 = att[(size_t)n * 2 * w + w + c];
        const float d0 = datt[(size_t)n * 2 * w + c], d1 = datt[(size_t)n * 2 * w + w + c];
        const float s = a0 * d0 + a1 * d1;
        const float da0 = a0 * (d0 - s), da1 = a1 * (d1 - s);
        sda[c] = da0;
        sda[w + c] = da1;
        wda[c] = da0;
        wda[w + c] = da1;
    }
    __syncthreads();
    // xhat of the folded BatchNorm: the pre-norm h = fc1 g + b1 once more (the forward's arithmetic)
    for (int j = wave; j < inter; j += NW) {
        const float h = splat_row_dot(fc1w + (size_t)j * w, sg, w, lane) + fc1b[j];
        if (lane == 0) wxh[j] = (h - mean[j]) * inv_sigma[j];
    }
    // dz = fc2^T da: thread j walks the rows k of fc2 (2w, inter) in ascending order, lanes on consecutive j
    for (int j = tid; j < inter; j += NT) {
        float s = 0.f;
        for (int k = 0; k < 2 * w; ++k) s = fmaf(fc2w[(size_t)k * inter + j], sda[k], s);
        const float dhp = z[(size_t)n * inter + j] > 0.f ? s : 0.f;
        const float dh = s1[j] * dhp;
        wdhp[j] = dhp;
        wdh[j] = dh;
        sdh[j] = dh;
    }
    __syncthreads();
    for (int c = tid; c < w; c += NT) {
        float s = 0.f;
        for (int j = 0; j < inter; ++j) s = fmaf(fc1w[(size_t)j * w + c], sdh[j], s);
        dg[(size_t)n * w + c] = s;
    }
}

// the six parameter gradients, one thread per element, images in ascending order.  Element ranges in turn: fc2.weight (2w * inter),
// fc2.bias (2w), fc1.weight (inter * w), fc1.bias (inter), bn1.weight (inter), bn1.bias (inter)
__global__ __launch_bounds__(256) void splat_attn_params_kernel(const float* __restrict__ ws, const float* __restrict__ z, const float* __restrict__ g,
                                                                float* __restrict__ gfc1w, float* __restrict__ gfc1b, float* __restrict__ gbnw,
                                                                float* __restrict__ gbnb, float* __restrict__ gfc2w, float* __restrict__ gfc2b,
                                                                int N, int w, int inter) {
    const int R = 2 * w + 3 * inter;
    long long i = blockIdx.x * 256ll + threadIdx.x;
    const float *a, *b = nullptr;          // sum over n of a[n * sa] (* b[n * sb])
    int sa = R, sb = 0;
    float* out;
    if (i < 2ll * w * inter) {
        const int k = (int)(i / inter), j = (int)(i % inter);
        a = ws + k, b = z + j, sb = inter, out = gfc2w ? gfc2w + i : nullptr;
    } else if ((i -= 2ll * w * inter) < 2 * w) {
        a = ws + i, out = gfc2b ? gfc2b + i : nullptr;
    } else if ((i -= 2 * w) < (long long)inter * w) {
        const int j = (int)(i / w), c = (int)(i % w);
        a = ws + 2 * w + inter + j, b = g + c, sb = w, out = gfc1w ? gfc1w + i : nullptr;
    } else if ((i -= (long long)inter * w) < inter) {
        a = ws + 2 * w + inter + i, out = gfc1b ? gfc1b + i : nullptr;
    } else if ((i -= inter) < inter) {
        a = ws + 2 * w + i, b = ws + 2 * w + 2 * inter + i, sb = R, out = gbnw ? gbnw + i : nullptr;
    } else if ((i -= inter) < inter) {
        a = ws + 2 * w + i, out = gbnb ? gbnb + i : nullptr;
    } else {
        return;
    }
    if (!out) return;
    float s = 0.f;
    if (b)
        for (int n = 0; n < N; ++n) s = fmaf(a[(size_t)n * sa], b[(size_t)n * sb], s);
    else
        for (int n = 0; n < N; ++n) s += a[(size_t)n * sa];
    *out = s;
}

extern "C" int cpr_splat_attn_bwd(const float* att, const float* datt, const float* z, const float* g, const float* fc1w, const float* fc1b,
                                  const float* s1, const float* mean, const float* inv_sigma, const float* fc2w, float* dg, float* ws,
                                  float* gfc1w, float* gfc1b, float* gbnw, float* gbnb, float* gfc2w, float* gfc2b, int N, int w, int inter,
                                  hipStream_t stream) {
    CPR_CHECK_ARG(att && datt && z && g && fc1w && fc1b && s1 && mean && inv_sigma && fc2w && dg && ws && N > 0 && w > 0 && w % 4 == 0 &&
                  w <= SPLAT_MAX_W && inter > 0 && inter <= SPLAT_MAX_INTER);
    hipLaunchKernelGGL(splat_attn_bwd_kernel, dim3(N), dim3(SPLAT_ATTN_THREADS), 0, stream, att, datt, z, g, fc1w, fc1b, s1, mean, inv_sigma, fc2w, dg, ws, w,
                       inter);
    if (gfc1w || gfc1b || gbnw || gbnb || gfc2w || gfc2b) {
        const long long total = 2ll * w * inter + 2 * w + (long long)inter * w + 3 * inter;
        hipLaunchKernelGGL(splat_attn_params_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, ws, z, g, gfc1w, gfc1b, gbnw,
                           gbnb, gfc2w, gfc2b, N, w, inter);
    }
    CPR_LAUNCH_STATUS();
}

// grid (K, N): block (k, n) writes du over its pixel chunk and its column sums into ws[n][k][2w]
template <bool POOL>
__global__ __launch_bounds__(256) void splat_apply_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ u, const float* __restrict__ att,
                                                              const float* __restrict__ dg, float* __restrict__ du, float* __restrict__ ws,
                                                              int H, int W, int OH, int OW, int WV, int CH, float inv_hw) {
    __shared__ f32x4 lds[512];
    const int cv = threadIdx.x % WV, prow = threadIdx.x / WV, PP = 256 / WV;
    const int k = blockIdx.x, n = blockIdx.y, HW = H * W;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (prow < PP) {
        const f32x4 a0 = reinterpret_cast<const f32x4*>(att)[(size_t)n * 2 * WV + cv];
        const f32x4 a1 = reinterpret_cast<const f32x4*>(att)[(size_t)n * 2 * WV + WV + cv];
        const f32x4 gm = reinterpret_cast<const f32x4*>(dg)[(size_t)n * WV + cv] * inv_hw;
        const int end = min(HW, (k + 1) * CH);
        for (int p = k * CH + prow; p < end; p += PP) {
            const f32x4 dv = splat_dv<POOL>(dout, n, p / W, p % W, H, W, OH, OW, WV, cv);
            const size_t base = ((size_t)n * HW + p) * 2 * WV;
            const f32x4 u0 = reinterpret_cast<const f32x4*>(u)[base + cv], u1 = reinterpret_cast<const f32x4*>(u)[base + WV + cv];
            f32x4 d0 = a0 * dv + gm, d1 = a1 * dv + gm;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                d0[e] = u0[e] > 0.f ? d0[e] : 0.f;
                d1[e] = u1[e] > 0.f ? d1[e] : 0.f;
            }
            reinterpret_cast<f32x4*>(du)[base + cv] = d0;
            reinterpret_cast<f32x4*>(du)[base + WV + cv] = d1;
            acc[0] += d0;
            acc[1] += d1;
        }
    }
    splat_block_sum<2>(acc, lds, prow, cv, PP, WV);
    if (prow == 0) {
        f32x4* o = reinterpret_cast<f32x4*>(ws) + ((size_t)n * gridDim.x + k) * 2 * WV;
        o[cv] = acc[0];
        o[WV + cv] = acc[1];
    }
}

extern "C" int cpr_splat_apply_bwd(const float* dout, const float* u, const float* att, const float* dg, float* du, float* colsum, float* ws,
                                   int N, int H, int W, int w, int pool, hipStream_t stream) {
    CPR_CHECK_ARG(dout && u && att && dg && du && colsum && ws && N > 0 && N <= 65535 && H > 0 && W > 0 && w > 0 && w % 4 == 0 &&
                  w <= SPLAT_MAX_W && (pool == 0 || pool == 1));
    const long long hw = (long long)H * W;
    if (hw * N >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    const int OH = pool ? (H - 1) / 2 + 1 : H, OW = pool ? (W - 1) / 2 + 1 : W;
    const int K = (int)cdivll(hw, splat_chunk(w));
    if (pool)
        hipLaunchKernelGGL(splat_apply_bwd_kernel<true>, dim3(K, N), dim3(256), 0, stream, dout, u, att, dg, du, ws, H, W, OH, OW, w / 4,
                           splat_chunk(w), 1.f / (float)hw);
    else
        hipLaunchKernelGGL(splat_apply_bwd_kernel<false>, dim3(K, N), dim3(256), 0, stream, dout, u, att, dg, du, ws, H, W, OH, OW, w / 4,
                           splat_chunk(w), 1.f / (float)hw);
    // the chunks of an image, then the images, each in ascending order
    float* per_image = ws + (size_t)N * K * 2 * w;
    splat_rows_sum(ws, per_image, N, K, 2 * w, 1.f, stream);
    splat_rows_sum(per_image, colsum, 1, N, 2 * w, 1.f, stream);
    CPR_LAUNCH_STATUS();
}
