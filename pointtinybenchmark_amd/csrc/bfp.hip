// BFP neck, the Balanced Feature Pyramid (T/mmdet/models/necks/bfp.py:69-101): two streaming passes over every pyramid level and their
// backward.  With r = refine_level and (h, w) the size of level r:
//   cpr_bfp_gather[_bf16]    bsf[n,y,x,c] = (sum_i feat_i[n,y,x,c]) / L;  feat_i = adaptive_max_pool2d(level_i, (h, w)) for i < r,
//                            nearest(level_i, (h, w)) for i >= r
//   cpr_bfp_scatter[_bf16]   out_i = residual_i + level_i;  residual_i = nearest(ref, size_i) for i < r, adaptive_max_pool2d(ref, size_i)
//                            for i >= r (level r: the identity)
//   cpr_bfp_scatter_bwd      d_ref = sum_i (g_i through nearest / max-pool backward)
//   cpr_bfp_gather_bwd       d_level_i = g_i + (d_bsf / L through max-pool / nearest backward)
// ONE launch each over a table of levels.  NHWC, 16 bytes of channels per lane in the forward passes (4 fp32 / 8 bf16; bf16: fp32
// arithmetic, one rounding at the store).  A level -- and the refined map of the scatter -- arrives materialised or as a raw conv output
// with the pending per-(image, channel) GroupNorm affine of its layer (and the refine layer's ReLU), applied ON LOAD, BEFORE the max:
// a negative `a` turns max into min on the raw values, so the pool does not commute with it.
//
// Index rules, restated from torch:
//   nearest       src = min((int)floorf((float)dst * scale), in - 1), scale = (float)in / (float)out formed by the HOST as one fp32
//                 division and passed in (the integer form dst * in / out differs from torch, e.g. in = 2, out = 82).
//   adaptive max  window i of an axis = [floor(i * in / out), ceil((i + 1) * in / out)); windows overlap when in % out != 0; ties go to the
//                 FIRST maximum in row-major order (strict >, torch's rule), an all -inf window to its origin.
// Recording (training): the argmax of every window as a window-local code, (ly << 4 | lx) in a uint8 when no window side exceeds 16, else
// (ly << 8 | lx) in a uint16.  The backward passes are in gather form -- each output cell walks the cells that route to it (the contiguous
// nearest pre-image; the windows that contain it and whose recorded argmax names it) -- so there are no atomics and the summation order
// is fixed: levels ascending, then rows, then columns.  Every cell is computed by one lane from its own image alone: bit-repeatable and
// independent of the batch size.
#include "common.h"

#define BFP_MAX_LEVELS 8

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

struct BfpLevel {       // include/cpr_hip.h: cpr_bfp_level
    const void* x;
    const float* a;
    const float* b;
    void* y;
    void* arg;
    int H, W;
    float sy, sx;
};

struct BfpTable {
    int L, r, h, w, wide;
    long long off[BFP_MAX_LEVELS + 1];      // scatter / gather_bwd: first flat (pixel, channel vector) index of every level
    BfpLevel lv[BFP_MAX_LEVELS];
};

__device__ __forceinline__ int nn_src(int d, float scale, int in) {
    const int s = (int)floorf(__fmul_rn((float)d, scale));
    return s < in - 1 ? s : in - 1;
}
// the first d in [0, out] with nn_src(d) >= s: [nn_first(s), nn_first(s + 1)) is the pre-image of source cell s.  The integer estimate is
// corrected with the float rule itself, so the pre-images are exactly torch's.
__device__ __forceinline__ int nn_first(int s, float scale, int in, int out) {
    if (s <= 0) return 0;
    if (s > in - 1) return out;
    long long e = ((long long)s * out + in - 1) / in;
    int d = e > out ? out : (int)e;
    while (d > 0 && nn_src(d - 1, scale, in) >= s) --d;
    while (d < out && nn_src(d, scale, in) < s) ++d;
    return d;
}
// adaptive pooling of an axis of `in` cells to `out` windows
__device__ __forceinline__ int win_lo(int i, int in, int out) { return (int)(((long long)i * in) / out); }
__device__ __forceinline__ int win_hi(int i, int in, int out) { return (int)((((long long)i + 1) * in + out - 1) / out); }
// the windows that contain cell c: [first, last]
__device__ __forceinline__ int win_first(int c, int in, int out) { return (int)(((long long)c * out) / in); }
__device__ __forceinline__ int win_last(int c, int in, int out) {
    const int i = (int)((((long long)c + 1) * out - 1) / in);
    return i < out - 1 ? i : out - 1;
}

template <bool BF16>
__device__ __forceinline__ void ldv(const void* p, size_t vec, float (&v)[BF16 ? 8 : 4]) {
    if constexpr (BF16) {
        const uint4 u = reinterpret_cast<const uint4*>(p)[vec];
        v[0] = __uint_as_float(u.x << 16), v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16), v[3] = __uint_as_float(u.y & 0xffff0000u);
        v[4] = __uint_as_float(u.z << 16), v[5] = __uint_as_float(u.z & 0xffff0000u);
        v[6] = __uint_as_float(u.w << 16), v[7] = __uint_as_float(u.w & 0xffff0000u);
    } else {
        const f32x4 t = reinterpret_cast<const f32x4*>(p)[vec];
        v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
    }
}

template <bool BF16>
__device__ __forceinline__ void stv(void* p, size_t vec, const float (&v)[BF16 ? 8 : 4]) {
    if constexpr (BF16) {
        uint4 o;
        o.x = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v[0], (__bf16)v[1]});
        o.y = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v[2], (__bf16)v[3]});
        o.z = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v[4], (__bf16)v[5]});
        o.w = __builtin_bit_cast(unsigned, bf16x2_t{(__bf16)v[6], (__bf16)v[7]});
        reinterpret_cast<uint4*>(p)[vec] = o;
    } else {
        reinterpret_cast<f32x4*>(p)[vec] = f32x4{v[0], v[1], v[2], v[3]};
    }
}

template <int V>
__device__ __forceinline__ void ld_affine(const float* a, const float* b, size_t t, float (&A)[V], float (&B)[V]) {
#pragma unroll
    for (int k = 0; k < V; k += 4) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(a + t + k), q = *reinterpret_cast<const f32x4*>(b + t + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) A[k + j] = p[j], B[k + j] = q[j];
    }
}

// the V window codes of one (cell, channel vector): element index e = cell * C + first channel
template <int V>
__device__ __forceinline__ void st_codes(void* arg, size_t e, const int (&code)[V], int wide) {
    if (wide) {
        unsigned short* p = reinterpret_cast<unsigned short*>(arg) + e;
#pragma unroll
        for (int k = 0; k < V; k += 2) *reinterpret_cast<unsigned*>(p + k) = (unsigned)code[k] | ((unsigned)code[k + 1] << 16);
    } else {
        unsigned char* p = reinterpret_cast<unsigned char*>(arg) + e;
#pragma unroll
        for (int k = 0; k < V; k += 4)
            *reinterpret_cast<unsigned*>(p + k) = (unsigned)code[k] | ((unsigned)code[k + 1] << 8) | ((unsigned)code[k + 2] << 16) |
                                                  ((unsigned)code[k + 3] << 24);
    }
}
__device__ __forceinline__ void ld_codes4(const void* arg, size_t e, int (&code)[4], int wide) {
    if (wide) {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(arg) + e);
        code[0] = u.x & 0xffff, code[1] = u.x >> 16, code[2] = u.y & 0xffff, code[3] = u.y >> 16;
    } else {
        const unsigned u = *reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(arg) + e);
        code[0] = u & 0xff, code[1] = (u >> 8) & 0xff, code[2] = (u >> 16) & 0xff, code[3] = u >> 24;
    }
}

// the max of the window [y0, y1) x [x0, x1) of image n of a (., IH, IW, C) map under its affine (and ReLU), first maximum, with its code
template <bool BF16, bool RELU>
__device__ __forceinline__ void window_max(const void* x, bool aff, const float (&A)[BF16 ? 8 : 4], const float (&B)[BF16 ? 8 : 4], int n,
                                           int IH, int IW, int CV, int cg, int y0, int y1, int x0, int x1, int shift,
                                           float (&m)[BF16 ? 8 : 4], int (&code)[BF16 ? 8 : 4]) {
    constexpr int V = BF16 ? 8 : 4;
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = -INFINITY, code[k] = 0;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            float v[V];
            ldv<BF16>(x, (((size_t)n * IH + yy) * IW + xx) * CV + cg, v);
            const int local = ((yy - y0) << shift) | (xx - x0);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float t = aff ? v[k] * A[k] + B[k] : v[k];
                if (RELU) t = aff ? fmaxf(t, 0.f) : t;
                if (t > m[k]) m[k] = t, code[k] = local;
            }
        }
}

// one lane: one (bsf cell, channel vector); total = N * h * w * CV
template <bool BF16>
__global__ __launch_bounds__(256) void bfp_gather_kernel(const BfpTable t, void* __restrict__ bsf, int CV, long long total) {
    constexpr int V = BF16 ? 8 : 4;
    const long long idx = blockIdx.x * 256ll + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % CV), C = CV * V;
    const long long pix = idx / CV;
    const int x = (int)(pix % t.w), y = (int)((pix / t.w) % t.h), n = (int)(pix / ((long long)t.w * t.h));
    const int shift = t.wide ? 8 : 4;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int i = 0; i < t.L; ++i) {
        const BfpLevel& lv = t.lv[i];
        const bool aff = lv.a != nullptr;
        float A[V], B[V], m[V];
        if (aff) ld_affine<V>(lv.a, lv.b, (size_t)n * C + cg * V, A, B);
        if (i < t.r) {
            int code[V];
            window_max<BF16, false>(lv.x, aff, A, B, n, lv.H, lv.W, CV, cg, win_lo(y, lv.H, t.h), win_hi(y, lv.H, t.h),
                                    win_lo(x, lv.W, t.w), win_hi(x, lv.W, t.w), shift, m, code);
            if (lv.arg) st_codes<V>(lv.arg, (size_t)pix * C + cg * V, code, t.wide);
        } else {
            const int sy = nn_src(y, lv.sy, lv.H), sx = nn_src(x, lv.sx, lv.W);
            ldv<BF16>(lv.x, (((size_t)n * lv.H + sy) * lv.W + sx) * CV + cg, m);
            if (aff) {
#pragma unroll
                for (int k = 0; k < V; ++k) m[k] = m[k] * A[k] + B[k];
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += m[k];
    }
    const float Lf = (float)t.L;
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = __fdiv_rn(acc[k], Lf);
    stv<BF16>(bsf, (size_t)idx, acc);
}

// the level of a flat index over the levels' (pixel, channel vector)s
__device__ __forceinline__ int level_of(const BfpTable& t, long long idx) {
    int i = 0;
    while (i + 1 < t.L && idx >= t.off[i + 1]) ++i;
    return i;
}

// one lane: one (level cell, channel vector) of any level; ref: the refined map (N, h, w, C), raw under (ra, rb) + ReLU when ra is given
template <bool BF16>
__global__ __launch_bounds__(256) void bfp_scatter_kernel(const BfpTable t, const void* __restrict__ ref, const float* __restrict__ ra,
                                                          const float* __restrict__ rb, int CV, long long total) {
    constexpr int V = BF16 ? 8 : 4;
    const long long idx = blockIdx.x * 256ll + threadIdx.x;
    if (idx >= total) return;
    const int i = level_of(t, idx);
    const BfpLevel& lv = t.lv[i];
    const long long loc = idx - t.off[i];
    const int cg = (int)(loc % CV), C = CV * V;
    const long long pix = loc / CV;
    const int x = (int)(pix % lv.W), y = (int)((pix / lv.W) % lv.H), n = (int)(pix / ((long long)lv.W * lv.H));
    const size_t ab = (size_t)n * C + cg * V;
    float v[V], A[V], B[V], RA[V], RB[V], res[V];
    ldv<BF16>(lv.x, (size_t)loc, v);
    if (lv.a) {
        ld_affine<V>(lv.a, lv.b, ab, A, B);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = v[k] * A[k] + B[k];
    }
    const bool raff = ra != nullptr;
    if (raff) ld_affine<V>(ra, rb, ab, RA, RB);
    if (i < t.r) {
        const int sy = nn_src(y, lv.sy, t.h), sx = nn_src(x, lv.sx, t.w);
        ldv<BF16>(ref, (((size_t)n * t.h + sy) * t.w + sx) * CV + cg, res);
        if (raff) {
#pragma unroll
            for (int k = 0; k < V; ++k) res[k] = fmaxf(res[k] * RA[k] + RB[k], 0.f);
        }
    } else {
        int code[V];
        window_max<BF16, true>(ref, raff, RA, RB, n, t.h, t.w, CV, cg, win_lo(y, t.h, lv.H), win_hi(y, t.h, lv.H), win_lo(x, t.w, lv.W),
                               win_hi(x, t.w, lv.W), t.wide ? 8 : 4, res, code);
        if (lv.arg && i > t.r) st_codes<V>(lv.arg, (size_t)pix * C + cg * V, code, t.wide);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = res[k] + v[k];
    stv<BF16>(lv.y, (size_t)loc, v);
}

// one lane: one (bsf cell, 4 channels); lv.x = g_i (fp32, the level's shape), lv.arg = the scatter's record (levels > r); CV = C / 4
__global__ __launch_bounds__(256) void bfp_scatter_bwd_kernel(const BfpTable t, float* __restrict__ d_ref, int CV, long long total) {
    const long long idx = blockIdx.x * 256ll + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % CV), C = CV * 4;
    const long long pix = idx / CV;
    const int x = (int)(pix % t.w), y = (int)((pix / t.w) % t.h), n = (int)(pix / ((long long)t.w * t.h));
    const int shift = t.wide ? 8 : 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < t.L; ++i) {
        const BfpLevel& lv = t.lv[i];
        const f32x4* g = reinterpret_cast<const f32x4*>(lv.x);
        if (i < t.r) {          // nearest (h, w) -> (H, W): this cell's contiguous pre-image in the level
            const int y0 = nn_first(y, lv.sy, t.h, lv.H), y1 = nn_first(y + 1, lv.sy, t.h, lv.H);
            const int x0 = nn_first(x, lv.sx, t.w, lv.W), x1 = nn_first(x + 1, lv.sx, t.w, lv.W);
            for (int yy = y0; yy < y1; ++yy)
                for (int xx = x0; xx < x1; ++xx) acc += g[(((size_t)n * lv.H + yy) * lv.W + xx) * CV + cg];
        } else if (i == t.r) {
            acc += g[idx];
        } else {                // adaptive max (h, w) -> (H, W): the coarse cells whose window holds this cell and whose argmax names it
            const int cy0 = win_first(y, t.h, lv.H), cy1 = win_last(y, t.h, lv.H), cx0 = win_first(x, t.w, lv.W), cx1 = win_last(x, t.w, lv.W);
            for (int cy = cy0; cy <= cy1; ++cy)
                for (int cx = cx0; cx <= cx1; ++cx) {
                    const int local = ((y - win_lo(cy, t.h, lv.H)) << shift) | (x - win_lo(cx, t.w, lv.W));
                    const size_t cell = ((size_t)n * lv.H + cy) * lv.W + cx;
                    int code[4];
                    ld_codes4(lv.arg, cell * C + cg * 4, code, t.wide);
                    const f32x4 gv = g[cell * CV + cg];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] += code[k] == local ? gv[k] : 0.f;
                }
        }
    }
    reinterpret_cast<f32x4*>(d_ref)[idx] = acc;
}

// one lane: one (level cell, 4 channels) of any level; lv.x = g_i, lv.y = d_level_i (fp32), lv.arg = the gather's record (levels < r)
__global__ __launch_bounds__(256) void bfp_gather_bwd_kernel(const BfpTable t, const float* __restrict__ d_bsf, int CV, long long total) {
    const long long idx = blockIdx.x * 256ll + threadIdx.x;
    if (idx >= total) return;
    const int i = level_of(t, idx);
    const BfpLevel& lv = t.lv[i];
    const long long loc = idx - t.off[i];
    const int cg = (int)(loc % CV), C = CV * 4;
    const long long pix = loc / CV;
    const int x = (int)(pix % lv.W), y = (int)((pix / lv.W) % lv.H), n = (int)(pix / ((long long)lv.W * lv.H));
    const int shift = t.wide ? 8 : 4;
    const float Lf = (float)t.L;
    const f32x4* d = reinterpret_cast<const f32x4*>(d_bsf);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (i < t.r) {              // adaptive max (H, W) -> (h, w): the bsf cells whose window holds this cell and whose argmax names it
        const int by0 = win_first(y, lv.H, t.h), by1 = win_last(y, lv.H, t.h), bx0 = win_first(x, lv.W, t.w), bx1 = win_last(x, lv.W, t.w);
        for (int by = by0; by <= by1; ++by)
            for (int bx = bx0; bx <= bx1; ++bx) {
                const int local = ((y - win_lo(by, lv.H, t.h)) << shift) | (x - win_lo(bx, lv.W, t.w));
                const size_t cell = ((size_t)n * t.h + by) * t.w + bx;
                int code[4];
                ld_codes4(lv.arg, cell * C + cg * 4, code, t.wide);
                const f32x4 dv = d[cell * CV + cg];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += code[k] == local ? __fdiv_rn(dv[k], Lf) : 0.f;
            }
    } else {                    // nearest (H, W) -> (h, w): this cell's contiguous pre-image in bsf
        const int y0 = nn_first(y, lv.sy, lv.H, t.h), y1 = nn_first(y + 1, lv.sy, lv.H, t.h);
        const int x0 = nn_first(x, lv.sx, lv.W, t.w), x1 = nn_first(x + 1, lv.sx, lv.W, t.w);
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) {
                const f32x4 dv = d[(((size_t)n * t.h + yy) * t.w + xx) * CV + cg];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += __fdiv_rn(dv[k], Lf);
            }
    }
    const f32x4 g = reinterpret_cast<const f32x4*>(lv.x)[loc];
    reinterpret_cast<f32x4*>(lv.y)[loc] = g + acc;
}

// ------------------------------------------------------------------------------------------------ launchers
static int max_window(int in, int out) {        // the widest adaptive-pooling window of an axis
    int m = 0;
    for (int i = 0; i < out; ++i) {
        const int s = (int)(((long long)i * in) / out), e = (int)((((long long)i + 1) * in + out - 1) / out);
        m = e - s > m ? e - s : m;
    }
    return m;
}

// The table as the kernels take it.  V: channels per lane; pooled_fine: the levels < r are pooled to (h, w) (gather and its backward),
// else the levels > r are pooled from (h, w) (scatter and its backward); need_y / need_arg: which pointers every level must bring.
static int bfp_table(const BfpLevel* levels, int L, int r, int N, int C, int V, int arg_wide, bool fine_side, bool need_y, bool need_arg,
                     bool flat, BfpTable& t, long long& total) {
    CPR_CHECK_ARG(levels && L >= 1 && L <= BFP_MAX_LEVELS && r >= 0 && r < L && N > 0 && C > 0 && C % V == 0);
    t.L = L, t.r = r, t.h = levels[r].H, t.w = levels[r].W, t.wide = arg_wide ? 1 : 0;
    CPR_CHECK_ARG(t.h > 0 && t.w > 0);
    const int CV = C / V, cap = arg_wide ? 256 : 16;
    long long off = 0;
    for (int i = 0; i < L; ++i) {
        const BfpLevel& lv = levels[i];
        CPR_CHECK_ARG(lv.x && lv.H > 0 && lv.W > 0 && (lv.a == nullptr) == (lv.b == nullptr) && (!need_y || lv.y));
        const bool pooled = fine_side ? i < r : i > r;
        if (pooled && (need_arg || lv.arg)) {
            CPR_CHECK_ARG(lv.arg);
            const int wy = fine_side ? max_window(lv.H, t.h) : max_window(t.h, lv.H);
            const int wx = fine_side ? max_window(lv.W, t.w) : max_window(t.w, lv.W);
            if (wy > cap || wx > cap) return CPR_ERR_UNSUPPORTED;
        }
        t.lv[i] = lv;
        t.off[i] = off;
        off += (long long)N * lv.H * lv.W * CV;
        CPR_CHECK_ARG((long long)N * lv.H * lv.W * C < (1ll << 31));
    }
    t.off[L] = off;
    total = flat ? off : (long long)N * t.h * t.w * CV;
    CPR_CHECK_ARG(total < (1ll << 31) * 256);
    return CPR_OK;
}

template <bool BF16>
static int bfp_gather_launch(const BfpLevel* levels, int L, int r, void* bsf, int N, int C, int arg_wide, hipStream_t stream) {
    constexpr int V = BF16 ? 8 : 4;
    BfpTable t{};
    long long total = 0;
    CPR_CHECK_ARG(bsf);
    const int st = bfp_table(levels, L, r, N, C, V, arg_wide, true, false, false, false, t, total);
    if (st != CPR_OK) return st;
    hipLaunchKernelGGL(bfp_gather_kernel<BF16>, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, t, bsf, C / V, total);
    CPR_LAUNCH_STATUS();
}

template <bool BF16>
static int bfp_scatter_launch(const BfpLevel* levels, int L, int r, const void* ref, const float* ra, const float* rb, int N, int C,
                              int arg_wide, hipStream_t stream) {
    constexpr int V = BF16 ? 8 : 4;
    BfpTable t{};
    long long total = 0;
    CPR_CHECK_ARG(ref && (ra == nullptr) == (rb == nullptr));
    const int st = bfp_table(levels, L, r, N, C, V, arg_wide, false, true, false, true, t, total);
    if (st != CPR_OK) return st;
    hipLaunchKernelGGL(bfp_scatter_kernel<BF16>, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, t, ref, ra, rb, C / V, total);
    CPR_LAUNCH_STATUS();
}

extern "C" int cpr_bfp_gather(const BfpLevel* levels, int L, int refine_level, float* bsf, int N, int C, int arg_wide, hipStream_t stream) {
    return bfp_gather_launch<false>(levels, L, refine_level, bsf, N, C, arg_wide, stream);
}
extern "C" int cpr_bfp_gather_bf16(const BfpLevel* levels, int L, int refine_level, void* bsf, int N, int C, int arg_wide,
                                   hipStream_t stream) {
    return bfp_gather_launch<true>(levels, L, refine_level, bsf, N, C, arg_wide, stream);
}
extern "C" int cpr_bfp_scatter(const BfpLevel* levels, int L, int refine_level, const float* ref, const float* ref_a, const float* ref_b,
                               int N, int C, int arg_wide, hipStream_t stream) {
    return bfp_scatter_launch<false>(levels, L, refine_level, ref, ref_a, ref_b, N, C, arg_wide, stream);
}
extern "C" int cpr_bfp_scatter_bf16(const BfpLevel* levels, int L, int refine_level, const void* ref, const float* ref_a,
                                    const float* ref_b, int N, int C, int arg_wide, hipStream_t stream) {
    return bfp_scatter_launch<true>(levels, L, refine_level, ref, ref_a, ref_b, N, C, arg_wide, stream);
}
extern "C" int cpr_bfp_scatter_bwd(const BfpLevel* levels, int L, int refine_level, float* d_ref, int N, int C, int arg_wide,
                                   hipStream_t stream) {
    BfpTable t{};
    long long total = 0;
    CPR_CHECK_ARG(d_ref);
    const int st = bfp_table(levels, L, refine_level, N, C, 4, arg_wide, false, false, true, false, t, total);
    if (st != CPR_OK) return st;
    hipLaunchKernelGGL(bfp_scatter_bwd_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, t, d_ref, C / 4, total);
    CPR_LAUNCH_STATUS();
}
extern "C" int cpr_bfp_gather_bwd(const BfpLevel* levels, int L, int refine_level, const float* d_bsf, int N, int C, int arg_wide,
                                  hipStream_t stream) {
    BfpTable t{};
    long long total = 0;
    CPR_CHECK_ARG(d_bsf);
    const int st = bfp_table(levels, L, refine_level, N, C, 4, arg_wide, true, true, true, true, t, total);
    if (st != CPR_OK) return st;
    hipLaunchKernelGGL(bfp_gather_bwd_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, t, d_bsf, C / 4, total);
    CPR_LAUNCH_STATUS();
}
