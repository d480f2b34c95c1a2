// Transposed convolution 4x4 / stride 2 / padding 1 (nn.ConvTranspose2d(Cin, Cout, 4, 2, 1, bias=False)) on the CDNA4 matrix cores,
// exact fp32 (v_mfma_f32_32x32x2_f32): the upsampling layers of CTResNetNeck (T/mmdet/models/necks/ct_resnet_neck.py:41-71).
//
//   y[n, 2i+a, 2j+b, co] = sum_ci sum_{t,u in {0,1}} x[n, i + a - t, j + b - u, ci] * w[ci, co, 1 - a + 2t, 1 - b + 2u]
//
// An output pixel of parity class (a, b) is reached by exactly 2 x 2 of the 16 taps (kh = a + 1 mod 2, kw = b + 1 mod 2), so every
// class is an implicit GEMM of its own over the INPUT-resolution pixels: M = N*H*W, N = Cout, K = 4*Cin, K ordered (t, u, ci) -- tap
// row t reads input row i + a - t, tap column u reads input column j + b - u; taps outside the map contribute zero.  One launch runs
// all four classes (the class is part of the tile index) and writes the interleaved (N, 2H, 2W, Cout) map directly: no zero
// insertion, no scatter pass, no atomics; each output element is one k-ordered fp32 chain whose order depends on nothing but K.
//
// The GEMM is the 64 x 64 x 32 tile of csrc/conv_mfma.hip with its interleaved K loop (one register set): 256 threads = 4 waves
// (2 x 2), double-buffered LDS rows padded to 36 floats, register-staged loads through buffer descriptors whose range check IS the
// zero padding.  The weight operand is the per-class image cpr_pack_weights_deconv writes: [class = 2a + b][Cout][4*Cin].
// Epilogue: y = acc * scale[c] + bias[c] (ReLU) -- eval-mode BatchNorm folded -- or the raw sums with neither operand.
#include <type_traits>
#include "common.h"

struct DeconvParams {
    const float* in;        // (N, H, W, Cin)
    const float* wgt;       // [4][Cout][4*Cin]
    float* out;             // (N, 2H, 2W, Cout)
    const float* scale;     // [Cout] or null
    const float* bias;      // [Cout] or null
    int N, H, W, Cin, Cout, M, K, relu, tilesM, tilesN;
};

constexpr int DBK = 32;
constexpr int DLDSW = 36;  // padded row (floats)

template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void deconv4x4s2_kernel(DeconvParams p) {
    constexpr int WM = BM / 2;
    constexpr int WN = BN / 2;
    constexpr int MI = WM / 32;
    constexpr int NI = WN / 32;
    constexpr int AL = BM * 8 / 256;  // float4 A loads per thread
    constexpr int BL = BN * 8 / 256;  // float4 B loads per thread
    __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * DLDSW];
    __shared__ unsigned orow[BM];     // byte offset of output pixel (n, 2i + a, 2j + b) of tile row r, 2^31 = no such row
    float* As = smem;
    float* Bs = smem + 2 * BM * DLDSW;

    // tile order (pixel tile, class, cout tile), cout tiles fastest; each XCD (block b runs on XCD b % 8) takes a contiguous run, so
    // the four classes of a pixel tile, which read the same 3 x 3 input neighbourhood, share one L2
    const int T = p.tilesM * 4 * p.tilesN;
    const int per = (T + 7) >> 3;
    const int tile = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (tile >= T) return;
    const int tm = tile / (4 * p.tilesN);
    const int rest = tile - tm * 4 * p.tilesN;
    const int cls = rest / p.tilesN, tn = rest - cls * p.tilesN;
    const int pa = cls >> 1, pb = cls & 1;
    const int m0 = tm * BM, n0 = tn * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c4 = tid & 7, r0 = tid >> 3;
    const int hw = p.H * p.W;

    if (tid < BM) {
        const int m = m0 + tid;
        unsigned off = 0x80000000u;
        if (m < p.M) {
            const int n = m / hw;
            const int rem = m - n * hw;
            const int i = rem / p.W, j = rem - i * p.W;
            off = (unsigned)(((n * 2 * p.H + 2 * i + pa) * 2 * p.W + 2 * j + pb) * p.Cout) * 4u;
        }
        orow[tid] = off;
    }

    // ---- per-thread A row descriptors (AL rows: r0 + 32 j): the input pixel of tap (0, 0)
    int iy0[AL], ix0[AL], rowoff[AL];
    bool mok[AL];
#pragma unroll
    for (int j = 0; j < AL; ++j) {
        const int m = m0 + r0 + 32 * j;
        mok[j] = m < p.M;
        const int mm = mok[j] ? m : 0;
        const int n = mm / hw;
        const int rem = mm - n * hw;
        const int i = rem / p.W;
        iy0[j] = i + pa;
        ix0[j] = rem - i * p.W + pb;
        rowoff[j] = ((n * p.H + iy0[j]) * p.W + ix0[j]) * p.Cin + c4 * 4;     // only used when the tap's pixel is in range
    }
    // Buffer descriptors: out-of-range offsets return 0, which IS the zero contribution of a tap outside the map
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in), 0, (int)((size_t)p.N * hw * p.Cin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.wgt) + (size_t)cls * p.Cout * p.K, 0, (int)((size_t)p.Cout * p.K * 4), 0x00020000);
    int woff[BL];  // byte offset of this thread's float4 in weight row j (-1 = row beyond Cout -> reads 0)
#pragma unroll
    for (int j = 0; j < BL; ++j) {
        const int c = n0 + r0 + 32 * j;
        woff[j] = c < p.Cout ? (c * p.K + c4 * 4) * 4 : -1;
    }

    f32x4 ra[AL], rb[BL];
    int tapoff = 0;              // byte offset of the current channel chunk (wave-uniform)
    int kt_ = 0, ku = 0, c0 = 0; // running tap state: tap row, tap column, channel chunk
    int voffA[AL];
    // per-row byte offsets (or -1 = outside the map) are invariant while the tap stays the same, i.e. for Cin/32 consecutive K-chunks
    auto refresh_rows = [&]() {
        const int tapshift = (kt_ * p.W + ku) * p.Cin;
#pragma unroll
        for (int j = 0; j < AL; ++j) {
            const int iy = iy0[j] - kt_, ix = ix0[j] - ku;
            const bool ok = mok[j] & ((unsigned)iy < (unsigned)p.H) & ((unsigned)ix < (unsigned)p.W);
            voffA[j] = ok ? (rowoff[j] - tapshift) * 4 : -1;
        }
    };
    refresh_rows();
    auto load_a = [&](int j) {
        if (j == 0) tapoff = c0 * 4;
        ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_in, voffA[j], tapoff, 0));
    };
    auto load_x_advance = [&]() {  // after the last A row of a tile: next channel chunk, then next tap
        c0 += DBK;
        if (c0 == p.Cin) {  // wave-uniform, once per Cin/32 chunks (taps past the fourth are prefetches nobody reads: in range or zero)
            c0 = 0;
            if (++ku == 2) { ku = 0; ++kt_; }
            refresh_rows();
        }
    };
    const int KT = p.K / DBK;
    const int kt_last = KT - 1;
    auto load_b = [&](int kt, int j) {  // tile indices past the end are clamped (the pipeline prefetches ahead)
        rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, woff[j], min(kt, kt_last) * (DBK * 4), 0));
    };
    auto store_a = [&](int buf, int j) {
        *reinterpret_cast<f32x4*>(As + buf * BM * DLDSW + (r0 + 32 * j) * DLDSW + c4 * 4) = ra[j];
    };
    auto store_b = [&](int buf, int j) {
        *reinterpret_cast<f32x4*>(Bs + buf * BN * DLDSW + (r0 + 32 * j) * DLDSW + c4 * 4) = rb[j];
    };
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int j = 0; j < AL; ++j) load_a(j);
        load_x_advance();
#pragma unroll
        for (int j = 0; j < BL; ++j) load_b(kt, j);
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int j = 0; j < AL; ++j) store_a(buf, j);
#pragma unroll
        for (int j = 0; j < BL; ++j) store_b(buf, j);
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int wm = wave & 1, wn = wave >> 1;
    const int arow = wm * WM + (lane & 31);
    const int brow = wn * WN + (lane & 31);
    const int koff = 4 * (lane >> 5);
    const float* a_lds = As + arow * DLDSW + koff;
    const float* b_lds = Bs + brow * DLDSW + koff;

    // The interleaved K loop of conv_mfma_kernel (PIPE == 1): every non-MFMA instruction of an iteration sits behind an MFMA
    //   kk0: MFMAs | prefetch frags kk1
    //   kk1: MFMAs | prefetch frags kk2 | write tile t+1 (loaded during iteration t-1) to the other LDS buffer
    //   kk2: MFMAs | prefetch frags kk3 | issue global loads of tile t+2
    //   barrier (all reads of this buffer are complete, all writes of the other are visible)
    //   kk3: MFMAs | prefetch frags kk0 of tile t+1
    f32x4 fa0[MI], fb0[NI], fa1[MI], fb1[NI];
    load_tile(0);
    store_tile(0);
    load_tile(1);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MI; ++i) fa0[i] = *reinterpret_cast<const f32x4*>(a_lds + i * 32 * DLDSW);
#pragma unroll
    for (int j = 0; j < NI; ++j) fb0[j] = *reinterpret_cast<const f32x4*>(b_lds + j * 32 * DLDSW);
    constexpr int NM = 4 * MI * NI;  // MFMAs (= slots) per k-group
    constexpr int NF = MI + NI;      // fragment reads per k-group
    constexpr int P1 = NF + AL + BL, P2 = NF + AL + 1 + BL;
    constexpr int PPF = (NF + NM - 1) / NM, PP1 = (P1 + NM - 1) / NM, PP2 = (P2 + NM - 1) / NM;
#define MFMA_SLOT(FA, FB, q)                                                                                  \
    acc[((q) / NI) % MI][(q) % NI] = __builtin_amdgcn_mfma_f32_32x32x2f32(                                   \
        FA[((q) / NI) % MI][(q) / (MI * NI)], FB[(q) % NI][(q) / (MI * NI)], acc[((q) / NI) % MI][(q) % NI], 0, 0, 0)
#define FRAG_PIECE(FA, FB, buf, kk, z)                                                                        \
    do {                                                                                                      \
        if ((z) < MI)                                                                                         \
            FA[(z) < MI ? (z) : 0] = *reinterpret_cast<const f32x4*>(a_lds + (buf) * BM * DLDSW +             \
                                                                     ((z) < MI ? (z) : 0) * 32 * DLDSW + (kk) * 8); \
        else                                                                                                  \
            FB[(z) >= MI ? (z) - MI : 0] = *reinterpret_cast<const f32x4*>(                                   \
                b_lds + (buf) * BN * DLDSW + ((z) >= MI ? (z) - MI : 0) * 32 * DLDSW + (kk) * 8);              \
    } while (0)
    for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            MFMA_SLOT(fa0, fb0, q);
#pragma unroll
            for (int z = q * PPF; z < (q + 1) * PPF; ++z)
                if (z < NF) FRAG_PIECE(fa1, fb1, buf, 1, z);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            MFMA_SLOT(fa1, fb1, q);
#pragma unroll
            for (int z = q * PP1; z < (q + 1) * PP1; ++z) {
                if (z < NF) FRAG_PIECE(fa0, fb0, buf, 2, z);
                else if (z < NF + AL) store_a(buf ^ 1, z - NF);
                else if (z < P1) store_b(buf ^ 1, z - NF - AL);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            MFMA_SLOT(fa0, fb0, q);
#pragma unroll
            for (int z = q * PP2; z < (q + 1) * PP2; ++z) {
                if (z < NF) FRAG_PIECE(fa1, fb1, buf, 3, z);
                else if (z < NF + AL) load_a(z - NF);
                else if (z == NF + AL) load_x_advance();
                else if (z < P2) load_b(kt + 2, z - NF - AL - 1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("" ::: "memory");       // no LDS access may be moved across the raw barrier by the compiler
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS reads/writes are done; loads stay in flight
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            MFMA_SLOT(fa1, fb1, q);
#pragma unroll
            for (int z = q * PPF; z < (q + 1) * PPF; ++z)
                if (z < NF) FRAG_PIECE(fa0, fb0, buf ^ 1, 0, z);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef MFMA_SLOT
#undef FRAG_PIECE

    // ---- epilogue.  D layout: col j = lane&31 (cout), row i = (r&3) + 8*(r>>2) + 4*(lane>>5) (input-resolution pixel).  The rows of a
    // tile are scattered over the doubled map (orow); rows >= M and channels >= Cout take offset 2^31, outside the descriptor: dropped.
    const int half = lane >> 5;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(
        p.out, 0, (int)((size_t)p.M * 4 * p.Cout * 4), 0x00020000);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int c = n0 + wn * WN + j * 32 + (lane & 31);
        const bool cok = c < p.Cout;
        const int cc = cok ? c : p.Cout - 1;
        const float sc = p.scale ? p.scale[cc] : 1.f;
        const float bi = p.bias ? p.bias[cc] : 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int rbase = wm * WM + i * 32 + 4 * half;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned ro = orow[rbase + (r & 3) + 8 * (r >> 2)];
                float v = acc[i][j][r] * sc + bi;
                if (p.relu) v = fmaxf(v, 0.f);
                const unsigned off = (cok && !(ro >> 31)) ? ro + (unsigned)c * 4u : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs_out, (int)off, 0, 0);
            }
        }
    }
}

// one launch: every tensor below 2 GiB
static int deconv_launch(const float* in, const float* wgt, float* out, const float* scale, const float* bias, int N, int H, int W,
                         int Cin, int Cout, int relu, int* variant_out, hipStream_t stream) {
    DeconvParams p;
    p.in = in; p.wgt = wgt; p.out = out; p.scale = scale; p.bias = bias;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.K = 4 * Cin; p.relu = relu;
    p.M = N * H * W;
    constexpr int bm = 64, bn = 64;      // the one instance
    if (variant_out) *variant_out = bm * 1000000 + bn * 1000 + 1;
    p.tilesM = (p.M + bm - 1) / bm;
    p.tilesN = (Cout + bn - 1) / bn;
    const long long T = (long long)p.tilesM * 4 * p.tilesN;
    if (T >= (1ll << 30)) return CPR_ERR_UNSUPPORTED;
    const int grid = (int)((T + 7) / 8) * 8;
    hipLaunchKernelGGL((deconv4x4s2_kernel<bm, bn>), dim3(grid), dim3(256), 0, stream, p);
    CPR_LAUNCH_STATUS();
}

// out (N, 2H, 2W, Cout) = epilogue(conv_transpose2d(in (N, H, W, Cin), w (Cin, Cout, 4, 4), stride 2, padding 1)); wgt: the four class
// images of cpr_pack_weights_deconv.  scale / bias may each be null (both null: the raw sums).  flags: CPR_CONV_RELU or 0.
extern "C" int cpr_deconv4x4s2_fwd(const float* in, const float* wgt, float* out, const float* scale, const float* bias, int N, int H,
                                   int W, int Cin, int Cout, int flags, int* variant_out, hipStream_t stream) {
    CPR_CHECK_ARG(in && wgt && out);
    CPR_CHECK_ARG(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (flags & ~CPR_CONV_RELU) == 0);
    CPR_CHECK_ARG(Cin % DBK == 0 && Cout % 32 == 0);
    if ((long long)Cout * 4 * Cin * 4 >= (1ll << 31)) return CPR_ERR_UNSUPPORTED;
    const long long in_img = (long long)H * W * Cin * 4, out_img = (long long)H * W * 4 * Cout * 4;
    const int per = cpr_images_per_launch(N, cpr_max2(in_img, out_img));
    if (per <= 0) return CPR_ERR_UNSUPPORTED;
    for (int n0 = 0; n0 < N; n0 += per) {
        const int n = N - n0 < per ? N - n0 : per;
        const int rc = deconv_launch(in + (size_t)n0 * H * W * Cin, wgt, out + (size_t)n0 * H * W * 4 * Cout, scale, bias, n, H, W, Cin,
                                     Cout, flags & CPR_CONV_RELU, n0 == 0 ? variant_out : nullptr, stream);
        if (rc != CPR_OK) return rc;
    }
    return CPR_OK;
}

// nn.ConvTranspose2d weight (Cin, Cout, 4, 4) -> out[class = 2a + b][co][(2t + u) * Cin + ci] = w[ci][co][1 - a + 2t][1 - b + 2u]:
// one [Cout][4*Cin] GEMM image per output-parity class, K ordered (tap row, tap column, cin).  One thread per output element.
__global__ void pack_weights_deconv_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cout) {
    const int K = 4 * Cin;
    const long long total = 4ll * Cout * K;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(idx % K);
        const long long rowi = idx / K;
        const int co = (int)(rowi % Cout), cls = (int)(rowi / Cout);
        const int ci = k % Cin, tap = k / Cin;
        const int kh = 1 - (cls >> 1) + 2 * (tap >> 1), kw = 1 - (cls & 1) + 2 * (tap & 1);
        out[idx] = w[(((size_t)ci * Cout + co) * 4 + kh) * 4 + kw];
    }
}
extern "C" int cpr_pack_weights_deconv(const float* w, float* out, int Cin, int Cout, hipStream_t stream) {
    CPR_CHECK_ARG(w && out && Cin > 0 && Cout > 0);
    CPR_CHECK_ARG(Cin % DBK == 0 && Cout % 32 == 0);
    const long long total = 16ll * Cout * Cin;
    const int grid = (int)(cdivll(total, 256) < 4096 ? cdivll(total, 256) : 4096);
    hipLaunchKernelGGL(pack_weights_deconv_kernel, dim3(grid), dim3(256), 0, stream, w, out, Cin, Cout);
    CPR_LAUNCH_STATUS();
}
