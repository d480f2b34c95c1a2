// Data side feeding the path: the per-image tail of the mmdet train/test pipeline on the device.
//   RandomFlip(horizontal) -> Normalize(mean, std, to_rgb) -> Pad(size_divisor) -> DefaultFormatBundle
//   (T/mmdet/datasets/pipelines/transforms.py:431-480 (flip), :560-600 (Normalize -> mmcv.imnormalize),
//    :603-680 (Pad, pad_val 0 AFTER normalisation), formating.py:180-214)
// fused into one pass from the decoded uint8 HWC image straight to the stem's input layout (N, Hp, Wp, 4) fp32 (4th channel
// zero), so the float NCHW image of the reference is never materialised.  One thread per output pixel: 3 B in, 16 B out.
// Arithmetic as mmcv.imnormalize_: float32(img); optional BGR->RGB; (x - mean_f32) * stdinv_f32, stdinv = 1/float64(std)
// rounded to fp32 (OpenCV arithmetic on a CV_32F array converts the scalar to float); no FMA contraction.
#include "common.h"

__global__ void preprocess_u8_kernel(const unsigned char* __restrict__ img, const int* __restrict__ flip,
                                     float m0, float m1, float m2, float s0, float s1, float s2, int to_rgb,
                                     float* __restrict__ out, int N, int H, int W, int Hp, int Wp) {
    const long long total = (long long)N * Hp * Wp;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wp);
        const long long r = i / Wp;
        const int y = (int)(r % Hp);
        const int n = (int)(r / Hp);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (y < H && x < W) {
            const int sx = (flip && flip[n]) ? W - 1 - x : x;
            const unsigned char* p = img + (((size_t)n * H + y) * W + sx) * 3;
            const float c0 = (float)p[0], c1 = (float)p[1], c2 = (float)p[2];
            const float r0 = to_rgb ? c2 : c0, r2 = to_rgb ? c0 : c2;
            v[0] = __fmul_rn(__fsub_rn(r0, m0), s0);
            v[1] = __fmul_rn(__fsub_rn(c1, m1), s1);
            v[2] = __fmul_rn(__fsub_rn(r2, m2), s2);
        }
        *reinterpret_cast<f32x4*>(out + i * 4) = v;
    }
}

extern "C" int cpr_preprocess_u8(const unsigned char* img, const int* flip, const float* mean3, const float* stdinv3,
                                 int to_rgb, float* out, int N, int H, int W, int Hp, int Wp, hipStream_t stream) {
    // img (N,H,W,3) uint8 on the device; mean3 / stdinv3 are HOST pointers (three floats each); flip (N) int32 or NULL
    CPR_CHECK_ARG(img && mean3 && stdinv3 && out && N > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W);
    const long long total = (long long)N * Hp * Wp;
    const int grid = (int)(cdivll(total, 256) < 65536 ? cdivll(total, 256) : 65536);
    hipLaunchKernelGGL(preprocess_u8_kernel, dim3(grid), dim3(256), 0, stream, img, flip, mean3[0], mean3[1], mean3[2],
                       stdinv3[0], stdinv3[1], stdinv3[2], to_rgb, out, N, H, W, Hp, Wp);
    CPR_LAUNCH_STATUS();
}

// Box side of Resize (scale 1) -> RandomFlip: Resize._resize_bboxes clips every bbox field to the image
// (bbox_clip_border=True: x to [0, W], y to [0, H]; transforms.py:241-249) BEFORE RandomFlip.bbox_flip mirrors it
// (transforms.py:397-415).  boxes (n,4) xyxy of image `img_of[i]`; hw (N,2) int32 = img_shape[:2]; flipped when flip[img].
__global__ void clip_flip_boxes_kernel(float* __restrict__ boxes, const int* __restrict__ img_of,
                                       const int* __restrict__ flip, const int* __restrict__ hw, int n, int clip) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int im = img_of[i];
    const float h = (float)hw[im * 2], w = (float)hw[im * 2 + 1];
    float x1 = boxes[i * 4], y1 = boxes[i * 4 + 1], x2 = boxes[i * 4 + 2], y2 = boxes[i * 4 + 3];
    if (clip) {
        x1 = fminf(fmaxf(x1, 0.f), w); x2 = fminf(fmaxf(x2, 0.f), w);
        y1 = fminf(fmaxf(y1, 0.f), h); y2 = fminf(fmaxf(y2, 0.f), h);
    }
    if (flip[im]) {
        const float t = x1;
        x1 = __fsub_rn(w, x2);
        x2 = __fsub_rn(w, t);
    }
    boxes[i * 4] = x1; boxes[i * 4 + 1] = y1; boxes[i * 4 + 2] = x2; boxes[i * 4 + 3] = y2;
}
extern "C" int cpr_clip_flip_boxes(float* boxes, const int* img_of, const int* flip, const int* img_hw, int n, int clip,
                                   hipStream_t stream) {
    CPR_CHECK_ARG(n >= 0);
    if (n == 0) return CPR_OK;
    CPR_CHECK_ARG(boxes && img_of && flip && img_hw);
    hipLaunchKernelGGL(clip_flip_boxes_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, boxes, img_of, flip, img_hw, n, clip);
    CPR_LAUNCH_STATUS();
}

// ---- Resize in all its forms + the test-time wrappers: crop -> cv2.resize(INTER_LINEAR) on uint8 -> flip -> the tail above ----
// The reference resizes the DECODED uint8 image (Resize._resize_img -> mmcv.imrescale / imresize -> cv2.resize, transforms.py:210-239)
// before Normalize, so the intermediate is a uint8 image and this kernel reproduces OpenCV's 8-bit fixed-point bilinear, not a float
// one (restated from OpenCV's resize.cpp; cv2 itself is un-vendored: PARITY UNPINNED, tests/test_resize_host.py holds the scheme to an
// fp64 bilinear).  Per axis, source extent s -> d, output index i:
//     scale = 1. / ((double)d / s)  (ops.preprocess_jobs computes it on the host, in double, into the job)
//     f = (float)((i + 0.5) * scale - 0.5);  k = floor(f);  f -= k;  coefficients short(rint((1.f - f) * 2048)), short(rint(f * 2048))
//     x axis: k < 0 -> k = 0, f = 0;  k >= s - 1 -> k = s - 1, f = 0           (xofs / ialpha; the tail columns use S[k] * 2048)
//     y axis: f stays as it is, the two ROWS clamp to [0, s - 1]                 (yofs / ibeta; resizeGeneric_Invoker clips sy + k)
//     R = S[k] * a0 + S[k+1] * a1 (int32, per row);  u8 = clip((((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2)
// Taps clamp to the CROP (the wrappers slice the tile out before Resize sees it).  An identity size gives a0 = b0 = 2048 and returns
// the source exactly; an exact 2:1 reduction gives the (a + b + c + d + 2) >> 2 that OpenCV's own shortcut to INTER_AREA computes.
// One thread per output pixel of a job's padded slot (grid.y = job): up to 12 B gathered through L1/L2, 16 B stored; the two fp64
// multiply-subtract pairs per pixel are hidden under the store.  A job at an identity size reads its one source pixel directly.  This file is compiled with -ffp-contract=off.
struct PreprocessJob {            // mirrors cpr_preprocess_job of include/cpr_hip.h (80 bytes)
    const unsigned char* src;
    long long out_off;
    double scale_x, scale_y;
    int pitch, src_w, src_h, x0, y0, cw, ch, dw, dh, flip, Hp, Wp;
};

__device__ __forceinline__ bool preprocess_job_ok(const PreprocessJob& j, long long total) {
    return j.src && j.src_w > 0 && j.src_h > 0 && j.pitch >= 0 && (long long)j.pitch >= 3ll * j.src_w && j.x0 >= 0 && j.y0 >= 0 && j.cw > 0 &&
           j.ch > 0 && j.cw <= j.src_w - j.x0 && j.ch <= j.src_h - j.y0 && j.dw > 0 && j.dh > 0 && j.Hp >= j.dh && j.Wp >= j.dw &&
           j.out_off >= 0 && (long long)j.Hp * j.Wp <= total - j.out_off;
}

// One pixel (dx, y) of the resized crop (dx already mirrored for a flipped job): the scheme of the header comment, channel by channel.
__device__ __forceinline__ void resized_pixel(const PreprocessJob& j, const unsigned char* __restrict__ base, int dx, int y, float* c) {
    float fx = (float)((dx + 0.5) * j.scale_x - 0.5);
    int kx = (int)floorf(fx);
    fx -= (float)kx;
    if (kx < 0) { kx = 0; fx = 0.f; }
    if (kx >= j.cw - 1) { kx = j.cw - 1; fx = 0.f; }
    const int a0 = (int)rintf((1.f - fx) * 2048.f), a1 = (int)rintf(fx * 2048.f);
    const int kx1 = min(kx + 1, j.cw - 1);
    float fy = (float)((y + 0.5) * j.scale_y - 0.5);
    const int ky = (int)floorf(fy);
    fy -= (float)ky;
    const int b0 = (int)rintf((1.f - fy) * 2048.f), b1 = (int)rintf(fy * 2048.f);
    const int ky0 = min(max(ky, 0), j.ch - 1), ky1 = min(max(ky + 1, 0), j.ch - 1);
    const unsigned char* r0 = base + (size_t)ky0 * j.pitch;
    const unsigned char* r1 = base + (size_t)ky1 * j.pitch;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int R0 = r0[kx * 3 + ch] * a0 + r0[kx1 * 3 + ch] * a1;
        const int R1 = r1[kx * 3 + ch] * a0 + r1[kx1 * 3 + ch] * a1;
        const int u = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2;
        c[ch] = (float)min(max(u, 0), 255);
    }
}

__global__ void __launch_bounds__(256) preprocess_jobs_u8_kernel(const PreprocessJob* __restrict__ jobs, float m0, float m1, float m2,
                                                                 float s0, float s1, float s2, int to_rgb, float* __restrict__ out,
                                                                 long long total) {
    const PreprocessJob j = jobs[blockIdx.y];
    if (!preprocess_job_ok(j, total)) return;              // a malformed job touches nothing (ops.preprocess_jobs refuses it earlier)
    const int slot = j.Hp * j.Wp;                           // < 2^31: checked against total_out_pixels by the launcher's caller
    float* __restrict__ o = out + j.out_off * 4;
    const unsigned char* __restrict__ base = j.src + (size_t)j.y0 * j.pitch + (size_t)j.x0 * 3;
    const bool identity = j.dw == j.cw && j.dh == j.ch;     // per job, so per block: tiles and ragged batches at scale 1
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < slot; i += gridDim.x * blockDim.x) {
        const int y = i / j.Wp, x = i - y * j.Wp;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (y < j.dh && x < j.dw) {
            const int dx = j.flip ? j.dw - 1 - x : x;       // mmcv.imflip of the RESIZED image
            float c[3];
            if (identity) {                                 // a0 = b0 = 2048, a1 = b1 = 0: the scheme returns the source pixel
                const unsigned char* p = base + (size_t)y * j.pitch + dx * 3;
                c[0] = (float)p[0]; c[1] = (float)p[1]; c[2] = (float)p[2];
            } else {
                resized_pixel(j, base, dx, y, c);
            }
            const float q0 = to_rgb ? c[2] : c[0], q2 = to_rgb ? c[0] : c[2];
            v[0] = __fmul_rn(__fsub_rn(q0, m0), s0);
            v[1] = __fmul_rn(__fsub_rn(c[1], m1), s1);
            v[2] = __fmul_rn(__fsub_rn(q2, m2), s2);
        }
        *reinterpret_cast<f32x4*>(o + (size_t)i * 4) = v;
    }
}

extern "C" int cpr_preprocess_jobs_u8(const void* jobs_dev, int n_jobs, const float* mean3, const float* stdinv3, int to_rgb,
                                      float* out, long long total_out_pixels, hipStream_t stream) {
    // jobs_dev: n_jobs PreprocessJob records ON THE DEVICE; mean3 / stdinv3 HOST pointers.  The launcher sees pointers and counts only:
    // each job's geometry is checked by the kernel (and by ops.preprocess_jobs on the host copy before the upload).
    CPR_CHECK_ARG(n_jobs >= 0 && n_jobs <= 65535);
    if (n_jobs == 0) return CPR_OK;
    CPR_CHECK_ARG(jobs_dev && mean3 && stdinv3 && out && total_out_pixels > 0 && total_out_pixels < (1ll << 31));
    const long long per = cdivll(cdivll(total_out_pixels, n_jobs) * 2, 256);        // blocks for a slot twice the mean
    const int gx = (int)(per < 1 ? 1 : per > 2048 ? 2048 : per);
    hipLaunchKernelGGL(preprocess_jobs_u8_kernel, dim3(gx, n_jobs), dim3(256), 0, stream, (const PreprocessJob*)jobs_dev, mean3[0],
                       mean3[1], mean3[2], stdinv3[0], stdinv3[1], stdinv3[2], to_rgb, out, total_out_pixels);
    CPR_LAUNCH_STATUS();
}

// Box side of Resize -> RandomFlip at any scale: Resize._resize_bboxes multiplies the float32 boxes by the float32
// [w_scale, h_scale, w_scale, h_scale] of _resize_img (one rounding per coordinate), clips to the RESIZED img_shape, then
// RandomFlip.bbox_flip mirrors.  scale4 (N,4) fp32 per image; hw (N,2) int32 = the resized img_shape[:2].
__global__ void scale_clip_flip_boxes_kernel(float* __restrict__ boxes, const int* __restrict__ img_of, const int* __restrict__ flip,
                                             const int* __restrict__ hw, const float* __restrict__ scale4, int n, int clip) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int im = img_of[i];
    const float h = (float)hw[im * 2], w = (float)hw[im * 2 + 1];
    const float* sc = scale4 + im * 4;
    float x1 = __fmul_rn(boxes[i * 4], sc[0]), y1 = __fmul_rn(boxes[i * 4 + 1], sc[1]);
    float x2 = __fmul_rn(boxes[i * 4 + 2], sc[2]), y2 = __fmul_rn(boxes[i * 4 + 3], sc[3]);
    if (clip) {
        x1 = fminf(fmaxf(x1, 0.f), w); x2 = fminf(fmaxf(x2, 0.f), w);
        y1 = fminf(fmaxf(y1, 0.f), h); y2 = fminf(fmaxf(y2, 0.f), h);
    }
    if (flip[im]) {
        const float t = x1;
        x1 = __fsub_rn(w, x2);
        x2 = __fsub_rn(w, t);
    }
    boxes[i * 4] = x1; boxes[i * 4 + 1] = y1; boxes[i * 4 + 2] = x2; boxes[i * 4 + 3] = y2;
}
extern "C" int cpr_scale_clip_flip_boxes(float* boxes, const int* img_of, const int* flip, const int* img_hw, const float* scale4,
                                         int n, int clip, hipStream_t stream) {
    CPR_CHECK_ARG(n >= 0);
    if (n == 0) return CPR_OK;
    CPR_CHECK_ARG(boxes && img_of && flip && img_hw && scale4);
    hipLaunchKernelGGL(scale_clip_flip_boxes_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, boxes, img_of, flip, img_hw, scale4, n,
                       clip);
    CPR_LAUNCH_STATUS();
}
