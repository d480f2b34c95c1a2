// Adam / AdamW step of the native trainer (training.CprTrainer): one launch over the flat fp32 parameter buffer, clip by the
// global norm + the update.  Sibling of sgd_kernel (backward.hip); the P2P configs train with
// optimizer = dict(type='Adam', lr=1e-4) (configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py:86-93).
//
// Per element, torch.optim.Adam's single-tensor update (torch/optim/adam.py, foreach=False) op for op, each op rounded on
// its own as torch's separate elementwise kernels round it (build.py compiles this file with -ffp-contract=off):
//   g  = coef * grad                       clip_grad_norm_'s coefficient (x 1/world_size), the expression of sgd_kernel
//   Adam:  g = g + wd * p                  grad.add(param, alpha=wd)
//   AdamW: p = p * (1 - lr*wd)             param.mul_(1 - lr * wd), before the moments
//   m  = lerp(m, g, 1 - beta1)             exp_avg.lerp_(grad, 1 - beta1)
//   v  = v * beta2;  v = v + (1-beta2) * (g*g)   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//   d  = sqrt(v) / bc2_sqrt + eps          (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
//   p  = p + (-step_size) * (m / d)        param.addcdiv_(exp_avg, denom, value=-step_size)
// step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) come from the host, computed in double as torch computes
// them in Python; the scalar weights (1 - beta1, 1 - lr*wd, ...) are formed in double and rounded once, as torch's Python
// scalars are when they reach an fp32 kernel.
//
// Streaming: 16 B per lane on the 16-byte-aligned body, a scalar tail for n % 4, grid-stride.  Reads p, grad,
// m, v and writes p, m, v: 28 B per parameter.
#include "common.h"

struct AdamScalars {
    float max_norm, grad_scale;     // clip: max_norm <= 0 -> none
    float wd, decay;                // L2 weight (Adam) / decoupled factor 1 - lr*wd (AdamW)
    float w1, b2, w2;               // 1 - beta1, beta2, 1 - beta2
    float step_size, bc2_sqrt, eps;
    int decoupled;
};

__device__ __forceinline__ void adam_elem(float& p, float gr, float& m, float& v, float coef, const AdamScalars& s) {
    float g = gr * coef;
    if (s.wd != 0.f) {
        if (s.decoupled) p = p * s.decay;
        else g = g + s.wd * p;
    }
    // at::lerp (ATen/native/Lerp.h): the form depends on the size of the weight
    m = fabsf(s.w1) < 0.5f ? m + s.w1 * (g - m) : g - (g - m) * (1.f - s.w1);
    v = v * s.b2;
    v = v + s.w2 * (g * g);
    const float d = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + (-s.step_size) * (m / d);
}

__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ grad,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   const double* __restrict__ norm2, long long n, long long n4,
                                                   AdamScalars s) {
    float coef = s.grad_scale;
    if (s.max_norm > 0.f) {
        const float tn = (float)sqrt(norm2[0]) * s.grad_scale;
        const float c = s.max_norm / (tn + 1e-6f);
        coef *= fminf(c, 1.f);
    }
    const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    for (long long i = tid; i < n4; i += stride) {
        float4 pv = reinterpret_cast<const float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(grad)[i];
        float4 mv = reinterpret_cast<const float4*>(m)[i];
        float4 vv = reinterpret_cast<const float4*>(v)[i];
        adam_elem(pv.x, gv.x, mv.x, vv.x, coef, s);
        adam_elem(pv.y, gv.y, mv.y, vv.y, coef, s);
        adam_elem(pv.z, gv.z, mv.z, vv.z, coef, s);
        adam_elem(pv.w, gv.w, mv.w, vv.w, coef, s);
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    for (long long i = 4 * n4 + tid; i < n; i += stride) {      // tail (n % 4), or everything when a pointer is unaligned
        float pv = p[i], mv = m[i], vv = v[i];
        adam_elem(pv, grad[i], mv, vv, coef, s);
        p[i] = pv;
        m[i] = mv;
        v[i] = vv;
    }
}

extern "C" int cpr_adam_step(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, const double* norm2, long long n,
                             double lr, double beta1, double beta2, double eps, double wd, float step_size, float bc2_sqrt,
                             float max_norm, float grad_scale, int decoupled, hipStream_t stream) {
    CPR_CHECK_ARG(p && grad && exp_avg && exp_avg_sq && n > 0 && (max_norm <= 0.f || norm2));
    CPR_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0 && lr >= 0.0 && bc2_sqrt > 0.f);
    AdamScalars s;
    s.max_norm = max_norm;
    s.grad_scale = grad_scale;
    s.wd = (float)wd;
    s.decay = (float)(1.0 - lr * wd);
    s.w1 = (float)(1.0 - beta1);
    s.b2 = (float)beta2;
    s.w2 = (float)(1.0 - beta2);
    s.step_size = step_size;
    s.bc2_sqrt = bc2_sqrt;
    s.eps = (float)eps;
    s.decoupled = decoupled ? 1 : 0;
    const unsigned long long a = (unsigned long long)p | (unsigned long long)grad | (unsigned long long)exp_avg |
                                 (unsigned long long)exp_avg_sq;
    const long long n4 = (a & 15) == 0 ? n / 4 : 0;
    const long long work = n4 > 0 ? n4 : n;
    const int grid = (int)(cdivll(work, 256) < 8192 ? cdivll(work, 256) : 8192);
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, stream, p, grad, exp_avg, exp_avg_sq, norm2, n, n4, s);
    CPR_LAUNCH_STATUS();
}
