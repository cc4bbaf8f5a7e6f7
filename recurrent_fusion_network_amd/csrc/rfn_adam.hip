// clip_gradient + Adam on flat f32 buckets: one kernel, one launch for up to RFN_ADAM_MAXBUCKET buckets, 16 B per lane on all
// seven streams where alignment allows.  The element arithmetic is pinned (adam_elem), so every entry point gives the same bits.
#include <string.h>

#include "rfn_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- clip_gradient + Adam (misc/utils.py:292-296, train.py:69-71) -----------------------------------
__device__ __forceinline__ void adam_elem(float& pv, float gv, float& mv, float& vv, float lr_over_bc1, float beta1,
                                          float beta2, float eps, float inv_sqrt_bc2, float wd, float clip,
                                          float gscale) {
    // The operation tree is pinned: no implicit contraction, fused multiply-adds only where written.  The kernel and its
    // graph-replayable form (scalars from memory instead of kernel arguments) must produce the same bits, and left to itself
    // the compiler fuses differently depending on where the scalars live.
#pragma clang fp contract(off)
    gv *= gscale;
    gv = fminf(fmaxf(gv, -clip), clip);
    gv = __builtin_fmaf(wd, pv, gv);
    mv = __builtin_fmaf(beta1, mv, (1.0f - beta1) * gv);
    vv = __builtin_fmaf(beta2, vv, ((1.0f - beta2) * gv) * gv);
    pv = pv - (lr_over_bc1 * mv) / __builtin_fmaf(sqrtf(vv), inv_sqrt_bc2, eps);
}
// The update for up to RFN_ADAM_MAXBUCKET flat buckets in ONE launch: every block walks the buckets in order with one
// grid-stride loop each.  VEC buckets (16-B aligned, a multiple of 4 long) move 16 B per lane on all seven streams.  Ten launches of 34-277 MB buckets each paid their own ramp and tail (4.7-5.1 TB/s over the
// step); one launch streams at the rate a single large bucket reaches (5.6 TB/s).  Element arithmetic is adam_elem's:
// a bucket's bits do not depend on which buckets share its launch.
struct AdamBuckets {
    float* p[RFN_ADAM_MAXBUCKET];
    const float* g[RFN_ADAM_MAXBUCKET];
    float* m[RFN_ADAM_MAXBUCKET];
    float* v[RFN_ADAM_MAXBUCKET];
    long n[RFN_ADAM_MAXBUCKET];
    int vec[RFN_ADAM_MAXBUCKET];
    int nb;
};
// coef != NULL: the two step-dependent scalars (lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) are read from device memory
// instead of the kernel arguments -- the form a captured HIP graph replays, where kernel arguments are frozen
// (rfn_adam_step_multi_coef).  Same values, same arithmetic.
__global__ __launch_bounds__(256) void adam_multi_k(const AdamBuckets B, float lr_over_bc1, float beta1, float beta2, float eps,
                                                    float inv_sqrt_bc2, float wd, float clip, float gscale,
                                                    const float* __restrict__ coef) {
    if (coef) {
        lr_over_bc1 = coef[0];
        inv_sqrt_bc2 = coef[1];
    }
    const long stride = (long)gridDim.x * 256, i0 = (long)blockIdx.x * 256 + threadIdx.x;
    for (int k = 0; k < B.nb; ++k) {
        if (B.vec[k]) {
            const long n4 = B.n[k] >> 2;
            f32x4* p4 = reinterpret_cast<f32x4*>(B.p[k]);
            const f32x4* g4 = reinterpret_cast<const f32x4*>(B.g[k]);
            f32x4* m4 = reinterpret_cast<f32x4*>(B.m[k]);
            f32x4* v4 = reinterpret_cast<f32x4*>(B.v[k]);
            for (long i = i0; i < n4; i += stride) {
                f32x4 pv = p4[i], mv = m4[i], vv = v4[i];
                const f32x4 gv = g4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pv[e], me = mv[e], ve = vv[e];
                    adam_elem(pe, gv[e], me, ve, lr_over_bc1, beta1, beta2, eps, inv_sqrt_bc2, wd, clip, gscale);
                    pv[e] = pe;
                    mv[e] = me;
                    vv[e] = ve;
                }
                m4[i] = mv;
                v4[i] = vv;
                p4[i] = pv;
            }
        } else {
            float* p = B.p[k];
            const float* g = B.g[k];
            float* m = B.m[k];
            float* v = B.v[k];
            for (long i = i0; i < B.n[k]; i += stride) {
                float pv = p[i], mv = m[i], vv = v[i];
                adam_elem(pv, g[i], mv, vv, lr_over_bc1, beta1, beta2, eps, inv_sqrt_bc2, wd, clip, gscale);
                m[i] = mv;
                v[i] = vv;
                p[i] = pv;
            }
        }
    }
}
static int adam_multi_launch(int nbuckets, float* const* p, const float* const* g, float* const* m, float* const* v,
                             const int64_t* n, float lr, float beta1, float beta2, float eps, float weight_decay,
                             float grad_clip, float grad_scale, int step, const float* coef, void* stream) {
    if (nbuckets < 1 || nbuckets > RFN_ADAM_MAXBUCKET || (!coef && step < 1)) return RFN_ERR_SHAPE;
    if (!p || !g || !m || !v || !n) return RFN_ERR_ARG;
    AdamBuckets B;
    memset(&B, 0, sizeof(B));
    long most = 0;
    for (int k = 0; k < nbuckets; ++k) {
        if (n[k] <= 0) return RFN_ERR_SHAPE;
        if (!p[k] || !g[k] || !m[k] || !v[k]) return RFN_ERR_ARG;
        B.p[k] = p[k]; B.g[k] = g[k]; B.m[k] = m[k]; B.v[k] = v[k]; B.n[k] = (long)n[k];
        B.vec[k] = (n[k] % 4 == 0) && rfn_aligned16(p[k]) && rfn_aligned16(g[k]) && rfn_aligned16(m[k]) && rfn_aligned16(v[k]);
        const long work = B.vec[k] ? (long)n[k] / 4 : (long)n[k];
        most = work > most ? work : most;
    }
    B.nb = nbuckets;
    float c0 = 0.f, c1 = 0.f;
    if (!coef) {
        const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
        c0 = (float)(lr / bc1);
        c1 = (float)(1.0 / sqrt(bc2));
    }
    const int blocks = (int)(most / 256 + 1 < 4096 ? most / 256 + 1 : 4096);
    hipLaunchKernelGGL(adam_multi_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, B, c0, beta1, beta2, eps, c1, weight_decay,
                       grad_clip, grad_scale, coef);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_adam_step_multi(int nbuckets, float* const* p, const float* const* g, float* const* m, float* const* v,
                                   const int64_t* n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                   float grad_clip, float grad_scale, int step, void* stream) {
    return adam_multi_launch(nbuckets, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, grad_clip, grad_scale, step, nullptr,
                             stream);
}
extern "C" int rfn_adam_step_multi_coef(int nbuckets, float* const* p, const float* const* g, float* const* m, float* const* v,
                                        const int64_t* n, const float* coef_dev, float beta1, float beta2, float eps,
                                        float weight_decay, float grad_clip, float grad_scale, void* stream) {
    if (!coef_dev) return RFN_ERR_ARG;
    return adam_multi_launch(nbuckets, p, g, m, v, n, 0.f, beta1, beta2, eps, weight_decay, grad_clip, grad_scale, 0, coef_dev,
                             stream);
}
// One bucket (n <= 0 or step < 1: RFN_ERR_SHAPE, before a NULL pointer's RFN_ERR_ARG -- the order of the launch's own checks)
extern "C" int rfn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, float grad_clip, float grad_scale, int step,
                             void* stream) {
    return adam_multi_launch(1, &p, &g, &m, &v, &n, lr, beta1, beta2, eps, weight_decay, grad_clip, grad_scale, step, nullptr,
                             stream);
}
