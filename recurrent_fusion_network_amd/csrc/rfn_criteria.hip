// The criteria and their gradients: the XE language loss (from log-probs, and fused from the logits), the same with a KL term
// towards a teacher's rows (distillation; dense rows, or their K <= 32 best entries), the RL reward criterion, and nn.MultiLabelMarginLoss for the reason heads.  One block of 256 per row writes the row's loss term; sum_k /
// sum_groups_k add the terms in a fixed order (no float atomics), so a loss is bitwise reproducible.
#include <string.h>

#include "rfn_rows.h"

// ---- fixed-order sum of n floats -> out[0] ---------------------------------------------------------
__global__ __launch_bounds__(256) void sum_k(const float* __restrict__ x, int n, float scale, float* __restrict__ out,
                                             int accumulate) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += x[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s * scale : s * scale;
}

// ---- XE language loss (misc/utils.py:163-184) -------------------------------------------------------
__global__ __launch_bounds__(256) void xe_loss_k(const float* __restrict__ logp, int T, int V1,
                                                 const int64_t* __restrict__ target, long ld_t,
                                                 const float* __restrict__ mask, long ld_m, float eps, float gcoef,
                                                 const float* __restrict__ gdev, float* __restrict__ row_loss,
                                                 float* __restrict__ dlogp) {
    __shared__ float red[4];
    const int r = blockIdx.x, b = r / T, t = r - b * T;
    const float* lp = logp + (long)r * V1;
    long tg = target[b * ld_t + t];
    if (tg < 0 || tg >= V1) tg = 0;
    const float mk = mask[b * ld_m + t];
    const float uni = eps / (float)V1;
    float term = 0.f;
    if (row_loss) {
        if (eps > 0.f) {
            float s = 0.f;
            for (int v = threadIdx.x; v < V1; v += 256) s += lp[v];
            s = block_sum_256(s, red);
            term = (1.0f - eps) * lp[tg] + uni * s;
        } else {
            term = lp[tg];
        }
        if (threadIdx.x == 0) row_loss[r] = -mk * term;
    }
    if (dlogp) {
        float* d = dlogp + (long)r * V1;
        const float gc = gdev ? gcoef * gdev[0] : gcoef;  // upstream d loss, read on the device (no host sync)
        const float base = -mk * gc * uni;              // 0 when eps == 0
        const float hot = -mk * gc * (1.0f - eps);
        for (int v = threadIdx.x; v < V1; v += 256) d[v] = (v == tg) ? base + hot : base;
    }
}
extern "C" int rfn_xe_loss_ex(const float* logp, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                              const float* mask, int64_t ld_mask, float eps, float gscale, const float* gscale_dev,
                              float* scratch, float* loss_out, int accumulate_loss, float* dlogp, void* stream) {
    if (B <= 0 || T <= 0 || V1 <= 0) return RFN_ERR_SHAPE;
    if (!logp || !target || !mask || (loss_out && !scratch)) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(xe_loss_k, dim3(B * T), dim3(256), 0, st, logp, T, V1, target, (long)ld_target, mask,
                       (long)ld_mask, eps, gscale / (float)B, gscale_dev, loss_out ? scratch : nullptr, dlogp);
    RFN_CHECK_LAUNCH();
    if (loss_out) {
        hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, scratch, B * T, 1.0f / (float)B, loss_out,
                           accumulate_loss);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}
extern "C" int rfn_xe_loss(const float* logp, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                           const float* mask, int64_t ld_mask, float eps, float gscale, float* scratch,
                           float* loss_out, int accumulate_loss, float* dlogp, void* stream) {
    return rfn_xe_loss_ex(logp, B, T, V1, target, ld_target, mask, ld_mask, eps, gscale, nullptr, scratch, loss_out,
                          accumulate_loss, dlogp, stream);
}

// ---- XE language loss straight from the logits (misc/utils.py:163-184 + F.log_softmax of :276) --------------
// The unfused pass writes log_prob (B, T, V+1), the criterion reads it back for the loss, writes d log_prob (B, T, V+1), and the
// log-softmax backward reads both to write d logits: four passes over a 165 MB tensor at C3 that exist only because
// `forward` has to hand `log_prob` to a caller-owned criterion (train.py:154-159).  When the caller asks for the LOSS
// (RecurrentFusionModel.forward_loss) neither tensor is needed:
//   forward : one pass over the time-major logits rows r = t * B + b -- the row's logsumexp (log_softmax_row: the same bits
//             rfn_log_softmax_fwd would subtract) -> lse[r], and the row's loss term
//             -mask * ((1 - eps) * (x[tg] - lse) + eps / V1 * (sum_v x[v] - V1 * lse)) -> row_loss[b * T + t]
//   backward: d logits[v] = mask * g / B * (exp(x[v] - lse) - (1 - eps) * [v == tg] - eps / V1), written over the logits.
// (sum_v d logp = -mask * g / B whatever eps is, which is what the log-softmax backward multiplies the probabilities with.)
template <bool VEC>
__global__ __launch_bounds__(256) void xe_logits_fwd_k(const float* __restrict__ logits, long ldl, int B, int T, int V1,
                                                       const int64_t* __restrict__ target, long ld_t,
                                                       const float* __restrict__ mask, long ld_m, float eps,
                                                       float* __restrict__ lse_out, float* __restrict__ row_loss) {
    __shared__ float red[4];
    const int r = blockIdx.x, t = r / B, b = r - t * B;      // time-major rows
    const float* x = logits + r * ldl;
    f32x4 xr[LSM_R4];
    const float lse = log_softmax_row<VEC>(x, V1, xr, red);
    long tg = target[b * ld_t + t];
    if (tg < 0 || tg >= V1) tg = 0;
    const float mk = mask[b * ld_m + t];
    float term = x[tg] - lse;
    if (eps > 0.f) {
        float s = 0.f;
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j)
                if (threadIdx.x + 256 * j < n4) s += ((xr[j][0] - lse) + (xr[j][1] - lse)) + ((xr[j][2] - lse) + (xr[j][3] - lse));
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) s += x[v] - lse;
        }
        s = block_sum_256(s, red);
        term = (1.0f - eps) * term + (eps / (float)V1) * s;
    }
    if (threadIdx.x == 0) {
        lse_out[r] = lse;
        row_loss[b * T + t] = -mk * term;
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void xe_logits_bwd_k(float* __restrict__ logits, long ldl, int B, int T, int V1,
                                                       const int64_t* __restrict__ target, long ld_t,
                                                       const float* __restrict__ mask, long ld_m, float eps, float gcoef,
                                                       const float* __restrict__ gdev, const float* __restrict__ lse_in) {
    const int r = blockIdx.x, t = r / B, b = r - t * B;
    float* x = logits + r * ldl;
    long tg = target[b * ld_t + t];
    if (tg < 0 || tg >= V1) tg = 0;
    const float c = mask[b * ld_m + t] * (gdev ? gcoef * gdev[0] : gcoef);     // mask * d loss / B
    const float lse = lse_in[r], uni = eps / (float)V1, hot = 1.0f - eps;
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i), o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = c * ((expf(v[e] - lse) - uni) - ((4 * i + e == tg) ? hot : 0.f));
            *reinterpret_cast<f32x4*>(x + 4 * i) = o;
        }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) x[v] = c * ((expf(x[v] - lse) - uni) - ((v == tg) ? hot : 0.f));
    }
}
extern "C" int rfn_xe_logits_fwd(const float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target,
                                 int64_t ld_target, const float* mask, int64_t ld_mask, float eps, float* lse,
                                 float* scratch, float* loss_out, int accumulate_loss, void* stream) {
    if (B <= 0 || T <= 0 || V1 <= 0 || ldl < V1 || eps < 0.f || eps >= 1.f) return RFN_ERR_SHAPE;
    if (!logits || !target || !mask || !lse || !scratch || !loss_out) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0))
        hipLaunchKernelGGL(xe_logits_fwd_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, lse, scratch);
    else
        hipLaunchKernelGGL(xe_logits_fwd_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, lse, scratch);
    RFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, scratch, B * T, 1.0f / (float)B, loss_out, accumulate_loss);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_xe_logits_bwd(float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                                 const float* mask, int64_t ld_mask, float eps, const float* lse, float gscale,
                                 const float* gscale_dev, void* stream) {
    if (B <= 0 || T <= 0 || V1 <= 0 || ldl < V1 || eps < 0.f || eps >= 1.f) return RFN_ERR_SHAPE;
    if (!logits || !target || !mask || !lse) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0))
        hipLaunchKernelGGL(xe_logits_bwd_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, gscale / (float)B, gscale_dev, lse);
    else
        hipLaunchKernelGGL(xe_logits_bwd_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, gscale / (float)B, gscale_dev, lse);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- distillation: the language term and a KL term towards a teacher row, straight from the logits (rfn.h) -----------------
// Rows as above (x = the student's time-major logits row r = t * B + b); z = the teacher's row (b, t), logits or log-probs
// (every term is invariant to a per-row shift of z), at teacher + b * z_sb + t * z_st.  it = 1 / temperature.
//   forward : lse(x) (log_softmax_row: xe_logits_fwd_k's bits), lse(x * it), lse(z * it) -> row_stats[0 / 1 / 2][r];
//             the xe row term, xe_logits_fwd_k's expression -> row_xe[b * T + t];
//             mask / it^2 * sum_{v : p_t(v) > 0} p_t(v) * (log p_t(v) - log p_s(v)) -> row_kd[b * T + t]
//   backward: d logits[v] = mask * g / B * ((1 - alpha) * (softmax(x)[v] - q[v]) + alpha / it * (p_s(v) - p_t(v))), written
//             over the logits.
// A -inf teacher entry has p_t = 0 and is skipped (no 0 * inf); a row with mask == 0 has exact zeros for its kd term and its
// gradient whatever its teacher row holds.  Vector form: both rows read once, 16 B per lane, into 2 x LSM_R4 f32x4.
// kd_each: f(x[v], z[v]) over this thread's share of the two rows, from the registers (vector form) or from memory.
template <bool VEC, class F>
__device__ __forceinline__ void kd_each(const float* __restrict__ x, const float* __restrict__ z, int V1,
                                        const f32x4 (&xr)[LSM_R4], const f32x4 (&zr)[LSM_R4], F f) {
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j)
            if (threadIdx.x + 256 * j < n4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) f(xr[j][e], zr[j][e]);
            }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) f(x[v], z[v]);
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void kd_logits_fwd_k(const float* __restrict__ logits, long ldl, int B, int T, int V1,
                                                       const int64_t* __restrict__ target, long ld_t,
                                                       const float* __restrict__ mask, long ld_m, float eps,
                                                       const float* __restrict__ teacher, long z_sb, long z_st, float it,
                                                       float* __restrict__ row_stats, float* __restrict__ row_xe,
                                                       float* __restrict__ row_kd) {
    __shared__ float red[4];
    const int r = blockIdx.x, t = r / B, b = r - t * B;      // time-major rows
    const float* x = logits + r * ldl;
    const float* z = teacher + b * z_sb + t * z_st;
    f32x4 xr[LSM_R4], zr[LSM_R4];
    const float lse = log_softmax_row<VEC>(x, V1, xr, red);
    long tg = target[b * ld_t + t];
    if (tg < 0 || tg >= V1) tg = 0;
    const float mk = mask[b * ld_m + t];
    float term = x[tg] - lse;                                // the xe term: xe_logits_fwd_k's expression, for its bits
    if (eps > 0.f) {
        float s = 0.f;
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j)
                if (threadIdx.x + 256 * j < n4) s += ((xr[j][0] - lse) + (xr[j][1] - lse)) + ((xr[j][2] - lse) + (xr[j][3] - lse));
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) s += x[v] - lse;
        }
        s = block_sum_256(s, red);
        term = (1.0f - eps) * term + (eps / (float)V1) * s;
    }
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) {
            const int i = threadIdx.x + 256 * j;
            zr[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (i < n4) zr[j] = *reinterpret_cast<const f32x4*>(z + 4 * i);
        }
    }
    // the tempered rows: it > 0, so max(x * it) is the rounded max(x) * it
    float mx = -INFINITY, mz = -INFINITY;
    kd_each<VEC>(x, z, V1, xr, zr, [&](float xv, float zv) {
        mx = fmaxf(mx, xv);
        mz = fmaxf(mz, zv);
    });
    mz = block_max_256(mz, red) * it;
    float lse_s = lse;
    if (it != 1.0f) mx = block_max_256(mx, red) * it;        // `it` is uniform over the grid
    float ss = 0.f, sz = 0.f;
    kd_each<VEC>(x, z, V1, xr, zr, [&](float xv, float zv) {
        if (it != 1.0f) ss += expf(xv * it - mx);
        sz += expf(zv * it - mz);                            // exp(-inf) = 0
    });
    if (it != 1.0f) lse_s = mx + logf(block_sum_256(ss, red));
    const float lse_t = mz + logf(block_sum_256(sz, red));
    float kl = 0.f;
    kd_each<VEC>(x, z, V1, xr, zr, [&](float xv, float zv) {
        const float lpt = zv * it - lse_t;
        const float pt = expf(lpt);
        kl += (pt > 0.f) ? pt * (lpt - (xv * it - lse_s)) : 0.f;
    });
    kl = block_sum_256(kl, red);
    if (threadIdx.x == 0) {
        const long n = (long)T * B;
        row_stats[r] = lse;
        row_stats[n + r] = lse_s;
        row_stats[2 * n + r] = lse_t;
        row_xe[b * T + t] = -mk * term;
        row_kd[b * T + t] = (mk != 0.f) ? mk * kl / (it * it) : 0.f;
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void kd_logits_bwd_k(float* __restrict__ logits, long ldl, int B, int T, int V1,
                                                       const int64_t* __restrict__ target, long ld_t,
                                                       const float* __restrict__ mask, long ld_m, float eps,
                                                       const float* __restrict__ teacher, long z_sb, long z_st, float alpha,
                                                       float it, float gcoef, const float* __restrict__ gdev,
                                                       const float* __restrict__ row_stats) {
    const int r = blockIdx.x, t = r / B, b = r - t * B;
    float* x = logits + r * ldl;
    const float* z = teacher + b * z_sb + t * z_st;
    long tg = target[b * ld_t + t];
    if (tg < 0 || tg >= V1) tg = 0;
    const float mk = mask[b * ld_m + t];
    if (mk == 0.f) {                                         // exact zeros, whatever the teacher row and its stats hold
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
            for (int i = threadIdx.x; i < n4; i += 256) *reinterpret_cast<f32x4*>(x + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) x[v] = 0.f;
        }
        return;
    }
    const float c = mk * (gdev ? gcoef * gdev[0] : gcoef);   // mask * d loss / B
    const long n = (long)T * B;
    const float lse = row_stats[r], lse_s = row_stats[n + r], lse_t = row_stats[2 * n + r];
    const float uni = eps / (float)V1, hot = 1.0f - eps, wx = 1.0f - alpha, wk = alpha / it;
    auto grad = [&](float xv, float zv, bool is_tg) {
        const float p = expf(xv - lse);
        const float ps = (it != 1.0f) ? expf(xv * it - lse_s) : p;      // it == 1: the two soft-maxes are one expf
        const float pt = expf(zv * it - lse_t);                          // exp(-inf) = 0
        return c * (wx * ((p - uni) - (is_tg ? hot : 0.f)) + wk * (ps - pt));
    };
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * i), zv = *reinterpret_cast<const f32x4*>(z + 4 * i);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = grad(xv[e], zv[e], 4 * i + e == tg);
            *reinterpret_cast<f32x4*>(x + 4 * i) = o;
        }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) x[v] = grad(x[v], z[v], v == tg);
    }
}
// out[0] (+)= (1 - alpha) * xe[0] + alpha * kd[0]
__global__ void kd_mix_k(const float* __restrict__ xe, const float* __restrict__ kd, float alpha, float* __restrict__ out,
                         int accumulate) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float l = (1.0f - alpha) * xe[0] + alpha * kd[0];
        out[0] = accumulate ? out[0] + l : l;
    }
}
static int kd_check(const void* logits, int64_t ldl, int B, int T, int V1, const void* target, const void* mask, float eps,
                    const void* teacher, int64_t z_sb, int64_t z_st, float alpha, float inv_temp) {
    if (B <= 0 || T <= 0 || V1 <= 0 || ldl < V1 || eps < 0.f || eps >= 1.f) return RFN_ERR_SHAPE;
    if (!(alpha >= 0.f && alpha <= 1.f) || !(inv_temp > 0.f) || !(inv_temp <= 3.402823466e38f)) return RFN_ERR_SHAPE;
    if ((z_sb < 0 ? -z_sb : z_sb) < V1 || (z_st < 0 ? -z_st : z_st) < V1) return RFN_ERR_SHAPE;
    if (!logits || !target || !mask || !teacher) return RFN_ERR_ARG;
    return RFN_OK;
}
// the vector form needs lsm_vec_ok for the student and its analogue for the teacher
static bool kd_vec_ok(const float* logits, int64_t ldl, int V1, const float* teacher, int64_t z_sb, int64_t z_st) {
    return lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0) && rfn_aligned16(teacher) && z_sb % 4 == 0 && z_st % 4 == 0;
}
extern "C" int rfn_kd_logits_fwd(const float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target,
                                 int64_t ld_target, const float* mask, int64_t ld_mask, float eps, const float* teacher,
                                 int64_t z_sb, int64_t z_st, float alpha, float inv_temp, float* row_stats, float* scratch,
                                 float* loss_out, int accumulate_loss, float* terms_out, void* stream) {
    const int rc = kd_check(logits, ldl, B, T, V1, target, mask, eps, teacher, z_sb, z_st, alpha, inv_temp);
    if (rc != RFN_OK) return rc;
    if (!row_stats || !scratch || !loss_out) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* row_kd = scratch + (size_t)B * T;
    if (kd_vec_ok(logits, ldl, V1, teacher, z_sb, z_st))
        hipLaunchKernelGGL(kd_logits_fwd_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, teacher, (long)z_sb, (long)z_st, inv_temp, row_stats,
                           scratch, row_kd);
    else
        hipLaunchKernelGGL(kd_logits_fwd_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, teacher, (long)z_sb, (long)z_st, inv_temp, row_stats,
                           scratch, row_kd);
    RFN_CHECK_LAUNCH();
    // the two sums by sum_k, in its order; without terms_out each lands on its own array's first slot (sum_k reads every
    // element before its one store)
    float* xe = terms_out ? terms_out : scratch;
    float* kd = terms_out ? terms_out + 1 : row_kd;
    hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, scratch, B * T, 1.0f / (float)B, xe, 0);
    RFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, row_kd, B * T, 1.0f / (float)B, kd, 0);
    RFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(kd_mix_k, dim3(1), dim3(64), 0, st, xe, kd, alpha, loss_out, accumulate_loss);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_kd_logits_bwd(float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                                 const float* mask, int64_t ld_mask, float eps, const float* teacher, int64_t z_sb,
                                 int64_t z_st, float alpha, float inv_temp, const float* row_stats, float gscale,
                                 const float* gscale_dev, void* stream) {
    const int rc = kd_check(logits, ldl, B, T, V1, target, mask, eps, teacher, z_sb, z_st, alpha, inv_temp);
    if (rc != RFN_OK) return rc;
    if (!row_stats) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (kd_vec_ok(logits, ldl, V1, teacher, z_sb, z_st))
        hipLaunchKernelGGL(kd_logits_bwd_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, teacher, (long)z_sb, (long)z_st, alpha, inv_temp,
                           gscale / (float)B, gscale_dev, row_stats);
    else
        hipLaunchKernelGGL(kd_logits_bwd_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, teacher, (long)z_sb, (long)z_st, alpha, inv_temp,
                           gscale / (float)B, gscale_dev, row_stats);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- distillation from a compact teacher: the K <= 32 best entries of each teacher row (rfn.h) ---------------------------
// The pair above with the teacher's row z given as K (id, value) pairs: z[id_k] = val_k, -inf everywhere else, so p_t lives
// on the K entries alone and the KL term and its gradient touch K elements of the student's row.  An entry whose id is
// outside [0, V1) or whose value is -inf is padding (never used as an index).  The student's row is read exactly as the XE
// pair reads it (log_softmax_row: 16 B per lane or element-wise); the K entries sit in the first K lanes of wave 0, one
// each, and their reductions are that wave's shuffles (K <= 32 < 64 lanes) in a fixed order: no atomics.
//   forward : lse(x), lse(x * it) as above; lse over the live entries of val * it -> row_stats[2][r]; the KL sum gathers
//             x[id_k] from the row this block has just read.
//   backward: d logits is written IN PLACE, so the order is (1) wave 0 gathers x[id_k] and waits for the loads, block
//             barrier, (2) all lanes write the teacher-free gradient c * (wx * (p - q) + wk * p_s) over the row and wait for
//             their stores, block barrier, (3) lane k rewrites element id_k in full, with p_t(k), from its gathered x[id_k]
//             (the dense kernel's expression; the live ids of a row are distinct, so no two lanes write one element).
// A row with mask == 0 reads neither its ids nor its values.
#define KD_TOPK 32
struct KdEntry {
    int id;          // in [0, V1) when live
    float z;         // val * it; -inf when not live
    bool live;
};
// lane k < K of wave 0 takes entry k of the row; every other lane, and every lane of a row with mask == 0, gets a dead entry
__device__ __forceinline__ KdEntry kd_topk_entry(const int* __restrict__ ids, const float* __restrict__ val, int K, int V1,
                                                 float it, bool row_live) {
    KdEntry e{0, -INFINITY, false};
    if (row_live && (int)threadIdx.x < K) {
        const int id = ids[threadIdx.x];
        const float v = val[threadIdx.x];
        if (id >= 0 && id < V1 && v != -INFINITY) {
            e.id = id;
            e.z = v * it;
            e.live = true;
        }
    }
    return e;
}
template <bool VEC>
__global__ __launch_bounds__(256) void kd_topk_fwd_k(const float* __restrict__ logits, long ldl, int B, int T, int V1,
                                                     const int64_t* __restrict__ target, long ld_t,
                                                     const float* __restrict__ mask, long ld_m, float eps,
                                                     const int* __restrict__ t_ids, long i_sb, long i_st,
                                                     const float* __restrict__ t_val, long v_sb, long v_st, int K, float it,
                                                     float* __restrict__ row_stats, float* __restrict__ row_xe,
                                                     float* __restrict__ row_kd) {
    __shared__ float red[4];
    const int r = blockIdx.x, t = r / B, b = r - t * B;      // time-major rows
    const float* x = logits + r * ldl;
    f32x4 xr[LSM_R4];
    const float lse = log_softmax_row<VEC>(x, V1, xr, red);
    long tg = target[b * ld_t + t];
    if (tg < 0 || tg >= V1) tg = 0;
    const float mk = mask[b * ld_m + t];
    float term = x[tg] - lse;                                // the xe term: xe_logits_fwd_k's expression, for its bits
    if (eps > 0.f) {
        float s = 0.f;
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j)
                if (threadIdx.x + 256 * j < n4) s += ((xr[j][0] - lse) + (xr[j][1] - lse)) + ((xr[j][2] - lse) + (xr[j][3] - lse));
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) s += x[v] - lse;
        }
        s = block_sum_256(s, red);
        term = (1.0f - eps) * term + (eps / (float)V1) * s;
    }
    float lse_s = lse;
    if (it != 1.0f) {                                        // `it` is uniform over the grid; it > 0: max(x * it) = max(x) * it
        float mx = -INFINITY, ss = 0.f;
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j)
                if (threadIdx.x + 256 * j < n4) mx = fmaxf(mx, fmaxf(fmaxf(xr[j][0], xr[j][1]), fmaxf(xr[j][2], xr[j][3])));
            mx = block_max_256(mx, red) * it;
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j)
                if (threadIdx.x + 256 * j < n4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) ss += expf(xr[j][e] * it - mx);
                }
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) mx = fmaxf(mx, x[v]);
            mx = block_max_256(mx, red) * it;
            for (int v = threadIdx.x; v < V1; v += 256) ss += expf(x[v] * it - mx);
        }
        lse_s = mx + logf(block_sum_256(ss, red));
    }
    if (threadIdx.x < 64) {                                  // wave 0: the K entries, one per lane
        const bool row_live = mk != 0.f;
        const KdEntry e = kd_topk_entry(t_ids + b * i_sb + t * i_st, t_val + b * v_sb + t * v_st, K, V1, it, row_live);
        const float mz = rfn_wave_max(e.z);
        const float lse_t = mz + logf(rfn_wave_sum(e.live ? expf(e.z - mz) : 0.f));
        float kl = 0.f;
        if (e.live) {
            const float lpt = e.z - lse_t;
            const float pt = expf(lpt);
            if (pt > 0.f) kl = pt * (lpt - (x[e.id] * it - lse_s));
        }
        kl = rfn_wave_sum(kl);
        if (threadIdx.x == 0) {
            const long n = (long)T * B;
            row_stats[r] = lse;
            row_stats[n + r] = lse_s;
            row_stats[2 * n + r] = row_live ? lse_t : 0.f;
            row_xe[b * T + t] = -mk * term;
            row_kd[b * T + t] = row_live ? mk * kl / (it * it) : 0.f;
        }
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void kd_topk_bwd_k(float* __restrict__ logits, long ldl, int B, int T, int V1,
                                                     const int64_t* __restrict__ target, long ld_t,
                                                     const float* __restrict__ mask, long ld_m, float eps,
                                                     const int* __restrict__ t_ids, long i_sb, long i_st,
                                                     const float* __restrict__ t_val, long v_sb, long v_st, int K, float alpha,
                                                     float it, float gcoef, const float* __restrict__ gdev,
                                                     const float* __restrict__ row_stats) {
    const int r = blockIdx.x, t = r / B, b = r - t * B;
    float* x = logits + r * ldl;
    long tg = target[b * ld_t + t];
    if (tg < 0 || tg >= V1) tg = 0;
    const float mk = mask[b * ld_m + t];
    if (mk == 0.f) {                                         // exact zeros; the teacher's entries are not read (block-uniform)
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
            for (int i = threadIdx.x; i < n4; i += 256) *reinterpret_cast<f32x4*>(x + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) x[v] = 0.f;
        }
        return;
    }
    const float c = mk * (gdev ? gcoef * gdev[0] : gcoef);   // mask * d loss / B
    const long n = (long)T * B;
    const float lse = row_stats[r], lse_s = row_stats[n + r], lse_t = row_stats[2 * n + r];
    const float uni = eps / (float)V1, hot = 1.0f - eps, wx = 1.0f - alpha, wk = alpha / it;
    auto grad = [&](float xv, float pt, bool is_tg) {        // kd_logits_bwd_k's expression
        const float p = expf(xv - lse);
        const float ps = (it != 1.0f) ? expf(xv * it - lse_s) : p;
        return c * (wx * ((p - uni) - (is_tg ? hot : 0.f)) + wk * (ps - pt));
    };
    // (1) the original x[id_k], before any lane of the block writes: the loads have returned when the barrier is passed
    const KdEntry e = kd_topk_entry(t_ids + b * i_sb + t * i_st, t_val + b * v_sb + t * v_st, K, V1, it, true);
    float xk = 0.f;
    if (e.live) xk = x[e.id];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // (2) the row without the teacher's term
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * i);
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = grad(xv[q], 0.f, 4 * i + q == tg);
            *reinterpret_cast<f32x4*>(x + 4 * i) = o;
        }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) x[v] = grad(x[v], 0.f, v == tg);
    }
    // (3) the K entries again, in full, behind every lane's stores of (2)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (e.live) x[e.id] = grad(xk, expf(e.z - lse_t), e.id == tg);
}
static int kd_topk_check(const void* logits, int64_t ldl, int B, int T, int V1, const void* target, const void* mask, float eps,
                         const void* t_ids, int64_t i_sb, int64_t i_st, const void* t_val, int64_t v_sb, int64_t v_st, int K,
                         float alpha, float inv_temp) {
    if (B <= 0 || T <= 0 || V1 <= 0 || ldl < V1 || eps < 0.f || eps >= 1.f) return RFN_ERR_SHAPE;
    if (!(alpha >= 0.f && alpha <= 1.f) || !(inv_temp > 0.f) || !(inv_temp <= 3.402823466e38f)) return RFN_ERR_SHAPE;
    if (K < 1 || K > KD_TOPK) return RFN_ERR_SHAPE;
    for (const int64_t s : {i_sb, i_st, v_sb, v_st})
        if ((s < 0 ? -s : s) < K) return RFN_ERR_SHAPE;
    if (!logits || !target || !mask || !t_ids || !t_val) return RFN_ERR_ARG;
    return RFN_OK;
}
extern "C" int rfn_kd_topk_fwd(const float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                               const float* mask, int64_t ld_mask, float eps, const int32_t* t_ids, int64_t i_sb, int64_t i_st,
                               const float* t_val, int64_t v_sb, int64_t v_st, int K, float alpha, float inv_temp,
                               float* row_stats, float* scratch, float* loss_out, int accumulate_loss, float* terms_out,
                               void* stream) {
    const int rc = kd_topk_check(logits, ldl, B, T, V1, target, mask, eps, t_ids, i_sb, i_st, t_val, v_sb, v_st, K, alpha, inv_temp);
    if (rc != RFN_OK) return rc;
    if (!row_stats || !scratch || !loss_out) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* row_kd = scratch + (size_t)B * T;
    if (lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0))
        hipLaunchKernelGGL(kd_topk_fwd_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, t_ids, (long)i_sb, (long)i_st, t_val, (long)v_sb, (long)v_st,
                           K, inv_temp, row_stats, scratch, row_kd);
    else
        hipLaunchKernelGGL(kd_topk_fwd_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, t_ids, (long)i_sb, (long)i_st, t_val, (long)v_sb, (long)v_st,
                           K, inv_temp, row_stats, scratch, row_kd);
    RFN_CHECK_LAUNCH();
    // the two sums and the mix as in rfn_kd_logits_fwd
    float* xe = terms_out ? terms_out : scratch;
    float* kd = terms_out ? terms_out + 1 : row_kd;
    hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, scratch, B * T, 1.0f / (float)B, xe, 0);
    RFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, row_kd, B * T, 1.0f / (float)B, kd, 0);
    RFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(kd_mix_k, dim3(1), dim3(64), 0, st, xe, kd, alpha, loss_out, accumulate_loss);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_kd_topk_bwd(float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                               const float* mask, int64_t ld_mask, float eps, const int32_t* t_ids, int64_t i_sb, int64_t i_st,
                               const float* t_val, int64_t v_sb, int64_t v_st, int K, float alpha, float inv_temp,
                               const float* row_stats, float gscale, const float* gscale_dev, void* stream) {
    const int rc = kd_topk_check(logits, ldl, B, T, V1, target, mask, eps, t_ids, i_sb, i_st, t_val, v_sb, v_st, K, alpha, inv_temp);
    if (rc != RFN_OK) return rc;
    if (!row_stats) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0))
        hipLaunchKernelGGL(kd_topk_bwd_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, t_ids, (long)i_sb, (long)i_st, t_val, (long)v_sb, (long)v_st,
                           K, alpha, inv_temp, gscale / (float)B, gscale_dev, row_stats);
    else
        hipLaunchKernelGGL(kd_topk_bwd_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, target,
                           (long)ld_target, mask, (long)ld_mask, eps, t_ids, (long)i_sb, (long)i_st, t_val, (long)v_sb, (long)v_st,
                           K, alpha, inv_temp, gscale / (float)B, gscale_dev, row_stats);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- RL reward criterion, policy + entropy terms (misc/utils.py:50-72) ------------------------------------
// One block per (b, t) row:  term = -pol(b,t) * mask(b,t) + entropy_reg * mask0(b,t) * sum_v lp*exp(lp),
// mask0 = seq > 0, mask = [1, mask0[:, :-1]] (the step AFTER an END still counts), pol = input*reward or the
// PPO-clip surrogate min(surr1, clamp(surr1, 1-c, 1+c)*reward) with surr1 = exp(input)/(1e-5+exp(old))*reward
// (written as in the reference: it clamps surr1, not the ratio).  Gradients w.r.t. input and logprobs_all.
__global__ __launch_bounds__(256) void rl_loss_k(const float* __restrict__ inp, long ld_in, const int64_t* __restrict__ seq,
                                                 long ld_seq, const float* __restrict__ reward, long ld_rw,
                                                 const float* __restrict__ lp_all, long lp_sb, long lp_st, int T, int V1,
                                                 float entropy_reg, const float* __restrict__ old_lp, long ld_old,
                                                 int use_ppo, float ppo_clip, float inv_B_host, float* __restrict__ row_loss,
                                                 float* __restrict__ d_inp, long ld_din, float* __restrict__ d_lp,
                                                 long dlp_sb, long dlp_st, int T_all, const float* __restrict__ gdev) {
    __shared__ float red[4];
    // T_all >= T rows per caption are launched; rows t >= T do not enter the loss: their d_logprobs_all row is zero
    const int r = blockIdx.x, b = r / T_all, t = r - b * T_all;
    if (t >= T) {
        if (d_lp) {
            float* d = d_lp + b * dlp_sb + t * dlp_st;
            for (int v = threadIdx.x; v < V1; v += 256) d[v] = 0.f;
        }
        return;
    }
    const float inv_B = gdev ? inv_B_host * gdev[0] : inv_B_host;   // upstream d loss, read on the device (no host sync)
    const float m0 = (seq[b * ld_seq + t] > 0) ? 1.f : 0.f;
    const float mk = (t == 0) ? 1.f : ((seq[b * ld_seq + t - 1] > 0) ? 1.f : 0.f);
    const float* lp = lp_all + b * lp_sb + t * lp_st;
    if (row_loss) {
        float e = 0.f;
        if (m0 != 0.f && entropy_reg != 0.f)
            for (int v = threadIdx.x; v < V1; v += 256) e += lp[v] * expf(lp[v]);
        e = block_sum_256(e, red);
        if (threadIdx.x == 0) {
            const float x = inp[b * ld_in + t], rw = reward[b * ld_rw + t];
            float pol;
            if (use_ppo) {
                const float ratio = expf(x) / (1e-5f + expf(old_lp[b * ld_old + t]));
                const float s1 = ratio * rw;
                const float s2 = fminf(fmaxf(s1, 1.f - ppo_clip), 1.f + ppo_clip) * rw;
                pol = fminf(s1, s2);
            } else {
                pol = x * rw;
            }
            row_loss[b * T + t] = -pol * mk + entropy_reg * m0 * e;
        }
    }
    if (d_lp) {
        float* d = d_lp + b * dlp_sb + t * dlp_st;
        const float c = entropy_reg * m0 * inv_B;
        for (int v = threadIdx.x; v < V1; v += 256) d[v] = (c != 0.f) ? c * expf(lp[v]) * (1.f + lp[v]) : 0.f;
    }
    if (d_inp && threadIdx.x == 0) {
        const float x = inp[b * ld_in + t], rw = reward[b * ld_rw + t];
        float g;
        if (use_ppo) {
            const float ratio = expf(x) / (1e-5f + expf(old_lp[b * ld_old + t]));
            const float s1 = ratio * rw;
            const float cl = fminf(fmaxf(s1, 1.f - ppo_clip), 1.f + ppo_clip);
            const float s2 = cl * rw;
            const float ds1 = ratio * rw;                                        // d surr1 / d input
            const float ds2 = (s1 > 1.f - ppo_clip && s1 < 1.f + ppo_clip) ? ds1 * rw : 0.f;
            g = (s1 <= s2) ? ds1 : ds2;
        } else {
            g = rw;
        }
        d_inp[b * ld_din + t] = -g * mk * inv_B;
    }
}
extern "C" int rfn_rl_loss_ex(const float* input, int64_t ld_in, const int64_t* seq, int64_t ld_seq, const float* reward,
                              int64_t ld_rw, const float* logprobs_all, int64_t lp_sb, int64_t lp_st, int B, int T, int T_all,
                              int V1, float entropy_reg, const float* old_logprobs, int64_t ld_old, int use_ppo,
                              float ppo_clip, const float* gscale_dev, float* scratch, float* loss_out, int accumulate_loss,
                              float* d_input, int64_t ld_din, float* d_logprobs_all, int64_t dlp_sb, int64_t dlp_st,
                              void* stream) {
    if (B <= 0 || T <= 0 || V1 <= 0 || T_all < T) return RFN_ERR_SHAPE;
    if (!input || !seq || !reward || !logprobs_all || (loss_out && !scratch) || (use_ppo && !old_logprobs))
        return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int rows = d_logprobs_all ? T_all : T;      // the extra rows exist only to zero d_logprobs_all[:, T:]
    hipLaunchKernelGGL(rl_loss_k, dim3(B * rows), dim3(256), 0, st, input, (long)ld_in, seq, (long)ld_seq, reward,
                       (long)ld_rw, logprobs_all, (long)lp_sb, (long)lp_st, T, V1, entropy_reg, old_logprobs,
                       (long)ld_old, use_ppo, ppo_clip, 1.0f / (float)B, loss_out ? scratch : nullptr, d_input,
                       (long)ld_din, d_logprobs_all, (long)dlp_sb, (long)dlp_st, rows, gscale_dev);
    RFN_CHECK_LAUNCH();
    if (loss_out) {
        hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, scratch, B * T, 1.0f / (float)B, loss_out, accumulate_loss);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}
extern "C" int rfn_rl_loss(const float* input, int64_t ld_in, const int64_t* seq, int64_t ld_seq, const float* reward,
                           int64_t ld_rw, const float* logprobs_all, int64_t lp_sb, int64_t lp_st, int B, int T, int V1,
                           float entropy_reg, const float* old_logprobs, int64_t ld_old, int use_ppo, float ppo_clip,
                           float* scratch, float* loss_out, int accumulate_loss, float* d_input, int64_t ld_din,
                           float* d_logprobs_all, int64_t dlp_sb, int64_t dlp_st, void* stream) {
    return rfn_rl_loss_ex(input, ld_in, seq, ld_seq, reward, ld_rw, logprobs_all, lp_sb, lp_st, B, T, T, V1, entropy_reg,
                          old_logprobs, ld_old, use_ppo, ppo_clip, nullptr, scratch, loss_out, accumulate_loss, d_input,
                          ld_din, d_logprobs_all, dlp_sb, dlp_st, stream);
}

// ---- the same criterion straight from the logits (rfn.h rfn_rl_logits_fwd; misc/utils.py:50-72 on F.log_softmax rows) ---------
// Rows as the XE pair takes them (x = the time-major logits row r = t * B + b), tok = seq[b, t] clamped as its targets are;
// m0, mk, pol exactly as rl_loss_k writes them, on lp_tok = x[tok] - lse (the bits rfn_log_softmax_fwd puts there).
//   forward : lse (log_softmax_row), Hm = sum_v lp_v * exp(lp_v) (only where entropy_reg * m0 != 0, else 0), lp_tok
//             -> row_stats[0 / 1 / 2][r]; tok_lp[b, t] = lp_tok; -pol * mk + entropy_reg * m0 * Hm -> row_loss[b * T + t]
//             (and, when the caller wants the two terms for logging, each on its own -> row_terms[0 / 1][b * T + t])
//   backward: d x_v = a * ([v == tok] - p_v) + e * p_v * (lp_v - Hm), written over the logits; a = -(g / B) * mk * d pol / d lp_tok,
//             e = (g / B) * entropy_reg * m0.  a == 0 and e == 0: exact zeros; e == 0: the entropy term is not evaluated.
struct RlRow {
    long tok;
    float m0, mk, rw, old;
};
__device__ __forceinline__ RlRow rl_row(const int64_t* __restrict__ seq, long ld_seq, const float* __restrict__ reward, long ld_rw,
                                        const float* __restrict__ old_lp, long ld_old, int use_ppo, int b, int t, int V1) {
    RlRow q;
    const int64_t s = seq[b * ld_seq + t];
    q.tok = (s < 0 || s >= V1) ? 0 : (long)s;
    q.m0 = (s > 0) ? 1.f : 0.f;
    q.mk = (t == 0) ? 1.f : ((seq[b * ld_seq + t - 1] > 0) ? 1.f : 0.f);
    q.rw = reward[b * ld_rw + t];
    q.old = use_ppo ? old_lp[b * ld_old + t] : 0.f;
    return q;
}
template <bool VEC>
__global__ __launch_bounds__(256) void rl_logits_fwd_k(const float* __restrict__ logits, long ldl, int B, int T, int V1,
                                                       const int64_t* __restrict__ seq, long ld_seq,
                                                       const float* __restrict__ reward, long ld_rw, float entropy_reg,
                                                       const float* __restrict__ old_lp, long ld_old, int use_ppo, float ppo_clip,
                                                       float* __restrict__ row_stats, float* __restrict__ tok_lp, long ld_tl,
                                                       float* __restrict__ row_loss, float* __restrict__ row_terms) {
    __shared__ float red[4];
    const int r = blockIdx.x, t = r / B, b = r - t * B;      // time-major rows
    const float* x = logits + r * ldl;
    f32x4 xr[LSM_R4];
    const float lse = log_softmax_row<VEC>(x, V1, xr, red);
    const RlRow q = rl_row(seq, ld_seq, reward, ld_rw, old_lp, ld_old, use_ppo, b, t, V1);
    float Hm = 0.f;
    if (entropy_reg != 0.f && q.m0 != 0.f) {                 // block-uniform
        float s = 0.f;
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j)
                if (threadIdx.x + 256 * j < n4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float lp = xr[j][e] - lse;
                        s += lp * expf(lp);
                    }
                }
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) {
                const float lp = x[v] - lse;
                s += lp * expf(lp);
            }
        }
        Hm = block_sum_256(s, red);
    }
    if (threadIdx.x == 0) {
        const float lpt = x[q.tok] - lse;
        float pol;
        if (use_ppo) {
            const float ratio = expf(lpt) / (1e-5f + expf(q.old));
            const float s1 = ratio * q.rw;
            const float s2 = fminf(fmaxf(s1, 1.f - ppo_clip), 1.f + ppo_clip) * q.rw;
            pol = fminf(s1, s2);
        } else {
            pol = lpt * q.rw;
        }
        const long n = (long)T * B;
        row_stats[r] = lse;
        row_stats[n + r] = Hm;
        row_stats[2 * n + r] = lpt;
        tok_lp[b * ld_tl + t] = lpt;
        row_loss[b * T + t] = -pol * q.mk + entropy_reg * q.m0 * Hm;
        if (row_terms) {                                     // the two terms on their own, for logging
            row_terms[b * T + t] = -pol * q.mk;
            row_terms[n + b * T + t] = entropy_reg * q.m0 * Hm;
        }
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void rl_logits_bwd_k(float* __restrict__ logits, long ldl, int B, int T, int V1,
                                                       const int64_t* __restrict__ seq, long ld_seq,
                                                       const float* __restrict__ reward, long ld_rw, float entropy_reg,
                                                       const float* __restrict__ old_lp, long ld_old, int use_ppo, float ppo_clip,
                                                       float gcoef, const float* __restrict__ gdev,
                                                       const float* __restrict__ row_stats) {
    const int r = blockIdx.x, t = r / B, b = r - t * B;
    float* x = logits + r * ldl;
    const RlRow q = rl_row(seq, ld_seq, reward, ld_rw, old_lp, ld_old, use_ppo, b, t, V1);
    const long n = (long)T * B;
    const float gc = gdev ? gcoef * gdev[0] : gcoef;         // d loss / B, read on the device
    float a = 0.f;
    if (q.mk != 0.f) {
        float dpol = q.rw;
        if (use_ppo) {                                       // rl_loss_k's d_inp
            const float ratio = expf(row_stats[2 * n + r]) / (1e-5f + expf(q.old));
            const float s1 = ratio * q.rw;
            const float s2 = fminf(fmaxf(s1, 1.f - ppo_clip), 1.f + ppo_clip) * q.rw;
            const float ds1 = ratio * q.rw;
            const float ds2 = (s1 > 1.f - ppo_clip && s1 < 1.f + ppo_clip) ? ds1 * q.rw : 0.f;
            dpol = (s1 <= s2) ? ds1 : ds2;
        }
        a = -gc * q.mk * dpol;
    }
    const float e = (q.m0 != 0.f && entropy_reg != 0.f) ? gc * entropy_reg * q.m0 : 0.f;
    if (a == 0.f && e == 0.f) {                              // exact zeros (block-uniform): masked rows, zero rewards
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
            for (int i = threadIdx.x; i < n4; i += 256) *reinterpret_cast<f32x4*>(x + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) x[v] = 0.f;
        }
        return;
    }
    const float lse = row_stats[r], Hm = row_stats[n + r];
    const long tok = q.tok;
    auto grad = [&](float xv, bool is_tok) {
        const float lp = xv - lse;
        const float p = expf(lp);
        const float pg = a * ((is_tok ? 1.f : 0.f) - p);
        return (e != 0.f) ? pg + e * p * (lp - Hm) : pg;     // e == 0: no trace of the entropy term
    };
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = grad(v[k], 4 * i + k == tok);
            *reinterpret_cast<f32x4*>(x + 4 * i) = o;
        }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) x[v] = grad(x[v], v == tok);
    }
}
static int rl_logits_check(const void* logits, int64_t ldl, int B, int T, int V1, const void* seq, const void* reward,
                           const void* old_logprobs, int use_ppo, const void* row_stats) {
    if (B <= 0 || T <= 0 || V1 <= 0 || ldl < V1) return RFN_ERR_SHAPE;
    if (!logits || !seq || !reward || !row_stats || (use_ppo && !old_logprobs)) return RFN_ERR_ARG;
    return RFN_OK;
}
extern "C" int rfn_rl_logits_fwd(const float* logits, int64_t ldl, int B, int T, int V1, const int64_t* seq, int64_t ld_seq,
                                 const float* reward, int64_t ld_rw, float entropy_reg, const float* old_logprobs, int64_t ld_old,
                                 int use_ppo, float ppo_clip, float* row_stats, float* tok_lp, int64_t ld_tok_lp, float* scratch,
                                 float* loss_out, int accumulate_loss, float* terms_out, void* stream) {
    const int rc = rl_logits_check(logits, ldl, B, T, V1, seq, reward, old_logprobs, use_ppo, row_stats);
    if (rc != RFN_OK) return rc;
    if (ld_tok_lp < T) return RFN_ERR_SHAPE;
    if (!tok_lp || !scratch || !loss_out) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* row_terms = terms_out ? scratch + (size_t)B * T : nullptr;
    if (lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0))
        hipLaunchKernelGGL(rl_logits_fwd_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, seq, (long)ld_seq,
                           reward, (long)ld_rw, entropy_reg, old_logprobs, (long)ld_old, use_ppo, ppo_clip, row_stats, tok_lp,
                           (long)ld_tok_lp, scratch, row_terms);
    else
        hipLaunchKernelGGL(rl_logits_fwd_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, seq, (long)ld_seq,
                           reward, (long)ld_rw, entropy_reg, old_logprobs, (long)ld_old, use_ppo, ppo_clip, row_stats, tok_lp,
                           (long)ld_tok_lp, scratch, row_terms);
    RFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, scratch, B * T, 1.0f / (float)B, loss_out, accumulate_loss);
    RFN_CHECK_LAUNCH();
    for (int k = 0; terms_out && k < 2; ++k) {
        hipLaunchKernelGGL(sum_k, dim3(1), dim3(256), 0, st, row_terms + (size_t)k * B * T, B * T, 1.0f / (float)B, terms_out + k, 0);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}
extern "C" int rfn_rl_logits_bwd(float* logits, int64_t ldl, int B, int T, int V1, const int64_t* seq, int64_t ld_seq,
                                 const float* reward, int64_t ld_rw, float entropy_reg, const float* old_logprobs, int64_t ld_old,
                                 int use_ppo, float ppo_clip, const float* row_stats, float gscale, const float* gscale_dev,
                                 void* stream) {
    const int rc = rl_logits_check(logits, ldl, B, T, V1, seq, reward, old_logprobs, use_ppo, row_stats);
    if (rc != RFN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0))
        hipLaunchKernelGGL(rl_logits_bwd_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, seq, (long)ld_seq,
                           reward, (long)ld_rw, entropy_reg, old_logprobs, (long)ld_old, use_ppo, ppo_clip, gscale / (float)B,
                           gscale_dev, row_stats);
    else
        hipLaunchKernelGGL(rl_logits_bwd_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, T, V1, seq, (long)ld_seq,
                           reward, (long)ld_rw, entropy_reg, old_logprobs, (long)ld_old, use_ppo, ppo_clip, gscale / (float)B,
                           gscale_dev, row_stats);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- nn.MultiLabelMarginLoss (mean) -----------------------------------------------------------------
// Row b: targets = ids before the first -1; loss_b = sum_{j in targets} sum_{i not target}
// max(0, 1 - x[j] + x[i]) / K.  One block per row; hit counts per target through LDS integer atomics.
struct MlmHeads {
    const float* pred[RFN_MAX_ENC + 1];
    float* dpred[RFN_MAX_ENC + 1];
};
__global__ __launch_bounds__(256) void mlm_k(const MlmHeads hd, int K, const int64_t* __restrict__ target, float gcoef,
                                             const float* __restrict__ gdev, float* __restrict__ row_loss) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* x = sm;                                   // [K]
    int* tg = reinterpret_cast<int*>(sm + K);        // [K] target list
    int* cnt = tg + K;                               // [K] hits per target slot
    unsigned char* is_t = reinterpret_cast<unsigned char*>(cnt + K);  // [K]
    __shared__ int nt_s;
    __shared__ float red[4];
    const int b = blockIdx.x, head = blockIdx.y;
    const float* pred = hd.pred[head];
    float* dpred = hd.dpred[head];
    if (gdev) gcoef *= gdev[0];
    for (int i = threadIdx.x; i < K; i += 256) {
        x[i] = pred[(long)b * K + i];
        is_t[i] = 0;
        cnt[i] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (; n < K; ++n) {
            const long t = target[(long)b * K + n];
            if (t < 0 || t >= K) break;
            tg[n] = (int)t;
            is_t[t] = 1;
        }
        nt_s = n;
    }
    __syncthreads();
    const int nt = nt_s;
    const float invK = 1.0f / (float)K;
    float loss = 0.f;
    for (int i = threadIdx.x; i < K; i += 256) {
        float gi = 0.f;
        if (!is_t[i]) {
            for (int n = 0; n < nt; ++n) {
                const float z = 1.0f - x[tg[n]] + x[i];
                if (z > 0.f) {
                    loss += z;
                    gi += 1.0f;
                    atomicAdd(&cnt[n], 1);
                }
            }
        }
        if (dpred) dpred[(long)b * K + i] = gi * invK * gcoef;  // targets fixed up below
    }
    loss = block_sum_256(loss, red);  // also orders the dpred writes above before the fix-up
    if (row_loss && threadIdx.x == 0) row_loss[(long)head * gridDim.x + b] = loss * invK;
    if (dpred && threadIdx.x == 0) {
        // a duplicated target id receives the hits of every slot that names it
        for (int n = 0; n < nt; ++n) dpred[(long)b * K + tg[n]] = 0.f;
        for (int n = 0; n < nt; ++n) dpred[(long)b * K + tg[n]] -= (float)cnt[n] * invK * gcoef;
    }
}
// out[0] (+)= scale * sum(x[g*n .. g*n+n)) for g = 0..G-1 in order: the per-head sums are added one after the other,
// exactly as G calls of sum_k would
__global__ __launch_bounds__(256) void sum_groups_k(const float* __restrict__ x, int n, int G, float scale,
                                                    float* __restrict__ out, int accumulate) {
    __shared__ float red[4];
    float total = accumulate ? out[0] : 0.f;
    for (int g = 0; g < G; ++g) {
        float s = 0.f;
        for (int i = threadIdx.x; i < n; i += 256) s += x[(long)g * n + i];
        s = block_sum_256(s, red);
        total = (g == 0 && !accumulate) ? s * scale : total + s * scale;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = total;
}
extern "C" int rfn_multilabel_margin_grouped(int nheads, const float* const* preds, int B, int K, const int64_t* target,
                                             float scale, float gscale, const float* gscale_dev, float* scratch,
                                             float* loss_out, int accumulate_loss, float* const* dpreds,
                                             void* stream) {
    if (nheads < 1 || nheads > RFN_MAX_ENC + 1 || B <= 0 || K <= 0) return RFN_ERR_SHAPE;
    if (!preds || !target || (loss_out && !scratch)) return RFN_ERR_ARG;
    const size_t lds = (size_t)K * (sizeof(float) + 2 * sizeof(int) + 1) + 16;
    if (lds > 60 * 1024) return RFN_ERR_SHAPE;
    MlmHeads hd;
    memset(&hd, 0, sizeof(hd));
    for (int h = 0; h < nheads; ++h) {
        if (!preds[h]) return RFN_ERR_ARG;
        hd.pred[h] = preds[h];
        hd.dpred[h] = dpreds ? dpreds[h] : nullptr;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mlm_k, dim3(B, nheads), dim3(256), lds, st, hd, K, target, scale * gscale / (float)B, gscale_dev,
                       loss_out ? scratch : nullptr);
    RFN_CHECK_LAUNCH();
    if (loss_out) {
        hipLaunchKernelGGL(sum_groups_k, dim3(1), dim3(256), 0, st, scratch, B, nheads, scale / (float)B, loss_out,
                           accumulate_loss);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}
extern "C" int rfn_multilabel_margin(const float* pred, int B, int K, const int64_t* target, float scale, float gscale,
                                     float* scratch, float* loss_out, int accumulate_loss, float* dpred,
                                     void* stream) {
    if (!pred) return RFN_ERR_ARG;
    return rfn_multilabel_margin_grouped(1, &pred, B, K, target, scale, gscale, nullptr, scratch, loss_out,
                                         accumulate_loss, dpred ? &dpred : nullptr, stream);
}
