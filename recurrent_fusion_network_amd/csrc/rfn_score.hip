// Scoring GIVEN captions from the decoder's logits, without materialising the log-probs (rfn.h "caption scoring"): per position
// the log-prob of the token that was given, its rank in the step's distribution and the distribution's entropy; per caption
// the fp64 sum of its log-probs and its length.  One block of 256 per logits row (rfn_rows.h): a row that qualifies is read
// once, 16 B per lane, and stays in registers for all three outputs.
#include "rfn_rows.h"

// integer twin of block_sum_256 (the rank is a count: exact in any order)
__device__ __forceinline__ int block_count_256(int v, int* red /* [4] LDS */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// an id outside [0, V1) reads as 0, for the gather and for the live rule alike
__device__ __forceinline__ int score_id(int64_t id, int V1) { return (id < 0 || id >= V1) ? 0 : (int)id; }

// one entry's share of -sum_v p_v * (x[v] - lse); an entry of probability 0 (a -inf logit, a padding lane) counts 0, not 0 * inf
__device__ __forceinline__ float score_ent_term(float x, float lse) {
    const float lp = x - lse, p = expf(lp);
    return p == 0.f ? 0.f : -(p * lp);
}

template <bool VEC>
__global__ __launch_bounds__(256) void score_logits_k(const float* __restrict__ logits, long ldl, int B, int t0, int V1,
                                                      const int64_t* __restrict__ target, long ld_t, int include_end,
                                                      float* __restrict__ tok_lp, int* __restrict__ tok_rank,
                                                      float* __restrict__ tok_ent, long ld_out) {
    __shared__ float red[4];
    __shared__ int redi[4];
    const int r = blockIdx.x, i = r / B, b = r - i * B, t = t0 + i;      // time-major rows
    const int64_t* trow = target + b * ld_t;
    const int tg = score_id(trow[t], V1);
    // every thread takes the same decision from the same (uniform) loads: no barrier sits under a divergent branch
    bool live = include_end || tg != 0;
    for (int u = 0; u < t && live; ++u) live = score_id(trow[u], V1) != 0;
    const long o = b * ld_out + t;
    if (!live) {                                                          // before the row is read
        if (threadIdx.x == 0) {
            tok_lp[o] = 0.f;
            if (tok_rank) tok_rank[o] = -1;
            if (tok_ent) tok_ent[o] = 0.f;
        }
        return;
    }
    const float* x = logits + r * ldl;
    f32x4 xr[LSM_R4];
    const float lse = log_softmax_row<VEC>(x, V1, xr, red);
    const float xt = x[tg];
    if (threadIdx.x == 0) tok_lp[o] = xt - lse;
    if (tok_rank) {                                                       // entries that a stable descending sort lists before tg
        int cnt = 0;
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j) {
                const int v = 4 * (threadIdx.x + 256 * j);               // a padding lane holds -inf at v >= V1 > tg: never before
#pragma unroll
                for (int e = 0; e < 4; ++e) cnt += row_before(xr[j][e], v + e, xt, tg) ? 1 : 0;
            }
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) cnt += row_before(x[v], v, xt, tg) ? 1 : 0;
        }
        cnt = block_count_256(cnt, redi);
        if (threadIdx.x == 0) tok_rank[o] = cnt;
    }
    if (tok_ent) {
        float s = 0.f;
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) s += score_ent_term(xr[j][e], lse);
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) s += score_ent_term(x[v], lse);
        }
        s = block_sum_256(s, red);
        if (threadIdx.x == 0) tok_ent[o] = s;
    }
}
extern "C" int rfn_score_logits(const float* logits, int64_t ldl, int B, int T, int t0, int V1, const int64_t* target,
                                int64_t ld_target, int include_end, float* tok_lp, int32_t* tok_rank, float* tok_ent,
                                int64_t ld_out, void* stream) {
    if (B <= 0 || T <= 0 || V1 <= 0 || t0 < 0 || ldl < V1 || ld_out < (int64_t)t0 + T || (int64_t)B * T > 0x7fffffffLL)
        return RFN_ERR_SHAPE;
    if (!logits || !target || !tok_lp) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0))
        hipLaunchKernelGGL(score_logits_k<true>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, t0, V1, target,
                           (long)ld_target, include_end, tok_lp, tok_rank, tok_ent, (long)ld_out);
    else
        hipLaunchKernelGGL(score_logits_k<false>, dim3(B * T), dim3(256), 0, st, logits, (long)ldl, B, t0, V1, target,
                           (long)ld_target, include_end, tok_lp, tok_rank, tok_ent, (long)ld_out);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- per caption: the fp64 sum of the live positions' log-probs, ascending, and their count -------------------------------
// One thread per caption; every step is one IEEE fp64 add of a converted float (nothing to contract), so a host loop over the
// same floats reproduces the sum exactly.
__global__ __launch_bounds__(256) void score_captions_k(const float* __restrict__ tok_lp, long ld_lp,
                                                        const int64_t* __restrict__ target, long ld_t, int B, int T, int V1,
                                                        int include_end, double* __restrict__ cap_lp, int* __restrict__ cap_len) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    int len = 0;
    for (int t = 0; t < T; ++t) {
        const int id = score_id(target[b * ld_t + t], V1);
        if (include_end || id != 0) {
            s += (double)tok_lp[b * ld_lp + t];
            ++len;
        }
        if (id == 0) break;                                               // nothing behind the first 0 is live
    }
    cap_lp[b] = s;
    if (cap_len) cap_len[b] = len;
}
extern "C" int rfn_score_captions(const float* tok_lp, int64_t ld_lp, const int64_t* target, int64_t ld_target, int B, int T,
                                  int V1, int include_end, double* cap_lp, int32_t* cap_len, void* stream) {
    if (B <= 0 || T <= 0 || V1 <= 0 || ld_lp < T) return RFN_ERR_SHAPE;
    if (!tok_lp || !target || !cap_lp) return RFN_ERR_ARG;
    hipLaunchKernelGGL(score_captions_k, dim3(rfn_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, tok_lp, (long)ld_lp, target,
                       (long)ld_target, B, T, V1, include_end, cap_lp, cap_len);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
