// Log-softmax over the vocabulary: forward, backward, and the top-W form (plain and masked) that hands the beam search a
// row's W best log-probs without materialising the row.  One block of 256 per row (rfn_rows.h); rows that qualify are read
// once, 16 B per lane, and held in registers.
#include <type_traits>
#include "rfn_rows.h"

// ---- log-softmax over the vocabulary --------------------------------------------------------------
// One block per row; log_softmax_row() (rfn_rows.h) keeps a vectorisable row in registers for the max, the sum and the output
// pass, other rows take the three-pass scalar form.
template <bool VEC>
__global__ __launch_bounds__(256) void log_softmax_fwd_k(const float* __restrict__ logits, long ldl, int V1,
                                                         int inner, long s_inner, long s_outer,
                                                         float* __restrict__ out) {
    __shared__ float red[4];
    const int r = blockIdx.x;
    const float* x = logits + r * ldl;
    float* o = out + (long)(r % inner) * s_inner + (long)(r / inner) * s_outer;
    f32x4 xr[LSM_R4];
    const float lse = log_softmax_row<VEC>(x, V1, xr, red);
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < n4) *reinterpret_cast<f32x4*>(o + 4 * i) = xr[j] - lse;
        }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) o[v] = x[v] - lse;
    }
}
extern "C" int rfn_log_softmax_fwd(const float* logits, int64_t ldl, int rows, int V1, int inner,
                                   int64_t out_s_inner, int64_t out_s_outer, float* out, void* stream) {
    if (rows <= 0 || V1 <= 0 || inner <= 0) return RFN_ERR_SHAPE;
    if (!logits || !out) return RFN_ERR_ARG;
    if (lsm_vec_ok(logits, ldl, V1, out, out_s_inner, out_s_outer))
        hipLaunchKernelGGL(log_softmax_fwd_k<true>, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ldl, V1,
                           inner, (long)out_s_inner, (long)out_s_outer, out);
    else
        hipLaunchKernelGGL(log_softmax_fwd_k<false>, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ldl, V1,
                           inner, (long)out_s_inner, (long)out_s_outer, out);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- log-softmax + top-W of every row, without materialising the log-probs (beam search) ---------------------------------
// sample_beam only ever looks at the W best log-probs of a beam row (misc/RecurrentFusionModel.py:463-466: a full sort, of
// which columns 0 .. beam_size-1 are read).  topv[r, c] / topi[r, c], c < W: the c-th largest log-prob of row r and its
// token, ordered (value descending, token ascending) -- the order the reference's descending sort lists them -- computed
// from the same log-prob bits rfn_log_softmax_fwd writes.  W <= LSM_TOPW (rfn_rows.h).
// MASK (rfn_log_softmax_topk_masked): the row's block list (blk[r, :blk_n[r]], duplicates allowed) becomes a bit per token in
// LDS; the log-sum-exp above it is still taken over ALL logits, and a blocked token then enters the selection as -inf, so the
// list is the one a stable descending sort of the masked log-prob row gives (short rows are filled with the lowest -inf ids).
// WANT (rfn_log_softmax_topk_want, rfn.h "lexically constrained beam search"): one more output, the log-probs of the NW tokens
// want[r / row_div, :] as the selection sees them (-inf when blocked or when the id is the -1 padding).  A register-resident row
// cannot be indexed by a run-time token without spilling, so both forms read the NW logits again: they lie in cache lines this
// block has just read, and x[v] - lse is the operation every other entry gets.
struct LsmWant {
    const int* want;
    long ld_want;
    int NW, row_div;
    float* wantv;
};
struct LsmNoWant {};
template <bool VEC, int LW, bool MASK, bool WANT = false>
__global__ __launch_bounds__(256) void log_softmax_topk_k(const float* __restrict__ logits, long ldl, int V1, int W,
                                                          float* __restrict__ topv, int* __restrict__ topi,
                                                          const int* __restrict__ blk, long ld_blk,
                                                          const int* __restrict__ blk_n,
                                                          std::conditional_t<WANT, LsmWant, LsmNoWant> wt = {}) {
    __shared__ float red[4];
    __shared__ float wv[4][LSM_TOPW];
    __shared__ int wi[4][LSM_TOPW];
    extern __shared__ unsigned lsm_bits[];       // MASK: (V1 + 31) / 32 words
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* x = logits + r * ldl;
    f32x4 xr[LSM_R4];
    const float lse = log_softmax_row<VEC>(x, V1, xr, red);
    const int cols = min(W, V1);
    if constexpr (MASK) {
        row_mask_build(lsm_bits, V1, blk, ld_blk, blk_n, r);
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < LSM_R4; ++j) {
                const int i = threadIdx.x + 256 * j;
                if (i < (V1 >> 2)) {
                    const unsigned b4 = lsm_bits[i >> 3] >> ((4 * i) & 31);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((b4 >> e) & 1u) xr[j][e] = -INFINITY;
                }
            }
        }
    }
    if constexpr (WANT) {
        if ((int)threadIdx.x < wt.NW) {
            const int id = wt.want[(long)(r / wt.row_div) * wt.ld_want + threadIdx.x];
            float lp = -INFINITY;
            if (id >= 0 && id < V1) {
                bool blocked = false;
                if constexpr (MASK) blocked = row_mask_has(lsm_bits, id);
                if (!blocked) lp = x[id] - lse;
            }
            wt.wantv[(long)r * wt.NW + threadIdx.x] = lp;
        }
    }
    // the logit of token v as the selection sees it (the non-VEC form re-reads the row)
    auto xat = [&](int v) {
        if constexpr (MASK) {
            if (row_mask_has(lsm_bits, v)) return -INFINITY;
        }
        return x[v];
    };
    // Threshold first: the `cols`-th largest of the 256 threads' LOCAL maxima is a lower bound of the row's `cols`-th largest
    // log-prob (those maxima are distinct elements of the row), so only entries >= it can make the list -- a handful per
    // row instead of every entry going through a sorted insert.
    float lm = -INFINITY;
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) lm = fmaxf(lm, fmaxf(fmaxf(xr[j][0], xr[j][1]), fmaxf(xr[j][2], xr[j][3])));
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) lm = fmaxf(lm, xat(v));
    }
    lm -= lse;      // x - lse is monotone in x: the maximum of the log-probs is the log-prob of the maximum
    {
        float mine = lm;
        for (int c = 0; c < cols; ++c) {         // wave: pop the largest local maximum `cols` times
            float best = mine;
            int bl_ = lane;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o, 64);
                const int ol = __shfl_xor(bl_, o, 64);
                if (ob > best || (ob == best && ol < bl_)) {
                    best = ob;
                    bl_ = ol;
                }
            }
            if (lane == bl_) mine = -INFINITY;
            if (lane == 0) wv[wave][c] = best;
        }
    }
    __syncthreads();
    float thr;
    {
        int pos[4] = {0, 0, 0, 0};
        thr = -INFINITY;
        for (int c = 0; c < cols; ++c) {         // every thread merges the four sorted lists redundantly (cols <= 32)
            int bp = 0;
            float bv = -INFINITY;
            for (int p = 0; p < 4; ++p)
                if (pos[p] < cols && wv[p][pos[p]] > bv) {
                    bv = wv[p][pos[p]];
                    bp = p;
                }
            thr = bv;
            ++pos[bp];
        }
    }
    __syncthreads();                             // wv is reused by the merge below
    RowTopList<LW> top;
    top.fill();
    auto offer = [&](float lp, int v) {      // the threshold first, then the sorted insert (ascending v per thread)
        if (lp >= thr) top.offer(lp, v);
    };
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < n4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) offer(xr[j][e] - lse, 4 * i + e);
            }
        }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) offer(xat(v) - lse, v);
    }
    for (int c = 0; c < cols; ++c) {             // wave merge: pop the best head `cols` times
        float best;
        int bi;
        top.wave_pop(best, bi);
        if (lane == 0) {
            wv[wave][c] = best;
            wi[wave][c] = bi;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                      // merge the four waves' sorted lists
        int pos[4] = {0, 0, 0, 0};
        for (int c = 0; c < cols; ++c) {
            int bp = -1;
            for (int p = 0; p < 4; ++p) {
                if (pos[p] >= cols || wi[p][pos[p]] == 0x7fffffff) continue;
                if (bp < 0 || row_before(wv[p][pos[p]], wi[p][pos[p]], wv[bp][pos[bp]], wi[bp][pos[bp]])) bp = p;
            }
            if (bp < 0) {                        // a row with fewer than `cols` comparable entries (NaN logits): no
                topv[(long)r * W + c] = -INFINITY;   // candidate is left -- never index the lists with -1; the slot
                topi[(long)r * W + c] = 0;           // reads as "token 0 at -inf", which the beam step can never pick
                continue;                            // over a real candidate
            }
            topv[(long)r * W + c] = wv[bp][pos[bp]];
            topi[(long)r * W + c] = wi[bp][pos[bp]];
            ++pos[bp];
        }
    }
}
static int log_softmax_topk_launch(const float* logits, int64_t ldl, int rows, int V1, int W, const int32_t* blk, int64_t ld_blk,
                                   const int32_t* blk_n, float* topv, int32_t* topi, void* stream,
                                   const int32_t* want = nullptr, int64_t ld_want = 0, int NW = 0, int row_div = 1,
                                   float* wantv = nullptr) {
    size_t bits;
    RFN_TRY(lsm_topk_check(rows, V1, W, logits && topv && topi, blk, ld_blk, blk_n, &bits));
    hipStream_t st = (hipStream_t)stream;
    lsm_topk_dispatch(lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0), W, blk != nullptr, [&](auto vec, auto lw, auto mask) {
        constexpr bool VEC = decltype(vec)::value, MASK = decltype(mask)::value;
        constexpr int LW = decltype(lw)::value;
        if (want)
            hipLaunchKernelGGL((log_softmax_topk_k<VEC, LW, MASK, true>), dim3(rows), dim3(256), bits, st, logits, (long)ldl, V1, W,
                               topv, topi, blk, (long)ld_blk, blk_n, LsmWant{want, (long)ld_want, NW, row_div, wantv});
        else
            hipLaunchKernelGGL((log_softmax_topk_k<VEC, LW, MASK>), dim3(rows), dim3(256), bits, st, logits, (long)ldl, V1, W, topv,
                               topi, blk, (long)ld_blk, blk_n, LsmNoWant{});
    });
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_log_softmax_topk(const float* logits, int64_t ldl, int rows, int V1, int W, float* topv, int32_t* topi,
                                    void* stream) {
    return log_softmax_topk_launch(logits, ldl, rows, V1, W, nullptr, 0, nullptr, topv, topi, stream);
}
extern "C" int rfn_log_softmax_topk_masked(const float* logits, int64_t ldl, int rows, int V1, int W, const int32_t* blk,
                                           int64_t ld_blk, const int32_t* blk_n, float* topv, int32_t* topi, void* stream) {
    return log_softmax_topk_launch(logits, ldl, rows, V1, W, blk, ld_blk, blk_n, topv, topi, stream);
}

extern "C" int rfn_log_softmax_topk_want(const float* logits, int64_t ldl, int rows, int V1, int W, int row_div, const int32_t* want,
                                         int64_t ld_want, int NW, const int32_t* blk, int64_t ld_blk, const int32_t* blk_n,
                                         float* topv, int32_t* topi, float* wantv, void* stream) {
    if (!want) return log_softmax_topk_launch(logits, ldl, rows, V1, W, blk, ld_blk, blk_n, topv, topi, stream);
    if (NW < 1 || NW > RFN_LEX_MAX_IDS || ld_want < NW || row_div < 1) return RFN_ERR_SHAPE;
    if (!wantv) return RFN_ERR_ARG;
    return log_softmax_topk_launch(logits, ldl, rows, V1, W, blk, ld_blk, blk_n, topv, topi, stream, want, ld_want, NW, row_div,
                                   wantv);
}

// d logits = g - softmax * sum(g), one block per row.  VEC: rows of up to 10240 logits (16-B aligned, V1 % 4 == 0) keep g in
// registers between the sum and the update: one read of g and of the log-probs, one write, 16 B per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void log_softmax_bwd_k(const float* __restrict__ g, const float* __restrict__ logp,
                                                         int V1, int inner, long s_inner, long s_outer,
                                                         float* __restrict__ dlogits, long ldd) {
    __shared__ float red[4];
    const int r = blockIdx.x;
    const long off = (long)(r % inner) * s_inner + (long)(r / inner) * s_outer;
    const float* gr = g + off;
    const float* lp = logp + off;
    float* d = dlogits + r * ldd;
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
        f32x4 gv[LSM_R4], lv[LSM_R4];
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) {
            const int i = threadIdx.x + 256 * j;
            gv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            lv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < n4) {
                gv[j] = *reinterpret_cast<const f32x4*>(gr + 4 * i);
                lv[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(lp + 4 * i));
            }
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) s += (gv[j][0] + gv[j][1]) + (gv[j][2] + gv[j][3]);
        s = block_sum_256(s, red);
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < n4) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = gv[j][e] - expf(lv[j][e]) * s;
                *reinterpret_cast<f32x4*>(d + 4 * i) = o;
            }
        }
    } else {
        float s = 0.f;
        for (int v = threadIdx.x; v < V1; v += 256) s += gr[v];
        s = block_sum_256(s, red);
        for (int v = threadIdx.x; v < V1; v += 256) d[v] = gr[v] - expf(lp[v]) * s;
    }
}
extern "C" int rfn_log_softmax_bwd(const float* g, const float* logp, int rows, int V1, int inner, int64_t s_inner,
                                   int64_t s_outer, float* dlogits, int64_t ldd, void* stream) {
    if (rows <= 0 || V1 <= 0 || inner <= 0) return RFN_ERR_SHAPE;
    if (!g || !logp || !dlogits) return RFN_ERR_ARG;
    const bool vec = V1 % 4 == 0 && V1 <= 256 * 4 * LSM_R4 && s_inner % 4 == 0 && s_outer % 4 == 0 && ldd % 4 == 0 &&
                     rfn_aligned16(g) && rfn_aligned16(logp) && rfn_aligned16(dlogits);
    if (vec)
        hipLaunchKernelGGL(log_softmax_bwd_k<true>, dim3(rows), dim3(256), 0, (hipStream_t)stream, g, logp, V1, inner,
                           (long)s_inner, (long)s_outer, dlogits, (long)ldd);
    else
        hipLaunchKernelGGL(log_softmax_bwd_k<false>, dim3(rows), dim3(256), 0, (hipStream_t)stream, g, logp, V1, inner,
                           (long)s_inner, (long)s_outer, dlogits, (long)ldd);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
