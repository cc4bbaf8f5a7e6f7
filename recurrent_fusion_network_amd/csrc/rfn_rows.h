// Device helpers of the kernels that give one block of 256 threads to a row of the vocabulary (rfn_logsoftmax.hip,
// rfn_criteria.hip, rfn_beam.hip, rfn_sbs.hip, rfn_score.hip): the block reductions, the row's log-sum-exp, the (value, token)
// order of a descending sort, a lane's sorted top-W list (fp32 or fp64 values), the row's block list as an LDS bitmap, and the
// host side of the two top-W row kernels (argument checks, launch ladder).  Reductions run in a fixed order (wave shuffles,
// then four LDS slots): no float atomics, results are bitwise reproducible.  A helper that one file uses stays in that file.
#pragma once
#include <type_traits>
#include "rfn_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float block_sum_256(float v, float* red /* [4] LDS */) {
    v = rfn_wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max_256(float v, float* red) {
    v = rfn_wave_max(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- the log-sum-exp of a row ----------------------------------------------------------------------
// Rows of up to 256 x 4 x LSM_R4 = 10240 logits (16-B aligned, V1 % 4 == 0: lsm_vec_ok) are read ONCE, 16 B per lane, and stay
// in `xr` for the caller's later passes; other rows take the scalar form (`xr` untouched).  Every kernel that needs a row's
// log-probs takes the log-sum-exp from here, so all of them produce the same log-prob bits for a row.
#define LSM_R4 10
template <bool VEC>
__device__ __forceinline__ float log_softmax_row(const float* __restrict__ x, int V1, f32x4 (&xr)[LSM_R4], float* red) {
    float m = -INFINITY, s = 0.f;
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) {
            const int i = threadIdx.x + 256 * j;
            xr[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (i < n4) xr[j] = *reinterpret_cast<const f32x4*>(x + 4 * i);
        }
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j) m = fmaxf(m, fmaxf(fmaxf(xr[j][0], xr[j][1]), fmaxf(xr[j][2], xr[j][3])));
        m = block_max_256(m, red);
#pragma unroll
        for (int j = 0; j < LSM_R4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) s += expf(xr[j][e] - m);      // exp(-inf) = 0 for the padding lanes
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) m = fmaxf(m, x[v]);
        m = block_max_256(m, red);
        for (int v = threadIdx.x; v < V1; v += 256) s += expf(x[v] - m);
    }
    s = block_sum_256(s, red);
    return m + logf(s);
}
static bool lsm_vec_ok(const float* logits, int64_t ldl, int V1, const float* out, int64_t s_inner, int64_t s_outer) {
    return V1 % 4 == 0 && V1 <= 256 * 4 * LSM_R4 && ldl % 4 == 0 && rfn_aligned16(logits) &&
           (!out || (rfn_aligned16(out) && s_inner % 4 == 0 && s_outer % 4 == 0));
}

// ---- (value descending, token ascending): the order in which a stable descending sort lists a row ---------------
// (fp64: the keys of the stochastic search, rfn_sbs.hip)
__device__ __forceinline__ bool row_before(float x, int i, float y, int j) { return x > y || (x == y && i < j); }
__device__ __forceinline__ bool row_before(double x, int i, double y, int j) { return x > y || (x == y && i < j); }

// ---- a lane's top-LW entries of its share of a row, sorted by row_before, in registers ---------------------------------
// Every loop over the list is fully unrolled with compile-time indices: anything else puts it in scratch memory.
template <int LW, class T = float>
struct RowTopList {
    T v[LW];
    int i[LW];
    __device__ __forceinline__ void fill() {          // empty slots: (-inf, 0x7fffffff), behind every real entry
#pragma unroll
        for (int j = 0; j < LW; ++j) {
            v[j] = -INFINITY;
            i[j] = 0x7fffffff;
        }
    }
    // Sorted insert by compare-exchange down the list.  A lane offers ascending tokens, so a later equal value stays behind
    // the earlier one, and a NaN never enters.
    __device__ __forceinline__ void offer(T x, int tok) {
        if (row_before(x, tok, v[LW - 1], i[LW - 1])) {
#pragma unroll
            for (int j = 0; j < LW; ++j) {
                const bool fwd = row_before(x, tok, v[j], i[j]);
                const T ov = v[j];
                const int oi = i[j];
                v[j] = fwd ? x : ov;
                i[j] = fwd ? tok : oi;
                x = fwd ? ov : x;
                tok = fwd ? oi : tok;
            }
        }
    }
    // Wave merge, one step: the best head of the 64 lanes' lists, to every lane; the lane that owned it pops it.
    __device__ __forceinline__ void wave_pop(T& best, int& bi) {
        best = v[0];
        bi = i[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const T ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (row_before(ob, oi, best, bi)) {
                best = ob;
                bi = oi;
            }
        }
        if (i[0] == bi && bi != 0x7fffffff) {
#pragma unroll
            for (int j = 0; j + 1 < LW; ++j) {
                v[j] = v[j + 1];
                i[j] = i[j + 1];
            }
            v[LW - 1] = -INFINITY;
            i[LW - 1] = 0x7fffffff;
        }
    }
};

// ---- a row's block list as one bit per token in LDS ------------------------------------------------------------------
// bits: (V1 + 31) / 32 words; blk[r, :blk_n[r]] may repeat ids, and ids outside [0, V1) are skipped.  All 256 threads call
// row_mask_build (two barriers); after it row_mask_has(bits, v) says whether token v is blocked.
__device__ __forceinline__ void row_mask_build(unsigned* bits, int V1, const int* __restrict__ blk, long ld_blk,
                                               const int* __restrict__ blk_n, int r) {
    for (int i = threadIdx.x; i < (V1 + 31) / 32; i += 256) bits[i] = 0u;
    __syncthreads();
    const int nb = blk_n[r];
    for (int i = threadIdx.x; i < nb; i += 256) {
        const int id = blk[r * ld_blk + i];
        if (id >= 0 && id < V1) atomicOr(&bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
}
__device__ __forceinline__ bool row_mask_has(const unsigned* bits, int v) { return (bits[v >> 5] >> (v & 31)) & 1u; }

// ---- the launchers of the top-W row kernels (rfn_logsoftmax.hip, rfn_sbs.hip) ----------------------------------------------
#define LSM_TOPW 32       /* entries a row hands over (= beams per image, rfn_beam_step.h) */
// The arguments both kernels share, in the order their entry points refuse them; ptrs_ok: logits and every output are there.
// *bits: the dynamic LDS of the row mask (0 without block lists).
static inline int lsm_topk_check(int rows, int V1, int W, bool ptrs_ok, const int32_t* blk, int64_t ld_blk, const int32_t* blk_n,
                                 size_t* bits) {
    if (rows <= 0 || V1 <= 0 || W < 1 || W > LSM_TOPW) return RFN_ERR_SHAPE;
    if (!ptrs_ok) return RFN_ERR_ARG;
    if (blk && (!blk_n || ld_blk < 1)) return RFN_ERR_ARG;
    *bits = blk ? (size_t)((V1 + 31) / 32) * sizeof(unsigned) : 0;
    if (*bits > 48 * 1024) return RFN_ERR_SHAPE;     // one bit per token in LDS
    return RFN_OK;
}
// launch(VEC, LW, MASK) with the kernels' template arguments as std::bool_constant / std::integral_constant tags: the list
// length is the smallest of 4, 8, 16, 32 that holds W.
template <class F>
static inline void lsm_topk_dispatch(bool vec, int W, bool mask, F&& launch) {
    auto by_w = [&](auto vec_c, auto mask_c) {
        if (W <= 4) launch(vec_c, std::integral_constant<int, 4>{}, mask_c);
        else if (W <= 8) launch(vec_c, std::integral_constant<int, 8>{}, mask_c);
        else if (W <= 16) launch(vec_c, std::integral_constant<int, 16>{}, mask_c);
        else launch(vec_c, std::integral_constant<int, 32>{}, mask_c);
    };
    if (vec && mask) by_w(std::true_type{}, std::true_type{});
    else if (vec) by_w(std::true_type{}, std::false_type{});
    else if (mask) by_w(std::false_type{}, std::true_type{});
    else by_w(std::false_type{}, std::false_type{});
}
