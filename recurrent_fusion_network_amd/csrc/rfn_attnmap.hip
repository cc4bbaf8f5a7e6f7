// Attention maps (rfn.h "attention maps"): the three levels of attention weights that the forward kernels already write --
// stage I over an encoder's regions, stage II over its thought vectors, the decoder over the fused thought vectors -- composed
// into one word-to-region map per (caption row, encoder), the per-(row, step) statistics of such a map, and the decoder
// weights copied out caption-major.  Nothing here is on a training path.
//
// rfn_attn_rollout: one wave per (caption row, column tile).  The row's decoder weights (S x T2) and its image's stage-II
// weights (T2 x T1) are staged in LDS, the stage-I rows a1[t1, k, tile] are streamed ONCE (16 B per lane where the map
// qualifies) into the T2 inner sums C[t2, l] = sum_t1 a2[t2, t1] * a1[t1, l], which live in LDS, each lane owning its columns
// (no barrier between the phases); then every live step takes sum_t2 aD[s, t2] * C[t2, l].  Both sums run ascending from 0.f
// in the nesting of the header's formula -- the (S x T2) . (T2 x T1) product of the two staged matrices is never formed, that
// would be the other association; no atomics.
#include "rfn_common.h"

typedef float am_f4 __attribute__((ext_vector_type(4)));

static inline size_t am_pad4(size_t n) { return (n + 3) & ~(size_t)3; }
__device__ __forceinline__ int am_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct AmRollout {
    const float *aD, *a2, *a1;
    long d_ss, d_sr, a2_st, a2_sb, a1_st, a1_sb;
    const int32_t *len, *att_len;
    int n, S, T1, T2, L;
    float* out;
    long o_sr, o_ss;
};

// W columns per lane: 4 (16-B loads and stores; L % 4 == 0, 16-B aligned bases, strides % 4 == 0) or 1
template <int W>
__global__ __launch_bounds__(64) void attn_rollout_k(const AmRollout a) {
    extern __shared__ __attribute__((aligned(16))) float am_lds[];
    const int lane = threadIdx.x, r = blockIdx.x, k = r / a.n;
    const int S = a.S, T1 = a.T1, T2 = a.T2, L = a.L;
    const int l0 = (blockIdx.y * 64 + lane) * W;
    float* sD = am_lds;                                   // (live, T2) the row's decoder weights
    float* s2 = sD + (((size_t)S * T2 + 3) & ~(size_t)3);  // (T2, T1) the image's stage-II weights of this encoder
    float* sC = s2 + (((size_t)T2 * T1 + 3) & ~(size_t)3); // (T2, 64, W) the inner sums, lane-major
    const int live = a.len ? am_clamp(a.len[r], 0, S) : S;
    const int alen = a.att_len ? am_clamp(a.att_len[k], 1, L) : L;
    const int nv = am_clamp(alen - l0, 0, W);             // this lane's columns inside the image's map
    float* orow = a.out + r * a.o_sr + l0;
    if (live > 0) {                                       // a dead row loads nothing (the decision is uniform over the wave)
        for (int i = lane; i < live * T2; i += 64) sD[i] = a.aD[(i / T2) * a.d_ss + r * a.d_sr + (i % T2)];
        for (int i = lane; i < T2 * T1; i += 64) s2[i] = a.a2[(i / T1) * a.a2_st + k * a.a2_sb + (i % T1)];
        for (int t2 = 0; t2 < T2; ++t2)
#pragma unroll
            for (int e = 0; e < W; ++e) sC[(t2 * 64 + lane) * W + e] = 0.f;
        __syncthreads();
        if (nv > 0) {
            const float* col = a.a1 + k * a.a1_sb + l0;
            for (int t1 = 0; t1 < T1; ++t1) {
                float v[W];
                if (W == 4 && nv == 4) {
                    const am_f4 q = *reinterpret_cast<const am_f4*>(col + t1 * a.a1_st);
#pragma unroll
                    for (int e = 0; e < W; ++e) v[e] = q[e];
                } else {                                  // the quad that straddles the image's length, or the scalar form
#pragma unroll
                    for (int e = 0; e < W; ++e) v[e] = e < nv ? col[t1 * a.a1_st + e] : 0.f;
                }
                for (int t2 = 0; t2 < T2; ++t2) {
                    const float c2 = s2[t2 * T1 + t1];
                    float* c = sC + (t2 * 64 + lane) * W;
#pragma unroll
                    for (int e = 0; e < W; ++e) c[e] += c2 * v[e];
                }
            }
        }
    }
    if (l0 >= L) return;
    for (int s = 0; s < S; ++s) {
        float acc[W];
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] = 0.f;
        if (s < live && nv > 0) {
            for (int t2 = 0; t2 < T2; ++t2) {
                const float d = sD[s * T2 + t2];
                const float* c = sC + (t2 * 64 + lane) * W;
#pragma unroll
                for (int e = 0; e < W; ++e) acc[e] += d * c[e];
            }
#pragma unroll
            for (int e = 0; e < W; ++e)
                if (e >= nv) acc[e] = 0.f;                // past the image's length: exact zeros whatever the weights hold
        }
        if (W == 4) {
            am_f4 q;
#pragma unroll
            for (int e = 0; e < W; ++e) q[e] = acc[e];
            *reinterpret_cast<am_f4*>(orow + s * a.o_ss) = q;
        } else {
            orow[s * a.o_ss] = acc[0];
        }
    }
}

extern "C" int rfn_attn_rollout(const float* aD, int64_t d_ss, int64_t d_sr, const float* a2, int64_t a2_st, int64_t a2_sb,
                                const float* a1, int64_t a1_st, int64_t a1_sb, const int32_t* len, const int32_t* att_len, int rows,
                                int n, int S, int T1, int T2, int L, float* out, int64_t o_sr, int64_t o_ss, void* stream) {
    if (rows < 1 || n < 1 || S < 1 || T1 < 1 || T2 < 1 || L < 1 || rows % n != 0) return RFN_ERR_SHAPE;
    if (o_sr < L || o_ss < L || d_sr < T2 || a2_sb < T1 || a1_sb < L || a1_st < L) return RFN_ERR_SHAPE;
    if (!aD || !a2 || !a1 || !out) return RFN_ERR_ARG;
    const size_t lds1 = (am_pad4((size_t)S * T2) + am_pad4((size_t)T2 * T1) + (size_t)T2 * 64) * sizeof(float);
    const size_t lds4 = lds1 + (size_t)T2 * 64 * 3 * sizeof(float);
    // the 16-byte form where the map qualifies and its 256-column tile fits; the 64-column tile otherwise
    const bool vec = L % 4 == 0 && rfn_aligned16(a1) && rfn_aligned16(out) && a1_st % 4 == 0 && a1_sb % 4 == 0 && o_sr % 4 == 0 &&
                     o_ss % 4 == 0 && lds4 <= 65536;
    const int W = vec ? 4 : 1;
    const size_t lds = vec ? lds4 : lds1;
    const long tiles = ((long)L + 64 * W - 1) / (64 * W);
    if (lds > 65536 || tiles > 65535) return RFN_ERR_UNSUPPORTED;
    const AmRollout a{aD, a2, a1, (long)d_ss, (long)d_sr, (long)a2_st, (long)a2_sb, (long)a1_st, (long)a1_sb, len, att_len,
                      n, S, T1, T2, L, out, (long)o_sr, (long)o_ss};
    const dim3 grid((unsigned)rows, (unsigned)tiles);
    if (vec)
        hipLaunchKernelGGL(attn_rollout_k<4>, grid, dim3(64), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(attn_rollout_k<1>, grid, dim3(64), lds, (hipStream_t)stream, a);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- per (row, step): first argmax, entropy, mass inside a region mask ------------------------------------------------------
// One wave per (row, step), four to a block; a dead step's wave returns before it reads its map row.  Lane-strided partial
// results, then xor shuffles: a fixed order.
__global__ __launch_bounds__(256) void attn_map_stats_k(const float* __restrict__ G, long g_sr, long g_ss,
                                                        const int32_t* __restrict__ len, const uint8_t* __restrict__ mask, long m_sr,
                                                        long m_ss, long pairs, int S, int L, int32_t* __restrict__ peak,
                                                        float* __restrict__ entropy, float* __restrict__ mass) {
    const int lane = threadIdx.x & 63;
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= pairs) return;
    const long r = pair / S;
    const int s = (int)(pair - r * S);
    const int live = len ? am_clamp(len[r], 0, S) : S;
    if (s >= live) {
        if (lane == 0) {
            peak[pair] = -1;
            entropy[pair] = 0.f;
            if (mask) mass[pair] = 0.f;
        }
        return;
    }
    const float* g = G + r * g_sr + s * g_ss;
    const uint8_t* m = mask ? mask + r * m_sr + s * m_ss : nullptr;
    float bv = -INFINITY, ent = 0.f, ms = 0.f;
    int bi = 0x7fffffff;
    for (int l = lane; l < L; l += 64) {
        const float v = g[l];
        if (v > bv) {
            bv = v;
            bi = l;
        }
        if (v > 0.f) ent -= v * logf(v);                  // 0 log 0 = 0
        if (m && m[l]) ms += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
    ent = rfn_wave_sum(ent);
    ms = rfn_wave_sum(ms);
    if (lane == 0) {
        peak[pair] = bi == 0x7fffffff ? 0 : bi;
        entropy[pair] = ent;
        if (mask) mass[pair] = ms;
    }
}

extern "C" int rfn_attn_map_stats(const float* G, int64_t g_sr, int64_t g_ss, const int32_t* len, const uint8_t* region_mask,
                                  int64_t m_sr, int64_t m_ss, int rows, int S, int L, int32_t* peak, float* entropy, float* mass,
                                  void* stream) {
    if (rows < 1 || S < 1 || L < 1 || g_sr < L || g_ss < L || (region_mask && (m_sr < L || m_ss < L))) return RFN_ERR_SHAPE;
    if (!G || !peak || !entropy || (region_mask && !mass)) return RFN_ERR_ARG;
    const long pairs = (long)rows * S;
    if ((pairs + 3) / 4 > 0x7fffffffL) return RFN_ERR_SHAPE;
    hipLaunchKernelGGL(attn_map_stats_k, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, G, (long)g_sr,
                       (long)g_ss, len, region_mask, (long)m_sr, (long)m_ss, pairs, S, L, peak, entropy, mass);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- the decoder's weights, time-major (S, rows, T2) -> caption-major (rows, S, T2), dead steps zeroed and not loaded ----------
__global__ __launch_bounds__(256) void attn_decoder_copy_k(const float* __restrict__ aD, long d_ss, long d_sr,
                                                           const int32_t* __restrict__ len, long total, int S, int T2,
                                                           float* __restrict__ out, long o_sr, long o_ss) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t2 = (int)(i % T2);
    const long rs = i / T2, r = rs / S;
    const int s = (int)(rs - r * S);
    const int live = len ? am_clamp(len[r], 0, S) : S;
    out[r * o_sr + s * o_ss + t2] = s < live ? aD[s * d_ss + r * d_sr + t2] : 0.f;
}

extern "C" int rfn_attn_decoder_copy(const float* aD, int64_t d_ss, int64_t d_sr, const int32_t* len, int rows, int S, int T2,
                                     float* out, int64_t o_sr, int64_t o_ss, void* stream) {
    if (rows < 1 || S < 1 || T2 < 1 || d_sr < T2 || o_ss < T2 || o_sr < T2) return RFN_ERR_SHAPE;
    if (!aD || !out) return RFN_ERR_ARG;
    const long total = (long)rows * S * T2;
    if ((total + 255) / 256 > 0x7fffffffL) return RFN_ERR_SHAPE;
    hipLaunchKernelGGL(attn_decoder_copy_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, aD, (long)d_ss,
                       (long)d_sr, len, total, S, T2, out, (long)o_sr, (long)o_ss);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
