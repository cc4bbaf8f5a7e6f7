// Glue kernels of the train step, the small streaming kernels between the GEMMs: bias-gradient column sums, fill / copy of
// small buffers, embedding gather / deterministic scatter, the reason heads' max over steps, axpby / divide on strided 2-D
// views, and the mean over / broadcast to the encoder groups.
// All are HBM/L2-bound byte movers: coalesced accesses (16 B per lane where alignment allows), fixed summation orders (no
// float atomics) so results are bitwise reproducible.
#include <string.h>

#include "rfn_common.h"
#include "rfn_rows.h"

// ---- out[n] (+)= sum_r X[r, n] ----------------------------------------------------------------
// block = CW columns x (1024 / CW) row lanes, 4 independent row streams per thread; the lanes' partial sums are
// combined through LDS in a fixed order.  Narrow matrices (the (S*B, A) attention partials) take CW = 16 so that
// 4x more blocks share the rows; wide ones keep 256-B row segments per wave.
template <int CW>
__global__ __launch_bounds__(1024) void colsum_k(const float* __restrict__ X, long ldx, int rows, int cols,
                                                 float* __restrict__ out, int accumulate) {
    constexpr int RL = 1024 / CW;
    __shared__ float red[RL][CW];
    const int cl = threadIdx.x % CW, rl = threadIdx.x / CW;
    const int c = blockIdx.x * CW + cl;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (c < cols) {
        const float* p = X + c;
        int r = rl;
        for (; r + 3 * RL < rows; r += 4 * RL) {
            a0 += p[(long)r * ldx];
            a1 += p[(long)(r + RL) * ldx];
            a2 += p[(long)(r + 2 * RL) * ldx];
            a3 += p[(long)(r + 3 * RL) * ldx];
        }
        for (; r < rows; r += RL) a0 += p[(long)r * ldx];
    }
    red[rl][cl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (rl == 0 && c < cols) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < RL; ++k) s += red[k][cl];
        out[c] = accumulate ? out[c] + s : s;
    }
}
extern "C" int rfn_colsum_f32(const float* X, int64_t ldx, int rows, int cols, float* out, int accumulate,
                              void* stream) {
    if (rows < 0 || cols <= 0) return RFN_ERR_SHAPE;
    if (!X || !out) return RFN_ERR_ARG;
    if (cols >= 64 * 128)
        hipLaunchKernelGGL(colsum_k<64>, dim3(rfn_cdiv(cols, 64)), dim3(1024), 0, (hipStream_t)stream, X, (long)ldx,
                           rows, cols, out, accumulate);
    else
        hipLaunchKernelGGL(colsum_k<16>, dim3(rfn_cdiv(cols, 16)), dim3(1024), 0, (hipStream_t)stream, X, (long)ldx,
                           rows, cols, out, accumulate);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

struct ColsumOuts { float* out[64]; };
// 64 columns x 16 row-lanes per block: a thread sums every 16th row of its column, the 16 partial sums are added in a
// fixed order through LDS (deterministic).
#define CSG_LANES 16
struct ColsumOuts2 { float* out[64]; float* out2[64]; };
__global__ __launch_bounds__(64 * CSG_LANES) void colsum_grouped_k(const float* __restrict__ X, long gstride, long ldx,
                                                                  int rows, int cols, const ColsumOuts2 outs) {
    __shared__ float red[CSG_LANES][64];
    const float* Xg = X + blockIdx.y * gstride;
    const int l = threadIdx.x & 63, c = blockIdx.x * 64 + l, rl = threadIdx.x >> 6;
    float acc = 0.f;
    if (c < cols)
        for (int r = rl; r < rows; r += CSG_LANES) acc += Xg[r * ldx + c];
    red[rl][l] = acc;
    __syncthreads();
    if (rl == 0 && c < cols) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < CSG_LANES; ++k) t += red[k][l];
        outs.out[blockIdx.y][c] = t;
        if (outs.out2[blockIdx.y]) outs.out2[blockIdx.y][c] = t;
    }
}
extern "C" int rfn_colsum_grouped2_f32(const float* X, int64_t group_stride, int64_t ldx, int rows, int cols,
                                       float* const* outs, float* const* outs2, int ngroups, void* stream) {
    if (rows < 0 || cols <= 0 || ngroups < 1) return RFN_ERR_SHAPE;
    if (!X || !outs) return RFN_ERR_ARG;
    for (int g0 = 0; g0 < ngroups; g0 += 64) {
        ColsumOuts2 o;
        const int ng = ngroups - g0 < 64 ? ngroups - g0 : 64;
        for (int g = 0; g < ng; ++g) {
            if (!outs[g0 + g]) return RFN_ERR_ARG;
            o.out[g] = outs[g0 + g];
            o.out2[g] = outs2 ? outs2[g0 + g] : nullptr;
        }
        hipLaunchKernelGGL(colsum_grouped_k, dim3(rfn_cdiv(cols, 64), ng), dim3(64 * CSG_LANES), 0, (hipStream_t)stream,
                           X + (long)g0 * group_stride, (long)group_stride, (long)ldx, rows, cols, o);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}
extern "C" int rfn_colsum_grouped_f32(const float* X, int64_t group_stride, int64_t ldx, int rows, int cols,
                                      float* const* outs, int ngroups, void* stream) {
    return rfn_colsum_grouped2_f32(X, group_stride, ldx, rows, cols, outs, nullptr, ngroups, stream);
}

// out[g][0..n) = value for up to 64 small buffers per launch (the exactly-zero att_h_2_out.bias gradients)
__global__ __launch_bounds__(64) void fill_small_k(const ColsumOuts outs, int n, float value) {
    float* o = outs.out[blockIdx.x];
    for (int i = threadIdx.x; i < n; i += 64) o[i] = value;
}
extern "C" int rfn_fill_small_f32(float* const* outs, int ngroups, int n, float value, void* stream) {
    if (ngroups < 1 || n < 1) return RFN_ERR_SHAPE;
    if (!outs) return RFN_ERR_ARG;
    for (int g0 = 0; g0 < ngroups; g0 += 64) {
        ColsumOuts o;
        const int ng = ngroups - g0 < 64 ? ngroups - g0 : 64;
        for (int g = 0; g < ng; ++g) {
            if (!outs[g0 + g]) return RFN_ERR_ARG;
            o.out[g] = outs[g0 + g];
        }
        hipLaunchKernelGGL(fill_small_k, dim3(ng), dim3(64), 0, (hipStream_t)stream, o, n, value);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}

// dst[g][0..n) = src[g][0..n) for up to 64 small buffer pairs per launch (equal-by-construction bias gradients)
struct CopyPairs { float* dst[64]; const float* src[64]; };
__global__ __launch_bounds__(64) void copy_small_k(const CopyPairs p, int n) {
    float* o = p.dst[blockIdx.x];
    const float* s = p.src[blockIdx.x];
    for (int i = threadIdx.x; i < n; i += 64) o[i] = s[i];
}
extern "C" int rfn_copy_small_f32(float* const* dst, const float* const* src, int ngroups, int n, void* stream) {
    if (ngroups < 1 || n < 1) return RFN_ERR_SHAPE;
    if (!dst || !src) return RFN_ERR_ARG;
    for (int g0 = 0; g0 < ngroups; g0 += 64) {
        CopyPairs p;
        const int ng = ngroups - g0 < 64 ? ngroups - g0 : 64;
        for (int g = 0; g < ng; ++g) {
            if (!dst[g0 + g] || !src[g0 + g]) return RFN_ERR_ARG;
            p.dst[g] = dst[g0 + g];
            p.src[g] = src[g0 + g];
        }
        hipLaunchKernelGGL(copy_small_k, dim3(ng), dim3(64), 0, (hipStream_t)stream, p, n);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}

// ---- embedding ----------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void embed_fwd_k(const float* __restrict__ W, int E, long V1,
                                                   const int64_t* __restrict__ ids, int inner, long si, long so,
                                                   float* __restrict__ out, long ldo) {
    const int r = blockIdx.x;
    long id = ids[(long)(r % inner) * si + (long)(r / inner) * so];
    if (id < 0 || id >= V1) id = 0;  // the reference would raise; never fault the GPU
    for (int e = threadIdx.x; e < E; e += 128) out[r * ldo + e] = W[id * E + e];
}
extern "C" int rfn_embed_fwd(const float* W, int E, int64_t V1, const int64_t* ids, int inner, int64_t ids_s_inner,
                             int64_t ids_s_outer, int rows, float* out, int64_t ldo, void* stream) {
    if (rows <= 0 || E <= 0 || V1 <= 0 || inner <= 0) return RFN_ERR_SHAPE;
    if (!W || !ids || !out) return RFN_ERR_ARG;
    hipLaunchKernelGGL(embed_fwd_k, dim3(rows), dim3(128), 0, (hipStream_t)stream, W, E, (long)V1, ids, inner,
                       (long)ids_s_inner, (long)ids_s_outer, out, (long)ldo);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
// One wave per vocabulary row.  The token list is scanned 64 entries at a time: every lane tests one entry, a ballot gives
// the matches, the matching rows are queued in LDS in scan order, and the queue is drained EMB_DEPTH rows at a time -- their
// loads in flight together, added in queue order: deterministic, no float atomics.  A hot token (BOS feeds step 0 of every
// caption: B matches) used to be one serial chain of dependent loads, the long pole of the launch (147 us at B = 256).
// The scan walks the ids in MEMORY order when the rows form a whole (inner x rows/inner) rectangle (time-major rows
// r = t*B + b read ids[b][t]), otherwise in row order; either way the order is a function of the shape only.
#define EMB_UNROLL 4
#define EMB_CH 2      /* chunks of 64 x W floats per lane: E = 512 is covered by one wave */
#define EMB_QCAP 512  /* queued rows before a drain (>= 64 * EMB_UNROLL) */
#define EMB_DEPTH 8
template <bool VEC>
__global__ __launch_bounds__(64) void embed_bwd_k(const float* __restrict__ dout, long ldo,
                                                  const int64_t* __restrict__ ids, int inner, long si, long so,
                                                  int rows, int E, float* __restrict__ dW) {
    constexpr int W = VEC ? 4 : 1;
    typedef float vec_t __attribute__((ext_vector_type(W)));
    __shared__ int queue[EMB_QCAP];
    const long v = blockIdx.x;
    const int lane = threadIdx.x;
    // scan index q -> (hi, lo) = (q / mod, q % mod), carried along (q advances by 64: no division in the loop)
    const bool mem_order = rows % inner == 0;
    const int mod = mem_order ? rows / inner : inner;
    const long s_hi = mem_order ? si : so, s_lo = mem_order ? so : si;
    const int step_q = 64 / mod, step_r = 64 - step_q * mod;
    for (int e0 = 0; e0 < E; e0 += 64 * W * EMB_CH) {
        vec_t acc[EMB_CH];
#pragma unroll
        for (int c = 0; c < EMB_CH; ++c)
#pragma unroll
            for (int k = 0; k < W; ++k) acc[c][k] = 0.f;
        int nq = 0;                                   // queued rows (uniform)
        auto drain = [&]() {                          // adds queue[0 .. nq) in order
            __syncthreads();
            for (int i0 = 0; i0 < nq; i0 += EMB_DEPTH) {
                vec_t x[EMB_DEPTH][EMB_CH];
#pragma unroll
                for (int j = 0; j < EMB_DEPTH; ++j) {
                    const long rr = queue[i0 + j < nq ? i0 + j : nq - 1];
#pragma unroll
                    for (int c = 0; c < EMB_CH; ++c) {
                        const int e = e0 + (c * 64 + lane) * W;
#pragma unroll
                        for (int k = 0; k < W; ++k) x[j][c][k] = 0.f;
                        if (e < E) x[j][c] = *reinterpret_cast<const vec_t*>(dout + rr * ldo + e);
                    }
                }
#pragma unroll
                for (int j = 0; j < EMB_DEPTH; ++j)
                    if (i0 + j < nq) {
#pragma unroll
                        for (int c = 0; c < EMB_CH; ++c) acc[c] += x[j][c];
                    }
            }
            nq = 0;
            __syncthreads();
        };
        int hi = lane / mod, lo = lane - hi * mod;
        for (int base = 0; base < rows; base += 64 * EMB_UNROLL) {
            long id[EMB_UNROLL];
            int row[EMB_UNROLL];
#pragma unroll
            for (int u = 0; u < EMB_UNROLL; ++u) {
                const int q = base + 64 * u + lane;
                id[u] = -1;
                if (q < rows) id[u] = ids[hi * s_hi + lo * s_lo];
                row[u] = mem_order ? lo * inner + hi : q;      // the row of d out this entry belongs to
                lo += step_r;
                hi += step_q;
                if (lo >= mod) { lo -= mod; ++hi; }
            }
            if (nq + 64 * EMB_UNROLL > EMB_QCAP) drain();
#pragma unroll
            for (int u = 0; u < EMB_UNROLL; ++u) {
                const bool hit = id[u] == v;
                const unsigned long long m = __ballot(hit);
                if (hit) queue[nq + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = row[u];
                nq += __builtin_popcountll(m);
            }
        }
        drain();
#pragma unroll
        for (int c = 0; c < EMB_CH; ++c) {
            const int e = e0 + (c * 64 + lane) * W;
            if (e < E) *reinterpret_cast<vec_t*>(dW + v * E + e) = acc[c];
        }
    }
}
extern "C" int rfn_embed_bwd(const float* dout, int64_t ldo, const int64_t* ids, int inner, int64_t ids_s_inner,
                             int64_t ids_s_outer, int rows, int E, int64_t V1, float* dW, void* stream) {
    if (rows < 0 || E <= 0 || V1 <= 0 || inner <= 0) return RFN_ERR_SHAPE;
    if (!dout || !ids || !dW) return RFN_ERR_ARG;
    const bool vec = (E % 4 == 0) && (ldo % 4 == 0) && rfn_aligned16(dout) && rfn_aligned16(dW);
    if (vec)
        hipLaunchKernelGGL(embed_bwd_k<true>, dim3((unsigned)V1), dim3(64), 0, (hipStream_t)stream, dout, (long)ldo,
                           ids, inner, (long)ids_s_inner, (long)ids_s_outer, rows, E, dW);
    else
        hipLaunchKernelGGL(embed_bwd_k<false>, dim3((unsigned)V1), dim3(64), 0, (hipStream_t)stream, dout,
                           (long)ldo, ids, inner, (long)ids_s_inner, (long)ids_s_outer, rows, E, dW);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- reason heads: max over steps ------------------------------------------------------------------
// blockIdx.y = head: X slabs (T, B*K) lie `T*BK` apart, out / arg / dout (B*K) `BK` apart.
__global__ __launch_bounds__(256) void max_steps_fwd_k(const float* __restrict__ X, int T, long BK,
                                                       float* __restrict__ out, int32_t* __restrict__ arg) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BK) return;
    X += (long)blockIdx.y * T * BK;
    float m = X[i];
    int a = 0;
    for (int t = 1; t < T; ++t) {
        const float v = X[t * BK + i];
        if (v > m) {
            m = v;
            a = t;
        }
    }
    out[blockIdx.y * BK + i] = m;
    if (arg) arg[blockIdx.y * BK + i] = a;
}
extern "C" int rfn_max_over_steps_fwd_grouped(const float* X, int T, int B, int K, float* out, int32_t* arg,
                                              int ngroups, void* stream) {
    if (T <= 0 || B <= 0 || K <= 0 || ngroups < 1) return RFN_ERR_SHAPE;
    if (!X || !out) return RFN_ERR_ARG;
    const long BK = (long)B * K;
    hipLaunchKernelGGL(max_steps_fwd_k, dim3(rfn_cdiv(BK, 256), ngroups), dim3(256), 0, (hipStream_t)stream, X, T, BK,
                       out, arg);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_max_over_steps_fwd(const float* X, int T, int B, int K, float* out, int32_t* arg, void* stream) {
    return rfn_max_over_steps_fwd_grouped(X, T, B, K, out, arg, 1, stream);
}
__global__ __launch_bounds__(256) void max_steps_bwd_k(const float* __restrict__ dout, const int32_t* __restrict__ arg,
                                                       int T, long BK, float* __restrict__ dX) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BK) return;
    const float g = dout ? dout[blockIdx.y * BK + i] : 0.f;
    const int a = arg[blockIdx.y * BK + i];
    dX += (long)blockIdx.y * T * BK;
    for (int t = 0; t < T; ++t) dX[t * BK + i] = (t == a) ? g : 0.f;
}
extern "C" int rfn_max_over_steps_bwd_grouped(const float* dout, const int32_t* arg, int T, int B, int K, float* dX,
                                              int ngroups, void* stream) {
    if (T <= 0 || B <= 0 || K <= 0 || ngroups < 1) return RFN_ERR_SHAPE;
    if (!arg || !dX) return RFN_ERR_ARG;
    const long BK = (long)B * K;
    hipLaunchKernelGGL(max_steps_bwd_k, dim3(rfn_cdiv(BK, 256), ngroups), dim3(256), 0, (hipStream_t)stream, dout, arg,
                       T, BK, dX);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_max_over_steps_bwd(const float* dout, const int32_t* arg, int T, int B, int K, float* dX,
                                      void* stream) {
    return rfn_max_over_steps_bwd_grouped(dout, arg, T, B, K, dX, 1, stream);
}

// ---- y = alpha*x + beta*y on a strided 2-D view ------------------------------------------------------
__global__ __launch_bounds__(256) void axpby_2d_k(float alpha, const float* __restrict__ x, long ldx, float beta,
                                                  float* __restrict__ y, long ldy, int rows, int cols) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i - (long)r * cols);
    const float xv = x ? alpha * x[r * ldx + c] : 0.f;
    float* p = y + r * ldy + c;
    *p = (beta == 0.f) ? xv : xv + beta * *p;
}
extern "C" int rfn_axpby_2d(float alpha, const float* x, int64_t ldx, float beta, float* y, int64_t ldy, int rows,
                            int cols, void* stream) {
    if (rows <= 0 || cols <= 0) return RFN_ERR_SHAPE;
    if (!y) return RFN_ERR_ARG;
    hipLaunchKernelGGL(axpby_2d_k, dim3(rfn_cdiv((long)rows * cols, 256)), dim3(256), 0, (hipStream_t)stream, alpha,
                       x, (long)ldx, beta, y, (long)ldy, rows, cols);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- y[r,c] /= divisor (true division: the state mean sum/M of misc/RecurrentFusionModel.py:234-235) ----
__global__ __launch_bounds__(256) void div_2d_k(float* __restrict__ y, long ldy, int rows, int cols, float divisor) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i - (long)r * cols);
    y[r * ldy + c] = y[r * ldy + c] / divisor;
}
extern "C" int rfn_div_2d(float* y, int64_t ldy, int rows, int cols, float divisor, void* stream) {
    if (rows <= 0 || cols <= 0 || divisor == 0.f) return RFN_ERR_SHAPE;
    if (!y) return RFN_ERR_ARG;
    hipLaunchKernelGGL(div_2d_k, dim3(rfn_cdiv((long)rows * cols, 256)), dim3(256), 0, (hipStream_t)stream, y,
                       (long)ldy, rows, cols, divisor);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- mean over the M encoder slices of a concatenated state and its backward (misc/RecurrentFusionModel.py:233-235)
// y[r, c] = (((x[r, c] + x[r, G1 + c]) + x[r, 2*G1 + c]) + ...) / G   -- summed first, then divided, like the
// reference; blockIdx.y selects one of up to two (x, y) pairs (h and c share the launch).
struct MeanArgs {
    const float* x[2];
    float* y[2];
    float beta[2];   // backward only: y = alpha*x + beta*y per pair
};
__global__ __launch_bounds__(256) void mean_groups_k(const MeanArgs a, long ldx, long gstride, int G, long ldy,
                                                     int rows, int cols) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i - (long)r * cols);
    const float* x = a.x[blockIdx.y] + r * ldx + c;
    float s = x[0];
    for (int g = 1; g < G; ++g) s += x[g * gstride];
    a.y[blockIdx.y][r * ldy + c] = s / (float)G;
}
extern "C" int rfn_mean_over_groups(int npairs, const float* const* x, int64_t ldx, int64_t gstride, int G,
                                    float* const* y, int64_t ldy, int rows, int cols, void* stream) {
    if (npairs < 1 || npairs > 2 || G < 1 || rows <= 0 || cols <= 0) return RFN_ERR_SHAPE;
    if (!x || !y) return RFN_ERR_ARG;
    MeanArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < npairs; ++p) {
        if (!x[p] || !y[p]) return RFN_ERR_ARG;
        a.x[p] = x[p];
        a.y[p] = y[p];
    }
    hipLaunchKernelGGL(mean_groups_k, dim3(rfn_cdiv((long)rows * cols, 256), npairs), dim3(256), 0,
                       (hipStream_t)stream, a, (long)ldx, (long)gstride, G, (long)ldy, rows, cols);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
// y[r, g*gstride + c] = alpha * x[r, c] + beta_p * y[r, g*gstride + c]  for every group g (the mean's backward)
__global__ __launch_bounds__(256) void bcast_groups_k(const MeanArgs a, float alpha, long ldx, long gstride, int G,
                                                      long ldy, int rows, int cols) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i - (long)r * cols);
    const float xv = alpha * a.x[blockIdx.y][r * ldx + c];
    const float beta = a.beta[blockIdx.y];
    float* y = a.y[blockIdx.y] + r * ldy + c;
    for (int g = 0; g < G; ++g) {
        float* p = y + g * gstride;
        *p = (beta == 0.f) ? xv : xv + beta * *p;
    }
}
extern "C" int rfn_bcast_to_groups(int npairs, float alpha, const float* const* x, int64_t ldx, const float* beta,
                                   float* const* y, int64_t ldy, int64_t gstride, int G, int rows, int cols,
                                   void* stream) {
    if (npairs < 1 || npairs > 2 || G < 1 || rows <= 0 || cols <= 0) return RFN_ERR_SHAPE;
    if (!x || !y || !beta) return RFN_ERR_ARG;
    MeanArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < npairs; ++p) {
        if (!x[p] || !y[p]) return RFN_ERR_ARG;
        a.x[p] = x[p];
        a.y[p] = y[p];
        a.beta[p] = beta[p];
    }
    hipLaunchKernelGGL(bcast_groups_k, dim3(rfn_cdiv((long)rows * cols, 256), npairs), dim3(256), 0,
                       (hipStream_t)stream, a, alpha, (long)ldx, (long)gstride, G, (long)ldy, rows, cols);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- y[r, :] = ((0 + x[r*n, :]) + x[r*n + 1, :]) + ... + x[r*n + n - 1, :]: the n consecutive rows of a group summed, j
// ascending (multi-sample self-critical, rfn.h: d Pd of an image's n decoder rows -> the image).  One output chunk per thread
// (16 B where cols, the strides and the pointers allow, else one float), no atomics.
template <bool VEC>
__global__ __launch_bounds__(256) void rowgroup_sum_k(const float* __restrict__ x, long ldx, int n, float* __restrict__ y, long ldy,
                                                      long rows, int cols) {
    constexpr int W = VEC ? 4 : 1;
    const int cpr = (cols + W - 1) / W;                  // chunks per row
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cpr) return;
    const long r = i / cpr;
    const int c = (int)(i - r * cpr) * W;
    const float* p = x + r * n * ldx + c;
    if constexpr (VEC) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < n; ++j) s += *reinterpret_cast<const f32x4*>(p + j * ldx);
        *reinterpret_cast<f32x4*>(y + r * ldy + c) = s;
    } else {
        float s = 0.f;
        for (int j = 0; j < n; ++j) s += p[j * ldx];
        y[r * ldy + c] = s;
    }
}
extern "C" int rfn_rowgroup_sum(const float* x, int64_t ldx, int n, float* y, int64_t ldy, int64_t rows, int cols, void* stream) {
    if (n < 1 || rows <= 0 || cols <= 0 || ldx < cols || ldy < cols) return RFN_ERR_SHAPE;
    if (!x || !y) return RFN_ERR_ARG;
    const bool vec = cols % 4 == 0 && (ldx | ldy) % 4 == 0 && rfn_aligned16(x) && rfn_aligned16(y);
    const long chunks = (long)rows * (vec ? cols / 4 : cols);
    if (chunks > 0x7fffffffL * 256) return RFN_ERR_SHAPE;
    if (vec)
        hipLaunchKernelGGL(rowgroup_sum_k<true>, dim3(rfn_cdiv(chunks, 256)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, n, y,
                           (long)ldy, (long)rows, cols);
    else
        hipLaunchKernelGGL(rowgroup_sum_k<false>, dim3(rfn_cdiv(chunks, 256)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, n, y,
                           (long)ldy, (long)rows, cols);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
