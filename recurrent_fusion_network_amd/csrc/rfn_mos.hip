// Mixture-of-softmaxes output head (rfn.h "mixture of softmaxes"; misc/MixtureOfSoftmax.py): K experts tanh(Linear(h)) share one
// vocabulary projection, a softmax prior over the experts mixes their softmaxes.  The three linear maps run on the f32 GEMM
// (rfn_path.h helpers: the vocabulary projection is ONE product over K * rows expert rows); what is new here are the mix
// kernels, which turn the K * rows * V1 expert logits into mixture log-probs, into the loss, and back into d logits without
// writing a softmax of any expert.  One block of 256 per hidden row (rfn_rows.h): the K log-sum-exps first, then the K expert
// rows are streamed once more -- 16 B per lane where the row qualifies (lsm_vec_ok), element-wise otherwise.
#include "rfn_path.h"
#include "rfn_rows.h"

namespace {

const size_t MOS_GEMM_WS_FLOATS = (size_t)16 << 20;   // 64 MiB of split-K partial tiles for the weight gradients (K = rows)

struct MosLayout {
    size_t c, logpi, lse, z, x, dz, dc, gws, total;
};
MosLayout mos_layout(const rfn_mos_dims* md, long rows, int train) {
    Bump b;
    MosLayout L;
    const size_t K = md->K, n = (size_t)rows;
    L.c = b.take(n * K);
    L.logpi = b.take(n * K);
    L.lse = b.take(K * n);
    L.z = b.take(K * n * md->E);
    L.x = b.take(K * n * md->V1);
    L.dz = L.dc = L.gws = 0;
    if (train) {
        L.dz = b.take(K * n * md->E);
        L.dc = b.take(n * K);
        L.gws = b.take(MOS_GEMM_WS_FLOATS);
    }
    L.total = b.off;
    return L;
}
int mos_check(const rfn_mos_dims* md) {
    if (!md) return RFN_ERR_ARG;
    if (md->K < 1 || md->K > RFN_MOS_MAXK || md->R < 1 || md->E < 1 || md->V1 < 2) return RFN_ERR_SHAPE;
    return RFN_OK;
}
// parameter slots in state_dict order
struct MIdx {
    int K;
    MIdx() : K(0) {}
    explicit MIdx(const rfn_mos_dims* md) : K(md->K) {}
    int prior() const { return 0; }
    int lat_w(int k) const { return 1 + 2 * k; }
    int lat_b(int k) const { return 2 + 2 * k; }
    int dec_w() const { return 1 + 2 * K; }
    int dec_b() const { return 2 + 2 * K; }
    int count() const { return 3 + 2 * K; }
};

// ---- small passes ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mos_tanh_k(float* __restrict__ z, long n) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) z[i] = tanhf(z[i]);
}
// d (pre-activation) = d z * (1 - z^2), in place over d z
__global__ __launch_bounds__(256) void mos_tanh_bwd_k(float* __restrict__ dz, const float* __restrict__ z, long n) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float t = z[i];
        dz[i] *= 1.0f - t * t;
    }
}
// rfn_criteria.hip's sum_k: the fixed order every loss of the library is summed in
__global__ __launch_bounds__(256) void mos_sum_k(const float* __restrict__ x, int n, float scale, float* __restrict__ out,
                                                 int accumulate) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += x[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s * scale : s * scale;
}
int mos_grid(long n) {
    long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---- the head of every mix kernel: the row's K log-sum-exps and its log prior -------------------------------------------------
// bk[k] = log pi_k - lse_k, so that a_kv = bk[k] + x_kv.  STORE: lse and log pi go to the workspace for the backward.
// Ends with a barrier: bk is visible to every thread.
template <bool VEC, bool STORE>
__device__ __forceinline__ void mos_row_head(const float* __restrict__ x, long rows, int r, int K, int V1,
                                             const float* __restrict__ c, float* __restrict__ lse_ws, float* __restrict__ logpi_ws,
                                             float* bk, float* red) {
    float cm = -INFINITY, cs = 0.f;
    for (int k = 0; k < K; ++k) cm = fmaxf(cm, c[(long)r * K + k]);
    for (int k = 0; k < K; ++k) cs += expf(c[(long)r * K + k] - cm);
    const float clse = cm + logf(cs);
    for (int k = 0; k < K; ++k) {
        f32x4 xr[LSM_R4];
        const float lse = log_softmax_row<VEC>(x + ((long)k * rows + r) * V1, V1, xr, red);
        if (threadIdx.x == 0) {
            const float lpi = c[(long)r * K + k] - clse;
            bk[k] = lpi - lse;
            if constexpr (STORE) {
                lse_ws[(long)k * rows + r] = lse;
                logpi_ws[(long)r * K + k] = lpi;
            }
        }
    }
    __syncthreads();
}
// the backward's: from the workspace
__device__ __forceinline__ void mos_row_head_saved(long rows, int r, int K, const float* __restrict__ lse_ws,
                                                   const float* __restrict__ logpi_ws, float* bk, float* lk, float* pk) {
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        const float lpi = logpi_ws[(long)r * K + k];
        lk[k] = lse_ws[(long)k * rows + r];
        bk[k] = lpi - lk[k];
        pk[k] = expf(lpi);
    }
    __syncthreads();
}

// logp_v = LSE_k (bk[k] + x_kv) for one v (T = float) or four (T = f32x4), online over k: one exp per expert entry.
// Inputs are finite (bk and x are), so the running maximum is finite after k = 0.
template <class T>
__device__ __forceinline__ T mos_ld(const float* p) { return *reinterpret_cast<const T*>(p); }
__device__ __forceinline__ float mos_mix1(float m, float& s, float a) {
    if (a > m) {
        s = s * expf(m - a) + 1.0f;
        return a;
    }
    s += expf(a - m);
    return m;
}

// ---- forward mix: logp written through the row remap ---------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void mos_mix_fwd_k(const float* __restrict__ x, long rows, int K, int V1,
                                                     const float* __restrict__ c, float* __restrict__ lse_ws,
                                                     float* __restrict__ logpi_ws, int inner, long s_inner, long s_outer,
                                                     float* __restrict__ out) {
    __shared__ float red[4];
    __shared__ float bk[RFN_MOS_MAXK];
    const int r = blockIdx.x;
    mos_row_head<VEC, true>(x, rows, r, K, V1, c, lse_ws, logpi_ws, bk, red);
    float* o = out + (long)(r % inner) * s_inner + (long)(r / inner) * s_outer;
    const float* x0 = x + (long)r * V1;
    const long ks = rows * (long)V1;          // expert stride
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            f32x4 m = mos_ld<f32x4>(x0 + 4 * i) + bk[0], s = f32x4{1.f, 1.f, 1.f, 1.f};
            for (int k = 1; k < K; ++k) {
                const f32x4 a = mos_ld<f32x4>(x0 + k * ks + 4 * i) + bk[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float se = s[e];
                    m[e] = mos_mix1(m[e], se, a[e]);
                    s[e] = se;
                }
            }
            f32x4 lp;
#pragma unroll
            for (int e = 0; e < 4; ++e) lp[e] = m[e] + logf(s[e]);
            *reinterpret_cast<f32x4*>(o + 4 * i) = lp;
        }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) {
            float m = x0[v] + bk[0], s = 1.f;
            for (int k = 1; k < K; ++k) m = mos_mix1(m, s, x0[k * ks + v] + bk[k]);
            o[v] = m + logf(s);
        }
    }
}

// ---- loss mix: the row's term of the masked, label-smoothed NLL (xe_logits_fwd_k's expression) ---------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void mos_mix_loss_k(const float* __restrict__ x, long rows, int K, int V1,
                                                      const float* __restrict__ c, float* __restrict__ lse_ws,
                                                      float* __restrict__ logpi_ws, int B, int T,
                                                      const int64_t* __restrict__ target, long ld_t, const float* __restrict__ mask,
                                                      long ld_m, float eps, float* __restrict__ row_loss) {
    __shared__ float red[4];
    __shared__ float bk[RFN_MOS_MAXK];
    const int r = blockIdx.x, t = r / B, b = r - t * B;      // time-major rows
    mos_row_head<VEC, true>(x, rows, r, K, V1, c, lse_ws, logpi_ws, bk, red);
    long tg = target[b * ld_t + t];
    if (tg < 0 || tg >= V1) tg = 0;
    const float mk = mask[b * ld_m + t];
    const float* x0 = x + (long)r * V1;
    const long ks = rows * (long)V1;
    float term;
    {   // K gathers
        float m = x0[tg] + bk[0], s = 1.f;
        for (int k = 1; k < K; ++k) m = mos_mix1(m, s, x0[k * ks + tg] + bk[k]);
        term = m + logf(s);
    }
    if (eps > 0.f) {   // sum_v logp_v, never written
        float sum = 0.f;
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
            for (int i = threadIdx.x; i < n4; i += 256) {
                f32x4 m = mos_ld<f32x4>(x0 + 4 * i) + bk[0], s = f32x4{1.f, 1.f, 1.f, 1.f};
                for (int k = 1; k < K; ++k) {
                    const f32x4 a = mos_ld<f32x4>(x0 + k * ks + 4 * i) + bk[k];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                    float se = s[e];
                    m[e] = mos_mix1(m[e], se, a[e]);
                    s[e] = se;
                }
                }
                sum += ((m[0] + logf(s[0])) + (m[1] + logf(s[1]))) + ((m[2] + logf(s[2])) + (m[3] + logf(s[3])));
            }
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) {
                float m = x0[v] + bk[0], s = 1.f;
                for (int k = 1; k < K; ++k) m = mos_mix1(m, s, x0[k * ks + v] + bk[k]);
                sum += m + logf(s);
            }
        }
        sum = block_sum_256(sum, red);
        term = (1.0f - eps) * term + (eps / (float)V1) * sum;
    }
    if (threadIdx.x == 0) row_loss[b * T + t] = -mk * term;
}

// ---- backward mix: d x over x, d c ----------------------------------------------------------------------------------------------
// G_v comes from d_logp (LOSS = false, through the row remap) or is -cf * (eps / V1 + (1 - eps) [v == tg]) with cf = mask * g / B
// (LOSS = true).  Pass 1: s_k = sum_v G_v r_kv, r_kv = exp(a_kv - m_v) / sum_j exp(a_jv - m_v): the K entries of a column are held
// in registers (every loop over k is unrolled to RFN_MOS_MAXK with compile-time indices).  Pass 2: d x_kv = G_v r_kv - p_kv s_k.
// With a one-hot G (LOSS, eps == 0) pass 1 is K gathers and pass 2 needs r at the target only.
struct MosLossArgs {
    int B, T;
    const int64_t* target;
    long ld_t;
    const float* mask;
    long ld_m;
    float eps, gcoef;
    const float* gdev;
};
template <class T>
__device__ __forceinline__ void mos_resp(const T (&xv)[RFN_MOS_MAXK], const float* bk, int K, T (&rv)[RFN_MOS_MAXK]) {
    T m = xv[0] + bk[0];
#pragma unroll
    for (int k = 1; k < RFN_MOS_MAXK; ++k)
        if (k < K) {
            const T a = xv[k] + bk[k];
            if constexpr (std::is_same<T, float>::value) {
                m = fmaxf(m, a);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], a[e]);
            }
        }
    T s = m - m;
#pragma unroll
    for (int k = 0; k < RFN_MOS_MAXK; ++k)
        if (k < K) {
            const T a = xv[k] + bk[k] - m;
            if constexpr (std::is_same<T, float>::value) {
                rv[k] = expf(a);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) rv[k][e] = expf(a[e]);
            }
            s += rv[k];
        }
    const T inv = 1.0f / s;
#pragma unroll
    for (int k = 0; k < RFN_MOS_MAXK; ++k)
        if (k < K) rv[k] *= inv;
}
template <bool VEC, bool LOSS>
__global__ __launch_bounds__(256) void mos_mix_bwd_k(float* __restrict__ x, long rows, int K, int V1,
                                                     const float* __restrict__ lse_ws, const float* __restrict__ logpi_ws,
                                                     const float* __restrict__ dlogp, int inner, long s_inner, long s_outer,
                                                     const MosLossArgs la, float* __restrict__ dc) {
    __shared__ float red[4];
    __shared__ float bk[RFN_MOS_MAXK], lk[RFN_MOS_MAXK], pk[RFN_MOS_MAXK], sk[RFN_MOS_MAXK];
    const int r = blockIdx.x;
    float* x0 = x + (long)r * V1;
    const long ks = rows * (long)V1;
    const float* g = nullptr;
    long tg = 0;
    float cf = 0.f, uni = 0.f, hot = 1.f;
    if constexpr (LOSS) {
        const int t = r / la.B, b = r - t * la.B;
        tg = la.target[b * la.ld_t + t];
        if (tg < 0 || tg >= V1) tg = 0;
        cf = la.mask[b * la.ld_m + t] * (la.gdev ? la.gcoef * la.gdev[0] : la.gcoef);
        uni = la.eps / (float)V1;
        hot = 1.0f - la.eps;
        if (cf == 0.f) {   // a masked-out row: exactly zero everywhere (uniform per block)
            for (int k = 0; k < K; ++k)
                for (int v = threadIdx.x; v < V1; v += 256) x0[k * ks + v] = 0.f;
            if ((int)threadIdx.x < K) dc[(long)r * K + threadIdx.x] = 0.f;
            return;
        }
    } else {
        g = dlogp + (long)(r % inner) * s_inner + (long)(r / inner) * s_outer;
    }
    mos_row_head_saved(rows, r, K, lse_ws, logpi_ws, bk, lk, pk);
    const bool onehot = LOSS && la.eps == 0.f;
    auto G1 = [&](int v) -> float {
        if constexpr (LOSS) return -cf * (uni + ((v == tg) ? hot : 0.f));
        else return g[v];
    };

    // ---- pass 1: s_k
    float rt[RFN_MOS_MAXK];    // onehot: r_k at the target, kept for pass 2
    if (onehot) {
        float xv[RFN_MOS_MAXK];
#pragma unroll
        for (int k = 0; k < RFN_MOS_MAXK; ++k) xv[k] = (k < K) ? x0[k * ks + tg] : 0.f;
        mos_resp<float>(xv, bk, K, rt);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < RFN_MOS_MAXK; ++k)
                if (k < K) sk[k] = -cf * rt[k];
        }
    } else {
        float acc[RFN_MOS_MAXK];
#pragma unroll
        for (int k = 0; k < RFN_MOS_MAXK; ++k) acc[k] = 0.f;
        if constexpr (VEC) {
            const int n4 = V1 >> 2;
            for (int i = threadIdx.x; i < n4; i += 256) {
                f32x4 xv[RFN_MOS_MAXK], rv[RFN_MOS_MAXK], gv;
#pragma unroll
                for (int k = 0; k < RFN_MOS_MAXK; ++k)
                    if (k < K) xv[k] = mos_ld<f32x4>(x0 + k * ks + 4 * i);
                mos_resp<f32x4>(xv, bk, K, rv);
                if constexpr (LOSS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) gv[e] = G1(4 * i + e);
                } else {
                    gv = mos_ld<f32x4>(g + 4 * i);
                }
#pragma unroll
                for (int k = 0; k < RFN_MOS_MAXK; ++k)
                    if (k < K) {
                        const f32x4 p = gv * rv[k];
                        acc[k] += (p[0] + p[1]) + (p[2] + p[3]);
                    }
            }
        } else {
            for (int v = threadIdx.x; v < V1; v += 256) {
                float xv[RFN_MOS_MAXK], rv[RFN_MOS_MAXK];
#pragma unroll
                for (int k = 0; k < RFN_MOS_MAXK; ++k)
                    if (k < K) xv[k] = x0[k * ks + v];
                mos_resp<float>(xv, bk, K, rv);
                const float gv = G1(v);
#pragma unroll
                for (int k = 0; k < RFN_MOS_MAXK; ++k)
                    if (k < K) acc[k] += gv * rv[k];
            }
        }
#pragma unroll
        for (int k = 0; k < RFN_MOS_MAXK; ++k)
            if (k < K) {       // K is uniform: every thread takes the same barriers
                const float s = block_sum_256(acc[k], red);
                if (threadIdx.x == 0) sk[k] = s;
            }
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {   // d c_k = s_k - pi_k sum_j s_j
        float tot = 0.f;
        for (int j = 0; j < K; ++j) tot += sk[j];
        const int k = threadIdx.x;
        dc[(long)r * K + k] = sk[k] - pk[k] * tot;
    }

    // ---- pass 2: d x over x
    if (onehot) {
        for (int k = 0; k < K; ++k) {
            float* xk = x0 + k * ks;
            const float s = sk[k], l = lk[k];
            if constexpr (VEC) {
                const int n4 = V1 >> 2;
                for (int i = threadIdx.x; i < n4; i += 256) {
                    const f32x4 v4 = mos_ld<f32x4>(xk + 4 * i);
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = -expf(v4[e] - l) * s;
                    *reinterpret_cast<f32x4*>(xk + 4 * i) = o;
                }
            } else {
                for (int v = threadIdx.x; v < V1; v += 256) xk[v] = -expf(xk[v] - l) * s;
            }
        }
        __syncthreads();       // the target's entries: G r_k - p s_k, p s_k already there (with its sign)
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < RFN_MOS_MAXK; ++k)
                if (k < K) x0[k * ks + tg] += -cf * rt[k];
        }
        return;
    }
    if constexpr (VEC) {
        const int n4 = V1 >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            f32x4 xv[RFN_MOS_MAXK], rv[RFN_MOS_MAXK], gv;
#pragma unroll
            for (int k = 0; k < RFN_MOS_MAXK; ++k)
                if (k < K) xv[k] = mos_ld<f32x4>(x0 + k * ks + 4 * i);
            mos_resp<f32x4>(xv, bk, K, rv);
            if constexpr (LOSS) {
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[e] = G1(4 * i + e);
            } else {
                gv = mos_ld<f32x4>(g + 4 * i);
            }
#pragma unroll
            for (int k = 0; k < RFN_MOS_MAXK; ++k)
                if (k < K) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = gv[e] * rv[k][e] - expf(xv[k][e] - lk[k]) * sk[k];
                    *reinterpret_cast<f32x4*>(x0 + k * ks + 4 * i) = o;
                }
        }
    } else {
        for (int v = threadIdx.x; v < V1; v += 256) {
            float xv[RFN_MOS_MAXK], rv[RFN_MOS_MAXK];
#pragma unroll
            for (int k = 0; k < RFN_MOS_MAXK; ++k)
                if (k < K) xv[k] = x0[k * ks + v];
            mos_resp<float>(xv, bk, K, rv);
            const float gv = G1(v);
#pragma unroll
            for (int k = 0; k < RFN_MOS_MAXK; ++k)
                if (k < K) x0[k * ks + v] = gv * rv[k] - expf(xv[k] - lk[k]) * sk[k];
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct MosCall {
    const rfn_mos_dims* md;
    MIdx P;
    long rows;
    const float* h;
    long ldh;
    const float* const* prm;
    float* W;
    MosLayout Lo;
    void* st;
};
int mos_open(const rfn_mos_dims* md, long rows, const float* h, int64_t ldh, const float* const* prm, void* ws, size_t ws_bytes,
             int train, void* st, MosCall* c) {
    RFN_TRY(mos_check(md));
    if (rows < 1 || rows * (long)md->K > 0x7fffffffL || ldh < md->R) return RFN_ERR_SHAPE;
    if (!h || !prm || !ws || !rfn_aligned16(ws)) return RFN_ERR_ARG;
    const MIdx P(md);
    for (int i = 0; i < P.count(); ++i)
        if (!prm[i]) return RFN_ERR_ARG;
    const MosLayout Lo = mos_layout(md, rows, train);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    *c = MosCall{md, P, rows, h, (long)ldh, prm, (float*)ws, Lo, st};
    return RFN_OK;
}
// c = h . prior^T, z_k = tanh(h . latent_k^T + b_k) (K same-shape products, grouped), x = z . decoder^T + b over K * rows rows.
// Never split along K: a row's log-probs do not depend on how many rows the call carries.
int mos_products(const MosCall& c) {
    const rfn_mos_dims* md = c.md;
    const int R = md->R, E = md->E, K = md->K, V1 = md->V1, rows = (int)c.rows;
    const GemmCtx gx{c.st, nullptr, 0, 0};
    float* z = c.W + c.Lo.z;
    RFN_TRY(gemm1(rows, K, seg_lin(c.h, c.ldh, c.prm[c.P.prior()], R, R, nullptr), c.W + c.Lo.c, K, 0, gx));
    rfn_gemm_problem pr[RFN_MOS_MAXK];
    for (int k = 0; k < K; ++k)
        pr[k] = prob1(z + (long)k * rows * E, E, seg_lin(c.h, c.ldh, c.prm[c.P.lat_w(k)], R, R, c.prm[c.P.lat_b(k)]));
    RFN_TRY(gemm_groups(rows, E, K, pr, 0, gx));
    const long nz = (long)K * rows * E;
    hipLaunchKernelGGL(mos_tanh_k, dim3(mos_grid(nz)), dim3(256), 0, (hipStream_t)c.st, z, nz);
    RFN_CHECK_LAUNCH();
    return gemm_logits(K * rows, V1, z, E, c.prm[c.P.dec_w()], c.prm[c.P.dec_b()], c.W + c.Lo.x, gx);
}
// everything after the backward mix: d z, the tanh, the weight gradients, d h
int mos_bwd_products(const MosCall& c, float* d_h, float* const* grd) {
    const rfn_mos_dims* md = c.md;
    const int R = md->R, E = md->E, K = md->K, V1 = md->V1, rows = (int)c.rows;
    const GemmCtx gx{c.st, c.W + c.Lo.gws, MOS_GEMM_WS_FLOATS * sizeof(float), 0};
    float *z = c.W + c.Lo.z, *dx = c.W + c.Lo.x, *dz = c.W + c.Lo.dz, *dc = c.W + c.Lo.dc;
    RFN_TRY(gemm_logits_dw(V1, E, grd[c.P.dec_w()], grd[c.P.dec_b()], dx, z, K * rows, gx));
    RFN_TRY(gemm_logits_dx(K * rows, E, V1, dx, c.prm[c.P.dec_w()], dz, gx));
    const long nz = (long)K * rows * E;
    hipLaunchKernelGGL(mos_tanh_bwd_k, dim3(mos_grid(nz)), dim3(256), 0, (hipStream_t)c.st, dz, z, nz);
    RFN_CHECK_LAUNCH();
    rfn_gemm_problem pr[RFN_MOS_MAXK];
    for (int k = 0; k < K; ++k)
        pr[k] = prob_dw(grd[c.P.lat_w(k)], R, grd[c.P.lat_b(k)], dz + (long)k * rows * E, E, c.h, c.ldh, rows);
    RFN_TRY(gemm_groups(E, R, K, pr, 0, gx));
    RFN_TRY(gemm_dw(K, R, grd[c.P.prior()], R, nullptr, dc, K, c.h, c.ldh, rows, gx));
    rfn_gemm_seg sg[RFN_MOS_MAXK + 1];
    sg[0] = seg_dx(dc, K, c.prm[c.P.prior()], R, K);
    for (int k = 0; k < K; ++k) sg[1 + k] = seg_dx(dz + (long)k * rows * E, E, c.prm[c.P.lat_w(k)], R, E);
    return gemm_segs(rows, R, K + 1, sg, d_h, R, 0, gx);
}
int mos_bwd_check(const MosCall& c, float* d_h, float* const* grd) {
    if (!d_h || !grd) return RFN_ERR_ARG;
    for (int i = 0; i < c.P.count(); ++i)
        if (!grd[i]) return RFN_ERR_ARG;
    return RFN_OK;
}
}  // namespace

extern "C" int rfn_mos_param_count(const rfn_mos_dims* md) {
    const int rc = mos_check(md);
    return rc != RFN_OK ? rc : MIdx(md).count();
}
extern "C" int rfn_mos_param_name(const rfn_mos_dims* md, int idx, char* buf, size_t n) {
    RFN_TRY(mos_check(md));
    if (!buf || n == 0) return RFN_ERR_ARG;
    const MIdx P(md);
    if (idx < 0 || idx >= P.count()) return RFN_ERR_SHAPE;
    if (idx == P.prior()) snprintf(buf, n, "prior.weight");
    else if (idx == P.dec_w()) snprintf(buf, n, "decoder.weight");
    else if (idx == P.dec_b()) snprintf(buf, n, "decoder.bias");
    else snprintf(buf, n, "latent.%d.0.%s", (idx - 1) / 2, ((idx - 1) & 1) ? "bias" : "weight");
    return RFN_OK;
}
extern "C" int rfn_mos_param_shape(const rfn_mos_dims* md, int idx, int64_t* rows, int64_t* cols) {
    RFN_TRY(mos_check(md));
    if (!rows || !cols) return RFN_ERR_ARG;
    const MIdx P(md);
    if (idx < 0 || idx >= P.count()) return RFN_ERR_SHAPE;
    if (idx == P.prior()) { *rows = md->K; *cols = md->R; }
    else if (idx == P.dec_w()) { *rows = md->V1; *cols = md->E; }
    else if (idx == P.dec_b()) { *rows = md->V1; *cols = 1; }
    else if ((idx - 1) & 1) { *rows = md->E; *cols = 1; }
    else { *rows = md->E; *cols = md->R; }
    return RFN_OK;
}
extern "C" size_t rfn_mos_ws_bytes(const rfn_mos_dims* md, int64_t rows, int train) {
    if (mos_check(md) != RFN_OK || rows < 1) return 0;
    return mos_layout(md, rows, train).total * sizeof(float);
}
extern "C" float* rfn_mos_ws_lse(const rfn_mos_dims* md, int64_t rows, void* ws) {
    if (mos_check(md) != RFN_OK || rows < 1 || !ws) return nullptr;
    return (float*)ws + mos_layout(md, rows, 0).lse;
}
extern "C" float* rfn_mos_ws_logpi(const rfn_mos_dims* md, int64_t rows, void* ws) {
    if (mos_check(md) != RFN_OK || rows < 1 || !ws) return nullptr;
    return (float*)ws + mos_layout(md, rows, 0).logpi;
}
extern "C" float* rfn_mos_ws_x(const rfn_mos_dims* md, int64_t rows, void* ws) {
    if (mos_check(md) != RFN_OK || rows < 1 || !ws) return nullptr;
    return (float*)ws + mos_layout(md, rows, 0).x;
}
extern "C" float* rfn_mos_ws_dc(const rfn_mos_dims* md, int64_t rows, void* ws) {
    if (mos_check(md) != RFN_OK || rows < 1 || !ws) return nullptr;
    return (float*)ws + mos_layout(md, rows, 1).dc;
}

extern "C" int rfn_mos_fwd(const rfn_mos_dims* md, int rows, const float* h, int64_t ldh, const float* const* prm, int inner,
                           int64_t out_s_inner, int64_t out_s_outer, float* logp, void* ws, size_t ws_bytes, int train, void* st) {
    MosCall c;
    if (md && mos_check(md) == RFN_OK && inner < 1) return RFN_ERR_SHAPE;
    RFN_TRY(mos_open(md, rows, h, ldh, prm, ws, ws_bytes, train, st, &c));
    if (!logp) return RFN_ERR_ARG;
    RFN_TRY(mos_products(c));
    float* W = c.W;
    const int K = md->K, V1 = md->V1;
    if (lsm_vec_ok(W + c.Lo.x, V1, V1, logp, out_s_inner, out_s_outer))
        hipLaunchKernelGGL(mos_mix_fwd_k<true>, dim3(rows), dim3(256), 0, (hipStream_t)st, W + c.Lo.x, (long)rows, K, V1, W + c.Lo.c,
                           W + c.Lo.lse, W + c.Lo.logpi, inner, (long)out_s_inner, (long)out_s_outer, logp);
    else
        hipLaunchKernelGGL(mos_mix_fwd_k<false>, dim3(rows), dim3(256), 0, (hipStream_t)st, W + c.Lo.x, (long)rows, K, V1, W + c.Lo.c,
                           W + c.Lo.lse, W + c.Lo.logpi, inner, (long)out_s_inner, (long)out_s_outer, logp);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_mos_loss_fwd(const rfn_mos_dims* md, int B, int T, const float* h, int64_t ldh, const float* const* prm,
                                const int64_t* target, int64_t ld_target, const float* mask, int64_t ld_mask, float eps,
                                float* scratch, float* loss_out, int accumulate_loss, void* ws, size_t ws_bytes, void* st) {
    MosCall c;
    if (B < 1 || T < 1 || (long)B * T > 0x7fffffffL || !(eps >= 0.f && eps < 1.f)) return md ? RFN_ERR_SHAPE : RFN_ERR_ARG;
    RFN_TRY(mos_open(md, (long)B * T, h, ldh, prm, ws, ws_bytes, 1, st, &c));
    if (!target || !mask || !scratch || !loss_out) return RFN_ERR_ARG;
    RFN_TRY(mos_products(c));
    float* W = c.W;
    const int K = md->K, V1 = md->V1, rows = B * T;
    if (lsm_vec_ok(W + c.Lo.x, V1, V1, nullptr, 0, 0))
        hipLaunchKernelGGL(mos_mix_loss_k<true>, dim3(rows), dim3(256), 0, (hipStream_t)st, W + c.Lo.x, (long)rows, K, V1, W + c.Lo.c,
                           W + c.Lo.lse, W + c.Lo.logpi, B, T, target, (long)ld_target, mask, (long)ld_mask, eps, scratch);
    else
        hipLaunchKernelGGL(mos_mix_loss_k<false>, dim3(rows), dim3(256), 0, (hipStream_t)st, W + c.Lo.x, (long)rows, K, V1, W + c.Lo.c,
                           W + c.Lo.lse, W + c.Lo.logpi, B, T, target, (long)ld_target, mask, (long)ld_mask, eps, scratch);
    RFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(mos_sum_k, dim3(1), dim3(256), 0, (hipStream_t)st, scratch, rows, 1.0f / (float)B, loss_out, accumulate_loss);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_mos_bwd(const rfn_mos_dims* md, int rows, const float* h, int64_t ldh, const float* const* prm,
                           const float* d_logp, int inner, int64_t s_inner, int64_t s_outer, float* d_h, float* const* grd, void* ws,
                           size_t ws_bytes, void* st) {
    MosCall c;
    if (md && mos_check(md) == RFN_OK && inner < 1) return RFN_ERR_SHAPE;
    RFN_TRY(mos_open(md, rows, h, ldh, prm, ws, ws_bytes, 1, st, &c));
    if (!d_logp) return RFN_ERR_ARG;
    RFN_TRY(mos_bwd_check(c, d_h, grd));
    float* W = c.W;
    const int K = md->K, V1 = md->V1;
    const MosLossArgs la{};
    if (lsm_vec_ok(W + c.Lo.x, V1, V1, d_logp, s_inner, s_outer))
        hipLaunchKernelGGL((mos_mix_bwd_k<true, false>), dim3(rows), dim3(256), 0, (hipStream_t)st, W + c.Lo.x, (long)rows, K, V1,
                           W + c.Lo.lse, W + c.Lo.logpi, d_logp, inner, (long)s_inner, (long)s_outer, la, W + c.Lo.dc);
    else
        hipLaunchKernelGGL((mos_mix_bwd_k<false, false>), dim3(rows), dim3(256), 0, (hipStream_t)st, W + c.Lo.x, (long)rows, K, V1,
                           W + c.Lo.lse, W + c.Lo.logpi, d_logp, inner, (long)s_inner, (long)s_outer, la, W + c.Lo.dc);
    RFN_CHECK_LAUNCH();
    return mos_bwd_products(c, d_h, grd);
}

extern "C" int rfn_mos_loss_bwd(const rfn_mos_dims* md, int B, int T, const float* h, int64_t ldh, const float* const* prm,
                                const int64_t* target, int64_t ld_target, const float* mask, int64_t ld_mask, float eps,
                                float gscale, const float* gscale_dev, float* d_h, float* const* grd, void* ws, size_t ws_bytes,
                                void* st) {
    MosCall c;
    if (B < 1 || T < 1 || (long)B * T > 0x7fffffffL || !(eps >= 0.f && eps < 1.f)) return md ? RFN_ERR_SHAPE : RFN_ERR_ARG;
    RFN_TRY(mos_open(md, (long)B * T, h, ldh, prm, ws, ws_bytes, 1, st, &c));
    if (!target || !mask) return RFN_ERR_ARG;
    RFN_TRY(mos_bwd_check(c, d_h, grd));
    float* W = c.W;
    const int K = md->K, V1 = md->V1, rows = B * T;
    const MosLossArgs la{B, T, target, (long)ld_target, mask, (long)ld_mask, eps, gscale / (float)B, gscale_dev};
    if (lsm_vec_ok(W + c.Lo.x, V1, V1, nullptr, 0, 0))
        hipLaunchKernelGGL((mos_mix_bwd_k<true, true>), dim3(rows), dim3(256), 0, (hipStream_t)st, W + c.Lo.x, (long)rows, K, V1,
                           W + c.Lo.lse, W + c.Lo.logpi, (const float*)nullptr, 1, 0L, 0L, la, W + c.Lo.dc);
    else
        hipLaunchKernelGGL((mos_mix_bwd_k<false, true>), dim3(rows), dim3(256), 0, (hipStream_t)st, W + c.Lo.x, (long)rows, K, V1,
                           W + c.Lo.lse, W + c.Lo.logpi, (const float*)nullptr, 1, 0L, 0L, la, W + c.Lo.dc);
    RFN_CHECK_LAUNCH();
    return mos_bwd_products(c, d_h, grd);
}
