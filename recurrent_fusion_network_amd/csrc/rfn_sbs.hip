// Stochastic beam search (rfn.h "stochastic beam search"; Kool, van Hoof, Welling, ICML 2019): a beam search of width W on
// Gumbel-perturbed log-probabilities draws W distinct captions, an exact sample without replacement.  Two kernels: the
// log-softmax of a beam row with its W best PERTURBED entries (one block per row, the structure of log_softmax_topk_k in
// rfn_logsoftmax.hip), and the per-image bookkeeping of one step (one block per image, the structure of beam_step_div_k in
// rfn_beam.hip).  Everything the definition states in fp64 is computed in fp64 here.
#include "rfn_beam_step.h"   // the scaffolding shared with rfn_beam.hip; rfn_rows.h through it

#define SBS_THREADS 256

// e = -ln(-ln u), u = (n + 0.5) / 2^24 with n the 24 bits rfn_philox_uniform turns into its float: that float is n * 2^-24
// exactly, and adding 2^-25 in fp64 is exact too.
__device__ __forceinline__ double sbs_gumbel(uint64_t seed, uint64_t offset, uint64_t idx) {
    const double u = (double)rfn_philox_uniform(seed, offset, idx) + 0x1p-25;
    return -log(-log(u));
}

// ---- log-softmax + the W best perturbed entries of every live row -------------------------------------------------------
// The log-sum-exp is log_softmax_row's, taken the way rfn_log_softmax_fwd takes it for this row (VEC or not), so x_v = x[v] - lse
// carries that kernel's bits.  The register copy of the row is not used beyond that: the pass below re-reads the row from cache
// in one rolled loop, which keeps the Philox rounds and the two fp64 logarithms of a key at one inlined copy per kernel instead
// of forty.
template <bool VEC, int LW, bool MASK>
__global__ __launch_bounds__(256) void log_softmax_topk_gumbel_k(const float* __restrict__ logits, long ldl, int V1, int W,
                                                                 const int* __restrict__ blk, long ld_blk,
                                                                 const int* __restrict__ blk_n, const int* __restrict__ live,
                                                                 uint64_t seed, uint64_t offset, double* __restrict__ topk64,
                                                                 float* __restrict__ topv, int* __restrict__ topi) {
    __shared__ float red[4];
    __shared__ double wv[4][LSM_TOPW];
    __shared__ int wi[4][LSM_TOPW];
    extern __shared__ unsigned lsm_bits[];       // MASK: (V1 + 31) / 32 words
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!live[r]) return;                        // the whole block: nothing of this row is written
    const float* x = logits + r * ldl;
    f32x4 xr[LSM_R4];
    const float lse = log_softmax_row<VEC>(x, V1, xr, red);
    const int cols = min(W, V1);
    if constexpr (MASK) row_mask_build(lsm_bits, V1, blk, ld_blk, blk_n, r);
    const uint64_t base = (uint64_t)r * (uint64_t)V1;
    // key_v, or -inf for a token that is no candidate (blocked, or a log-prob that is -inf or NaN)
    auto key_of = [&](int v) -> double {
        if constexpr (MASK) {
            if (row_mask_has(lsm_bits, v)) return -INFINITY;
        }
        const float lp = x[v] - lse;
        if (!(lp > -INFINITY)) return -INFINITY;
        return (double)lp + sbs_gumbel(seed, offset, base + (uint64_t)v);
    };
    // No threshold pass in front of the insert, unlike log_softmax_topk_k: there an entry costs one subtraction and the inserts
    // dominate; here a key costs ten Philox rounds and two fp64 logarithms, so evaluating every key once and letting the list's
    // own last entry turn most of them away is the cheaper order.
    RowTopList<LW, double> top;
    top.fill();
    for (int v = threadIdx.x; v < V1; v += 256) {
        const double key = key_of(v);
        if (key > -INFINITY) top.offer(key, v);                 // a non-candidate never enters
    }
    for (int c = 0; c < cols; ++c) {             // wave merge: pop the best head `cols` times
        double best;
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
        for (int c = 0; c < W; ++c) {
            int bp = -1;
            if (c < cols)
                for (int p = 0; p < 4; ++p) {
                    if (pos[p] >= cols || wi[p][pos[p]] == 0x7fffffff) continue;
                    if (bp < 0 || row_before(wv[p][pos[p]], wi[p][pos[p]], wv[bp][pos[bp]], wi[bp][pos[bp]])) bp = p;
                }
            const long at = (long)r * W + c;
            if (bp < 0) {                        // fewer candidates than W: the slot says so
                topk64[at] = -INFINITY;
                topv[at] = -INFINITY;
                topi[at] = 0;
                continue;
            }
            const int tok = wi[bp][pos[bp]];
            topk64[at] = wv[bp][pos[bp]];
            topv[at] = x[tok] - lse;             // the subtraction every entry of rfn_log_softmax_fwd's row gets
            topi[at] = tok;
            ++pos[bp];
        }
    }
}

extern "C" int rfn_log_softmax_topk_gumbel(const float* logits, int64_t ldl, int rows, int V1, int W, const int32_t* blk,
                                           int64_t ld_blk, const int32_t* blk_n, const int32_t* live, uint64_t seed,
                                           uint64_t offset, double* topk64, float* topv, int32_t* topi, void* stream) {
    size_t bits;
    RFN_TRY(lsm_topk_check(rows, V1, W, logits && topv && topi && topk64 && live, blk, ld_blk, blk_n, &bits));
    hipStream_t st = (hipStream_t)stream;
    lsm_topk_dispatch(lsm_vec_ok(logits, ldl, V1, nullptr, 0, 0), W, blk != nullptr, [&](auto vec, auto lw, auto mask) {
        hipLaunchKernelGGL((log_softmax_topk_gumbel_k<decltype(vec)::value, decltype(lw)::value, decltype(mask)::value>), dim3(rows),
                           dim3(256), bits, st, logits, (long)ldl, V1, W, blk, (long)ld_blk, blk_n, live, seed, offset, topk64, topv,
                           topi);
    });
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- the state before step 1 -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_sbs_begin_k(int rows, int W, int V1, uint64_t seed, uint64_t offset0,
                                                        double* __restrict__ phi, double* __restrict__ gum,
                                                        int32_t* __restrict__ live) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const bool root = r % W == 0;                // the root's G is the draw of (row k * W, token 0) at step 0
    phi[r] = root ? 0.0 : -INFINITY;
    gum[r] = root ? sbs_gumbel(seed, offset0, (uint64_t)r * (uint64_t)V1) : -INFINITY;
    live[r] = root ? 1 : 0;
}
extern "C" int rfn_beam_sbs_begin(int NB, int W, int V1, uint64_t seed, uint64_t offset0, double* phi, double* gumbel,
                                  int32_t* live, void* stream) {
    if (NB < 1 || W < 1 || W > BEAM_MAX_W || V1 < 1) return RFN_ERR_SHAPE;
    if (!phi || !gumbel || !live) return RFN_ERR_ARG;
    const int rows = NB * W;
    hipLaunchKernelGGL(beam_sbs_begin_k, dim3(rfn_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, rows, W, V1, seed, offset0,
                       phi, gumbel, live);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- one step of the search, one block per image ---------------------------------------------------------------------------
// ln(1 - exp(a)), a <= 0 (Maechler's split at -ln 2); a == 0 gives -inf.
__device__ __forceinline__ double sbs_log1mexp(double a) { return a > -0.6931471805599453 ? log(-expm1(a)) : log1p(-exp(a)); }

// Slot q * cols + c holds candidate c of row q (its list's column c, or "itself" in column 0 of a finished row), or is invalid
// (c_q < 0).  Every valid slot counts the valid slots that precede it in (G' descending, row ascending, token ascending): its
// rank, and ranks < W are the new rows -- the order is total, so no rank is taken twice.  All threads then write the rows.
__global__ __launch_bounds__(SBS_THREADS) void beam_step_sbs_k(const double* __restrict__ topk64, const float* __restrict__ topv,
                                                               const int32_t* __restrict__ topi, int V1, int W, int S, int t, int NB,
                                                               int64_t* __restrict__ bs, float* __restrict__ bl,
                                                               double* __restrict__ phi, double* __restrict__ gum,
                                                               int32_t* __restrict__ live, int32_t* __restrict__ order,
                                                               int64_t* __restrict__ nxt, double* __restrict__ weight,
                                                               int32_t* __restrict__ n_live) {
    __shared__ int prev_seq[BEAM_MAX_S][BEAM_MAX_W];
    __shared__ float prev_lp[BEAM_MAX_S][BEAM_MAX_W];
    __shared__ double p_phi[BEAM_MAX_W], p_g[BEAM_MAX_W];
    __shared__ int p_live[BEAM_MAX_W];
    __shared__ double c_g[BEAM_MAX_W * BEAM_MAX_W], c_phi[BEAM_MAX_W * BEAM_MAX_W];
    __shared__ float c_lp[BEAM_MAX_W * BEAM_MAX_W];
    __shared__ int c_tok[BEAM_MAX_W * BEAM_MAX_W], c_q[BEAM_MAX_W * BEAM_MAX_W];
    __shared__ int sel[BEAM_MAX_W];
    __shared__ int nc_s;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int cols = min(W, V1), total = W * cols;
    beam_snapshot(prev_seq, prev_lp, bs, bl, k, W, NB, t, tid, SBS_THREADS);
    if (tid < W) {
        p_phi[tid] = phi[k * W + tid];
        p_g[tid] = gum[k * W + tid];
        p_live[tid] = live[k * W + tid];
    }
    if (tid == 0) nc_s = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < total; i += SBS_THREADS) {
        const int q = i / cols, c = i - q * cols;
        const bool fin = t > 1 && prev_seq[t - 2][q] == 0;
        int ok = 0;
        if (p_live[q] && fin) {                  // a finished row is carried: the single candidate "itself"
            if (c == 0) {
                ok = 1;
                c_g[i] = p_g[q];
                c_phi[i] = p_phi[q];
                c_lp[i] = 0.f;
                c_tok[i] = 0;
            }
        } else if (p_live[q]) {
            const long at = (long)(k * W + q) * W;
            const double key = topk64[at + c];
            if (key > -INFINITY) {
                ok = 1;
                const float lp = topv[at + c];
                const double gq = p_g[q], gamma = p_phi[q] + key;
                double g = gq;                   // the argmax child keeps its parent's G exactly
                if (c > 0) {
                    const double z = p_phi[q] + topk64[at];
                    const double d = gq - gamma + sbs_log1mexp(gamma - z);
                    g = gq - fmax(0.0, d) - log1p(exp(-fabs(d)));
                }
                c_g[i] = g;
                c_phi[i] = p_phi[q] + (double)lp;
                c_lp[i] = lp;
                c_tok[i] = topi[at + c];
            }
        }
        c_q[i] = ok ? q : -1;
        mine += ok;
    }
    if (mine) atomicAdd(&nc_s, mine);
    __syncthreads();
    const int nnew = min(W, nc_s);
    for (int i = tid; i < total; i += SBS_THREADS) {
        const int qi = c_q[i];
        if (qi < 0) continue;
        const double gi = c_g[i];
        const int ti = c_tok[i];
        const int rank = beam_rank(total, W, i, [&](int j) { return c_q[j] >= 0; }, [&](int j, int) {
            const int qj = c_q[j];
            const double gj = c_g[j];
            return (gj > gi) || (gj == gi && (qj < qi || (qj == qi && c_tok[j] < ti)));
        });
        if (rank < W) sel[rank] = i;
    }
    __syncthreads();
    for (int i = tid; i < W * S; i += SBS_THREADS) {
        const int vix = i / S, s = i - vix * S;
        const long at = ((long)s * NB + k) * W + vix;
        if (vix < nnew) {
            const int ci = sel[vix], qq = c_q[ci];
            if (s < t - 1) {
                bs[at] = prev_seq[s][qq];
                bl[at] = prev_lp[s][qq];
            } else if (s == t - 1) {
                bs[at] = c_tok[ci];
                bl[at] = c_lp[ci];
            }                                    // later columns: still the initial zeros
        } else if (s <= t - 1) {                 // a dead row holds nothing
            bs[at] = 0;
            bl[at] = 0.f;
        }
    }
    if (tid < W) {
        const int row = k * W + tid;
        if (tid < nnew) {
            const int ci = sel[tid];
            order[row] = k * W + c_q[ci];
            nxt[row] = c_tok[ci];
            phi[row] = c_phi[ci];
            gum[row] = c_g[ci];
            live[row] = 1;
        } else {
            order[row] = row;
            nxt[row] = 0;
            phi[row] = -INFINITY;
            gum[row] = -INFINITY;
            live[row] = 0;
        }
        if (t == S) {                            // Kool et al.'s weights: the last live row is the threshold
            double w = 0.0;
            if (tid < nnew - 1) {
                const double kappa = c_g[sel[nnew - 1]], ph = c_phi[sel[tid]];
                w = exp(ph) / -expm1(-exp(ph - kappa));
            }
            weight[row] = w;
            if (tid == 0) n_live[k] = nnew;
        }
    }
}

extern "C" int rfn_beam_step_sbs(const double* topk64, const float* topv, const int32_t* topi, int V1, int W, int S, int t, int NB,
                                 int64_t* beam_seq, float* beam_lp, double* phi, double* gumbel, int32_t* live, int32_t* order,
                                 int64_t* next_ids, double* weight, int32_t* n_live, void* stream) {
    if (W < 1 || W > BEAM_MAX_W || S < 1 || S > BEAM_MAX_S || t < 1 || t > S || NB < 1 || V1 < 1) return RFN_ERR_SHAPE;
    if (!topk64 || !topv || !topi || !beam_seq || !beam_lp || !phi || !gumbel || !live || !order || !next_ids || !weight || !n_live)
        return RFN_ERR_ARG;
    hipLaunchKernelGGL(beam_step_sbs_k, dim3(NB), dim3(SBS_THREADS), 0, (hipStream_t)stream, topk64, topv, topi, V1, W, S, t, NB,
                       beam_seq, beam_lp, phi, gumbel, live, order, next_ids, weight, n_live);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
