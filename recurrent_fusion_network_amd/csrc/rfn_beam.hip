// Batched, device-resident beam search bookkeeping for sample_beam (misc/RecurrentFusionModel.py:451-531).
//
// The reference searches one image at a time with a full-vocabulary sort on the host and Python lists.  Here all
// images' beams share one decoder batch (NB*W rows) and one block per image does the step's bookkeeping on the
// device, reproducing the reference exactly:
//   * per beam row the top min(W, V+1) log-probs in descending order (only those columns are ever used, :466);
//   * candidates in (sorted column c outer, beam q inner) order, skipping beams that already emitted END (:470-478);
//     at t == 1 only row 0 is live (:468-469);
//   * STABLE descending sort by cumulative log-prob p (Python's sorted, :482), fp32 sums as the reference's tensors;
//   * fork bookkeeping of beam_seq / beam_seq_logprobs / beam_logprobs_sum and the recurrent-state gather (:491-506);
//   * done beams appended in construction order when END is emitted or t == seq_length (:508-514);
//   * an image with no candidate left stops (:480-481).
// Nothing is read back per step; the host sorts the (few) done beams once at the end.
// The diverse search (beam groups with a Hamming penalty, which the reference does not have) is the second kernel below, the
// lexically constrained search (required words: one beam per subset of satisfied sets) the third.
#include "rfn_beam_step.h"   // BEAM_MAX_W / BEAM_MAX_S and the scaffolding shared with rfn_sbs.hip; rfn_rows.h through it

#define BEAM_THREADS 1024
#define BEAM_WAVES 16

// One block per image.  Phase 1: top `cols` columns of every live beam row -- each row is cut over 16 / rows waves,
// every lane keeps a sorted top-LW list of its strided share in registers (one pass over the row), the wave merges
// the lanes' lists with `cols` arg-max butterflies, one lane merges the waves' lists.  The list and its order (row_before:
// value desc, index asc, as the reference's descending sort lists the columns it uses) are rfn_rows.h's, the ones
// rfn_log_softmax_topk uses: the two forms of the step agree because they share them.  Phase 2: thread 0 builds and
// stably sorts the <= W*W candidates in LDS and decides forks / done slots; all threads then write the forked
// beam_seq / beam_logprobs columns and the done beams in parallel.
template <int LW>
__global__ __launch_bounds__(BEAM_THREADS) void beam_step_k(
    const float* __restrict__ logp, long ldl, int V1, int W, int S, int t, int NB, int MAXD, int64_t* __restrict__ bs,
    float* __restrict__ bl, float* __restrict__ bsum, int32_t* __restrict__ order, int64_t* __restrict__ nxt,
    int64_t* __restrict__ done_seq, float* __restrict__ done_lp, float* __restrict__ done_p,
    int32_t* __restrict__ done_n, int32_t* __restrict__ active, const float* __restrict__ topv,
    const int32_t* __restrict__ topi) {
    __shared__ float ys[BEAM_MAX_W][BEAM_MAX_W];
    __shared__ int ix[BEAM_MAX_W][BEAM_MAX_W];
    __shared__ float wys[BEAM_WAVES][BEAM_MAX_W];
    __shared__ int wix[BEAM_WAVES][BEAM_MAX_W];
    __shared__ int prev_seq[BEAM_MAX_S][BEAM_MAX_W];
    __shared__ float prev_lp[BEAM_MAX_S][BEAM_MAX_W];
    __shared__ float cand_p[BEAM_MAX_W * BEAM_MAX_W], cand_r[BEAM_MAX_W * BEAM_MAX_W];
    __shared__ int cand_c[BEAM_MAX_W * BEAM_MAX_W], cand_q[BEAM_MAX_W * BEAM_MAX_W], cand_ord[BEAM_MAX_W * BEAM_MAX_W];
    __shared__ int sel_ci[BEAM_MAX_W], slot_s[BEAM_MAX_W];
    __shared__ int nnew_s;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cols = min(W, V1);
    if (!active[k]) return beam_rows_inert(order, nxt, k, W, 0, W, tid);   // this image's search has ended
    // ---- phase 1: top `cols` of every live beam row (descending, lowest index first on ties) -----------------
    const int live_rows = (t == 1) ? 1 : W;
    const int wpr = topv ? 1 : BEAM_WAVES / live_rows;   // waves per row (full-row form: >= 1, the host checks W <= BEAM_WAVES)
    const int q = wave / wpr, part = wave - q * wpr;
    if (topv) {
        // the rows' top-W lists were produced with their log-softmax (rfn_log_softmax_topk): same values, same order
    } else if (q < live_rows) {
        const float* row = logp + (long)(k * W + q) * ldl;
        const int chunk = (V1 + wpr - 1) / wpr;
        const int v0 = part * chunk, v1 = min(V1, v0 + chunk);
        RowTopList<LW> top;
        top.fill();
        for (int v = v0 + lane; v < v1; v += 64) top.offer(row[v], v);   // ascending v per lane: a later equal value stays behind
        for (int c = 0; c < cols; ++c) {             // wave merge: pop the best head `cols` times
            float best;
            int bi;
            top.wave_pop(best, bi);
            if (lane == 0) {
                wys[wave][c] = best;
                wix[wave][c] = bi;
            }
        }
    }
    beam_snapshot(prev_seq, prev_lp, bs, bl, k, W, NB, t, tid, (int)blockDim.x);
    __syncthreads();
    if (topv) {
        beam_load_lists(ys, ix, topv, topi, k, W, live_rows, cols, tid, (int)blockDim.x);
    } else if (tid < live_rows) {                    // merge the row's wave lists (each already sorted)
        int pos[BEAM_WAVES];
        for (int p = 0; p < wpr; ++p) pos[p] = 0;
        for (int c = 0; c < cols; ++c) {
            int bp = -1;
            for (int p = 0; p < wpr; ++p) {
                if (pos[p] >= cols) continue;
                const int w = tid * wpr + p;
                if (wix[w][pos[p]] == 0x7fffffff) continue;
                if (bp < 0 || row_before(wys[w][pos[p]], wix[w][pos[p]], wys[tid * wpr + bp][pos[bp]],
                                         wix[tid * wpr + bp][pos[bp]]))
                    bp = p;
            }
            ys[tid][c] = wys[tid * wpr + bp][pos[bp]];
            ix[tid][c] = wix[tid * wpr + bp][pos[bp]];
            ++pos[bp];
        }
    }
    __syncthreads();

    // ---- phase 2a (thread 0): candidates in (c outer, q inner) order, stable sort, fork / done decisions --------
    if (tid == 0) {
        int nc = 0;
        for (int c = 0; c < cols; ++c)
            for (int qq = 0; qq < live_rows; ++qq) {
                if (t > 1 && prev_seq[t - 2][qq] == 0) continue;
                const float local = ys[qq][c];
                cand_c[nc] = ix[qq][c];
                cand_q[nc] = qq;
                cand_r[nc] = local;
                cand_p[nc] = bsum[k * W + qq] + local;  // fp32 add, as the reference's tensor arithmetic
                ++nc;
            }
        if (nc == 0) active[k] = 0;  // :480-481
        for (int i = 0; i < nc; ++i) {  // stable insertion sort of indices by descending p
            int j = i;
            const float pi = cand_p[i];
            while (j > 0 && cand_p[cand_ord[j - 1]] < pi) {
                cand_ord[j] = cand_ord[j - 1];
                --j;
            }
            cand_ord[j] = i;
        }
        const int nnew = min(W, nc);
        int n = done_n[k];
        for (int vix = 0; vix < W; ++vix) {
            slot_s[vix] = -1;
            if (vix >= nnew) continue;
            const int ci = cand_ord[vix];
            sel_ci[vix] = ci;
            slot_s[vix] = beam_take_done_slot(cand_c[ci], cand_p[ci], t, S, k, MAXD, n, done_p);
        }
        done_n[k] = n;
        nnew_s = (nc == 0) ? -1 : nnew;
    }
    __syncthreads();
    const int nnew = nnew_s;
    if (nnew < 0) return beam_rows_inert(order, nxt, k, W, 0, W, tid);   // no candidate left: the image stops
    beam_fork_write(k, tid, (int)blockDim.x, W, 0, W, nnew, S, t, NB, MAXD, bs, bl, bsum, order, nxt, done_seq, done_lp, prev_seq,
                    prev_lp, cand_p, cand_r, cand_c, cand_q, sel_ci, slot_s);
}

static int beam_step_launch(const float* logp, int64_t ldl, const float* topv, const int32_t* topi, int V1, int W, int S, int t,
                            int NB, int max_done, int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order,
                            int64_t* next_ids, int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n,
                            int32_t* active, void* stream) {
    if (W < 1 || W > BEAM_MAX_W || S < 1 || S > BEAM_MAX_S || t < 1 || t > S || NB < 1 || V1 < 1 || max_done < 1)
        return RFN_ERR_SHAPE;
    if (!topv && W > BEAM_WAVES) return RFN_ERR_SHAPE;   // the full-row form cuts a row over 16 / W waves
    if ((!logp && !(topv && topi)) || !beam_seq || !beam_lp || !beam_sum || !order || !next_ids || !done_seq || !done_lp ||
        !done_p || !done_n || !active)
        return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int threads = topv ? 256 : BEAM_THREADS;      // without the row scan the block only does the bookkeeping
#define BEAM_LAUNCH(LWV)                                                                                             \
    hipLaunchKernelGGL(beam_step_k<LWV>, dim3(NB), dim3(threads), 0, st, logp, (long)ldl, V1, W, S, t, NB,            \
                       max_done, beam_seq, beam_lp, beam_sum, order, next_ids, done_seq, done_lp, done_p, done_n,     \
                       active, topv, topi)
    if (W <= 2) BEAM_LAUNCH(2);
    else if (W <= 4) BEAM_LAUNCH(4);
    else if (W <= 8) BEAM_LAUNCH(8);
    else BEAM_LAUNCH(16);
#undef BEAM_LAUNCH
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_beam_step(const float* logp, int64_t ldl, int V1, int W, int S, int t, int NB, int max_done,
                             int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* next_ids,
                             int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active,
                             void* stream) {
    if (!logp) return RFN_ERR_ARG;
    return beam_step_launch(logp, ldl, nullptr, nullptr, V1, W, S, t, NB, max_done, beam_seq, beam_lp, beam_sum, order, next_ids,
                            done_seq, done_lp, done_p, done_n, active, stream);
}
// The same step fed with every beam row's W best log-probs (rfn_log_softmax_topk) instead of the full rows.
extern "C" int rfn_beam_step_topk(const float* topv, const int32_t* topi, int V1, int W, int S, int t, int NB, int max_done,
                                  int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* next_ids,
                                  int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active,
                                  void* stream) {
    if (!topv || !topi) return RFN_ERR_ARG;
    return beam_step_launch(nullptr, 0, topv, topi, V1, W, S, t, NB, max_done, beam_seq, beam_lp, beam_sum, order, next_ids,
                            done_seq, done_lp, done_p, done_n, active, stream);
}

// =============================================================================================
// diverse beam search: G groups of Wg = W / G beams with a Hamming penalty (rfn.h "diverse beam search")
// =============================================================================================
#define BEAM_DIV_THREADS 256
#define BEAM_DIV_MAXC (BEAM_MAX_W * BEAM_MAX_W / 2)   /* candidates of one group: cols * Wg <= W * W / G, G >= 2 */

// The ranking key of a penalised candidate: three fp32 operations, each rounded on its own (no FMA).
__device__ __forceinline__ float beam_div_key(float sum, float local, float lambda, int count) {
#pragma clang fp contract(off)
    const float pen = lambda * (float)count;
    const float aug = local - pen;
    return sum + aug;
}

// One block per image, the groups one after the other.  Per group: thread 0 lists the live rows; every candidate (column c
// outer, live row inner) gets its unaugmented p and its key from the LDS list of the tokens the earlier groups chose at this
// step; every candidate counts the candidates that precede it in the stable descending order of the keys (greater key, or
// equal key and lower construction index) -- that count is its rank, and ranks < Wg are the group's new beams; thread 0
// hands out the done slots in rank order and appends the chosen tokens to the list; all threads write the forks
// (beam_fork_write, as beam_step_k).  A group reads and writes its own beams' columns and sums only.
__global__ __launch_bounds__(BEAM_DIV_THREADS) void beam_step_div_k(
    const float* __restrict__ topv, const int32_t* __restrict__ topi, int V1, int W, int G, float lambda, int S, int t, int NB,
    int MAXD, int64_t* __restrict__ bs, float* __restrict__ bl, float* __restrict__ bsum, int32_t* __restrict__ order,
    int64_t* __restrict__ nxt, int64_t* __restrict__ done_seq, float* __restrict__ done_lp, float* __restrict__ done_p,
    int32_t* __restrict__ done_n, int32_t* __restrict__ done_group, int32_t* __restrict__ active) {
    __shared__ float ys[BEAM_MAX_W][BEAM_MAX_W];
    __shared__ int ix[BEAM_MAX_W][BEAM_MAX_W];
    __shared__ int prev_seq[BEAM_MAX_S][BEAM_MAX_W];
    __shared__ float prev_lp[BEAM_MAX_S][BEAM_MAX_W];
    __shared__ float cand_key[BEAM_DIV_MAXC], cand_p[BEAM_DIV_MAXC], cand_r[BEAM_DIV_MAXC];
    __shared__ int cand_c[BEAM_DIV_MAXC], cand_q[BEAM_DIV_MAXC];
    __shared__ int sel_ci[BEAM_MAX_W], slot_s[BEAM_MAX_W], pen_tok[BEAM_MAX_W], liveq[BEAM_MAX_W];
    __shared__ int nl_s, npen_s;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int cols = min(W, V1), Wg = W / G;
    if (!active[k]) return beam_rows_inert(order, nxt, k, W, 0, W, tid);   // this image's search has ended
    beam_load_lists(ys, ix, topv, topi, k, W, W, cols, tid, BEAM_DIV_THREADS);
    beam_snapshot(prev_seq, prev_lp, bs, bl, k, W, NB, t, tid, BEAM_DIV_THREADS);
    __syncthreads();
    int npen = 0, n = 0, any = 0;                    // thread 0's: penalised tokens so far, done beams so far, a group had a candidate
    if (tid == 0) n = done_n[k];
    for (int g = 0; g < G; ++g) {
        const int b0 = g * Wg;
        if (tid == 0) {
            int nl = 0;
            for (int j = 0; j < (t == 1 ? 1 : Wg); ++j) {
                if (t > 1 && prev_seq[t - 2][b0 + j] == 0) continue;
                liveq[nl++] = b0 + j;
            }
            nl_s = nl;
            npen_s = npen;
            for (int v = 0; v < Wg; ++v) sel_ci[v] = 0;
        }
        __syncthreads();
        const int nl = nl_s, nc = cols * nl, np = npen_s;
        for (int i = tid; i < nc; i += BEAM_DIV_THREADS) {
            const int c = i / nl, q = liveq[i - c * nl];
            const float local = ys[q][c], sum = bsum[k * W + q];
            const int v = ix[q][c];
            const float p = sum + local;             // fp32 add, as the reference's tensor arithmetic
            int count = 0;
            if (v != 0)
                for (int j = 0; j < np; ++j) count += pen_tok[j] == v;
            cand_c[i] = v;
            cand_q[i] = q;
            cand_r[i] = local;
            cand_p[i] = p;
            cand_key[i] = count ? beam_div_key(sum, local, lambda, count) : p;
        }
        __syncthreads();
        for (int i = tid; i < nc; i += BEAM_DIV_THREADS) {
            const float ki = cand_key[i];
            const int rank = beam_rank(nc, Wg, i, [](int) { return true; }, [&](int j, int me) {
                const float kj = cand_key[j];
                return (kj > ki) || (kj == ki && j < me);
            });
            if (rank < Wg) sel_ci[rank] = i;
        }
        __syncthreads();
        const int nnew = min(Wg, nc);
        if (tid == 0) {
            for (int vix = 0; vix < Wg; ++vix) {
                slot_s[vix] = -1;
                if (vix >= nnew) continue;
                const int ci = sel_ci[vix], tok = cand_c[ci];
                const int slot = beam_take_done_slot(tok, cand_p[ci], t, S, k, MAXD, n, done_p);   // in order: group, then vix
                slot_s[vix] = slot;
                if (slot >= 0) done_group[(long)k * MAXD + slot] = g;
                if (tok != 0) pen_tok[npen++] = tok;     // END is never counted
            }
            any |= nc > 0;
        }
        __syncthreads();
        if (nc == 0) {  // no candidate left for the group
            beam_rows_inert(order, nxt, k, W, b0, Wg, tid);
        } else {
            beam_fork_write(k, tid, BEAM_DIV_THREADS, W, b0, Wg, nnew, S, t, NB, MAXD, bs, bl, bsum, order, nxt, done_seq, done_lp,
                            prev_seq, prev_lp, cand_p, cand_r, cand_c, cand_q, sel_ci, slot_s);
        }
        __syncthreads();                             // the next group reuses the candidate arrays
    }
    if (tid == 0) {
        done_n[k] = n;
        if (!any) active[k] = 0;
    }
}

extern "C" int rfn_beam_step_div(const float* topv, const int32_t* topi, int V1, int W, int G, float lambda, int S, int t, int NB,
                                 int max_done, int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order,
                                 int64_t* next_ids, int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n,
                                 int32_t* done_group, int32_t* active, void* stream) {
    if (G < 1 || W < 1 || W % G || !(lambda >= 0.f)) return RFN_ERR_SHAPE;
    if (G == 1)
        return rfn_beam_step_topk(topv, topi, V1, W, S, t, NB, max_done, beam_seq, beam_lp, beam_sum, order, next_ids, done_seq,
                                  done_lp, done_p, done_n, active, stream);
    if (W > BEAM_MAX_W || S < 1 || S > BEAM_MAX_S || t < 1 || t > S || NB < 1 || V1 < 1 || max_done < 1) return RFN_ERR_SHAPE;
    if (!topv || !topi || !beam_seq || !beam_lp || !beam_sum || !order || !next_ids || !done_seq || !done_lp || !done_p ||
        !done_n || !done_group || !active)
        return RFN_ERR_ARG;
    hipLaunchKernelGGL(beam_step_div_k, dim3(NB), dim3(BEAM_DIV_THREADS), 0, (hipStream_t)stream, topv, topi, V1, W, G, lambda, S,
                       t, NB, max_done, beam_seq, beam_lp, beam_sum, order, next_ids, done_seq, done_lp, done_p, done_n,
                       done_group, active);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// =============================================================================================
// lexically constrained beam search: 2^C states of Wb = W / 2^C beams (rfn.h "lexically constrained beam search")
// =============================================================================================
#define BEAM_LEX_THREADS 256
#define BEAM_LEX_MAXG (1 << RFN_LEX_MAX_SETS)
// Candidate slots of one target state: its own rows' list columns (cols * Wb <= 32 * Wb) and the other states' rows' want entries
// (NW * (W - Wb)).  With W <= 32, Wb <= W / 2 and NW <= min(16, W - Wb) the largest is Wb = 16, W = 32, NW = 16: 512 + 256.
#define BEAM_LEX_MAXC (BEAM_MAX_W * (BEAM_MAX_W / 2) + RFN_LEX_MAX_IDS * (BEAM_MAX_W / 2))
// Static LDS: ys + ix 8 KiB, prev_seq + prev_lp 16 KiB, four candidate arrays 12 KiB, the want values 2 KiB, small change: about
// 38.5 KiB of the 64 KiB a block may declare.

// One block per image, the target states one after the other, all of them reading the LDS snapshot of the beams before the step
// (a target reads rows of the states below it, which this step has already rewritten in memory).  Per target: every slot of the
// construction order (source states ascending; a source's want entries j outer / row inner when it moves here, its list columns
// c outer / row inner when it is the target itself) is filled or marked invalid (row not live, another destination, -inf); every
// valid slot counts the valid slots that precede it in the stable descending order of p -- its rank, as beam_step_div_k; thread
// 0 hands out the done slots; all threads write the forks (beam_fork_write) and the inert rest of the state's rows.
__global__ __launch_bounds__(BEAM_LEX_THREADS) void beam_step_lex_k(
    const float* __restrict__ topv, const int32_t* __restrict__ topi, const float* __restrict__ wantv,
    const int32_t* __restrict__ want, const int32_t* __restrict__ want_bits, int NW, int C, int V1, int W, int S, int t, int NB,
    int MAXD, int64_t* __restrict__ bs, float* __restrict__ bl, float* __restrict__ bsum, int32_t* __restrict__ order,
    int64_t* __restrict__ nxt, int64_t* __restrict__ done_seq, float* __restrict__ done_lp, float* __restrict__ done_p,
    int32_t* __restrict__ done_n, int32_t* __restrict__ state_n, int32_t* __restrict__ done_state,
    const int32_t* __restrict__ init_state, int32_t* __restrict__ active) {
    __shared__ float ys[BEAM_MAX_W][BEAM_MAX_W];
    __shared__ int ix[BEAM_MAX_W][BEAM_MAX_W];
    __shared__ float wv[BEAM_MAX_W][RFN_LEX_MAX_IDS];
    __shared__ int wid[RFN_LEX_MAX_IDS], wb[RFN_LEX_MAX_IDS];
    __shared__ int prev_seq[BEAM_MAX_S][BEAM_MAX_W];
    __shared__ float prev_lp[BEAM_MAX_S][BEAM_MAX_W];
    __shared__ float prev_sum[BEAM_MAX_W];
    __shared__ int prev_n[BEAM_LEX_MAXG];
    __shared__ float cand_p[BEAM_LEX_MAXC], cand_r[BEAM_LEX_MAXC];
    __shared__ int cand_c[BEAM_LEX_MAXC], cand_q[BEAM_LEX_MAXC];      // cand_q < 0: an invalid slot
    __shared__ int sel_ci[BEAM_MAX_W], slot_s[BEAM_MAX_W];
    __shared__ int nvalid_s, first_s, nnew_s;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int G = 1 << C, Wb = W / G, cols = min(W, V1);
    if (!active[k]) return beam_rows_inert(order, nxt, k, W, 0, W, tid);   // this image's search has ended
    beam_load_lists(ys, ix, topv, topi, k, W, W, cols, tid, BEAM_LEX_THREADS);
    for (int i = tid; i < W * NW; i += BEAM_LEX_THREADS) {
        const int q = i / NW, j = i - q * NW;
        wv[q][j] = wantv[(long)(k * W + q) * NW + j];
    }
    if (tid < NW) {   // an id outside [1, V1) (the -1 padding) is in no set: never a move, never met in a list
        const int id = want[k * NW + tid];
        wid[tid] = id;
        wb[tid] = (id >= 1 && id < V1) ? (want_bits[k * NW + tid] & (G - 1)) : 0;
    }
    beam_snapshot(prev_seq, prev_lp, bs, bl, k, W, NB, t, tid, BEAM_LEX_THREADS);
    if (tid < W) prev_sum[tid] = bsum[k * W + tid];
    if (tid < G) {   // before step 1 only the first row of the initial state is occupied
        int n = (t == 1) ? (tid == (init_state[k] & (G - 1)) ? 1 : 0) : state_n[k * G + tid];
        prev_n[tid] = min(max(n, 0), Wb);
    }
    __syncthreads();
    int n = 0, any = 0;                              // thread 0's: done beams so far, a state had a candidate
    if (tid == 0) n = done_n[k];
    for (int s = 0; s < G; ++s) {
        const int b0 = s * Wb;
        int total = 0;                               // the slots of target s
        for (int sp = 0; sp <= s; ++sp)
            if ((sp & ~s) == 0) total += (sp == s ? cols : NW) * prev_n[sp];
        if (tid == 0) {
            nvalid_s = 0;
            first_s = BEAM_LEX_MAXC;
        }
        if (tid < Wb) sel_ci[tid] = -1;
        __syncthreads();
        int mine = 0, first = BEAM_LEX_MAXC;
        for (int i = tid; i < total; i += BEAM_LEX_THREADS) {
            int sp = 0, off = 0;                     // the source state of slot i and the first slot of its segment
            for (;; ++sp) {
                if ((sp & ~s) != 0) continue;
                const int len = (sp == s ? cols : NW) * prev_n[sp];
                if (i < off + len) break;
                off += len;
            }
            const int np = prev_n[sp], a = (i - off) / np, q = sp * Wb + (i - off) - a * np;   // a: column, or want index
            bool ok = t == 1 || prev_seq[t - 2][q] != 0;
            float local;
            int v;
            if (sp == s) {
                local = ys[q][a];
                v = ix[q][a];
                int vb = 0;
                for (int j = 0; j < NW; ++j) vb |= (wid[j] == v) ? wb[j] : 0;
                ok = ok && (vb & ~s) == 0;
            } else {
                local = wv[q][a];
                v = wid[a];
                ok = ok && (wb[a] & ~sp) != 0 && (sp | wb[a]) == s;
            }
            ok = ok && !(local == -INFINITY);
            cand_c[i] = v;
            cand_q[i] = ok ? q : -1;
            cand_r[i] = local;
            cand_p[i] = prev_sum[q] + local;         // fp32 add, as the reference's tensor arithmetic
            if (ok) {
                ++mine;
                first = min(first, i);
            }
        }
        if (mine) {
            atomicAdd(&nvalid_s, mine);
            atomicMin(&first_s, first);
        }
        __syncthreads();
        for (int i = tid; i < total; i += BEAM_LEX_THREADS) {
            if (cand_q[i] < 0) continue;
            const float pi = cand_p[i];
            const int rank = beam_rank(total, Wb, i, [&](int j) { return cand_q[j] >= 0; }, [&](int j, int me) {
                const float pj = cand_p[j];
                return (pj > pi) || (pj == pi && j < me);
            });
            if (rank < Wb) sel_ci[rank] = i;
        }
        __syncthreads();
        if (tid == 0) {
            const int nvalid = nvalid_s, nnew = min(Wb, nvalid);
            for (int vix = 0; vix < Wb; ++vix) {
                slot_s[vix] = -1;
                if (vix >= nnew) continue;
                if (sel_ci[vix] < 0) sel_ci[vix] = first_s;   // only under NaN keys: stay on a valid slot
                const int ci = sel_ci[vix];
                const int slot = beam_take_done_slot(cand_c[ci], cand_p[ci], t, S, k, MAXD, n, done_p);   // in order: state, then rank
                slot_s[vix] = slot;
                if (slot >= 0) done_state[(long)k * MAXD + slot] = s;
            }
            state_n[k * G + s] = nnew;
            any |= nvalid > 0;
            nnew_s = nnew;
        }
        __syncthreads();
        const int nnew = nnew_s;
        beam_fork_write(k, tid, BEAM_LEX_THREADS, W, b0, nnew, nnew, S, t, NB, MAXD, bs, bl, bsum, order, nxt, done_seq, done_lp,
                        prev_seq, prev_lp, cand_p, cand_r, cand_c, cand_q, sel_ci, slot_s);
        beam_rows_inert(order, nxt, k, W, b0 + nnew, Wb - nnew, tid);   // the state's unoccupied rows: nothing stale is kept
        __syncthreads();                            // the next state reuses the candidate arrays
    }
    if (tid == 0) {
        done_n[k] = n;
        if (!any) active[k] = 0;
    }
}

extern "C" int rfn_beam_step_lex(const float* topv, const int32_t* topi, const float* wantv, const int32_t* want,
                                 const int32_t* want_bits, int NW, int C, int V1, int W, int S, int t, int NB, int max_done,
                                 int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* next_ids,
                                 int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* state_n,
                                 int32_t* done_state, const int32_t* init_state, int32_t* active, void* stream) {
    if (C < 0 || C > RFN_LEX_MAX_SETS) return RFN_ERR_SHAPE;
    if (C == 0)
        return rfn_beam_step_topk(topv, topi, V1, W, S, t, NB, max_done, beam_seq, beam_lp, beam_sum, order, next_ids, done_seq,
                                  done_lp, done_p, done_n, active, stream);
    if (W < 1 || W > BEAM_MAX_W || W % (1 << C) || NW < 0 || NW > RFN_LEX_MAX_IDS || NW > W - W / (1 << C)) return RFN_ERR_SHAPE;
    if (S < 1 || S > BEAM_MAX_S || t < 1 || t > S || NB < 1 || V1 < 1 || max_done < 1) return RFN_ERR_SHAPE;
    if (!topv || !topi || !beam_seq || !beam_lp || !beam_sum || !order || !next_ids || !done_seq || !done_lp || !done_p ||
        !done_n || !state_n || !done_state || !init_state || !active || (NW > 0 && (!wantv || !want || !want_bits)))
        return RFN_ERR_ARG;
    hipLaunchKernelGGL(beam_step_lex_k, dim3(NB), dim3(BEAM_LEX_THREADS), 0, (hipStream_t)stream, topv, topi, wantv, want, want_bits,
                       NW, C, V1, W, S, t, NB, max_done, beam_seq, beam_lp, beam_sum, order, next_ids, done_seq, done_lp, done_p,
                       done_n, state_n, done_state, init_state, active);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// dst[r, :] = src[order[r], :]  -- recurrent-state re-gather of the forked beams (:499-501)
__global__ __launch_bounds__(256) void gather_rows_k(const float* __restrict__ src, float* __restrict__ dst,
                                                     const int32_t* __restrict__ order, int R) {
    const int r = blockIdx.x;
    const float* s = src + (long)order[r] * R;
    for (int j = threadIdx.x; j < R; j += 256) dst[(long)r * R + j] = s[j];
}
extern "C" int rfn_gather_rows(const float* src, float* dst, const int32_t* order, int rows, int R, void* stream) {
    if (rows < 1 || R < 1) return RFN_ERR_SHAPE;
    if (!src || !dst || !order || src == dst) return RFN_ERR_ARG;
    hipLaunchKernelGGL(gather_rows_k, dim3(rows), dim3(256), 0, (hipStream_t)stream, src, dst, order, R);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
