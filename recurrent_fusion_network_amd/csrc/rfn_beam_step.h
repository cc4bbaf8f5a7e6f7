// The scaffolding the beam-step kernels share (rfn_beam.hip: plain, diverse, lexical; rfn_sbs.hip: stochastic): one block per
// image, the image's beams snapshotted in LDS before the step, candidates ranked by counting, forks written by all threads.
// The searches' algorithms differ and stay in their kernels; the helpers take the kernel's own __shared__ arrays by pointer.
#pragma once
#include "rfn_rows.h"

#define BEAM_MAX_W 32     /* beams per image; the full-row form (rfn_beam_step) serves up to BEAM_WAVES of them */
#define BEAM_MAX_S 64     /* decode steps a block keeps the beams' histories for (seq_length) */
static_assert(BEAM_MAX_W == LSM_TOPW, "a beam row hands over one list entry per beam");

// Rows b0 .. b0+nb-1 of image k stay where they are and feed token 0: a search that has ended, a group or state without a
// candidate, the unoccupied rows of a state.
__device__ __forceinline__ void beam_rows_inert(int32_t* __restrict__ order, int64_t* __restrict__ nxt, int k, int W, int b0, int nb,
                                                int tid) {
    if (tid < nb) {
        order[k * W + b0 + tid] = k * W + b0 + tid;
        nxt[k * W + b0 + tid] = 0;
    }
}

// The image's beams before this step (forks read the OLD columns, :488-489).  The caller's barrier follows.
__device__ __forceinline__ void beam_snapshot(int (*prev_seq)[BEAM_MAX_W], float (*prev_lp)[BEAM_MAX_W], const int64_t* bs,
                                              const float* bl, int k, int W, int NB, int t, int tid, int nthr) {
    for (int i = tid; i < (t - 1) * W; i += nthr) {
        const int s = i / W, w = i - s * W;
        prev_seq[s][w] = (int)bs[((long)s * NB + k) * W + w];
        prev_lp[s][w] = bl[((long)s * NB + k) * W + w];
    }
}

// The top-W lists (rfn_log_softmax_topk and its kin) of the image's first `rows` beam rows, `cols` entries each.
__device__ __forceinline__ void beam_load_lists(float (*ys)[BEAM_MAX_W], int (*ix)[BEAM_MAX_W], const float* __restrict__ topv,
                                                const int32_t* __restrict__ topi, int k, int W, int rows, int cols, int tid,
                                                int nthr) {
    for (int i = tid; i < rows * cols; i += nthr) {
        const int q = i / cols, c = i - q * cols;
        ys[q][c] = topv[(long)(k * W + q) * W + c];
        ix[q][c] = topi[(long)(k * W + q) * W + c];
    }
}

// The rank of candidate i: how many valid candidates precede it in the search's stable order (before(j, i): j comes first).
// Ranks < cap are the new rows, so the count stops at cap.
template <class Valid, class Before>
__device__ __forceinline__ int beam_rank(int total, int cap, int i, Valid valid, Before before) {
    int rank = 0;
    for (int j = 0; j < total && rank < cap; ++j) rank += valid(j) && before(j, i);
    return rank;
}

// The reference's done-beam rule (:508-514), thread 0's: a new beam that emitted END, and every new beam of the last step, is
// appended to the image's done beams in construction order while there is room -> its slot (n moves on), or -1.
__device__ __forceinline__ int beam_take_done_slot(int tok, float p, int t, int S, int k, int MAXD, int& n,
                                                   float* __restrict__ done_p) {
    if (!((tok == 0 || t == S) && n < MAXD)) return -1;
    done_p[(long)k * MAXD + n] = p;
    return n++;
}

// Phase 2b of a step (all threads of the block): the forked columns and the done beams of the beams b0 .. b0+nb-1 of image k
// (the whole image, or one group of a diverse search).  sel_ci[vix] is the candidate that becomes beam b0 + vix (vix < nnew),
// cand_q its source beam within the image, slot_s[vix] its done slot or -1; prev_* is the snapshot of the image's beams before
// the step.  Needs nthr >= nb.
__device__ __forceinline__ void beam_fork_write(int k, int tid, int nthr, int W, int b0, int nb, int nnew, int S, int t, int NB,
                                                int MAXD, int64_t* __restrict__ bs, float* __restrict__ bl,
                                                float* __restrict__ bsum, int32_t* __restrict__ order, int64_t* __restrict__ nxt,
                                                int64_t* __restrict__ done_seq, float* __restrict__ done_lp,
                                                const int (*prev_seq)[BEAM_MAX_W], const float (*prev_lp)[BEAM_MAX_W],
                                                const float* cand_p, const float* cand_r, const int* cand_c, const int* cand_q,
                                                const int* sel_ci, const int* slot_s) {
    for (int i = tid; i < nnew * S; i += nthr) {
        const int vix = i / S, s = i - vix * S;
        const int ci = sel_ci[vix], qq = cand_q[ci];
        int64_t tok;
        float lp;
        const long at = ((long)s * NB + k) * W + b0 + vix;
        if (s < t - 1) {
            tok = prev_seq[s][qq];
            lp = prev_lp[s][qq];
            bs[at] = tok;
            bl[at] = lp;
        } else if (s == t - 1) {
            tok = cand_c[ci];
            lp = cand_r[ci];
            bs[at] = tok;
            bl[at] = lp;
        } else {  // columns this search has not reached yet (still the initial zeros)
            tok = bs[at];
            lp = bl[at];
        }
        const int slot = slot_s[vix];
        if (slot >= 0) {
            done_seq[((long)k * MAXD + slot) * S + s] = tok;
            done_lp[((long)k * MAXD + slot) * S + s] = lp;
        }
    }
    if (tid < nb) {
        const int vix = tid, row = k * W + b0 + vix;
        if (vix < nnew) {
            const int ci = sel_ci[vix];
            order[row] = k * W + cand_q[ci];
            nxt[row] = cand_c[ci];
            bsum[row] = cand_p[ci];                  // every read of these beams' bsum happened before the caller's barrier
        } else {  // keeps its previous state and tokens (new_state = clone(state), :485)
            order[row] = row;
            nxt[row] = bs[((long)(t - 1) * NB + k) * W + b0 + vix];
        }
    }
}
